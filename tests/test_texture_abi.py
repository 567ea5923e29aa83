"""The texture modality's part of the C-ABI on the CPU: the two new structs as a C compiler lays them out against their
ctypes mirrors (size, every field's offset, the header's defaults), and the new entry points among the HIP-only names."""
import ctypes
import os
import subprocess

import numpy as np

import util

ROOT = util.ROOT
NAMES = ("texture_modality_create", "texture_modality_model_occlusions", "texture_modality_get_region_of_interest",
         "texture_modality_set_features", "texture_modality_get_points", "texture_modality_get_keyframes")


def test_struct_sizes_offsets_and_defaults_match_the_header(tmp_path):
    capi = util.pkg._capi
    pairs = [("m3t_texture_modality_params", capi.TextureModalityParams), ("m3t_texture_data_point", capi.TextureDataPoint)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "m3t_types.h"', "int main(void) {",
             "  m3t_texture_modality_params p;", "  m3t_texture_modality_params_default(&p);"]
    for c_name, py in pairs:
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for field, _ in py._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, field, c_name, field))
    for field, kind in capi.TextureModalityParams._fields_:
        if field == "standard_deviations":
            lines.append('  printf("default.%s %%a %%a %%a\\n", p.%s[0], p.%s[1], p.%s[2]);' % (field, field, field, field))
        elif kind is ctypes.c_float:
            lines.append('  printf("default.%s %%a\\n", p.%s);' % (field, field))
        else:
            lines.append('  printf("default.%s %%d\\n", p.%s);' % (field, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                           str(exe)])
    layout = {}
    for line in subprocess.check_output([str(exe)], text=True).splitlines():
        key, *values = line.split()
        layout[key] = values
    for c_name, py in pairs:
        assert int(layout[c_name][0]) == ctypes.sizeof(py), c_name
        for field, _ in py._fields_:
            assert int(layout[c_name + "." + field][0]) == getattr(py, field).offset, (c_name, field)
    assert ctypes.sizeof(capi.TextureDataPoint) == capi.TEXTURE_DATA_POINT_DTYPE.itemsize == 40
    # the header's defaults are the reference's (texture_modality.h:400-407, 431-436) and the Python mirror's
    p = capi.TextureModalityParams()
    for field, kind in capi.TextureModalityParams._fields_:
        c_value = layout["default." + field]
        if field == "standard_deviations":
            assert [float.fromhex(v) for v in c_value] == [15.0, 5.0, 0.0] == list(p.standard_deviations)[:3]
        elif kind is ctypes.c_float:
            assert np.float32(float.fromhex(c_value[0])) == np.float32(getattr(p, field)), field
        else:
            assert int(c_value[0]) == getattr(p, field), field
    assert (p.descriptor_bytes, p.focused_image_size, p.n_standard_deviations, p.max_keyframe_age, p.n_keyframes,
            p.measure_occlusions) == (32, 200, 2, 100, 1, 0)
    assert np.float32(p.descriptor_distance_threshold) == np.float32(0.7) and p.tukey_norm_constant == 20.0
    assert np.float32(p.max_keyframe_rotation_difference) == np.float32(10.0) * np.float32(3.1415926535897) / np.float32(180.0)
    assert [np.float32(v) for v in (p.measured_occlusion_radius, p.measured_occlusion_threshold, p.modeled_occlusion_radius,
                                    p.modeled_occlusion_threshold)] == [np.float32(v) for v in (0.01, 0.03, 0.01, 0.03)]


def test_new_entry_points_are_hip_only_and_exported():
    capi = util.pkg._capi
    for name in NAMES:
        assert name in capi._HIP_ONLY and name not in capi._SIGNATURES, name
    lib = ctypes.CDLL(util.pkg.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, "m3t_hip_" + n)] == []
    header = open(os.path.join(ROOT, "include", "m3t_hip.h")).read()
    assert [n for n in NAMES if "m3t_hip_" + n + "(" not in header] == []
