"""The L2 texture modality's part of the C-ABI and of the configuration front-end on the CPU: the new entry point is
declared, HIP-only and exported beside the others (132 in all); GenerateConfiguredTracker takes descriptor_type SIFT and
DAISY with the caller's detector and l2_descriptors=True and sizes the descriptors (a recording stand-in for the device
context shows what it would create), and refuses them without the opt-in as it did; host.TextureModality refuses descriptors of another dtype or width before anything is called."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import util
from test_generator import reference_tree
from test_gpu_texture_generator import CONFIG

generator = util.pkg.generator
F = np.float32


def test_the_entry_point_is_declared_hip_only_and_exported():
    capi = util.pkg._capi
    name = "texture_modality_create_l2"
    assert name in capi._HIP_ONLY and name not in capi._SIGNATURES
    assert capi._HIP_ONLY[name] == capi._HIP_ONLY["texture_modality_create"]
    lib = ctypes.CDLL(util.pkg.LIB_PATH)
    assert hasattr(lib, "m3t_hip_" + name)
    header = open(os.path.join(util.ROOT, "include", "m3t_hip.h")).read()
    assert "m3t_hip_" + name + "(" in header
    exported = [line.split()[-1] for line in subprocess.check_output(["nm", "-D", "--defined-only", util.pkg.LIB_PATH],
                                                                     text=True).splitlines()]
    exported = [s for s in exported if s.startswith("m3t_hip_")]
    assert len(exported) == len(set(exported)) == 132
    assert set(exported) == set(re.findall(r"\b(m3t_hip_\w+)\(", header))


class Recorder:
    """stands in for a device context: hands out ids and keeps the calls"""
    is_hip = True

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))
        return len(self.calls)

    raw = call


def _generate(tmp_path, metafile, **kw):
    root = reference_tree(tmp_path)
    config = root / "tracker_test" / "texture_config.yaml"
    config.write_text(CONFIG)
    (root / "tracker_test" / "texture_modality.yaml").write_text("%YAML:1.2\n" + metafile)
    api = Recorder()
    tracker = generator.GenerateConfiguredTracker(api, str(config), **kw)
    return api, tracker.objects["TextureModality"]["triangle_texture_modality"]


@pytest.mark.parametrize("metafile, n_floats, params", [
    ('descriptor_type: "SIFT"\nsift_n_features: 400\norb_n_features: 300\n', 128,
     {"descriptor_type": "SIFT", "sift_n_features": 400, "orb_n_features": 300}),
    ("descriptor_type: 3\n", 128, {"descriptor_type": 3}),
    # DAISY: (daisy_q_radius * daisy_q_theta + 1) * daisy_q_hist, the reference's defaults 3, 4, 8
    # (texture_modality.h:417-419); 3, 8, 8 are OpenCV's own
    ('descriptor_type: "DAISY"\n', 104, {"descriptor_type": "DAISY"}),
    ('descriptor_type: "DAISY"\ndaisy_q_theta: 8\n', 200, {"descriptor_type": "DAISY", "daisy_q_theta": 8}),
    ("descriptor_type: 1\ndaisy_q_radius: 2\ndaisy_q_theta: 5\ndaisy_q_hist: 4\n", 44,
     {"descriptor_type": 1, "daisy_q_radius": 2, "daisy_q_theta": 5, "daisy_q_hist": 4}),
])
def test_generator_takes_sift_and_daisy_with_the_callers_detector(tmp_path, metafile, n_floats, params):
    api, mod = _generate(tmp_path, metafile, feature_detector=lambda image, roi, scale: ([], []), l2_descriptors=True)
    created = [name for name, _ in api.calls if name.startswith("texture_modality_create")]
    assert created == ["texture_modality_create_l2"]
    assert mod.params.descriptor_bytes == 4 * n_floats
    assert (mod.descriptor_norm, mod.descriptor_width, mod.descriptor_dtype) == ("l2", n_floats, np.float32)
    assert mod.detector_params == params


def test_generator_keeps_hamming_types_where_they_were_and_refuses_l2_with_the_builtin_detector(tmp_path):
    api, mod = _generate(tmp_path / "a", 'descriptor_type: "BRISK"\n', feature_detector=lambda image, roi, scale: ([], []))
    assert [name for name, _ in api.calls if name.startswith("texture_modality_create")] == ["texture_modality_create"]
    assert (mod.params.descriptor_bytes, mod.descriptor_norm, mod.descriptor_dtype) == (64, "hamming", np.uint8)
    for k, descriptor_type in enumerate(('"SIFT"', '"DAISY"', "1", "3")):
        with pytest.raises(ValueError, match="not a Hamming-norm descriptor"):
            _generate(tmp_path / ("b%d" % k), "descriptor_type: %s\n" % descriptor_type, feature_detector="builtin")
        with pytest.raises(ValueError, match="not a Hamming-norm descriptor"):
            _generate(tmp_path / ("d%d" % k), "descriptor_type: %s\n" % descriptor_type, feature_detector="builtin",
                      l2_descriptors=True)
        with pytest.raises(ValueError, match="l2_descriptors=True"):  # the opt-in: a callable that returns float32 rows
            _generate(tmp_path / ("e%d" % k), "descriptor_type: %s\n" % descriptor_type,
                      feature_detector=lambda image, roi, scale: ([], []))
    with pytest.raises(ValueError, match="descriptor_type"):
        _generate(tmp_path / "c", 'descriptor_type: "SURF"\n', feature_detector=lambda image, roi, scale: ([], []),
                  l2_descriptors=True)


def test_host_modality_refuses_descriptors_of_another_dtype_or_width():
    class Handle:
        id = 0

    api = Recorder()
    mod = util.host.TextureModality(api, Handle, Handle, Handle, descriptor_norm="l2", descriptor_bytes=512)
    assert api.calls[0][0] == "texture_modality_create_l2"
    keypoints = np.zeros((3, 2), F)
    for bad in (np.zeros((3, 128), np.float64), np.zeros((3, 512), np.uint8), np.zeros((3, 127), F), np.zeros((2, 128), F),
                np.zeros(3 * 128, F)):
        with pytest.raises(ValueError):
            mod.SetFeatures(keypoints, bad)
        with pytest.raises(ValueError):
            mod.SetFocusedFeatures((0, 0, 10, 10), 1.0, keypoints, bad)
    assert len(api.calls) == 1
    mod.SetFeatures(keypoints, np.zeros((3, 128), F))
    mod.SetFeatures(np.zeros((0, 2), F), np.zeros((0, 128), F))
    assert [name for name, _ in api.calls[1:]] == ["texture_modality_set_features"] * 2
    with pytest.raises(ValueError):
        util.host.TextureModality(api, Handle, Handle, Handle, descriptor_norm="l1")
