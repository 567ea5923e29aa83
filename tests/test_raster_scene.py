"""The focused renderers' device path restated on the host with the device's own arithmetic (csrc/m3t_raster.h: set-up,
survivor list, row scan in the pieces the kernels cut it into, minimum of the packed words) against the ORACLE's
focused renderer on the scene of tools/raster_probe.py (prism + bottle of 20 950 triangles, both cameras): depth and
silhouette images equal, pixel for pixel."""
import ctypes as C
import os
import subprocess

import numpy as np

import golden_scene as gs
import render_edges
import util
from util import host


def test_host_restatement_of_the_device_rasteriser_equals_the_oracle(tmp_path):
    so = str(tmp_path / "libraster_stats.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", so,
                    os.path.join(util.ROOT, "tests", "cpp", "raster_stats.cpp")], check=True)
    lib = C.CDLL(so)
    api = util.open_oracle()
    f = gs.TrackerFixture(api, measure_occlusions=False, region_params=dict(n_unoccluded_iterations=0),
                          depth_params=dict(n_unoccluded_iterations=0))
    geometry, schauma = gs.fixture_renderer_geometry(api, f.body)
    S = 200
    load_obj = util.pkg.config.load_obj
    bodies = []
    for order, (name, body2world, g2b, body_id) in enumerate((
            ("triangle", f.body.body2world_pose(), np.asarray(gs.mtv.GEOMETRY2BODY, np.float32), 150),
            ("schauma", np.linalg.inv(gs.SCHAUMA_WORLD2BODY.astype(np.float64)).astype(np.float32),
             np.asarray(gs.SCHAUMA_GEOMETRY2BODY, np.float32), 50))):
        v, t = load_obj(os.path.join(util.GOLDEN, "_body/%s.obj" % name))
        bodies.append((order, np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32),
                       np.asarray(body2world, np.float32), g2b.reshape(4, 4), body_id))
    f32 = np.float32
    for camera, k, w2c in ((f.color_camera, gs.mtv.COLOR_INTRINSICS, np.eye(4, dtype=f32)),
                           (f.depth_camera, gs.mtv.DEPTH_INTRINSICS, np.linalg.inv(gs.mtv.DEPTH_CAMERA2WORLD).astype(f32))):
        r = host.FocusedSilhouetteRenderer(api, geometry, camera, id_type=0, image_size=S)
        r.AddReferencedBody(f.body)
        r.StartRendering()
        depth, sil, corner_u, corner_v, scale, n_visible = r.images()
        assert n_visible == 1
        # FocusedRenderer::CalculateProjectionMatrix renderer.cpp:348-405 in float32, operation for operation like
        # focused_projection (render_edges.focused_projection; the crop's side d itself is needed: S / scale does not
        # give it back to the last bit)
        tv, _ = load_obj(os.path.join(util.GOLDEN, "_body/triangle.obj"))
        diameter = render_edges.maximum_body_diameter(tv, np.asarray(gs.mtv.GEOMETRY2BODY, f32).reshape(4, 4))
        pr = render_edges.focused_projection(k, w2c, [(f.body.body2world_pose(), diameter)], S, 0.02, 10.0)
        assert pr["n_visible"] == 1
        assert pr["corner_u"] == f32(corner_u) and pr["corner_v"] == f32(corner_v) and pr["scale"] == f32(scale)  # the oracle's crop
        P, mul44 = pr["P"], render_edges.mul44
        packed = np.full(S * S, 0xFFFFFFFF, np.uint32)
        for order, v, t, b2w, g2b, body_id in bodies:
            trans = mul44(P, mul44(w2c, mul44(b2w, g2b.astype(f32))))
            low = (order << 8) | body_id
            lib.raster_body(np.ascontiguousarray(trans.T).ctypes.data_as(C.POINTER(C.c_float)),
                            v.ctypes.data_as(C.POINTER(C.c_float)), t.ctypes.data_as(C.POINTER(C.c_int)), len(t), 1, S,
                            C.c_uint(low), packed.ctypes.data_as(C.POINTER(C.c_uint)))
        got_depth = np.where(packed == 0xFFFFFFFF, 65535, packed >> 16).astype(np.uint16).reshape(S, S)
        got_sil = np.where(packed == 0xFFFFFFFF, 0, packed & 0xFF).astype(np.uint8).reshape(S, S)
        assert np.array_equal(got_depth, depth)
        assert np.array_equal(got_sil, sil)
        assert (depth != 65535).sum() > 10000
