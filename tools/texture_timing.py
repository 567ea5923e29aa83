"""Developer tool: the texture modality (csrc/m3t_texture.hip) in numbers.

    python tools/texture_timing.py [--reps 7] [--no-cpu]

1. The matcher alone: m3t_hip_calculate_correspondences(corr_iteration 0) of 1, 8 and 64 texture modalities in one
   context (one workgroup each), at 300 keyframe points x 300 features x 32 bytes (ORB's defaults) and at 4096 x 4096 x
   64 bytes; host clock around call + sync, median [min .. max].  Beside it the same match as a plain C++ loop over
   csrc/m3t_texture.h with OpenMP at OMP_NUM_THREADS (16) threads, tools/texture_match_cpu.cpp, for ONE modality; the
   number of kept queries must agree with the device's number of data points.  A reference point for readers, no ratio
   is required.
2. The whole step, one launch per sub-step (set_fused_step(0)), host clock per ExecuteTrackingStep: a Region body,
   and the same body with a texture modality of 300 x 300 x 32 beside the region modality."""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
pkg = importlib.import_module("3dobjecttracking_amd")
import make_triangle_views as mtv  # noqa: E402  (the triangle fixture: pose, intrinsics, mesh placement)

host = pkg.host
F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference")


def summary(values):
    return "%10.1f us  [%10.1f .. %10.1f]  n=%d" % (statistics.median(values), min(values), max(values), len(values))


class Body:
    def __init__(self, api, camera, n_bytes, with_region=False, n_keyframes=1):
        self.body = host.Body(api, mtv.body2world())
        tv, tf = pkg.config.load_obj(os.path.join(GOLDEN, "_body", "triangle.obj"))
        self.body.set_geometry(tv, tf, np.asarray(mtv.GEOMETRY2BODY, F), body_id=150, region_id=150)
        geometry = host.RendererGeometry(api)
        geometry.AddBody(self.body)
        self.renderer = host.FocusedSilhouetteRenderer(api, geometry, camera, id_type=0)
        self.renderer.AddReferencedBody(self.body)
        self.texture = host.TextureModality(api, self.body, camera, self.renderer, descriptor_bytes=n_bytes,
                                            n_keyframes=n_keyframes)
        modalities = [self.texture]
        if with_region:
            v = np.load(os.path.join(ROOT, "tests", "golden", "triangle_views.npz"))
            model = host.RegionModel(api, data_points=v["region_points"], orientations=v["region_orientations"],
                                     contour_lengths=v["region_contour_lengths"])
            modalities = [host.RegionModality(api, self.body, camera, model), self.texture]
        host.Optimizer(api, body=self.body, modalities=modalities)

    def on_body(self, n, rng):
        self.renderer.StartRendering()
        _, sil, cu, cv, scale, _ = self.renderer.images()
        vs, us = np.nonzero(sil == 150)
        pick = rng.permutation(len(vs))[:n]
        return np.stack([F(cu) + us[pick].astype(F) / F(scale), F(cv) + vs[pick].astype(F) / F(scale)], 1).astype(F)


def features(rng, n_query, n_train, n_bytes):
    train = rng.integers(0, 256, (n_train, n_bytes), dtype=np.uint8)
    queries = rng.integers(0, 256, (n_query, n_bytes), dtype=np.uint8)
    for q in range(0, n_query, 2):  # every other query has a near twin: about half survive the ratio test
        queries[q] = train[(q * 7) % n_train]
        queries[q, 3] ^= np.uint8(4)
    return queries, train


def matcher(reps, with_cpu):
    print("matcher: calculate_correspondences(0, 0) + sync")
    for n_query, n_train, n_bytes in ((300, 300, 32), (4096, 4096, 64)):
        rng = np.random.default_rng(n_bytes)
        queries, train = features(rng, n_query, n_train, n_bytes)
        for n_modalities in (1, 8, 64):
            api = pkg.open_context(0)
            camera = host.ColorCamera(api, **mtv.COLOR_INTRINSICS)
            tracker = host.Tracker(api)
            bodies = [Body(api, camera, n_bytes) for _ in range(n_modalities)]
            keypoints = bodies[0].on_body(n_query, rng)
            for b in bodies:
                b.texture.SetFeatures(keypoints, queries)
            assert tracker.StartModalities(0)
            xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
            for b in bodies:
                b.texture.SetFeatures(xy, train)
            assert tracker.CalculateCorrespondences(0, 0) and tracker.Sync()
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                tracker.CalculateCorrespondences(0, 0)
                tracker.Sync()
                times.append((time.perf_counter() - t0) * 1e6)
            kept = len(bodies[0].texture.points())
            print("  %4d x %4d x %2d bytes, %2d modalities: %s   kept %d per modality" %
                  (n_query, n_train, n_bytes, n_modalities, summary(times), kept))
        if with_cpu:
            binary = os.path.join(ROOT, "tools", "bin", "texture_match_cpu")
            os.makedirs(os.path.dirname(binary), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-o", binary,
                                   os.path.join(ROOT, "tools", "texture_match_cpu.cpp")])
            with tempfile.TemporaryDirectory() as d:
                queries.tofile(os.path.join(d, "q"))
                train.tofile(os.path.join(d, "t"))
                seconds, cpu_kept = subprocess.check_output(
                    [binary, os.path.join(d, "q"), os.path.join(d, "t"), str(n_query), str(n_train), str(n_bytes),
                     str(reps)]).split()
            assert int(cpu_kept) == kept, (int(cpu_kept), kept)
            print("  %4d x %4d x %2d bytes, C++ loop with OpenMP (%s threads), 1 modality: %10.1f us (best of %d)   kept %d"
                  % (n_query, n_train, n_bytes, os.environ.get("OMP_NUM_THREADS", "all"), float(seconds) * 1e6, reps,
                     int(cpu_kept)))


def whole_step(reps):
    print("whole step, one launch per sub-step: ExecuteTrackingStep + sync")
    from PIL import Image
    image = np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, "_sequence", "color_camera_image_200.png")))[..., ::-1])
    for with_texture in (False, True):
        api = pkg.open_context(0)
        api.call("set_fused_step", 0)
        camera = host.ColorCamera(api, **mtv.COLOR_INTRINSICS)
        camera.UpdateImage(image)
        tracker = host.Tracker(api)
        rng = np.random.default_rng(1)
        if with_texture:
            b = Body(api, camera, 32, with_region=True)
            queries, train = features(rng, 300, 300, 32)
            keypoints = b.on_body(300, rng)
            b.texture.SetFeatures(keypoints, queries)
        else:
            body = host.Body(api, mtv.body2world())
            v = np.load(os.path.join(ROOT, "tests", "golden", "triangle_views.npz"))
            model = host.RegionModel(api, data_points=v["region_points"], orientations=v["region_orientations"],
                                     contour_lengths=v["region_contour_lengths"])
            host.Optimizer(api, body=body, modalities=[host.RegionModality(api, body, camera, model)])
        assert tracker.StartModalities(0)
        if with_texture:
            order = rng.permutation(300)
            b.texture.SetFeatures((keypoints[order] + rng.uniform(-2, 2, (300, 2))).astype(F), queries[order])
        times = []
        for k in range(reps + 2):
            t0 = time.perf_counter()
            assert tracker.ExecuteTrackingStep(k)
            tracker.Sync()
            if k >= 2:
                times.append((time.perf_counter() - t0) * 1e6)
        print("  Region%s: %s" % (" + Texture (300 x 300 x 32)" if with_texture else "                           ",
                                  summary(times)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    matcher(args.reps, not args.no_cpu)
    whole_step(args.reps)
