"""Developer tool: the L2 matcher of the texture modality (csrc/m3t_texture_l2.hip) in numbers.

    python tools/texture_l2_timing.py [--reps 7] [--no-cpu]

m3t_hip_calculate_correspondences(corr_iteration 0) of 1, 8 and 64 L2 texture modalities in one context at 300 keyframe
points x 300 features x 128 floats, and of 1 and 8 at 4096 x 4096 x 128 (SIFT's width; integer-valued descriptors);
host clock around call + sync, median [min .. max].  The call launches texture_match_l2_kernel on a (modality, ring slot
x query tile) grid and texture_collect_l2_kernel behind it.  Beside it the same match as a plain C++ loop over
csrc/m3t_texture.h (the sequential sum, -ffp-contract=off) with OpenMP at OMP_NUM_THREADS (16) threads,
tools/texture_l2_match_cpu.cpp, for ONE modality; the number of kept queries must agree with the device's number of
data points.  A reference point for readers, no ratio is required."""
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
N_FLOATS = 128


def summary(values):
    return "%10.1f us  [%10.1f .. %10.1f]  n=%d" % (statistics.median(values), min(values), max(values), len(values))


class Body:
    def __init__(self, api, camera):
        self.body = host.Body(api, mtv.body2world())
        tv, tf = pkg.config.load_obj(os.path.join(GOLDEN, "_body", "triangle.obj"))
        self.body.set_geometry(tv, tf, np.asarray(mtv.GEOMETRY2BODY, F), body_id=150, region_id=150)
        geometry = host.RendererGeometry(api)
        geometry.AddBody(self.body)
        self.renderer = host.FocusedSilhouetteRenderer(api, geometry, camera, id_type=0)
        self.renderer.AddReferencedBody(self.body)
        self.texture = host.TextureModality(api, self.body, camera, self.renderer, descriptor_norm="l2",
                                            descriptor_bytes=4 * N_FLOATS)
        host.Optimizer(api, body=self.body, modalities=[self.texture])

    def on_body(self, n, rng):
        self.renderer.StartRendering()
        _, sil, cu, cv, scale, _ = self.renderer.images()
        vs, us = np.nonzero(sil == 150)
        pick = rng.permutation(len(vs))[:n]
        return np.stack([F(cu) + us[pick].astype(F) / F(scale), F(cv) + vs[pick].astype(F) / F(scale)], 1).astype(F)


def features(rng, n_query, n_train):
    train = rng.integers(0, 256, (n_train, N_FLOATS)).astype(F)
    queries = rng.integers(0, 256, (n_query, N_FLOATS)).astype(F)
    for q in range(0, n_query, 2):  # every other query has a near twin: about half survive the ratio test
        queries[q] = train[(q * 7) % n_train]
        queries[q, 3] += F(4.0)
    return queries, train


def matcher(reps, with_cpu):
    print("L2 matcher: calculate_correspondences(0, 0) + sync")
    for n_query, n_train, counts in ((300, 300, (1, 8, 64)), (4096, 4096, (1, 8))):
        rng = np.random.default_rng(n_query)
        queries, train = features(rng, n_query, n_train)
        for n_modalities in counts:
            api = pkg.open_context(0)
            camera = host.ColorCamera(api, **mtv.COLOR_INTRINSICS)
            tracker = host.Tracker(api)
            bodies = [Body(api, camera) for _ in range(n_modalities)]
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
            print("  %4d x %4d x %3d floats, %2d modalities: %s   kept %d per modality" %
                  (n_query, n_train, N_FLOATS, n_modalities, summary(times), kept))
        if with_cpu:
            binary = os.path.join(ROOT, "tools", "bin", "texture_l2_match_cpu")
            os.makedirs(os.path.dirname(binary), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-o", binary,
                                   os.path.join(ROOT, "tools", "texture_l2_match_cpu.cpp")])
            with tempfile.TemporaryDirectory() as d:
                queries.tofile(os.path.join(d, "q"))
                train.tofile(os.path.join(d, "t"))
                seconds, cpu_kept = subprocess.check_output(
                    [binary, os.path.join(d, "q"), os.path.join(d, "t"), str(n_query), str(n_train), str(N_FLOATS),
                     str(reps)]).split()
            assert int(cpu_kept) == kept, (int(cpu_kept), kept)
            print("  %4d x %4d x %3d floats, C++ loop with OpenMP (%s threads), 1 modality: %10.1f us (best of %d)   kept %d"
                  % (n_query, n_train, N_FLOATS, os.environ.get("OMP_NUM_THREADS", "all"), float(seconds) * 1e6, reps,
                     int(cpu_kept)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    matcher(args.reps, not args.no_cpu)
