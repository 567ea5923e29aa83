"""Developer tool: the two forms of the texture modality's Hamming match (the developer override M3T_HIP_TEXTURE_MATCH) in numbers, beside
an older build of the library.

    python tools/texture_match_timing.py [--reps 9] [--parent PATH/libm3t_hip.so] [--no-step]

1. calculate_correspondences(0, 0) + sync, warmed, host clock, median [min .. max]: this build forced to ONE_WORKGROUP
   and to TILED and, with --parent, that library twice (two contexts of its own: their difference is the run-to-run
   spread every other difference has to be read against).  The contexts take turns call by call, so that a drift of
   the machine reaches all of them alike.  Sizes: 300 x 300 x 32 bytes (the evaluators': 300 features, one keyframe),
   500 x 500 x 32 and 4096 x 4096 x 64, each with 1, 8 and 64 modalities, the two small ones also with 3 keyframes.
   The number of data points must agree between all contexts.
2. ExecuteTrackingStep + sync of a Region + Texture body (300 x 300 x 32), the same contexts in turn.
Kernel times: run the tool under `rocprofv3 --kernel-trace --stats -- python tools/texture_match_timing.py --no-step`."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("3dobjecttracking_amd")
import texture_timing as tt  # noqa: E402  (the bodies and the features of the older tool)

host = pkg.host
F = np.float32


def open_contexts(parent):
    """[(label, api)]: the parent twice (if given), this build in both forms"""
    out = []
    if parent:
        out.append(("parent a", pkg._capi.CApi(parent, "m3t_hip_", 0)))
    for label, mode in (("one workgroup", "one"), ("tiled", "tiled")):
        os.environ["M3T_HIP_TEXTURE_MATCH"] = mode  # (a context looks at it when it is made)
        out.append((label, pkg.open_context(0)))
        del os.environ["M3T_HIP_TEXTURE_MATCH"]
    if parent:
        out.append(("parent b", pkg._capi.CApi(parent, "m3t_hip_", 0)))
    return out


def line(label, values, parent_median=None):
    text = "    %-14s %10.1f us  [%10.1f .. %10.1f]  n=%d" % (label, statistics.median(values), min(values), max(values),
                                                               len(values))
    if parent_median:
        text += "   %+6.1f %% of parent a" % (100.0 * (statistics.median(values) - parent_median) / parent_median)
    return text


def matcher(reps, parent):
    print("matcher: calculate_correspondences(0, 0) + sync")
    for n_query, n_train, n_bytes, keyframes in ((300, 300, 32, 1), (300, 300, 32, 3), (500, 500, 32, 1),
                                                  (500, 500, 32, 3), (4096, 4096, 64, 1)):
        for n_modalities in (1, 8, 64):
            rng = np.random.default_rng(n_bytes)
            queries, train = tt.features(rng, n_query, n_train, n_bytes)
            xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
            runs, keypoints = [], None
            for label, api in open_contexts(parent):
                camera = host.ColorCamera(api, **tt.mtv.COLOR_INTRINSICS)
                tracker = host.Tracker(api)
                bodies = [tt.Body(api, camera, n_bytes, n_keyframes=keyframes) for _ in range(n_modalities)]
                if keypoints is None:
                    keypoints = bodies[0].on_body(n_query, np.random.default_rng(7))
                runs.append((label, api, tracker, bodies))
            for label, api, tracker, bodies in runs:
                for _ in range(keyframes):
                    for b in bodies:
                        b.texture.SetFeatures(keypoints, queries)
                    assert tracker.StartModalities(0)
                for b in bodies:
                    b.texture.SetFeatures(xy, train)
                for _ in range(3):  # warm
                    assert tracker.CalculateCorrespondences(0, 0) and tracker.Sync()
            times = {label: [] for label, _, _, _ in runs}
            for _ in range(reps):
                for label, api, tracker, bodies in runs:
                    t0 = time.perf_counter()
                    tracker.CalculateCorrespondences(0, 0)
                    tracker.Sync()
                    times[label].append((time.perf_counter() - t0) * 1e6)
            kept = {len(bodies[-1].texture.points()) for _, _, _, bodies in runs}
            assert len(kept) == 1, kept
            print("  %4d x %4d x %2d bytes, %d keyframe(s), %2d modalities, %d data points per modality" %
                  (n_query, n_train, n_bytes, keyframes, n_modalities, kept.pop()))
            base = statistics.median(times["parent a"]) if parent else None
            for label, _, _, _ in runs:
                print(line(label, times[label], base if label != "parent a" else None))
            for _, api, _, _ in runs:
                api.close()


def whole_step(reps, parent):
    print("whole step of a Region + Texture body (300 x 300 x 32), one launch per sub-step: ExecuteTrackingStep + sync")
    from PIL import Image
    image = np.ascontiguousarray(np.array(Image.open(os.path.join(tt.GOLDEN, "_sequence", "color_camera_image_200.png")))[..., ::-1])
    runs = []
    for label, api in open_contexts(parent):
        camera = host.ColorCamera(api, **tt.mtv.COLOR_INTRINSICS)
        camera.UpdateImage(image)
        tracker = host.Tracker(api)
        rng = np.random.default_rng(1)
        b = tt.Body(api, camera, 32, with_region=True)
        queries, train = tt.features(rng, 300, 300, 32)
        keypoints = b.on_body(300, rng)
        b.texture.SetFeatures(keypoints, queries)
        assert tracker.StartModalities(0)
        order = rng.permutation(300)
        b.texture.SetFeatures((keypoints[order] + rng.uniform(-2, 2, (300, 2))).astype(F), queries[order])
        for k in range(3):
            assert tracker.ExecuteTrackingStep(k) and tracker.Sync()
        runs.append((label, tracker, b))
    times = {label: [] for label, _, _ in runs}
    for k in range(reps):
        for label, tracker, _ in runs:
            t0 = time.perf_counter()
            assert tracker.ExecuteTrackingStep(3 + k)
            tracker.Sync()
            times[label].append((time.perf_counter() - t0) * 1e6)
    poses = {b.body.body2world_pose().tobytes() for _, _, b in runs}
    assert len(poses) == 1, "the contexts disagree on the pose"
    base = statistics.median(times["parent a"]) if parent else None
    for label, _, _ in runs:
        print(line(label, times[label], base if label != "parent a" else None))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent", default=None, help="an older libm3t_hip.so to time beside this build")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    matcher(args.reps, args.parent)
    if not args.no_step:
        whole_step(args.reps, args.parent)
