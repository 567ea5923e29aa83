"""Developer tool: the restart of texture modalities with the built-in detector inside the enqueued calls
(m3t_hip_reset_bodies, m3t_hip_judge_bodies; texture_*_list_kernel) in numbers.

    python tools/texture_reset_timing.py reset [--bodies 16,64] [--reps 20] [--runs 5]
    python tools/texture_reset_timing.py loop [--bodies 16] [--frames 40] [--runs 3]

Scene: that of tools/texture_detector_timing.py -- n plates in front of one 640 x 480 colour camera, each with a texture
modality of focused_image_size 200 and the built-in detector, a seeded frame of small rectangles.

reset: device time between two stream events (m3t_hip_set_kernel_timing(2): one event pair around a region, nothing
  inserted between the launches) around `reps` calls, divided by `reps`; median [min .. max] over `runs` regions after
  one region of warm-up.
    reset_bodies of 1 body among n    what a lost body costs with this build
    start_modalities of the context   all that the parent offers a context with texture bodies
loop: evaluation.evaluate_rbot_sequences on the plates, host clock around the whole call (the first StartModalities, the
  creation of the judge and its final read included) divided by the frames, the same frame shown throughout, judged on
  the host (a Sync() and a pose read per body and frame,
  Tracker.ResetBodies for the lost ones) against judge_on_device (no wait per frame, the judge restarts them).  Ground
  truth: every plate's own pose, and for plate (frame mod n) of frame `frame` that pose moved by 6 cm in x -- a body is
  lost in every frame, and usually once more in the next one, when its ground truth is back."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("3dobjecttracking_amd")
import texture_detector_timing as base  # noqa: E402

host = pkg.host
F = np.float32


def region_us(api, call, reps):
    api.call("set_kernel_timing", 2)
    for _ in range(reps):
        assert call()
    ms = np.zeros(2, np.float32)
    launches = np.zeros(2, np.int32)
    api.call("get_kernel_timing", pkg._capi.fptr(ms), pkg._capi.iptr(launches))
    api.call("set_kernel_timing", 0)
    return float(ms[0]) * 1e3 / reps


def reset(bodies, reps, runs):
    print("device time per call between two stream events, %d calls per region, %d regions after one of warm-up" %
          (reps, runs))
    for n in bodies:
        api, image, plates = base.scene(n, True)
        tracker = host.Tracker(api, 2, 2)
        assert tracker.StartModalities(0) and tracker.ExecuteTrackingStep(0) and tracker.Sync()
        lost = plates[n // 2]
        pose = lost.pose.copy()
        pose[0, 3] += F(0.002)
        one = [region_us(api, lambda: tracker.ResetBodies([lost.body], [pose], 0), reps) for _ in range(runs + 1)][1:]
        everything = [region_us(api, lambda: tracker.StartModalities(0), reps) for _ in range(runs + 1)][1:]
        print("  %2d bodies, %d features each:" % (n, len(lost.texture.features()[0])))
        print("    reset_bodies of 1 body   %s" % base.summary(one))
        print("    start_modalities         %s" % base.summary(everything))
        print("    ratio of the medians     %10.1f" % (statistics.median(everything) / statistics.median(one)))


def loop(bodies, frames, runs):
    ev = pkg.evaluation
    print("evaluate_rbot_sequences per frame (host clock), %d frames, %d runs each, alternating" % (frames, runs))
    for n in bodies:
        times = {False: [], True: []}
        success = {}
        for run in range(runs):
            for on_device in (False, True):
                api, image, plates = base.scene(n, True)
                tracker = host.Tracker(api, 2, 2)
                gt = [np.stack([p.pose] * (frames + 1)) for p in plates]
                for frame in range(1, frames + 1):
                    gt[frame % n][frame, 0, 3] += F(0.06)
                t0 = time.perf_counter()
                _, averages = ev.evaluate_rbot_sequences(tracker, [p.body for p in plates], gt, lambda k: None, frames,
                                                         judge_on_device=on_device, reset_renderers=True)
                times[on_device].append((time.perf_counter() - t0) * 1e6 / frames)
                success[on_device] = float(np.mean([a["tracking_success"] for a in averages]))
        print("  %2d bodies:" % n)
        print("    judged on the host   %s   mean tracking_success %.4f" % (base.summary(times[False]), success[False]))
        print("    judge_on_device      %s   mean tracking_success %.4f" % (base.summary(times[True]), success[True]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["reset", "loop"])
    ap.add_argument("--bodies", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--frames", type=int, default=40)
    args = ap.parse_args()
    if args.mode == "reset":
        reset([int(b) for b in (args.bodies or "16,64").split(",")], args.reps, args.runs or 5)
    else:
        loop([int(b) for b in (args.bodies or "16").split(",")], args.frames, args.runs or 3)
