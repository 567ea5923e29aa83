"""Developer tool: what a per-body reset costs on the device.

    python tools/reset_bodies_timing.py [--reps 40] [--dataset-reps 3]

1. m3t_hip_reset_bodies for 1, 8 and 64 of 64 RBOT-shape bodies (Inputs(64, 3, n_divides=4, n_models=18), poses
   device-authoritative after two tracking steps) against the way to do the same without it: body_set_body2world_pose
   x k + start_modalities (which restarts all 64).  Host clock from before the call(s) to the end of a stream
   synchronise behind them, the two ways alternating in one process; for reset_bodies also the time until the call
   returns (the enqueue).  Median [min .. max] over the repetitions, after warm-up calls of both.
2. evaluate_rbot_dataset over the synthetic four-body dataset of tests/selective_reset.py (8 frames) at batch = 1 and
   batch = 4: wall time of the whole call (contexts, model upload, PNG decoding, tracking), alternating."""
import argparse
import importlib
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("3dobjecttracking_amd")


def summary(values):
    return "%8.1f us  [%8.1f .. %8.1f]  n=%d" % (statistics.median(values), min(values), max(values), len(values))


def reset_timings(reps):
    import bench_inputs
    inputs = bench_inputs.Inputs(64, 3, n_divides=4, n_models=18)
    api = pkg.open_context(0)
    inst = bench_inputs.Instance(api, inputs)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    for k in (1, 2):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
    assert inst.tracker.Sync()
    targets = [np.asarray(inputs.gt[i][2], np.float32) for i in range(64)]

    def selective(ids):
        t0 = time.perf_counter()
        assert inst.tracker.ResetBodies([inst.bodies[i] for i in ids], [targets[i] for i in ids], 0)
        t1 = time.perf_counter()
        assert inst.tracker.Sync()
        return (time.perf_counter() - t0) * 1e6, (t1 - t0) * 1e6

    def batch_wide(ids):
        t0 = time.perf_counter()
        for i in ids:
            inst.bodies[i].set_body2world_pose(targets[i])
        assert inst.tracker.StartModalities(0)
        assert inst.tracker.Sync()
        return (time.perf_counter() - t0) * 1e6

    for n in (1, 8, 64):
        ids = list(range(0, 64, 64 // n))[:n]
        for _ in range(3):  # warm-up of both
            selective(ids)
            batch_wide(ids)
            inst.upload_frame(2)
            assert inst.tracker.ExecuteTrackingStep(2) and inst.tracker.Sync()  # poses device-authoritative again
        a, enqueue, b = [], [], []
        for _ in range(reps):
            total, returned = selective(ids)
            a.append(total)
            enqueue.append(returned)
            assert inst.tracker.ExecuteTrackingStep(2) and inst.tracker.Sync()
            b.append(batch_wide(ids))
            assert inst.tracker.ExecuteTrackingStep(2) and inst.tracker.Sync()
        print("%2d of 64 bodies  reset_bodies, call + sync          %s" % (n, summary(a)))
        print("                 reset_bodies, until the call returns %s" % summary(enqueue))
        print("                 set_pose x %-2d + start_modalities + sync %s" % (n, summary(b)))
        sys.stdout.flush()


def dataset_timings(reps):
    import selective_reset as sr
    ev = pkg.evaluation
    with tempfile.TemporaryDirectory() as tmp:
        from pathlib import Path
        dataset, external, names, model_parameters = sr.write_rbot_dataset(Path(tmp), 8)
        times = {1: [], 4: []}
        results = {}
        for rep in range(reps + 1):  # the first round warms up (code objects, file cache)
            for batch in (1, 4):
                t0 = time.perf_counter()
                results[batch] = ev.evaluate_rbot_dataset(lambda: pkg.open_context(0), str(dataset), str(external), names,
                                                          ["a_regular"], n_frames=8, model_parameters=model_parameters,
                                                          batch=batch)
                if rep:
                    times[batch].append((time.perf_counter() - t0) * 1e3)
        for key in results[1][0]:
            for field in ("translation_error", "rotation_error", "tracking_success"):
                assert results[1][0][key][field] == results[4][0][key][field], (key, field)
        for batch in (1, 4):
            print("evaluate_rbot_dataset, 4 runs x 8 frames, batch = %d: %8.1f ms  [%8.1f .. %8.1f]  n=%d (same results)" %
                  (batch, statistics.median(times[batch]), min(times[batch]), max(times[batch]), len(times[batch])))
            steps = [results[batch][0][key]["complete_cycle"] for key in results[batch][0]]
            print("    mean step + sync per context (complete_cycle): %s us" % ", ".join("%.0f" % s for s in steps))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=40)
    parser.add_argument("--dataset-reps", type=int, default=3)
    args = parser.parse_args()
    reset_timings(args.reps)
    dataset_timings(args.dataset_reps)
