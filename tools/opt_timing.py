"""Developer tool: the OPT evaluator's device paths (csrc/m3t_opt.hip) in numbers.

    python tools/opt_timing.py [--reps 7] [--frames 60] [--no-cpu] [--no-diameter] [--no-loops]

1. m3t_hip_vertices_diameter: device time of its launches (event pairs, set_kernel_timing(1)) and the whole call's
   host time (padding, upload, launches, read-back) at 1 000, 2^14, 2^16 and 2^18 vertices; pairs per second and the
   share of the packed f32 rate without fma (half of the 157.3 Tflop/s vector peak: one flop per lane and operation),
   counting the kernel's 8 flops per formed pair (the maximum rides on v_max3_f32 beside them); the time a 1 << 20 call
   would take at the 2^18 rate, whole and per launch.  Beside it the reference's loop (opt_evaluator.cpp:580-600: all
   V^2 pairs, OpenMP) in the same arithmetic on the CPU, tools/diameter_cpu.cpp at OMP_NUM_THREADS (16) threads; the
   bits of both results must agree.
2. Whole-loop time per frame of the evaluator's loop for 24 Region + Depth bodies x 1 000 vertices and for 6 bodies x
   2^16 vertices: judged on the host (evaluate_opt_sequences), judged on the device by the ADD + ADD-S path (the bodies
   unmarked), judged on the device ADD-only (set_add_only); the two device-judged legs are one loop and differ in the
   marks alone, their judges are made before the clock starts.  Frames staged in device-side rings and visited back and
   forth; host clock around the whole loop, its final read included, divided by the frames; the legs alternate in one
   process after a warm-up each; median [min .. max].  Asserted: ADD-only is not slower than the unmarked path beyond
   the run-to-run spread of these very runs (it does a strict subset of that work).
3. The tracking step's own device time per frame (event pairs around its launches) with no judge, with the unmarked
   judge and with the ADD-only judge behind every step; asserted: not slower with the ADD-only judge than with the
   unmarked one beyond the spread (the unmarked judge's kernels and the step's are the parent commit's, byte for byte:
   tools/device_code_id.sh --kernels)."""
import argparse
import ctypes as C
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
pkg = importlib.import_module("3dobjecttracking_amd")
import bench_inputs  # noqa: E402

ev = pkg.evaluation
F = np.float32
PACKED_F32_NO_FMA = 157.3e12 / 2.0


def summary(values, unit="us"):
    return "%11.1f %s  [%11.1f .. %11.1f]  n=%d" % (statistics.median(values), unit, min(values), max(values), len(values))


def kernel_ms(api, which):
    ms, launches = (C.c_float * 2)(), (C.c_int * 2)()
    api.call("get_kernel_timing", ms, launches)
    return ms[which], launches[which]


def cpu_diameter(vertices):
    """(seconds, diameter) of tools/diameter_cpu.cpp on `vertices`"""
    binary = os.path.join(ROOT, "tools", "bin", "diameter_cpu")
    if not os.path.exists(binary):
        os.makedirs(os.path.dirname(binary), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-ffp-contract=off", "-o", binary,
                               os.path.join(ROOT, "tools", "diameter_cpu.cpp")])
    with tempfile.NamedTemporaryFile(suffix=".f32") as f:
        vertices.tofile(f)
        f.flush()
        seconds, bits = subprocess.check_output([binary, f.name, str(len(vertices))]).split()
    return float(seconds), np.asarray([int(bits)], np.uint32).view(F)[0]


def diameter_timings(reps, with_cpu):
    api = pkg.open_context(0)
    tracker = pkg.host.Tracker(api)
    rng = np.random.default_rng(5)
    tile = 1024
    print("m3t_hip_vertices_diameter")
    rate = None
    for n in (1000, 1 << 14, 1 << 16, 1 << 18):
        v = rng.uniform(-0.07, 0.07, (n, 3)).astype(F)
        got = tracker.VerticesDiameter(v)  # warm-up
        device, whole = [], []
        for _ in range(reps):
            api.call("set_kernel_timing", 1)
            t0 = time.perf_counter()
            again = tracker.VerticesDiameter(v)
            whole.append((time.perf_counter() - t0) * 1e6)
            device.append(kernel_ms(api, 1)[0] * 1e3)
            assert again.tobytes() == got.tobytes()
        api.call("set_kernel_timing", 0)
        tiles = -(-n // tile)
        formed = tiles * (tiles + 1) // 2 * tile * tile  # the pairs the launch forms, padding included
        rate = formed / (statistics.median(device) * 1e-6)
        print("  n = %7d  device %s   whole call %s" % (n, summary(device), summary(whole)))
        print("               %.3g formed pairs/s, %.1f %% of the packed f32 rate without fma (8 flops per pair)" %
              (rate, 100.0 * rate * 8.0 / PACKED_F32_NO_FMA))
        if with_cpu:
            seconds, cpu = cpu_diameter(v)
            assert cpu.tobytes() == got.tobytes(), (cpu, got)
            print("               CPU, all V^2 pairs, %s threads: %11.1f us (x %.0f)" %
                  (os.environ.get("OMP_NUM_THREADS", "all"), seconds * 1e6, seconds * 1e6 / statistics.median(device)))
        sys.stdout.flush()
    tiles = (1 << 20) // tile
    whole = tiles * (tiles + 1) // 2 * tile * tile / rate
    first = sum(tiles - r for r in range(256)) * tile * tile / rate
    print("  1 << 20 vertices at the 2^18 rate: %.0f ms in all, %.0f ms for the longest of its four launches" %
          (whole * 1e3, first * 1e3))
    api.close()


def back_and_forth(n_staged, n):
    period = list(range(n_staged)) + list(range(n_staged - 2, 0, -1))
    return [period[k % len(period)] for k in range(n)]


class Loop:
    def __init__(self, inputs, n_vertices, n_frames):
        self.inputs, self.n_frames = inputs, n_frames
        self.inst = bench_inputs.Instance(pkg.open_context(0), inputs, use_region=True, use_depth=True)
        self.api, self.tracker = self.inst.api, self.inst.tracker
        rng = np.random.default_rng(6)
        self.evaluations = []
        for i in range(inputs.n_objects):
            vertices = rng.uniform(-0.05, 0.05, (n_vertices, 3)).astype(F)
            offset = ev.opt_geometry2body_pose(ev.OPT_BODY_NAMES[i % 6])
            self.evaluations.append(ev.OPTBodyEvaluation(vertices, offset, 0.12))
        bench_inputs.stage_frames(self.api, self.inst, inputs, inputs.n_frames)
        self.order = back_and_forth(inputs.n_frames, n_frames + 1)
        self.gt = [[np.asarray([inputs.gt[i][k] for k in self.order], F)] for i in range(inputs.n_objects)]
        self.judges = {}

    def load(self, s, q, k):
        if s == 0:
            self.tracker.select_slot(self.order[k])

    def judge_of(self, variant):
        """the judge of a device-judged leg, made once outside the timed loops (its calls wait for the stream)"""
        if variant not in self.judges:
            judge = self.tracker.CreateJudge(self.inst.bodies, self.n_frames)
            for s, evaluation in enumerate(self.evaluations):
                judge.set_vertices(s, evaluation.vertices)
                if variant == "device ADD-only":
                    judge.set_add_only(s, evaluation.geometry2body)
            self.judges[variant] = judge
        return self.judges[variant]

    def run(self, variant, timing=False):
        """one loop over n_frames frames; returns (us per frame, ADD of the last frame per body, the step's device
        time per frame).  The device-judged legs and the leg without a judge are one loop -- the evaluator's, without
        its bookkeeping of sequences -- and differ in the judge alone."""
        judge = self.judge_of(variant) if variant.startswith("device") else None
        if judge is not None:
            judge.clear()
        if timing:
            self.api.call("set_kernel_timing", 1)
        t0 = time.perf_counter()
        if variant == "host":
            results = ev.evaluate_opt_sequences(self.tracker, self.inst.bodies, self.evaluations, self.gt, self.load)
            last = [r[0][-1]["add_error"] for r in results]
        else:
            for body, gt in zip(self.inst.bodies, self.gt):
                body.set_body2world_pose(gt[0][0])
            self.load(0, 0, 0)
            assert self.tracker.StartModalities(0)
            for i in range(self.n_frames):
                self.load(0, 0, i + 1)
                assert self.tracker.ExecuteTrackingStep(i)
                if judge is not None:
                    judge.judge([gt[0][i + 1] for gt in self.gt], -1)
            if judge is not None:
                last = [float(r["add_error"]) for r in judge.read(0, self.n_frames)[-1]]
            else:
                assert self.tracker.Sync()
                last = None
        us = (time.perf_counter() - t0) * 1e6 / self.n_frames
        step = kernel_ms(self.api, 0)[0] * 1e3 / self.n_frames if timing else None
        if timing:
            self.api.call("set_kernel_timing", 0)
        return us, last, step


def loop_timings(title, inputs, n_vertices, reps, n_frames):
    loop = Loop(inputs, n_vertices, n_frames)
    variants = ("host", "device ADD + ADD-S", "device ADD-only")
    last = {v: loop.run(v)[1] for v in variants}  # warm-up of each
    whole = ev.evaluate_opt_sequences(loop.tracker, loop.inst.bodies, loop.evaluations, loop.gt, loop.load,
                                      judge_on_device=True)  # the evaluator's own device-judged loop: the same numbers
    assert [r[0][-1]["add_error"] for r in whole] == last["device ADD-only"]
    # (the unmarked leg forms another number: ADD without the geometry-to-body pose, and ADD-S beside it)
    assert np.allclose(last["device ADD-only"], last["host"], rtol=2e-5, atol=1e-7), "ADD differs between the legs"
    assert np.all(np.isfinite(last["device ADD + ADD-S"]))
    times = {v: [] for v in variants}
    for _ in range(reps):
        for v in variants:
            times[v].append(loop.run(v)[0])
    print("%s, %d frames per loop" % (title, n_frames))
    for v in variants:
        print("  whole loop per frame, %-20s %s" % (v, summary(times[v])))
    spread = max(max(times[v]) - min(times[v]) for v in variants[1:])
    print("  run-to-run spread of the device-judged legs %.1f us" % spread)
    step = {v: [] for v in ("no judge",) + variants[1:]}
    for _ in range(max(3, reps // 2)):
        for v in step:
            step[v].append(loop.run(v, timing=True)[2])
    for v in step:
        print("  tracking step, device time per frame, %-20s %s" % (v, summary(step[v])))
    step_spread = max(max(x) - min(x) for x in step.values())
    print("  run-to-run spread of these runs %.1f us" % step_spread)
    sys.stdout.flush()
    assert statistics.median(times["device ADD-only"]) <= statistics.median(times["device ADD + ADD-S"]) + spread, \
        "ADD-only judging is slower than the ADD + ADD-S path"
    assert statistics.median(step["device ADD-only"]) <= statistics.median(step["device ADD + ADD-S"]) + step_spread, \
        "the tracking step is slower with an ADD-only judge behind it than with the ADD + ADD-S judge"
    loop.api.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=7)
    parser.add_argument("--frames", type=int, default=60)
    parser.add_argument("--no-cpu", action="store_true")
    parser.add_argument("--no-loops", action="store_true")
    parser.add_argument("--no-diameter", action="store_true")
    args = parser.parse_args()
    if not args.no_diameter:
        diameter_timings(args.reps, not args.no_cpu)
    if not args.no_loops:
        base = bench_inputs.Inputs(6, 3, n_divides=2, with_depth=True)
        loop_timings("24 Region + Depth bodies x 1 000 vertices", bench_inputs.replicate(base, 24), 1000, args.reps,
                     args.frames)
        loop_timings("6 Region + Depth bodies x 2^16 vertices", base, 1 << 16, args.reps, max(10, args.frames // 3))
