"""Developer tool: what the device-decided resets through renderers (m3t_hip_judge_set_reset_renderers,
m3t_hip_judge_set_reset_target) do to the RBOT evaluator's loop with modelled occlusions.

    python tools/occlusion_judge_timing.py [--reps 5] [--frames 100] [--runs 1,16,32]

Whole-loop time per frame of evaluation.evaluate_rbot_occlusion_sequences for N runs in one context (2 N bodies with
the octahedron mesh, N FocusedBasicDepthRenderers of 200 pixels, ModelOcclusions on both region modalities of a run),
in three configurations:
  host      judged on the host: Sync, a pose read per body, two Tracker.ResetBodies calls per frame
  device    judged on the device: two judges behind the step, both with set_reset_renderers
  always    judged on the device with M3T_HIP_JUDGE_RENDER_ALWAYS set (a developer switch the library reads once per
            context): every renderer pair a judge lists is rendered at every call, lost reader or not
and for two sequences:
  reference   judge_occluder_on_own_pose=False and poses_second 10.4 cm from poses_first: the MAIN pose is judged against
              poses_second (rbot_evaluator.cpp:204), so every occluder is lost and reset at every frame and the second
              judge renders all N pairs -- the skip is never taken.  This is what the reference's column costs.
  never lost  judge_occluder_on_own_pose=True and poses_second = poses_first: no body is ever lost (counted on the
              host-judged leg: no ResetBodies call inside the loop; printed if it is otherwise), so a device-judged
              frame renders nothing.
The occluder of a run has the main body's model and start pose (it tracks the same image, which keeps it found in the
"never lost" sequence); the frame is uploaded once and tracked again and again, so a loop times the step, the
judgements and the resets and nothing else.  Host clock around the whole evaluate call (it ends in a read of the rows)
divided by the frames; the legs alternate in one process, one warm-up call each; median [min .. max].  The warm-up
calls also say whether the three legs judged the main bodies alike (printed).
The two expectations are printed as MET / NOT MET per size:
  1. device <= host on the reference sequence;
  2. device <= always on the never-lost sequence (a frame without a loss costs no more than an unconditional render)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("3dobjecttracking_amd")
import bench_inputs  # noqa: E402

ev, host, syn = pkg.evaluation, pkg.host, pkg.synthetic
F = np.float32
OCTAHEDRON = np.array([(60, 0, 0), (-60, 0, 0), (0, 50, 0), (0, -50, 0), (0, 0, 40), (0, 0, -40)], F) * F(0.001)
FACES = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int32)
SWITCH = "M3T_HIP_JUDGE_RENDER_ALWAYS"


def summary(values):
    return "%9.1f us  [%9.1f .. %9.1f]  n=%d" % (statistics.median(values), min(values), max(values), len(values))


class Runs:
    """n runs behind one context: main body i on object i's frame, its occluder on the same model and start pose"""

    def __init__(self, inputs, n, render_always):
        self.render_always = render_always
        self.api = api = pkg.open_context(0)
        self.inputs, self.n = inputs, n
        rp = dict(syn.RBOT_REGION_PARAMS, measure_occlusions=0, n_unoccluded_iterations=0)
        tp = syn.RBOT_TRACKER
        models = [host.RegionModel(api, data_points=m[0], orientations=m[1], contour_lengths=m[2])
                  for m in inputs.region_models]
        self.mains, self.occluders, self.cams = [], [], []
        for i in range(n):
            cam = host.ColorCamera(api, **inputs.intr)
            pair = [host.Body(api, inputs.start[i]) for _ in range(2)]
            geometry = host.RendererGeometry(api)
            for body in pair:
                body.set_geometry(OCTAHEDRON, FACES)
                geometry.AddBody(body)
            renderer = host.FocusedBasicDepthRenderer(api, geometry, cam, image_size=ev.RBOT_FOCUSED_IMAGE_SIZE)
            for body in pair:
                renderer.AddReferencedBody(body)
            for body in pair:
                modality = host.RegionModality(api, body, cam, models[inputs.model_of[i]], **rp)
                modality.ModelOcclusions(renderer)
                host.Optimizer(api, body=body, modalities=[modality],
                               tikhonov_parameter_rotation=tp["tikhonov_parameter_rotation"],
                               tikhonov_parameter_translation=tp["tikhonov_parameter_translation"])
            self.mains.append(pair[0])
            self.occluders.append(pair[1])
            self.cams.append(cam)
        self.tracker = host.Tracker(api, tp["n_corr_iterations"], tp["n_update_iterations"])
        self.loop_resets = 0

    def run(self, sequence, on_device, n_frames):
        """one evaluate call; returns (us per frame, the main bodies' tracking_success per frame)"""
        inputs, n = self.inputs, self.n
        first = [np.asarray([inputs.gt[i][0]] + [inputs.gt[i][1]] * n_frames, F) for i in range(n)]
        second = [p.copy() for p in first]
        if sequence == "reference":
            for p in second:
                p[:, :3, 3] += np.asarray((0.03, 0.0, -0.1), F)

        def load_images(k):
            if k <= 1:  # afterwards the frame stays: the loop tracks it again
                for i, cam in enumerate(self.cams):
                    cam.UpdateImage(inputs.color[i][k])

        # every call starts from the same state: the first reset of a sequence renders the occluders where they are
        for i, body in enumerate(self.occluders):
            body.set_body2world_pose(inputs.start[i])
        reset_bodies, calls = self.tracker.ResetBodies, [0]

        def counted(*a, **kw):
            calls[0] += 1
            return reset_bodies(*a, **kw)

        self.tracker.ResetBodies = counted
        if self.render_always:  # (the library reads the switch at the context's first judge_bodies call)
            os.environ[SWITCH] = "1"
        try:
            t0 = time.perf_counter()
            frames, _ = ev.evaluate_rbot_occlusion_sequences(
                self.tracker, self.mains, self.occluders, first, second, load_images, n_frames,
                judge_on_device=on_device, judge_occluder_on_own_pose=sequence == "never lost")
            dt = (time.perf_counter() - t0) * 1e6 / n_frames
        finally:
            del self.tracker.ResetBodies
            os.environ.pop(SWITCH, None)
        self.loop_resets = calls[0] - 2  # (the two calls that start the sequence)
        return dt, [[f["tracking_success"] for f in fs] for fs in frames]


def measure(inputs, n, reps, n_frames):
    plain, always = Runs(inputs, n, False), Runs(inputs, n, True)
    legs = (("host", plain, False), ("device", plain, True), ("always", always, True))
    out = {}
    for sequence in ("reference", "never lost"):
        flags = {}
        for name, runs, on_device in legs:  # warm-up of every leg, and what the legs have to agree on
            flags[name] = runs.run(sequence, on_device, n_frames)[1]
            if name == "host":
                resets = runs.loop_resets
        lost = {name: sum(f == 0.0 for fs in flags[name] for f in fs) for name in flags}
        agree = flags["host"] == flags["device"] == flags["always"]
        print("%2d runs, %s sequence: frames with a main body lost %s; tracking_success %s between the legs" %
              (n, sequence, lost, "agrees" if agree else "DIFFERS"))
        if sequence == "never lost" and (resets != 0 or lost["host"] != 0):
            print("  NOTE: the never-lost sequence had %d ResetBodies calls inside the host-judged loop" % resets)
        times = {name: [] for name, _, _ in legs}
        for _ in range(reps):
            for name, runs, on_device in legs:
                times[name].append(runs.run(sequence, on_device, n_frames)[0])
        print("%2d runs (%d bodies, %d renderers), %s sequence, %d frames per loop, %d ResetBodies calls inside the "
              "host-judged loop" % (n, 2 * n, n, sequence, n_frames, resets))
        for name, _, _ in legs:
            print("  whole loop per frame, %-6s  %s" % (name, summary(times[name])))
        out[sequence] = {name: statistics.median(v) for name, v in times.items()}
        sys.stdout.flush()
    a, b = out["reference"], out["never lost"]
    print("  expectation 1 (device <= host, reference sequence):    %s  (%.1f against %.1f us, host / device %.2f)" %
          ("MET" if a["device"] <= a["host"] else "NOT MET", a["device"], a["host"], a["host"] / a["device"]))
    print("  expectation 2 (device <= always, never-lost sequence): %s  (%.1f against %.1f us)" %
          ("MET" if b["device"] <= b["always"] else "NOT MET", b["device"], b["always"]))
    print("  never-lost sequence, host / device %.2f" % (b["host"] / b["device"]))
    sys.stdout.flush()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--frames", type=int, default=100)
    parser.add_argument("--runs", default="1,16,32")
    args = parser.parse_args()
    sizes = [int(x) for x in args.runs.split(",")]
    inputs = bench_inputs.Inputs(max(sizes), 2, n_divides=2, n_models=min(max(sizes), 6))
    for n in sizes:
        measure(inputs, n, args.reps, args.frames)
