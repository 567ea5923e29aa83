"""Developer tool: what putting ONE kinematic structure of a batch on new poses costs per frame.

    python tools/reset_structures_timing.py [--structures 4] [--frames 60] [--out profiles/r09_reset_structures.txt]

A batch of 8-body chains (bench_chain.chain_inputs / Chain: bench.py --config chain8's structure, n_divides = 2 models)
in one context.  The timed loop is the whole frame loop of an evaluator of independent structure sequences in which
one structure starts a new sequence every frame: [reset one structure, round robin] -> execute_tracking_step, a stream
synchronise once per frame behind the step (what a host-judged evaluator does anyway).  Two ways to reset:

  reset_structures   Tracker.ResetStructures([optimizer], poses): enqueued, nothing read back, no table uploaded
  host               what the library offered before: link_get_joint_poses of the structure's links (PullLinks: a
                     stream synchronise and every link copied back), joint2parent on the host, body_set_body2world_pose
                     + link_set_joint_poses (tables dirty: every table uploaded again), start_modalities (EVERY
                     structure's histograms restarted -- the neighbours' state is lost, which the timing ignores)

Host clock around the whole loop of --frames frames, ending in the synchronise; both ways warmed up, then alternating
in one process, five windows each; the figure is the median window divided by its frames.  The step alone (no reset)
is timed the same way: its time must not depend on this feature."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("3dobjecttracking_amd")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--structures", type=int, default=4)
    parser.add_argument("--frames", type=int, default=60)
    parser.add_argument("--windows", type=int, default=5)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    import bench_chain
    import scenes
    host, syn, ev = pkg.host, pkg.synthetic, pkg.evaluation
    n_bodies = 8
    inputs, joints, gt = bench_chain.chain_inputs(scenes, syn, n_bodies, 3, 2)
    api = pkg.open_context(0)
    chains = [bench_chain.Chain(api, host, syn, inputs, joints,
                                syn.perturb_pose(gt[0][0][0], np.random.default_rng(5 + s), rot_deg=0.5, trans=0.001),
                                gt[0][1] + 0.01, range(n_bodies)) for s in range(args.structures)]
    tracker = chains[0].tracker
    targets = [np.asarray(p, np.float32) for p in gt[1][0]]

    def upload(k):
        for ch in chains:
            ch.upload(inputs, k)

    def reset_device(ch):
        assert tracker.ResetStructures([ch.opt], targets, 0, 0)

    def reset_host(ch):
        body2joint = [link.body2joint_pose() for link in ch.links]  # (PullLinks: synchronise + copy)
        for j, (body, link) in enumerate(zip(ch.bodies, ch.links)):
            body.set_body2world_pose(targets[j])
            if j:
                link.set_joint2parent_pose(ev._mul_pose_f32(ev._mul_pose_f32(ev._inverse_pose_f32(targets[j - 1]), targets[j]),
                                                            ev._inverse_pose_f32(body2joint[j])))
        assert tracker.StartModalities(0)

    def window(reset):
        t0 = time.perf_counter()
        for f in range(args.frames):
            if reset:
                reset(chains[f % len(chains)])
            assert tracker.ExecuteTrackingStep(f)
            assert tracker.Sync()
        return (time.perf_counter() - t0) * 1e6 / args.frames

    upload(0)
    assert tracker.StartModalities(0)
    upload(1)
    # the two resets give the same joints (the device's arithmetic restated on the host)
    reset_device(chains[0])
    a = [link.joint2parent_pose() for link in chains[0].links[1:]]
    reset_host(chains[0])
    b = [link.joint2parent_pose() for link in chains[0].links[1:]]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for reset in (reset_device, reset_host, None):  # warm-up of all three loops
        window(reset)
    times = {"reset_structures": [], "host": [], "step alone": []}
    for _ in range(args.windows):
        times["reset_structures"].append(window(reset_device))
        times["host"].append(window(reset_host))
        times["step alone"].append(window(None))
    lines = ["reset_structures_timing: %d structures x %d bodies, one structure reset per frame, %d frames per window, "
             "%d windows each, alternating" % (len(chains), n_bodies, args.frames, args.windows)]
    med = {}
    for key, values in times.items():
        med[key] = statistics.median(values)
        lines.append("%-18s %9.1f us per frame  [%9.1f .. %9.1f]" % (key, med[key], min(values), max(values)))
    lines.append("host / reset_structures, whole loop per frame: %.2f" % (med["host"] / med["reset_structures"]))
    lines.append("cost of the reset itself (loop - step alone): reset_structures %.1f us, host %.1f us" %
                 (med["reset_structures"] - med["step alone"], med["host"] - med["step alone"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
