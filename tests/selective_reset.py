"""The reset-on-loss loop of tests/reset_loop.py with the reset an evaluator of INDEPENDENT sequences performs
(M3T/examples/rbot_evaluator.cpp ResetBody :334-342): a lost body gets its ground-truth pose and ITS modalities are
started again; every other body of the batch goes on untouched.

The expectation never comes from the code under test: object i of a batch is expected to do what it does in a context
of its own -- the reference's one tracker per sequence -- driven through the CPU oracle, where StartModalities of a
one-body context IS ResetBody.  The ground truth with its injected offsets is the batch's (reset_loop.ground_truth:
the offset seeds depend on the object's index in the batch).

Also here: the synthetic RBOT-layout dataset of the batched evaluator tests (four bodies, one of them lost once
mid-sequence while the others track on)."""
import os

import numpy as np

import bench_inputs
import reset_loop
import scenes
import util
from util import pkg

ev = pkg.evaluation


def single_inputs(inputs, i):
    """object i of a batch as a batch of its own, with its own model only (Instance uploads every model of the inputs
    into each context)"""
    sub = bench_inputs.subset(inputs, [i])
    m = inputs.model_of[i]
    sub.region_models = [inputs.region_models[m]]
    if inputs.depth_models is not None:
        sub.depth_models = [inputs.depth_models[m]]
    sub.model_of = [0]
    return sub


def single_kw(instance_kw, i):
    kw = dict(instance_kw or {})
    if kw.get("kinds") is not None:
        kw["kinds"] = [kw["kinds"][i]]
    return kw


def lost_bodies(poses, gt_k):
    return [i for i in range(len(poses)) if ev.rbot_pose_result(poses[i], gt_k[i])[2] == 0.0]


def run_single(api, inputs, i, gt, instance_kw=None, iteration_is_frame=False, fused=None):
    """object i alone in a context: step, judge, set the pose, StartModalities (= ResetBody in a one-body context).
    Returns (pose after every step, frames with a reset, histograms or None)."""
    inst = scenes.Instance(api, single_inputs(inputs, i), **single_kw(instance_kw, i))
    if fused is not None:
        api.call("set_fused_step", fused)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    poses, resets = [], []
    for k in range(1, inputs.n_frames):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
        p = inst.poses()[0]
        poses.append(p)
        if ev.rbot_pose_result(p, gt[k][i])[2] == 0.0:
            inst.bodies[0].set_body2world_pose(gt[k][i])
            assert inst.tracker.StartModalities(k if iteration_is_frame else 0)
            resets.append(k)
    return poses, resets, [r.histograms() for r in inst.region]


def expectation(inputs, schedule, instance_kw=None, iteration_is_frame=False, open_api=None):
    """every object in an oracle context of its own, merged into the shape of reset_loop.run's result:
    (poses [frame][object], sorted (frame, object) resets, the region modalities' histograms in object order)"""
    gt = reset_loop.ground_truth(inputs, schedule)
    singles = [run_single((open_api or util.open_oracle)(), inputs, i, gt, instance_kw, iteration_is_frame)
               for i in range(inputs.n_objects)]
    poses = [np.stack([s[0][k] for s in singles]) for k in range(inputs.n_frames - 1)]
    resets = sorted((k, i) for i, s in enumerate(singles) for k in s[1])
    hist = [h for s in singles for h in s[2]]
    assert resets
    return poses, resets, hist


def run_batch(api, inputs, schedule, reset="bodies", instance_kw=None, iteration_is_frame=False, setup=None, frame=None,
              after_step=None, before_reset=None):
    """The batch loop.  reset "bodies": the lost bodies of a frame through ONE Tracker.ResetBodies call (poses and
    restart); "all": their poses one by one and the batch-wide StartModalities (what reset_loop.run does).
    Hooks as in reset_loop.run; `before_reset(inst, k, lost)` runs in front of the reset of a frame.
    Returns (poses after every step, (frame, object) resets, final histograms)."""
    assert reset in ("bodies", "all"), reset
    inst = scenes.Instance(api, inputs, **(instance_kw or {}))
    if setup:
        setup(inst)
    gt = reset_loop.ground_truth(inputs, schedule)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    poses, resets = [], []
    for k in range(1, inputs.n_frames):
        if frame:
            frame(inst, k)
        else:
            inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
        if after_step:
            after_step(inst, k)
        p = np.stack(inst.poses())
        poses.append(p)
        lost = lost_bodies(p, gt[k])
        resets += [(k, i) for i in lost]
        if not lost:
            continue
        if before_reset:
            before_reset(inst, k, lost)
        iteration = k if iteration_is_frame else 0
        if reset == "bodies":
            assert inst.tracker.ResetBodies([inst.bodies[i] for i in lost], [gt[k][i] for i in lost], iteration)
        else:
            for i in lost:
                inst.bodies[i].set_body2world_pose(gt[k][i])
            assert inst.tracker.StartModalities(iteration)
    assert resets
    return poses, resets, [r.histograms() for r in inst.region]


def check_schedule(schedule, n_objects, n_frames):
    """what the comparison needs of a schedule: a frame with two lost bodies, a body that is never lost, a reset at
    the last frame"""
    frames = [f for f, _, _ in schedule]
    assert any(frames.count(f) >= 2 for f in frames), schedule
    assert set(range(n_objects)) - {i for _, i, _ in schedule}, schedule
    assert n_frames - 1 in frames, schedule


# ---- the batched evaluator's dataset ----------------------------------------------------------------------------------
DATASET_BODIES = ["ape", "cat", "cube", "duck"]
DATASET_LOST_BODY = "cat"


def write_rbot_dataset(tmp_path, n_frames=8):
    """the recipe of test_evaluation.write_rbot_dataset for four bodies (util.syn.Scene(0 .. 3)), one sequence and
    n_divides = 2 models -- with the images k >= 2 of body `cat` rendered at the shared trajectory's pose plus
    0.03 m * (k - 1) along world x: all bodies of an RBOT dataset share poses_first.txt, so an offset in THAT file
    would lose all of them together and a batch-wide restart would pass; here `cat` alone drifts away from the ground
    truth, is lost once, reset, and tracks on.  Returns (dataset, external, body names, model parameters)."""
    from PIL import Image
    cfg = pkg.config
    dataset, external = tmp_path / "RBOT_dataset", tmp_path / "external"
    scenes_ = [util.syn.Scene(i, intr=dict(zip(("fu", "fv", "ppu", "ppv", "width", "height"), ev.RBOT_INTRINSICS)))
               for i in range(len(DATASET_BODIES))]
    trajectory = [scenes_[0].pose.copy()]
    for _ in range(n_frames):
        scenes_[0].step_pose()
        trajectory.append(scenes_[0].pose.copy())
    os.makedirs(dataset)
    with open(dataset / "poses_first.txt", "w") as f:
        f.write("header\n")
        for p in trajectory:
            f.write("\t".join("%.9g" % v for v in list(p[:3, :3].reshape(-1)) + list(p[:3, 3] * 1000.0)) + "\n")
    model_parameters = dict(ev.RBOT_MODEL_PARAMETERS, n_divides=2)
    octahedron = [(60, 0, 0), (-60, 0, 0), (0, 50, 0), (0, -50, 0), (0, 0, 40), (0, 0, -40)]
    faces = [(1, 3, 5), (3, 2, 5), (2, 4, 5), (4, 1, 5), (3, 1, 6), (2, 3, 6), (4, 2, 6), (1, 4, 6)]
    for name, scene in zip(DATASET_BODIES, scenes_):
        os.makedirs(dataset / name / "frames")
        with open(dataset / name / (name + ".obj"), "w") as f:
            f.writelines("v %d %d %d\n" % v for v in octahedron)
            f.writelines("f %d %d %d\n" % t for t in faces)
        for k, p in enumerate(trajectory):
            shown = p.copy()
            if name == DATASET_LOST_BODY and k >= 2:
                shown[0, 3] += 0.03 * (k - 1)
            Image.fromarray(np.ascontiguousarray(scene.render(shown)[:, :, ::-1])).save(
                dataset / name / "frames" / ("a_regular%04d.png" % k))
        points, orientations, lengths = util.syn.make_region_model(scene.body, n_divides=2, n_points=200)
        vertices, _ = cfg.load_obj(str(dataset / name / (name + ".obj")), 0.001)
        data = cfg.BodyData(str(dataset / name / (name + ".obj")), 0.001, True, False,
                            cfg.maximum_body_diameter(vertices), np.eye(4))
        cfg.write_model_bin(str(external / "models" / (name + "_model.bin")), True, model_parameters, data, points,
                            orientations, lengths)
    return dataset, external, list(DATASET_BODIES), model_parameters


def same_results(a, b):
    """two result dictionaries of the evaluators, float for float (complete_cycle is a wall-clock time)"""
    assert a.keys() == b.keys()
    for key in a:
        if key == "complete_cycle":
            continue
        va, vb = a[key], b[key]
        if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
            assert np.array_equal(np.asarray(va), np.asarray(vb)), key
        else:
            assert va == vb, (key, va, vb)
