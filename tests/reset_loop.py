"""The RBOT evaluator's reset-on-loss loop (M3T/examples/rbot_evaluator.cpp:174-210, ResetBody :334-342) over a whole
batch, driven the same way through either C-ABI context: track a frame, judge every object with the 5 cm / 5 degree
criterion against a ground truth that holds injected offsets, set every lost body to that ground truth and (restart
mode) start the modalities again.  Each library decides from its own poses, as an evaluator does.

A loss schedule entry (frame, object, kind) replaces that object's ground truth at that frame:
  "a" -- translated by 20 cm;
  "b" -- rotated by 30-40 degrees about a seeded axis through the body's origin, across the line of sight (the
         closest view of the model changes by as much);
  "c" -- shifted sideways until the body's origin lies on the nearest vertical image border (half the silhouette off
         the image).
The object is then judged lost and reset to the offset pose, is lost again on the next (honest) frame because it now
starts far from what the image shows, and is reset to the true pose: two resets per entry, one for an entry at the last
frame (pose-only mode: see expected_resets)."""
import numpy as np

from util import pkg

ev = pkg.evaluation


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def offset_pose(pose, kind, intr, seed):
    p = np.asarray(pose, np.float64).copy()
    if kind == "a":
        p[:3, 3] += (0.2, 0.0, 0.0)
    elif kind == "b":
        rng = np.random.default_rng(seed)
        axis = rng.normal(size=3)
        sight = p[:3, 3] / np.linalg.norm(p[:3, 3])
        axis -= (axis @ sight) * sight  # across the line of sight: the viewing direction turns by the full angle
        p[:3, :3] = rotation(axis, np.deg2rad(rng.uniform(30.0, 40.0))) @ p[:3, :3]
    elif kind == "c":
        x, z = p[0, 3], p[2, 3]
        u = intr["fu"] * x / z + intr["ppu"]
        border = 0.0 if u < intr["width"] / 2 else float(intr["width"])
        p[0, 3] = (border - intr["ppu"]) * z / intr["fu"]
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def default_schedule(n_objects, n_frames):
    """one entry of every kind, one reset after the first step and one at the last frame (frames are those of
    ExecuteTrackingStep: 1 .. n_frames - 1)"""
    last = n_frames - 1
    mid = max(2, last // 2)
    return [(1, 0, "a"), (mid, n_objects // 3, "b"), (mid, (2 * n_objects) // 3, "c"),
            (min(mid + 1, last - 1), n_objects // 2, "b"), (last, n_objects - 1, "a")]


def ground_truth(inputs, schedule, seed=11):
    gt = [[np.asarray(inputs.gt[i][k], np.float32) for i in range(inputs.n_objects)] for k in range(inputs.n_frames)]
    for frame, obj, kind in schedule:
        gt[frame][obj] = offset_pose(inputs.gt[obj][frame], kind, inputs.intr, seed + 1000 * frame + obj)
    return gt


def expected_resets(schedule, n_frames, mode="restart"):
    """the (frame, object) resets the schedule makes.  In pose-only mode a body's histograms survive its reset, and
    the tracker turns a body that was only rotated back onto the image within one step: one reset for a kind (b)
    entry there"""
    out = []
    for frame, obj, kind in schedule:
        out.append((frame, obj))
        if frame + 1 < n_frames and not (mode == "pose-only" and kind == "b"):
            out.append((frame + 1, obj))
    return sorted(out)


def closest_view(orientations, pose):
    """RegionModel::GetClosestView (region_model.cpp:105-130) for a camera at the world origin: the first maximum of
    the dot products of the views' orientations with the direction to the camera in body coordinates"""
    p = np.asarray(pose, np.float64)
    t = p[:3, 3] / np.linalg.norm(p[:3, 3])
    o = np.linalg.inv(p[:3, :3]) @ t
    return int(np.argmax(np.asarray(orientations, np.float64) @ o))


def view_neighbors(orientations, view, n_neighbors=18):
    """the M3T_VIEW_NEIGHBORS (18) nearest views of `view` (m3t_view_rows.h): the row closest_view_local searches"""
    ori = np.asarray(orientations, np.float64)
    d = ori @ ori[view]
    d[view] = 4.0
    order = sorted(range(len(ori)), key=lambda w: (-d[w], w))
    return set(order[1:n_neighbors + 1])


def run(api, inputs, schedule, mode, instance_kw=None, setup=None, frame=None, after_step=None, restart=None):
    """The loop over frames 1 .. n_frames - 1 (StartModalities on frame 0 at the inputs' start poses).
    mode "restart": after the resets of a frame, StartModalities(0) (ResetBody); "pose-only": the poses alone, the
    histograms go on.  Hooks, for other ways of handing frames over: `setup(inst)` before frame 0,
    `frame(inst, k)` makes frame k current (default: upload_frame), `after_step(inst, k)` runs after every step,
    `restart(inst, k)` replaces the default restart.
    Returns (poses after every step, before any reset; the (frame, object) resets; the final histograms; the
    pre-reset poses of the resets, keyed by (frame, object))."""
    import scenes
    assert mode in ("restart", "pose-only"), mode
    inst = scenes.Instance(api, inputs, **(instance_kw or {}))
    if setup:
        setup(inst)
    gt = ground_truth(inputs, schedule)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    poses, resets, before = [], [], {}
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
        lost = [i for i in range(inputs.n_objects) if ev.rbot_pose_result(p[i], gt[k][i])[2] == 0.0]
        for i in lost:
            inst.bodies[i].set_body2world_pose(gt[k][i])
            resets.append((k, i))
            before[(k, i)] = p[i]
        if lost and mode == "restart":
            if restart:
                restart(inst, k)
            else:
                assert inst.tracker.StartModalities(0)
    return poses, resets, [r.histograms() for r in inst.region], before


def assert_same(got, ref):
    """bit-for-bit equality of two run() results (poses after every step, resets, final histograms)"""
    poses, resets, hist = got[:3]
    ref_poses, ref_resets, ref_hist = ref[:3]
    assert resets == ref_resets and resets, (resets, ref_resets)
    assert len(poses) == len(ref_poses)
    for k, (a, b) in enumerate(zip(poses, ref_poses)):
        assert np.array_equal(a, b), (k + 1, np.argwhere(np.any(a != b, axis=(1, 2))).ravel().tolist())
    assert len(hist) == len(ref_hist)
    for j, ((fa, ba), (fb, bb)) in enumerate(zip(hist, ref_hist)):
        assert np.array_equal(fa, fb) and np.array_equal(ba, bb), j


def check_tracked(inputs, poses, schedule):
    """after the last step every object lies within 5 cm / 5 degrees of the (injected) ground truth"""
    gt = ground_truth(inputs, schedule)
    k = inputs.n_frames - 1
    bad = [i for i in range(inputs.n_objects) if ev.rbot_pose_result(poses[-1][i], gt[k][i])[2] == 0.0]
    # an object whose entry is the last frame was lost there, by construction
    return [i for i in bad if (k, i) not in {(f, o) for f, o, _ in schedule}]


def view_jumps(inputs, schedule, before):
    """for every kind (b) entry: (closest view before the reset, closest view at the reset pose, is the latter outside
    the former's neighbour row)"""
    gt = ground_truth(inputs, schedule)
    out = []
    for frame, obj, kind in schedule:
        if kind != "b":
            continue
        ori = inputs.region_models[inputs.model_of[obj]][1]
        v0 = closest_view(ori, before[(frame, obj)])
        v1 = closest_view(ori, gt[frame][obj])
        out.append((v0, v1, v1 != v0 and v1 not in view_neighbors(ori, v0)))
    return out
