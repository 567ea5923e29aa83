"""Tracker.ResetBodies and a resetting Judge.judge on bodies whose texture modality has the built-in detector
(m3t_hip_reset_bodies / m3t_hip_judge_bodies: texture_*_list_kernel of csrc/m3t_features.hip and csrc/m3t_texture.hip).

The expectation never comes from the call under test.  A plate of a batch is expected to do what it does in a context
of its own -- one tracker per plate -- that gets set_body2world_pose + StartModalities(0) where the batch resets the
plate, and nothing where the batch resets another one; a device-judged context is expected to do what the same context
does when it is judged on the host and reset with ResetBodies.  Every comparison is bit for bit: the pose, points(),
keyframes(), features() and focused_image() as uint32 / byte arrays.

Scenes: the three plates, the 160 x 120 frame and SEQUENCE_IMAGE of tests/test_gpu_texture_detector.py, n_keyframes = 2,
fast_threshold = 15."""
import numpy as np
import pytest

import util
from test_gpu_texture_detector import PLATES, SEQUENCE_IMAGE, Frame, Plate, _pose
from util import host

pytestmark = pytest.mark.gpu
capi = util.pkg._capi
F = np.float32

SHIFTS = [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (4, 3)]  # pixels the frame has moved by, frame k


def _moved(k, dx, dy, dz=0.0):
    pose = PLATES[k][0].copy()
    pose[:3, 3] += np.array([dx, dy, dz], F)
    return pose


# plate 1 moved by 3 and 2 pixels (fu = fv = 200, z = 0.55); a pose whose region of interest is invalid (z < 1.5 r)
MOVED = _moved(1, 0.008, -0.005)
MOVED_AGAIN = _moved(1, -0.006, 0.004)
TOO_CLOSE = _pose(-0.01, 0.003, 0.07)


class Context:
    def __init__(self, which, builtin=None):
        self.api = util.open_hip()
        self.frame = Frame(self.api)
        builtin = [True] * len(which) if builtin is None else builtin
        self.plates = [Plate(self.api, self.frame, *PLATES[k][:2], builtin=b, focused_image_size=PLATES[k][2],
                             fast_threshold=15, body_id=100 + k, n_keyframes=2) for k, b in zip(which, builtin)]
        self.tracker = host.Tracker(self.api, 2, 2)

    def show(self, k):
        self.frame.show(np.roll(SEQUENCE_IMAGE, (SHIFTS[k][1], SHIFTS[k][0]), axis=(0, 1)))

    def bodies(self, indices):
        return [self.plates[i].body for i in indices]


def compared(plate):
    """the compared arrays of a plate, as bytes"""
    age, keyframes = plate.texture.keyframes()
    keypoints, descriptors = plate.texture.features()
    focused = plate.texture.focused_image()
    return dict(pose=plate.body.body2world_pose().view(np.uint32).tobytes(),
                points=plate.texture.points().tobytes(),
                keyframe_age=age, keyframes=[k.view(np.uint32).tobytes() for k in keyframes],
                keypoints=keypoints.view(np.uint32).tobytes(), descriptors=descriptors.tobytes(),
                focused=None if focused is None else (focused.shape, focused.tobytes()))


def assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key] == b[key], (what, key)


def run(context, script, own=None, wait=False, snapshots=True):
    """script: ("show", k) | ("start",) | ("step", i) | ("reset", [plate indices], [poses] or None).  own = k: the
    context holds plate k of the batch alone -- a reset that lists k is set_body2world_pose + StartModalities(0), one
    that does not is nothing.  wait: Sync() after every call.  Returns the compared arrays of every plate after every
    call (snapshots) or after the last one."""
    history = []
    for op in script:
        if op[0] == "show":
            context.show(op[1])
            continue
        if op[0] == "start":
            assert context.tracker.StartModalities(0)
        elif op[0] == "step":
            assert context.tracker.ExecuteTrackingStep(op[1])
        elif own is None:
            assert context.tracker.ResetBodies(context.bodies(op[1]), op[2], 0), context.api.last_error()
        elif own in op[1]:
            if op[2] is not None:
                context.plates[0].body.set_body2world_pose(op[2][op[1].index(own)])
            assert context.tracker.StartModalities(0)
        if wait:
            assert context.tracker.Sync()
        if snapshots:
            history.append([compared(p) for p in context.plates])
    return history if snapshots else [[compared(p) for p in context.plates]]


def batch_and_own(script):
    """the script in a context of the three plates and in three contexts of one plate each: (history of the batch,
    [history of plate k's own tracker]), equal call for call"""
    batch = run(Context([0, 1, 2]), script)
    own = [run(Context([k]), script, own=k) for k in range(3)]
    for call, state in enumerate(batch):
        for k in range(3):
            assert_same(state[k], own[k][call][0], (call, k))
    return batch, own


# ---- 1 -----------------------------------------------------------------------------------------------------------------
def test_one_of_three_plates_is_reset_and_every_plate_equals_its_own_tracker():
    script = [("show", 0), ("start",), ("show", 1), ("step", 0), ("reset", [1], [MOVED]), ("show", 2), ("step", 1)]
    batch, _ = batch_and_own(script)
    started, stepped, reset, after = batch
    for k in (0, 2):  # the plates not listed keep every compared array across the call
        assert_same(stepped[k], reset[k], k)
    # not vacuous: a second keyframe, other features than before, data points in the step that follows
    assert len(stepped[1]["keyframes"]) == 1 and len(reset[1]["keyframes"]) == 2
    assert reset[1]["keypoints"] != stepped[1]["keypoints"] and len(reset[1]["keypoints"]) > 8 * 10
    assert reset[1]["pose"] == MOVED.view(np.uint32).tobytes()
    assert len(after[1]["points"]) > 10 * capi.TEXTURE_DATA_POINT_DTYPE.itemsize
    assert after[1]["pose"] != reset[1]["pose"]


# ---- 2 -----------------------------------------------------------------------------------------------------------------
def test_two_resets_in_a_row_pop_the_oldest_keyframe():
    script = [("show", 0), ("start",), ("show", 1), ("step", 0), ("reset", [1], [MOVED]), ("reset", [1], [MOVED_AGAIN]),
              ("show", 2), ("step", 1)]
    batch, _ = batch_and_own(script)
    first, second = batch[2][1], batch[3][1]
    assert len(first["keyframes"]) == 2 and len(second["keyframes"]) == 2
    assert second["keyframes"][0] == first["keyframes"][1] and second["keyframes"][1] != first["keyframes"][1]
    assert len(first["keyframes"][0]) > 0 and first["keyframes"][0] != second["keyframes"][0]


def test_a_reset_to_an_invalid_region_of_interest_detects_nothing_and_appends_no_keyframe():
    """TOO_CLOSE: z < 1.5 r -- no region of interest (no features) and the body is not visible to its silhouette
    renderer (no keyframe appended); the ring is full before the call, so the oldest keyframe is still popped"""
    script = [("show", 0), ("start",), ("reset", [1], [MOVED]), ("reset", [1], [TOO_CLOSE]), ("reset", [1], [MOVED_AGAIN]),
              ("show", 1), ("step", 0)]
    batch, _ = batch_and_own(script)
    full, invalid, again = batch[1][1], batch[2][1], batch[3][1]
    assert len(full["keyframes"]) == 2
    assert invalid["keypoints"] == b"" and invalid["focused"] is None
    assert invalid["keyframes"] == full["keyframes"][1:]
    assert len(again["keypoints"]) > 0 and again["keyframes"][0] == full["keyframes"][1] and len(again["keyframes"]) == 2


def test_a_reset_without_poses_restarts_at_the_pose_the_device_holds():
    script = [("show", 0), ("start",), ("show", 1), ("step", 0), ("reset", [2, 0], None), ("show", 2), ("step", 1)]
    batch, _ = batch_and_own(script)
    stepped, reset = batch[1], batch[2]
    assert_same(stepped[1], reset[1])
    for k in (0, 2):
        assert reset[k]["pose"] == stepped[k]["pose"] and len(stepped[k]["keyframes"]) == 1
        assert len(reset[k]["keyframes"]) == 2 and len(reset[k]["keyframes"][1]) > 0


# ---- 3 -----------------------------------------------------------------------------------------------------------------
def test_a_caller_fed_plate_is_refused_and_the_built_in_ones_are_accepted():
    context = Context([0, 1, 2], builtin=[True, False, True])
    context.show(0)
    context.plates[1].feed(context.plates[1].reference())
    assert context.tracker.StartModalities(0)
    context.show(1)
    context.plates[1].feed(context.plates[1].reference())
    assert context.tracker.ExecuteTrackingStep(0)
    before = [compared(p) if p.texture.detector is not None else None for p in context.plates]
    fed_before = (context.plates[1].body.body2world_pose().tobytes(), context.plates[1].texture.points().tobytes(),
                  context.plates[1].texture.keyframes(), context.plates[1].texture.features())
    pose = np.ascontiguousarray(capi.pose_arg(MOVED), F)
    for listed in ([1], [0, 1], [1, 2]):
        ids = np.asarray([context.plates[i].body.id for i in listed], np.int32)
        poses = np.ascontiguousarray(np.concatenate([pose] * len(listed)), F)
        rc = context.api.raw("reset_bodies", capi.iptr(ids), capi.fptr(poses), len(ids), 0)
        assert rc == capi.M3T_ERR_UNSUPPORTED and "texture modality" in context.api.last_error(), listed
        for k in (0, 2):
            assert_same(before[k], compared(context.plates[k]), (listed, k))
        fed_after = (context.plates[1].body.body2world_pose().tobytes(), context.plates[1].texture.points().tobytes(),
                     context.plates[1].texture.keyframes(), context.plates[1].texture.features())
        assert fed_after[:2] == fed_before[:2] and fed_after[2][0] == fed_before[2][0]
        assert all(np.array_equal(a, b) for a, b in zip(fed_after[2][1], fed_before[2][1]))
        assert all(np.array_equal(a, b) for a, b in zip(fed_after[3], fed_before[3]))
    ids = np.asarray([context.plates[i].body.id for i in (0, 2)], np.int32)
    assert context.api.raw("reset_bodies", capi.iptr(ids), None, 2, 0) == 0, context.api.last_error()
    for k in (0, 2):
        assert len(compared(context.plates[k])["keyframes"]) == 2


# ---- 4 -----------------------------------------------------------------------------------------------------------------
def _tracked(n_bodies=3):
    """a context after StartModalities and one step, frame 2 shown; the poses the device holds"""
    context = Context(list(range(n_bodies)))
    run(context, [("show", 0), ("start",), ("show", 1), ("step", 0), ("show", 2)], snapshots=False)
    return context, [p.body.body2world_pose() for p in context.plates]


def test_the_judge_resets_the_lost_plate_like_a_host_judged_reset_bodies():
    device, poses = _tracked()
    judge = device.tracker.CreateJudge(device.bodies([0, 1, 2]), 4)
    judge.set_reset_renderers()
    gt = [poses[0], _moved(1, 0.06, 0.0), poses[2]]  # plate 1 alone is more than 5 cm from its ground truth
    before = [compared(p) for p in device.plates]
    row = judge.judge(gt, 0)
    rows = judge.read(row, 1)
    assert list(rows[0]["was_reset"]) == [0, 1, 0] and list(rows[0]["tracking_success"]) == [1.0, 0.0, 1.0]
    on_host, host_poses = _tracked()
    assert all(np.array_equal(a, b) for a, b in zip(poses, host_poses))
    lost = [k for k in range(3) if util.pkg.evaluation.rbot_pose_result(host_poses[k], gt[k])[2] == 0.0]
    assert lost == [1]
    assert on_host.tracker.ResetBodies(on_host.bodies(lost), [gt[k] for k in lost], 0)
    after = [compared(p) for p in device.plates]
    for k in range(3):
        assert_same(after[k], compared(on_host.plates[k]), k)
    for k in (0, 2):
        assert_same(before[k], after[k], k)
    assert len(after[1]["keyframes"]) == 2 and after[1]["keypoints"] != before[1]["keypoints"]
    # ... and the step that follows
    for context in (device, on_host):
        assert context.tracker.ExecuteTrackingStep(1)
    for k in range(3):
        assert_same(compared(device.plates[k]), compared(on_host.plates[k]), k)
    assert len(device.plates[1].texture.points()) > 10
    # a frame without a loss: nothing changes
    poses = [p.body.body2world_pose() for p in device.plates]
    before = [compared(p) for p in device.plates]
    row = judge.judge(poses, 0)
    assert list(judge.read(row, 1)[0]["was_reset"]) == [0, 0, 0]
    for k in range(3):
        assert_same(before[k], compared(device.plates[k]), k)


def test_the_judge_without_the_renderer_opt_in_refuses_texture_bodies():
    device, poses = _tracked()
    judge = device.tracker.CreateJudge(device.bodies([0, 1, 2]), 4)
    before = [compared(p) for p in device.plates]
    rc, _ = judge.raw_judge([poses[0], _moved(1, 0.06, 0.0), poses[2]], 0)
    assert rc == capi.M3T_ERR_UNSUPPORTED and "start-modality renderer" in device.api.last_error()
    for k in range(3):
        assert_same(before[k], compared(device.plates[k]), k)
    assert judge.judge(poses, -1) == 0  # judging alone needs no opt-in


def test_the_judge_restarts_a_reset_target_and_leaves_the_judged_plate_alone():
    device, poses = _tracked()
    judge = device.tracker.CreateJudge(device.bodies([0, 1]), 4)
    judge.set_reset_renderers()
    judge.set_reset_target(0, device.plates[2].body)
    target_pose = _moved(2, -0.006, 0.004)  # plate 0 is judged against it: more than 5 cm away
    before = [compared(p) for p in device.plates]
    row = judge.judge([target_pose, poses[1]], 0)
    assert list(judge.read(row, 1)[0]["was_reset"]) == [1, 0]
    on_host, _ = _tracked()
    assert on_host.tracker.ResetBodies(on_host.bodies([2]), [target_pose], 0)
    after = [compared(p) for p in device.plates]
    for k in range(3):
        assert_same(after[k], compared(on_host.plates[k]), k)
    for k in (0, 1):
        assert_same(before[k], after[k], k)
    assert after[2]["pose"] == target_pose.view(np.uint32).tobytes() and len(after[2]["keyframes"]) == 2


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def test_six_resets_queued_without_a_wait_equal_a_context_that_waits_after_every_call():
    """more calls in flight than the ring of argument blocks has (four): a block is taken again only once its call ran"""
    script = [("show", 0), ("start",)]
    for call in range(6):
        listed = [[1], [0, 2], [2], [1, 0], [0], [2, 1]][call]
        poses = [_moved(k, 0.002 * (call + 1) * (1 if k != 1 else -1), 0.001 * call) for k in listed]
        script += [("show", call + 1), ("step", call), ("reset", listed, poses if call != 2 else None)]
    script += [("show", 7), ("step", 6)]
    queued = run(Context([0, 1, 2]), script, snapshots=False)[0]
    waited = run(Context([0, 1, 2]), script, wait=True, snapshots=False)[0]
    for k in range(3):
        assert_same(queued[k], waited[k], k)
        assert len(queued[k]["keyframes"]) == 2 and len(queued[k]["points"]) > 0
