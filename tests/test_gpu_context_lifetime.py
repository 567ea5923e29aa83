"""A context destroyed while one of its lazily made resources is still outstanding (csrc/m3t_host_resources.h owns
them: the timing event pairs, the camera table's staging ring, the ROI snapshot events and miss block, a judge's row
tables and events, the blocks of set_features, the split step's abort word, streams with a CU mask): the exercise runs,
the context goes, and a fresh context on the same scene tracks two steps to the poses of a context that never saw the
exercise, bit for bit.  Where the exercise itself must not change the poses, they are compared as well."""
import ctypes as C

import numpy as np
import pytest

import scenes
import util
from test_gpu_reset_on_loss import KNOBS
from test_gpu_texture_modality import Scene as TextureScene
from util import host

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def inputs():
    """one Region body, its camera, the start frame and two frames to track"""
    return scenes.Inputs(1, 3, n_divides=2)


def two_steps(api, inputs):
    inst = scenes.Instance(api, inputs, use_depth=inputs.with_depth)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    for k in (1, 2):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
    return inst, np.stack(inst.poses())


@pytest.fixture(scope="module")
def reference(inputs):
    return two_steps(util.open_hip(), inputs)[1]


def destroy_then_track_afresh(api, inputs, reference):
    api.close()
    poses = two_steps(util.open_hip(), inputs)[1]
    assert poses.tobytes() == reference.tobytes()


@pytest.mark.parametrize("mode", [1, 2])
def test_destroyed_with_kernel_timing_on(mode, inputs, reference):
    """mode 1: an event pair per launch, never collected by get_kernel_timing; mode 2: the pair around the region"""
    api = util.open_hip()
    api.call("set_kernel_timing", mode)
    poses = two_steps(api, inputs)[1]
    assert poses.tobytes() == reference.tobytes()
    destroy_then_track_afresh(api, inputs, reference)


def test_destroyed_with_the_camera_staging_ring_in_use():
    """a colour and a depth camera on different ring slots: every switch stages the camera table through the pinned
    ring of 8 blocks.  Ten switches, three more cameras (five tables no longer fit blocks made for two times two),
    two more switches -- the poses of a context that had all five cameras from the start, step for step"""
    inputs = scenes.Inputs(1, 3, n_divides=2, with_depth=True)

    def run(cameras_first):
        api = util.open_hip()
        inst = scenes.Instance(api, inputs, use_depth=True)
        extra = [host.ColorCamera(api, **inputs.intr) for _ in range(3)] if cameras_first else []
        inst.upload_frame(0)
        assert inst.tracker.StartModalities(0)
        color, depth = inst.color_cams[0], inst.depth_cams[0]
        color.set_ring(2)
        depth.set_ring(2)
        for slot in (0, 1):  # frame 1 + slot in the colour ring, the other way round in the depth ring
            color.upload_slot(slot, inputs.color[0][1 + slot])
            depth.upload_slot(1 - slot, inputs.depth[0][1 + slot])
        poses = []
        for switch in range(12):
            if switch == 10 and not cameras_first:
                extra = [host.ColorCamera(api, **inputs.intr) for _ in range(3)]
            color.select_slot(switch % 2)
            depth.select_slot(1 - switch % 2)
            assert inst.tracker.ExecuteTrackingStep(1 + switch)
            poses.append(np.stack(inst.poses()))
        assert len(extra) == 3
        return api, np.stack(poses)

    _, all_along = run(True)
    api, added = run(False)
    assert added.tobytes() == all_along.tobytes()
    assert not np.array_equal(added[0], added[1])  # (the body moves)
    reference = two_steps(util.open_hip(), inputs)[1]
    destroy_then_track_afresh(api, inputs, reference)


def test_destroyed_after_a_rectangle_upload(inputs, reference):
    """ROI ingest: the snapshot events, the miss block, the copy streams and a registered host block"""
    api = util.open_hip()
    inst = scenes.Instance(api, inputs)
    api.call("set_roi_ingest", 1, C.c_float(24.0))
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    h, w = inputs.color[0][0].shape[:2]
    blocks = []
    for k in range(3):
        b = np.ascontiguousarray(inputs.color[0][k].reshape(1, h, w * 3))
        inst.tracker.register_host_buffer(b)
        blocks.append(b)
    ids = (C.c_int * 1)(inst.color_cams[0].id)
    api.call("cameras_set_ring", ids, 1, 2)

    def upload(slot, k):
        b = blocks[k]
        api.call("cameras_upload_batch_roi_async", ids, 1, slot, b.ctypes.data_as(C.c_void_p), b.strides[0], b.strides[1])

    upload(1, 1)  # (no step recorded yet: goes as a whole frame)
    inst.tracker.select_slot(1)
    assert inst.tracker.ExecuteTrackingStep(1)
    upload(0, 2)  # the rectangle
    inst.tracker.select_slot(0)
    assert inst.tracker.ExecuteTrackingStep(2)
    poses = np.stack(inst.poses())
    bodies, n, pulls = (C.c_int * 4)(), C.c_int(0), C.c_longlong(0)
    api.call("roi_get_status", bodies, 4, C.byref(n), C.byref(pulls))
    assert pulls.value == 1 and n.value == 0, (pulls.value, n.value)
    assert poses.tobytes() == reference.tobytes()
    destroy_then_track_afresh(api, inputs, reference)  # (nothing unregistered, no ingest_sync: the context lets go itself)
    assert len(blocks) == 3


def test_destroyed_with_a_judged_row_unread(inputs, reference):
    """a judge's mapped row table and row event, and a structures table set twice (the second replaces the first)"""
    api = util.open_hip()
    inst, poses = two_steps(api, inputs)
    judge = inst.tracker.CreateJudge(inst.bodies, 2)
    judge.set_vertices(0, inputs.vertices[0])
    judge.set_structures([[[0]]], [0.05])
    judge.set_structures([[[0]]], [0.02])
    assert judge.judge([np.asarray(inputs.gt[0][2], F)], -1) == 0
    assert np.stack(inst.poses()).tobytes() == reference.tobytes()  # (judging alone moves nothing)
    assert poses.tobytes() == reference.tobytes()
    destroy_then_track_afresh(api, inputs, reference)


def test_destroyed_with_feature_blocks_in_the_ring():
    """set_features six times -- its ring has four blocks -- with more features from the fifth call on, which has to
    replace the block it takes"""
    def steps(api, exercise):
        s = TextureScene(api)
        s.tracker = host.Tracker(api, 3, 2)
        rng = np.random.default_rng(9)
        n = 150
        base = s.on_body_keypoints(n, seed=9)
        descriptors = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if exercise:
            for call in range(6):
                count = 40 if call < 4 else n
                s.texture.SetFeatures(base[:count], descriptors[:count])
        s.texture.SetFeatures(base, descriptors)
        assert s.tracker.StartModalities(0)
        start = s.body.body2world_pose()
        for frame in range(2):
            order = rng.permutation(n)[:n - 10 * frame]
            xy = (base[order] + rng.uniform(-2, 2, (len(order), 2))).astype(F)
            s.texture.SetFeatures(xy, descriptors[order])
            assert s.tracker.ExecuteTrackingStep(frame)
        assert not np.array_equal(s.body.body2world_pose(), start)  # (the features moved, the body follows)
        return s.body.body2world_pose()

    reference = steps(util.open_hip(), False)
    api = util.open_hip()
    assert steps(api, True).tobytes() == reference.tobytes()
    api.close()
    assert steps(util.open_hip(), False).tobytes() == reference.tobytes()


def test_destroyed_after_a_split_step(inputs, reference):
    """several workgroups per object: the exchange buffer and the mapped abort word"""
    api = util.open_hip()
    api.call("set_object_split", 4)
    poses = two_steps(api, inputs)[1]
    shape = (C.c_int * 4)()
    api.call("get_step_shape", shape)
    assert shape[0] == 1 and shape[1] > 1, list(shape)
    assert poses.tobytes() == reference.tobytes()
    destroy_then_track_afresh(api, inputs, reference)


def test_destroyed_after_reserving_and_returning_cus(inputs, reference):
    """reserve_ingest_cus replaces the compute stream and, with asynchronous ingest started, the copy streams -- twice"""
    api = util.open_hip()
    name, cus = C.create_string_buffer(256), C.c_int(0)
    api.call("device_info", name, 256, C.byref(cus), None)
    if b"gfx950" not in name.value or cus.value != 256:
        pytest.skip("CU reservation is laid out for MI355X (gfx950, 256 CUs in one partition)")
    inst = scenes.Instance(api, inputs)
    first = np.ascontiguousarray(inputs.color[0][0])
    inst.color_cams[0].upload_slot(0, first, asynchronous=True)  # (starts the copy streams)
    inst.tracker.ingest_sync()
    assert inst.tracker.StartModalities(0)
    for k, cus_reserved in ((1, 32), (2, 0)):
        api.call("reserve_ingest_cus", cus_reserved)
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
    assert np.stack(inst.poses()).tobytes() == reference.tobytes()
    destroy_then_track_afresh(api, inputs, reference)
