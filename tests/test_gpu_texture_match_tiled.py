"""The tiled Hamming matcher of the texture modality (csrc/m3t_texture_tiled.hip) against
the scalar restatement (tests/texture_reference.py), bit for bit in data points and keyframes, and against a twin
context in the one-workgroup form: at the tile edge, with fewer train rows than waves, with ranges that end inside and
on a group of rows, with a wrapped ring and an empty keyframe, at full size, and beside modalities of every other kind.
The form is the library's developer override M3T_HIP_TEXTURE_MATCH, which a context looks at once, when it is made; the
library has no call that reports the form, so one test reads the HIP runtime's own launch log of child processes to see
which kernels each setting launches; the others hold that both settings give the restatement's bits."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import feature_scenes as FS
import texture_reference as T
import util
from test_gpu_texture_detector import HEIGHT, PLATES, WIDTH, Frame, Plate
from test_gpu_texture_modality import Scene, _descriptors, _keyframes_equal, _points_equal, _rotated
from util import host

pytestmark = pytest.mark.gpu
F = np.float32
ONE, TILED = "one", "tiled"
WAVES = 4  # of a workgroup of texture_match_tiled_kernel: the train rows are split into that many ranges


def _open(mode):
    """a context made while M3T_HIP_TEXTURE_MATCH says `mode`"""
    before = os.environ.get("M3T_HIP_TEXTURE_MATCH")
    os.environ["M3T_HIP_TEXTURE_MATCH"] = mode
    try:
        return util.open_hip()
    finally:
        if before is None:
            del os.environ["M3T_HIP_TEXTURE_MATCH"]
        else:
            os.environ["M3T_HIP_TEXTURE_MATCH"] = before


def _same_points(a, b):
    assert len(a) == len(b)
    assert a.tobytes() == b.tobytes()


def _tiled_descriptors(rng, n_query, n_train, n_bytes):
    """_descriptors' scheme (even queries: a train row with one bit flipped; the ratio exactly at the threshold 0.75 on
    query 4) with the tie planted across the join of two waves: the last row of wave 0's range is copied into the first
    row of wave 1's and query 2 equals both (the lower index has to win, 0 / 0 has to be kept)"""
    queries, train = _descriptors(rng, n_query, n_train, n_bytes, planted=False)
    wave_range = (n_train + WAVES - 1) // WAVES
    tie = n_train >= wave_range + 2 and n_query >= 6
    ratio = n_train >= 2 and n_query >= 6
    if tie:
        train[wave_range] = train[wave_range - 1]
    if ratio:  # rows 0 and 1 differ in one bit
        train[0] = 0
        train[1] = 0
        train[1, 0] = 0x01
    for q in range(0, n_query, 2):  # (again: the rows above have changed)
        if n_train:
            queries[q] = train[(q * 7) % n_train]
            queries[q, (q + 5) % n_bytes] ^= np.uint8(1 << (q % 8))
    if tie:
        queries[2] = train[wave_range - 1]
    if ratio:
        queries[4] = 0
        queries[4, 1] = 0x07  # 3 bits from row 0, 4 bits from row 1, far from every random row
    return queries, train, (wave_range - 1 if tie else None)


N_QUERY = [0, 1, 2, 63, 64, 65, 129]
N_TRAIN = [0, 1, 2, 3, 4, 5, 31, 32, 33, 257]


@pytest.mark.parametrize("n_bytes", [32, 64])
def test_tiled_matcher_equals_the_restatement_and_the_one_workgroup_form_at_every_size(n_bytes):
    tiled, one = _open(TILED), _open(ONE)
    scenes = [Scene(api, descriptor_bytes=n_bytes, descriptor_distance_threshold=0.75) for api in (tiled, one)]
    keypoints = scenes[0].on_body_keypoints(max(N_QUERY), seed=1)
    rng = np.random.default_rng(n_bytes)
    for n_query in N_QUERY:
        for n_train in N_TRAIN:
            queries, train, tie_row = _tiled_descriptors(rng, n_query, n_train, n_bytes)
            train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
            state = scenes[0].state()
            for s in scenes:
                s.texture.SetFeatures(keypoints[:n_query], queries)
                assert s.tracker.StartModalities(0)
            state.set_features(keypoints[:n_query], queries)
            scenes[0].reference_keyframe(state)
            assert [len(k) for k in state.points_keyframes] == [n_query]  # every keypoint is on the body
            for s in scenes:
                s.texture.SetFeatures(train_xy, train)
                assert s.tracker.CalculateCorrespondences(0, 0)
            state.set_features(train_xy, train)
            state.calculate_correspondences(scenes[0].body.body2world_pose(), scenes[0].cam, 0)
            if n_query >= 2 and n_train >= 2:  # not vacuous: the restatement alone keeps some and rejects some
                assert 0 < len(state.data_points) < n_query, (n_query, n_train)
            else:
                assert n_train >= 2 or len(state.data_points) == 0
            if tie_row is not None and tie_row >= 2:  # the tie across the join (where the ratio's rows 0 and 1 leave it
                # alone): the restatement takes the lower index, and 0 / 0 is kept
                assert T.knn_match2(queries[2:3], train)[0] == (0, 0, tie_row), (n_query, n_train)
                assert T.ratio_keeps(0, 0, F(0.75))
            if n_query >= 6 and n_train >= 2:  # the planted ratio is exactly the threshold, and is rejected
                d0, d1, _ = T.knn_match2(queries[4:5], train)[0]
                assert (d0, d1) == (3, 4) and not T.ratio_keeps(d0, d1, F(0.75)), (n_query, n_train)
            points = scenes[0].texture.points()
            _points_equal(points, state.data_points)
            _keyframes_equal(scenes[0].texture, state)
            _same_points(points, scenes[1].texture.points())


@pytest.mark.parametrize("n_bytes", [32, 64])
def test_wrapped_ring_with_an_empty_keyframe_then_the_collect_pass_alone(n_bytes):
    tiled, one = _open(TILED), _open(ONE)
    scenes = [Scene(api, descriptor_bytes=n_bytes, n_keyframes=3) for api in (tiled, one)]
    keypoints = scenes[0].on_body_keypoints(129, seed=3)
    off_body = np.tile(np.array([[1.5, 1.5]], F), (40, 1))  # a corner of the image: no keypoint is on the body
    rng = np.random.default_rng(200 + n_bytes)
    state = scenes[0].state()
    held = []
    # four StartModalities on a ring of three: the head has wrapped, the ring holds 65, none and 129 points
    for xy, n in ((keypoints, 10), (keypoints, 65), (off_body, 40), (keypoints, 129)):
        descriptors = rng.integers(0, 256, (n, n_bytes), dtype=np.uint8)
        for s in scenes:
            s.texture.SetFeatures(xy[:n], descriptors)
            assert s.tracker.StartModalities(0)
        state.set_features(xy[:n], descriptors)
        scenes[0].reference_keyframe(state)
        held.append(descriptors)
    assert [len(k) for k in state.points_keyframes] == [65, 0, 129]  # the restatement agrees: the third frame gave none
    n_train = 257
    train = rng.integers(0, 256, (n_train, n_bytes), dtype=np.uint8)
    for k, descriptors in ((1, held[1]), (3, held[3])):  # every other query has a near twin among the train rows
        for q in range(0, len(descriptors), 2):
            train[(q * 3 + k) % n_train] = descriptors[q]
            train[(q * 3 + k) % n_train, 5] ^= np.uint8(4)
    train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
    for s in scenes:
        s.texture.SetFeatures(train_xy, train)
        assert s.tracker.CalculateCorrespondences(0, 0)
    state.set_features(train_xy, train)
    state.calculate_correspondences(scenes[0].body.body2world_pose(), scenes[0].cam, 0)
    assert 40 < len(state.data_points) < 65 + 129
    _points_equal(scenes[0].texture.points(), state.data_points)
    _keyframes_equal(scenes[0].texture, state)
    _same_points(scenes[0].texture.points(), scenes[1].texture.points())
    # corr_iteration 1 after a pose change: the collect kernel alone, which only projects
    pose = scenes[0].body.body2world_pose()
    pose[:3, 3] += np.array([0.002, -0.001, 0.003], F)
    for s in scenes:
        s.body.set_body2world_pose(pose)
        assert s.tracker.CalculateCorrespondences(0, 1)
    state.calculate_correspondences(pose, scenes[0].cam, 1)
    _points_equal(scenes[0].texture.points(), state.data_points)
    _same_points(scenes[0].texture.points(), scenes[1].texture.points())


def test_full_size_with_one_keyframe():
    n, n_bytes = T.MAX_FEATURES, 64
    tiled, one = _open(TILED), _open(ONE)
    scenes = [Scene(api, descriptor_bytes=n_bytes) for api in (tiled, one)]
    keypoints = scenes[0].on_body_keypoints(n, seed=2)
    rng = np.random.default_rng(164)
    queries = rng.integers(0, 256, (n, n_bytes), dtype=np.uint8)
    train = rng.integers(0, 256, (n, n_bytes), dtype=np.uint8)
    for q in range(0, n, 3):  # every third query has a near twin among the train rows
        train[(q * 5) % n] = queries[q]
        train[(q * 5) % n, 3] ^= np.uint8(16)
    train_xy = rng.uniform(0, 900, (n, 2)).astype(F)
    state = scenes[0].state()
    for s in scenes:
        s.texture.SetFeatures(keypoints, queries)
        assert s.tracker.StartModalities(0)
        s.texture.SetFeatures(train_xy, train)
        assert s.tracker.CalculateCorrespondences(0, 0)
    state.set_features(keypoints, queries)
    scenes[0].reference_keyframe(state)
    state.set_features(train_xy, train)
    state.calculate_correspondences(scenes[0].body.body2world_pose(), scenes[0].cam, 0)
    assert 1000 < len(state.data_points) < n
    _points_equal(scenes[0].texture.points(), state.data_points)
    _same_points(scenes[0].texture.points(), scenes[1].texture.points())


# ---- one context with modalities of every kind ----------------------------------------------------------------------
KINDS = [dict(n_keyframes=1), dict(n_keyframes=3), dict(descriptor_bytes=64),
         dict(descriptor_norm="l2", descriptor_bytes=64), "plate"]
IMAGE = FS.blocks(HEIGHT, WIDTH, seed=21, n=300, low=3, high=9)


def _run_kinds(api, which):
    """two StartModalities (the ring of three then holds two keyframes) and two tracking steps; the poses, data points
    and keyframes of every modality after every call"""
    members, feeds = [], []
    frame = None
    for k in which:
        if KINDS[k] == "plate":
            frame = Frame(api)
            plate = Plate(api, frame, *PLATES[0][:2], focused_image_size=PLATES[0][2], fast_threshold=15, body_id=100,
                          n_keyframes=2, max_keyframe_age=2)
            members.append(plate)
            feeds.append(None)
            continue
        s = Scene(api, **KINDS[k])
        rng = np.random.default_rng(50 + k)
        count = (70, 150, 129, 66)[k]
        keypoints = s.on_body_keypoints(count, seed=50 + k)
        if KINDS[k].get("descriptor_norm") == "l2":
            rows = rng.integers(0, 256, (count, 16)).astype(F)
        else:
            rows = rng.integers(0, 256, (count, KINDS[k].get("descriptor_bytes", 32)), dtype=np.uint8)
        members.append(s)
        feeds.append((keypoints, rows, rng))
    tracker = host.Tracker(api, 2, 2)
    history = []
    for call in range(4):
        if frame is not None:
            frame.show(np.roll(IMAGE, (call // 2, call % 2), axis=(0, 1)))
        for s, feed in zip(members, feeds):
            if feed is None:
                continue
            keypoints, rows, rng = feed
            order = rng.permutation(len(keypoints))[:len(keypoints) - 7 * call]
            xy = (keypoints[order] + rng.uniform(-3, 3, (len(order), 2))).astype(F) if call >= 2 else keypoints[order]
            s.texture.SetFeatures(xy, rows[order])
        assert tracker.StartModalities(0) if call < 2 else tracker.ExecuteTrackingStep(call)
        history.append([(m.body.body2world_pose(), m.texture.points(), m.texture.keyframes()) for m in members])
    return history


def test_modalities_of_every_kind_in_one_context_equal_each_alone():
    api = _open(TILED)
    together = _run_kinds(api, range(len(KINDS)))
    # after the second StartModalities the ring of three holds two keyframes, the rings of one hold one; every modality
    # had data points in the last step
    assert [len(keys[1]) for _, _, keys in together[1]][:4] == [1, 2, 1, 1]
    assert all(len(points) > 10 for _, points, _ in together[-1])
    for k in range(len(KINDS)):
        alone = _run_kinds(util.open_hip(), [k])
        for call, (step_together, step_alone) in enumerate(zip(together, alone)):
            (pose_a, points_a, keys_a), (pose_b, points_b, keys_b) = step_together[k], step_alone[0]
            assert pose_a.tobytes() == pose_b.tobytes(), (k, call)
            _same_points(points_a, points_b)
            assert keys_a[0] == keys_b[0] and len(keys_a[1]) == len(keys_b[1]), (k, call)
            for x, y in zip(keys_a[1], keys_b[1]):
                assert x.tobytes() == y.tobytes(), (k, call)
        assert not np.array_equal(alone[-1][0][0], alone[0][0][0]), k  # the steps moved the body


# ---- the override is looked at when the context is made, not later -----------------------------------------------------
def test_a_sequence_with_keyframe_renewal_is_the_same_in_both_forms_and_by_default():
    """the loop of test_sequence_with_keyframe_renewal_equals_a_restatement_driven_loop on three contexts: made under
    "one", under "tiled" and with no override; the variable changes between the frames, which no context may notice"""
    apis = [_open(ONE), _open(TILED), util.open_hip()]
    scenes = [Scene(api, n_keyframes=2, max_keyframe_age=1) for api in apis]
    for s in scenes:
        s.tracker = host.Tracker(s.api, 3, 2)
    rng = np.random.default_rng(9)
    n = 150
    base = scenes[0].on_body_keypoints(n, seed=9)
    descriptors = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for s in scenes:
        s.texture.SetFeatures(base, descriptors)
        assert s.tracker.StartModalities(0)
    renewed = False
    before = os.environ.get("M3T_HIP_TEXTURE_MATCH")
    try:
        for frame in range(6):
            os.environ["M3T_HIP_TEXTURE_MATCH"] = (TILED, ONE)[frame % 2]
            if frame == 4:
                pose = _rotated(scenes[0].body.body2world_pose(), 12.0)
                for s in scenes:
                    s.body.set_body2world_pose(pose)
            count = n - 10 * frame if frame != 4 else 0
            order = rng.permutation(n)[:count]
            xy = (base[order] + rng.uniform(-2, 2, (count, 2))).astype(F)
            for s in scenes:
                s.texture.SetFeatures(xy, descriptors[order])
                assert s.tracker.ExecuteTrackingStep(frame)
            a = scenes[0]
            points = a.texture.points()
            assert len(points) > 20 or frame == 4
            age_a, keys_a = a.texture.keyframes()
            for b in scenes[1:]:
                assert a.body.body2world_pose().tobytes() == b.body.body2world_pose().tobytes(), frame
                _same_points(points, b.texture.points())
                age_b, keys_b = b.texture.keyframes()
                assert age_a == age_b and len(keys_a) == len(keys_b)
                for x, y in zip(keys_a, keys_b):
                    assert x.tobytes() == y.tobytes()
            renewed = renewed or len(keys_a) == 2
    finally:
        if before is None:
            os.environ.pop("M3T_HIP_TEXTURE_MATCH", None)
        else:
            os.environ["M3T_HIP_TEXTURE_MATCH"] = before
    assert renewed


# ---- which kernels a setting launches -----------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import util
from test_gpu_texture_modality import Scene
s = Scene(util.open_hip())
xy = s.on_body_keypoints(70, seed=1)
rows = np.random.default_rng(1).integers(0, 256, (70, 32), dtype=np.uint8)
s.texture.SetFeatures(xy, rows)
assert s.tracker.StartModalities(0)
assert s.tracker.CalculateCorrespondences(0, 0) and s.tracker.CalculateCorrespondences(0, 1) and s.tracker.Sync()
print("points", len(s.texture.points()))
"""


@pytest.mark.parametrize("setting, launched", [
    ("one", {"texture_match_kernel": 2}),
    ("tiled", {"texture_match_tiled_kernel": 1, "texture_collect_kernel": 2}),
    (None, {"texture_match_tiled_kernel": 1, "texture_collect_kernel": 2}),   # the default is the tiled form
    ("ONE", {"texture_match_tiled_kernel": 1, "texture_collect_kernel": 2}),  # an unknown text is "auto"
])
def test_the_override_decides_which_kernels_a_process_launches(setting, launched):
    """a child process makes one context under the setting and runs two correspondence searches (corr_iteration 0 and
    1); the HIP runtime logs every launch with the kernel's name (AMD_LOG_LEVEL=3), and the matcher's kernels in that
    log are exactly the form's: the one-workgroup kernel at both iterations, or the tiled match once and the collect
    kernel twice.  This is what keeps the twin-context comparisons of this file from comparing a form with itself"""
    env = dict(os.environ, AMD_LOG_LEVEL="3")
    env.pop("M3T_HIP_TEXTURE_MATCH", None)
    if setting is not None:
        env["M3T_HIP_TEXTURE_MATCH"] = setting
    tests = os.path.dirname(os.path.abspath(__file__))
    child = subprocess.run([sys.executable, "-c", _CHILD % (util.ROOT, tests)], env=env, capture_output=True, text=True, timeout=120,
                           cwd=util.ROOT)
    assert child.returncode == 0 and "points 70" in child.stdout, child.stdout + child.stderr[-2000:]
    names = re.findall(r"ShaderName : (\w+)", child.stderr)
    assert "texture_keyframe_kernel" in names, "the runtime's log names no kernel: " + child.stderr[-2000:]
    matcher = {n: names.count(n) for n in ("texture_match_kernel", "texture_match_tiled_kernel", "texture_collect_kernel")
               if n in names}
    assert matcher == launched, (setting, matcher)
