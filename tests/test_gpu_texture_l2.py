"""The texture modality with L2-norm descriptors on the device (csrc/m3t_texture_l2.hip behind
m3t_hip_texture_modality_create_l2) against its scalar np.float32 restatement (tests/texture_l2_reference.py), bit for
bit in the data points (count, order, all ten floats), the keyframes and g/H: descriptors of 4, 128, 200 and 256 floats
at the sizes around the kernel's tiles, several keyframes with an empty one among them, duplicated rows, two sums that
round to one distance, NaN rows, all-equal rows, a ratio exactly at the threshold, a Hamming and an L2 modality in one
context, the refusals, and two tracking steps against a restatement-driven loop.  The scene and the comparisons are
those of tests/test_gpu_texture_modality.py; descriptors come from a seeded generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_scene as gs
import texture_l2_reference as L
import util
from test_generator import reference_tree
from test_gpu_texture_generator import CONFIG
from test_gpu_texture_modality import Scene, _keyframes_equal, _oracle_stand_in, _points_equal
from util import host

pytestmark = pytest.mark.gpu
mtv = gs.mtv
F = np.float32


def _header_constant(name):
    text = open(os.path.join(util.ROOT, "3dobjecttracking_amd", "csrc", "m3t_texture.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


QUERY_TILE = _header_constant("M3T_TEXTURE_L2_QUERY_TILE")  # queries per workgroup
TRAIN_TILE = _header_constant("M3T_TEXTURE_L2_TRAIN_TILE")  # train rows per pass of a workgroup: ROWS for each of four waves
ROWS = _header_constant("M3T_TEXTURE_L2_ROWS")


def _scene(api, n_floats, **params):
    return Scene(api, descriptor_norm="l2", descriptor_bytes=4 * n_floats, **params)


def _state(s):
    state = s.state()
    state.__class__ = L.TextureStateL2
    return state


def _feed(s, state, keypoints, descriptors):
    s.texture.SetFeatures(keypoints, descriptors)
    state.set_features(keypoints, descriptors)


def _keyframe(s, state, keypoints, descriptors):
    _feed(s, state, keypoints, descriptors)
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    assert len(state.points_keyframes[-1]) == len(keypoints)  # every keypoint is on the body


def _match(s, state, train_xy, train):
    _feed(s, state, train_xy, train)
    assert s.tracker.CalculateCorrespondences(0, 0)
    state.calculate_correspondences(s.body.body2world_pose(), s.cam, 0)
    _points_equal(s.texture.points(), state.data_points)
    _keyframes_equal(s.texture, state)


def _gradient_hessian_equal(s, state, corr_iteration):
    assert s.tracker.CalculateGradientAndHessian(0, corr_iteration, 0)
    g, h = state.gradient_hessian(s.body.body2world_pose(), s.cam, corr_iteration)
    dg, dh = s.texture.gradient_hessian()
    assert np.array_equal(dg.view(np.uint32), g.view(np.uint32)) and np.array_equal(dh.view(np.uint32), h.view(np.uint32))
    _points_equal(s.texture.points(), state.data_points)


def _descriptors(rng, n_query, n_train, n_floats, integer):
    """train rows at random; even queries a train row moved a little (kept by the ratio test), odd ones random (two
    random rows are about equally far: rejected at 128 floats and more)"""
    train = L.seeded_rows(rng, n_train, n_floats, integer)
    queries = L.seeded_rows(rng, n_query, n_floats, integer)
    for q in range(0, n_query, 2):
        if n_train:
            queries[q] = train[(q * 7) % n_train]
            k = (q + 5) % n_floats
            queries[q, k] = queries[q, k] + F(1.0) if integer else queries[q, k] * F(0.75)
    return queries, train


# ---- 1. matcher: every size around the tiles -----------------------------------------------------------------------------
TRAIN_SIZES = sorted({0, 1, 2, ROWS - 1, ROWS, ROWS + 1, TRAIN_TILE - 1, TRAIN_TILE, TRAIN_TILE + 1, 2 * TRAIN_TILE + 1})
QUERY_SIZES = sorted({1, 2, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1, 2 * QUERY_TILE + 2})


@pytest.mark.parametrize("n_floats", [4, 128, 200, 256])
def test_matcher_equals_the_restatement_at_every_size(n_floats):
    integer = n_floats == 128  # what OpenCV's SIFT writes; uniform floats at the other widths
    api = util.open_hip()
    s = _scene(api, n_floats, descriptor_distance_threshold=0.75)
    keypoints = s.on_body_keypoints(max(QUERY_SIZES), seed=1)
    rng = np.random.default_rng(5)
    kept = rejected = 0
    for n_query, n_train in [(5, n) for n in TRAIN_SIZES] + [(n, TRAIN_TILE + 1) for n in QUERY_SIZES]:
        queries, train = _descriptors(rng, n_query, n_train, n_floats, integer)
        train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
        state = _state(s)
        _keyframe(s, state, keypoints[:n_query], queries)
        _match(s, state, train_xy, train)
        assert n_train >= 2 or len(state.data_points) == 0  # fewer than two train descriptors: no match
        kept += len(state.data_points)
        rejected += n_query - len(state.data_points)
        if n_query > QUERY_TILE and n_floats >= 128:
            assert 0 < len(state.data_points) < n_query
        if n_query == QUERY_TILE + 1:  # features survive the round trip as floats
            xy, rows = s.texture.features()
            assert rows.dtype == np.float32 and rows.tobytes() == train.tobytes() and np.array_equal(xy, train_xy)
            _gradient_hessian_equal(s, state, 0)
    assert kept > 20 and rejected > 20


def test_three_keyframes_one_of_them_empty_and_later_iterations_only_project():
    api = util.open_hip()
    s = _scene(api, 128, n_keyframes=3)
    counts = (QUERY_TILE + 1, 0, 3)
    keypoints = s.on_body_keypoints(max(counts), seed=2)
    rng = np.random.default_rng(6)
    state = _state(s)
    n_train = 2 * TRAIN_TILE + 3
    train = L.seeded_rows(rng, n_train, 128, True)
    for k, n_query in enumerate(counts):  # every keyframe descriptor has a near twin among the train rows
        queries = train[(np.arange(n_query) * 5 + k) % n_train].copy()
        queries[:, 7] += F(2.0)
        _keyframe(s, state, keypoints[:n_query], queries)
    assert [len(p) for p in state.points_keyframes] == list(counts)
    train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
    _match(s, state, train_xy, train)
    assert len(state.data_points) == sum(counts)  # across the query tiles of the first keyframe, then the third's
    _gradient_hessian_equal(s, state, 0)
    # a fourth keyframe pops the oldest; at corr_iteration > 0 the points are projected at the new pose and kept
    _keyframe(s, state, keypoints[:QUERY_TILE - 1], train[:QUERY_TILE - 1])
    assert [len(p) for p in state.points_keyframes] == [0, 3, QUERY_TILE - 1]
    _keyframes_equal(s.texture, state)
    pose = s.body.body2world_pose()
    pose[:3, 3] += np.array([0.002, -0.001, 0.003], F)
    s.body.set_body2world_pose(pose)
    assert s.tracker.CalculateCorrespondences(0, 1)
    state.calculate_correspondences(pose, s.cam, 1)
    assert len(state.data_points) == sum(counts)
    _points_equal(s.texture.points(), state.data_points)
    _gradient_hessian_equal(s, state, 1)
    _match(s, state, train_xy, train)  # and a new match sees the three keyframes the ring holds now
    assert len(state.data_points) == 3 + QUERY_TILE - 1


# ---- 2. the rule at its edges -------------------------------------------------------------------------------------------
def _far_rows(rng, n, n_floats):
    return (F(5000.0) + F(100.0) * L.seeded_rows(rng, n, n_floats, True)).astype(F)


def test_duplicated_rows_the_lower_index_wins():
    api = util.open_hip()
    s = _scene(api, 200, descriptor_distance_threshold=0.75)
    rng = np.random.default_rng(7)
    n_train = 4 * TRAIN_TILE + 5  # ranges of 40 rows a wave
    train = L.seeded_rows(rng, n_train, 200, False)
    pairs = [(3, 5), (ROWS - 1, ROWS), (10, 39 + 2), (39, 40), (50, 3 * 40 + 7), (131, 132)]  # within a pass, across
    for a, b in pairs:                                                                      # passes, across waves
        train[b] = train[a]
    queries = np.stack([train[a] for a, _ in pairs] + [train[a] * F(0.5) + train[60] * F(0.5) for a, _ in pairs])
    keypoints = s.on_body_keypoints(len(queries), seed=3)
    state = _state(s)
    _keyframe(s, state, keypoints, queries)
    train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
    _match(s, state, train_xy, train)
    # the first six queries: d0 = d1 = 0 (0 / 0: kept) with the lower of the two indexes; the other six: d0 = d1 > 0,
    # a ratio of 1 -- dropped
    assert len(state.data_points) == len(pairs)
    for p, (a, _) in zip(state.data_points, pairs):
        assert np.array_equal(p["correspondence_center"], train_xy[a])


def test_two_sums_that_round_to_one_distance_rank_by_index():
    api = util.open_hip()
    s = _scene(api, 4, descriptor_distance_threshold=1.5)  # (a ratio of 1 is kept: the best index shows)
    rng = np.random.default_rng(8)
    keypoints = s.on_body_keypoints(2, seed=4)
    for first, second in ((3, 20), (20, 3), (ROWS - 1, ROWS), (5, 2 * TRAIN_TILE)):
        n_train = 2 * TRAIN_TILE + 2
        train = _far_rows(rng, n_train, 4)
        train[first] = [2000, 2000, 1, 0]    # s = 8 000 001
        train[second] = [2000, 2000, 0, 0]   # s = 8 000 000: the same distance in f32
        state = _state(s)
        _keyframe(s, state, keypoints, np.zeros((2, 4), F))
        sums = [L.l2_squared(np.zeros(4, F), train[i]) for i in (first, second)]
        assert sums[0] != sums[1] and np.sqrt(sums[0]) == np.sqrt(sums[1])
        train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
        _match(s, state, train_xy, train)
        assert len(state.data_points) == 2
        assert np.array_equal(state.data_points[0]["correspondence_center"], train_xy[min(first, second)])


def test_nan_rows_all_equal_rows_and_a_ratio_exactly_at_the_threshold():
    api = util.open_hip()
    s = _scene(api, 4, descriptor_distance_threshold=0.75)
    rng = np.random.default_rng(9)
    keypoints = s.on_body_keypoints(6, seed=5)
    n_train = TRAIN_TILE + 3
    train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
    # NaN rows among the train descriptors (never a match), a NaN query (no match at all), rows whose sum overflows
    train = _far_rows(rng, n_train, 4)
    train[0] = np.nan
    train[9, 2] = np.nan
    train[4] = [1, 0, 0, 0]
    train[12] = [3e38, 3e38, 0, 0]
    queries = np.zeros((3, 4), F)
    queries[1] = np.nan
    queries[2] = [0, 0, 0, -3e38]
    state = _state(s)
    _keyframe(s, state, keypoints[:3], queries)
    _match(s, state, train_xy, train)
    assert len(state.data_points) == 2  # the zero query: row 4; the huge one: every distance inf, inf / inf kept, row 1
    assert np.array_equal(state.data_points[0]["correspondence_center"], train_xy[4])
    assert np.array_equal(state.data_points[1]["correspondence_center"], train_xy[1])
    # one train row beside NaN rows: fewer than two entries, no match
    lonely = np.full((n_train, 4), np.nan, F)
    lonely[TRAIN_TILE + 1] = [1, 0, 0, 0]
    _match(s, state, train_xy, lonely)
    assert len(state.data_points) == 0
    # all-equal descriptors: 0 / 0 is kept, the first train row is the best of every query
    state = _state(s)
    _keyframe(s, state, keypoints, np.ones((6, 4), F))
    _match(s, state, train_xy, np.ones((n_train, 4), F))
    assert len(state.data_points) == 6
    assert all(np.array_equal(p["correspondence_center"], train_xy[0]) for p in state.data_points)
    # 3 / 4 is the threshold exactly: dropped; one float below it: kept
    train = _far_rows(rng, n_train, 4)
    train[20] = [4, 0, 0, 0]
    train[TRAIN_TILE + 2] = [3, 0, 0, 0]
    state = _state(s)
    _keyframe(s, state, keypoints[:2], np.zeros((2, 4), F))
    _match(s, state, train_xy, train)
    assert len(state.data_points) == 0
    train[TRAIN_TILE + 2, 0] = np.nextafter(F(3.0), F(0.0))
    _match(s, state, train_xy, train)
    assert len(state.data_points) == 2


# ---- 3. Hamming and L2 in one context -------------------------------------------------------------------------------------
def test_a_hamming_body_beside_an_l2_body_equals_the_hamming_body_alone():
    n = 150

    def run(api, kinds):
        scenes, later, out = [], [], {}
        for kind in kinds:
            rng = np.random.default_rng(40)
            if kind == "l2":
                s = _scene(api, 128)
                descriptors = L.seeded_rows(rng, n, 128, True)
            else:
                s = Scene(api, descriptor_bytes=32)
                descriptors = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            keypoints = s.on_body_keypoints(n, seed=41)
            s.texture.SetFeatures(keypoints, descriptors)
            order = rng.permutation(n)
            later.append(((keypoints + rng.uniform(-6, 6, keypoints.shape)).astype(F)[order], descriptors[order]))
            scenes.append(s)
        tracker = host.Tracker(api, 2, 2)
        assert tracker.StartModalities(0)
        for s, (keypoints, descriptors) in zip(scenes, later):
            s.texture.SetFeatures(keypoints, descriptors)
        assert tracker.ExecuteTrackingStep(0)
        for kind, s in zip(kinds, scenes):
            assert len(s.texture.points()) == n  # every keyframe point found its feature
            out[kind] = (s.texture.points().copy(), s.body.body2world_pose())
        return out

    both = run(util.open_hip(), ("hamming", "l2"))
    swapped = run(util.open_hip(), ("l2", "hamming"))
    for kind in ("hamming", "l2"):
        alone = run(util.open_hip(), (kind,))[kind]
        for got in (both[kind], swapped[kind]):
            assert np.array_equal(got[0], alone[0]) and got[0].tobytes() == alone[0].tobytes()
            assert np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32))
        assert not np.array_equal(alone[1], mtv.body2world())


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    capi = util.pkg._capi
    api = util.open_hip()
    s = _scene(api, 128)
    rng = np.random.default_rng(10)
    keypoints = s.on_body_keypoints(40, seed=6)
    rows = L.seeded_rows(rng, 40, 128, True)
    state = _state(s)
    _keyframe(s, state, keypoints, rows)
    _match(s, state, keypoints, rows)
    points, pose = s.texture.points().copy(), s.body.body2world_pose()
    assert len(points) == 40
    # the built-in detector writes 32-byte binary descriptors
    detector = capi.TextureDetectorParams()
    assert api.raw("texture_modality_set_detector", s.texture.id, C.byref(detector)) == capi.M3T_ERR_UNSUPPORTED
    assert "32-byte" in api.last_error()
    with pytest.raises(capi.M3TError):
        s.texture.SetDetector(n_features=100)
    assert s.texture.detector is None
    # ... and is refused on an L2 modality of 8 floats too, whose rows are as long as that detector's descriptors
    narrow = host.TextureModality(api, s.body, s.color_camera, s.sil, descriptor_norm="l2", descriptor_bytes=32)
    assert api.raw("texture_modality_set_detector", narrow.id, C.byref(detector)) == capi.M3T_ERR_UNSUPPORTED
    assert "L2 norm" in api.last_error()
    narrow.SetFeatures(keypoints[:3], np.ones((3, 8), F))  # (still fed by the caller: a set detector would refuse this)
    xy, narrow_rows = narrow.features()
    assert np.array_equal(xy, keypoints[:3]) and np.array_equal(narrow_rows, np.ones((3, 8), F))
    # rows of another size or type never reach the library
    for bad in (np.zeros((40, 127), F), np.zeros((40, 512), np.uint8), np.zeros((40, 128), np.float64)):
        with pytest.raises(ValueError):
            s.texture.SetFeatures(keypoints, bad)
    # what is refused for a caller-fed modality stays refused
    ids = np.array([s.body.id], np.int32)
    poses = capi.pose_arg(np.eye(4)).copy()
    opt = np.array([0], np.int32)
    row = C.c_int()
    judge = host.Judge(api, [s.body], 4)
    refused = [api.raw("reset_bodies", capi.iptr(ids), capi.fptr(poses), 1, 0),
               api.raw("reset_structures", capi.iptr(opt), 1, capi.fptr(poses), 0, 0),
               api.raw("judge_bodies", judge.id, capi.fptr(poses), 0, C.byref(row)),
               api.raw("set_roi_ingest", 1, 4.0),
               api.raw("comm_set", C.c_void_p(8))]
    assert refused == [capi.M3T_ERR_UNSUPPORTED] * len(refused), refused
    assert np.array_equal(s.body.body2world_pose(), pose)
    assert s.tracker.CalculateCorrespondences(0, 0)  # the features, the keyframe and the matcher are where they were
    assert np.array_equal(s.texture.points(), points)
    xy, kept_rows = s.texture.features()
    assert np.array_equal(xy, keypoints) and kept_rows.tobytes() == rows.tobytes()
    # descriptor_bytes: 4 * D with D a multiple of 4 in [4, 256]; the Hamming entry point keeps its two sizes
    for bad in (0, 8, 12, 20, 1028, 2048, -16):
        with pytest.raises(capi.M3TError) as e:
            host.TextureModality(api, s.body, s.color_camera, s.sil, descriptor_norm="l2", descriptor_bytes=bad)
        assert e.value.code == capi.M3T_ERR_INVALID_ARGUMENT and "multiple of 16" in str(e.value)
    for good in (16, 1024):
        host.TextureModality(api, s.body, s.color_camera, s.sil, descriptor_norm="l2", descriptor_bytes=good)
    with pytest.raises(capi.M3TError) as e:
        host.TextureModality(api, s.body, s.color_camera, s.sil, descriptor_bytes=512)
    assert "Hamming-norm descriptors only" in str(e.value)


# ---- 5. two tracking steps -------------------------------------------------------------------------------------------------
def test_two_tracking_steps_equal_a_restatement_driven_loop():
    api = util.open_hip()
    s = _scene(api, 128, n_keyframes=2, max_keyframe_age=1)
    ora = _oracle_stand_in()
    s.tracker = host.Tracker(api, 4, 2)
    state = _state(s)
    rng = np.random.default_rng(12)
    n = 2 * QUERY_TILE + 10
    base = s.on_body_keypoints(n, seed=7)
    rows = L.seeded_rows(rng, n, 128, True)
    _keyframe(s, state, base, rows)
    renewals = []
    for frame in range(2):
        count = n - 15 * frame
        order = rng.permutation(n)[:count]
        xy = (base[order] + rng.uniform(-2, 2, (count, 2))).astype(F)
        noisy = np.clip(rows[order] + rng.integers(-2, 3, (count, 128)).astype(F), 0, 255).astype(F)
        _feed(s, state, xy, noisy)
        assert s.tracker.ExecuteTrackingStep(frame)
        pose = ora.body.body2world_pose()
        for corr_iteration in range(4):
            state.calculate_correspondences(pose, s.cam, corr_iteration)
            for update_iteration in range(2):
                g, h = state.gradient_hessian(pose, s.cam, corr_iteration)
                ora.stand_in.set_gradient_hessian(g, h)
                assert ora.tracker.CalculateOptimization(frame, corr_iteration, update_iteration)
                pose = ora.body.body2world_pose()
        assert len(state.data_points) > n // 2
        assert np.array_equal(s.body.body2world_pose().view(np.uint32), pose.view(np.uint32)), frame
        _points_equal(s.texture.points(), state.data_points)
        dg, dh = s.texture.gradient_hessian()  # of the step's last iteration
        assert np.array_equal(dg.view(np.uint32), g.view(np.uint32)) and np.array_equal(dh.view(np.uint32), h.view(np.uint32))
        due = state.renewal_due(pose, s.cam)
        renewals.append(due)
        if due:
            s.reference_keyframe(state, pose)
        _keyframes_equal(s.texture, state)
    assert renewals == [False, True]  # by age
    assert not np.array_equal(pose, mtv.body2world())


# ---- 6. a generated tracker with the caller's L2 detector ----------------------------------------------------------------
def test_generated_tracker_with_an_l2_stub_detector_equals_the_hand_built_context(tmp_path):
    """GenerateConfiguredTracker on a SIFT metafile with a callable that returns float32 rows (l2_descriptors=True):
    DetectFeatures -> SetFocusedFeatures -> the L2 matcher, against a hand-built context fed with the same features;
    then a frame without a valid region of interest, which leaves the modality without features"""
    generator = util.pkg.generator
    root = reference_tree(tmp_path)
    config = root / "tracker_test" / "texture_config.yaml"
    config.write_text(CONFIG)
    (root / "tracker_test" / "texture_modality.yaml").write_text(
        '%YAML:1.2\ndescriptor_type: "SIFT"\nn_keyframes: 2\nsift_n_features: 200\ntukey_norm_constant: 15.0\n')
    hand_api = util.open_hip()
    body = host.Body(hand_api)
    tv, tf = util.pkg.config.load_obj(util.GOLDEN + "/_body/triangle.obj")
    body.set_geometry(tv, tf, np.asarray(mtv.GEOMETRY2BODY, F), body_id=150, region_id=150)
    camera = host.ColorCamera(hand_api, **mtv.COLOR_INTRINSICS)
    geometry = host.RendererGeometry(hand_api)
    geometry.AddBody(body)
    renderer = host.FocusedSilhouetteRenderer(hand_api, geometry, camera, id_type=0)
    renderer.AddReferencedBody(body)
    texture = host.TextureModality(hand_api, body, camera, renderer, descriptor_norm="l2", descriptor_bytes=512,
                                   n_keyframes=2, tukey_norm_constant=15.0)
    link = host.Link(hand_api, body)
    link.AddModality(texture)
    host.Optimizer(hand_api, link)
    body.set_body2world_pose(mtv.body2world())
    hand_tracker = host.Tracker(hand_api)
    roi, scale = texture.RegionOfInterest()
    renderer.StartRendering()
    _, silhouette, corner_u, corner_v, render_scale, _ = renderer.images()
    vs, us = np.nonzero(silhouette == 150)
    rng = np.random.default_rng(14)
    pick = rng.permutation(len(vs))[:200]
    full = np.stack([F(corner_u) + us[pick].astype(F) / F(render_scale), F(corner_v) + vs[pick].astype(F) / F(render_scale)], 1)
    focused = ((full - np.array(roi[:2], F)) * scale).astype(F)
    rows = L.seeded_rows(rng, 200, 128, True)
    planted = [(focused, rows), ((focused[:150] + rng.uniform(-3, 3, (150, 2))).astype(F), rows[:150])]
    calls = []

    def detector(image, roi, scale, params):
        assert image.shape == (540, 960, 3) and params == {"descriptor_type": "SIFT", "sift_n_features": 200}
        calls.append((roi, scale))
        return planted[len(calls) - 1]

    api = util.open_hip()
    tracker = generator.GenerateConfiguredTracker(api, str(config), feature_detector=detector, pass_detector_params=True,
                                                  l2_descriptors=True)
    generated_body = tracker.objects["Body"]["triangle"]
    generated_body.set_body2world_pose(mtv.body2world())
    assert tracker.SetUp() and tracker.StartModalities(0) and tracker.ExecuteTrackingStep(0)
    assert len(calls) == 2 and calls[0] == (roi, scale)
    generated = tracker.objects["TextureModality"]["triangle_texture_modality"]
    assert (generated.params.descriptor_bytes, generated.descriptor_norm, generated.params.n_keyframes) == (512, "l2", 2)
    for step, (keypoints, descriptors) in enumerate(planted):
        texture.SetFocusedFeatures(*texture.RegionOfInterest(), keypoints, descriptors)
        assert hand_tracker.StartModalities(0) if step == 0 else hand_tracker.ExecuteTrackingStep(0)
    pose = body.body2world_pose()
    assert np.array_equal(generated_body.body2world_pose().view(np.uint32), pose.view(np.uint32))
    assert not np.array_equal(pose, mtv.body2world())
    points = texture.points()
    assert len(points) > 100 and np.array_equal(generated.points(), points)
    assert generated.keyframes()[0] == texture.keyframes()[0]
    assert all(np.array_equal(a, b) for a, b in zip(generated.keyframes()[1], texture.keyframes()[1]))
    held = generated.features()[1]
    assert held.dtype == np.float32 and held.tobytes() == planted[1][1].tobytes()
    # a detector that answers with rows of bytes is stopped at the modality, before the library is called
    calls.clear()
    planted[0] = (focused, np.zeros((200, 512), np.uint8))
    with pytest.raises(ValueError, match="float32"):
        tracker.DetectFeatures()
    assert generated.features()[1].tobytes() == held.tobytes()
    # too close to the camera: no region of interest, the detector is not asked and the modality holds no features
    calls.clear()
    close = mtv.body2world()
    close[:3, 3] = [0.0, 0.0, 0.02]
    generated_body.set_body2world_pose(close)
    assert generated.RegionOfInterest() is None
    tracker.DetectFeatures()
    xy, none = generated.features()
    assert calls == [] and xy.shape == (0, 2) and none.shape == (0, 128) and none.dtype == np.float32
