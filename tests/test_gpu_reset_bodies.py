"""m3t_hip_reset_bodies (RBOTEvaluator::ResetBody for the lost bodies of a batch, and for no other) on the device:
the batch loop of tests/selective_reset.py with Tracker.ResetBodies against every object tracked in an oracle context
of its own -- poses after every step, the resets and the final histograms bit for bit, in every launch shape; that
the call leaves every other body alone; ROI ingest; the refused calls; and the batched dataset evaluator."""
import ctypes as C

import numpy as np
import pytest

import reset_loop
import scenes
import selective_reset as sr
import util
from test_gpu_reset_on_loss import KNOBS, RBOT64_CASES, YCB_CASES, kernel_of, shape_of

pytestmark = pytest.mark.gpu

capi = util.pkg._capi
fptr, iptr, pose_arg = capi.fptr, capi.iptr, capi.pose_arg


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def hip_loop(monkeypatch, inputs, env, instance_kw=None, fused=None, iteration_is_frame=False):
    """the batch loop with ResetBodies on the device, launch knobs `env`; returns (result, kernel per step, shape)"""
    set_knobs(monkeypatch, env)
    api = util.open_hip()
    kernels = []
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    out = sr.run_batch(api, inputs, schedule, "bodies", instance_kw=instance_kw, iteration_is_frame=iteration_is_frame,
                       setup=(lambda inst: api.call("set_fused_step", fused)) if fused is not None else None,
                       after_step=lambda inst, k: kernels.append(kernel_of(api)))
    return out, kernels, shape_of(api)


def expect(inputs, **kw):
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    sr.check_schedule(schedule, inputs.n_objects, inputs.n_frames)
    return sr.expectation(inputs, schedule, **kw)


def raw_reset(api, ids, poses=None, n=None, iteration=0):
    ids = np.asarray(ids, np.int32)
    flat = None if poses is None else np.ascontiguousarray(np.concatenate([pose_arg(p) for p in poses]), np.float32)
    return api.raw("reset_bodies", iptr(ids), fptr(flat) if flat is not None else None, len(ids) if n is None else n,
                   iteration)


# ---- the benchmarked batch: 64 Region objects, 18 models of 2562 views ------------------------------------------------
@pytest.fixture(scope="module")
def rbot64():
    return scenes.Inputs(64, 8, n_divides=4, n_models=18)


@pytest.fixture(scope="module")
def rbot64_singles(rbot64):
    return expect(rbot64)


@pytest.mark.parametrize("case", list(RBOT64_CASES))
def test_rbot64_reset_bodies_match_the_single_runs(rbot64, rbot64_singles, case, monkeypatch):
    env, kernel, shape = RBOT64_CASES[case]
    got, kernels, got_shape = hip_loop(monkeypatch, rbot64, env)
    reset_loop.assert_same(got, rbot64_singles)
    assert 1 not in {i for _, i in got[1]}  # a body that is never lost rides along
    if kernel is not None:
        assert set(kernels) == {kernel}, kernels
    if shape is not None:
        assert got_shape == shape, got_shape
    if case.startswith("one workgroup"):
        assert all("split" not in k and "compact" not in k and k.startswith("tracking_step_") for k in kernels), kernels
    if case == "compact_table overflow":
        # (reset_bodies leaves the overflow latch alone: which kernel runs after a reset is not part of the contract)
        assert kernels[0] == "tracking_step_compact_table_kernel", kernels


def test_rbot64_unfused_reset_bodies_match_the_single_runs(rbot64, rbot64_singles, monkeypatch):
    """one launch per sub-step (set_fused_step 0)"""
    got, kernels, _ = hip_loop(monkeypatch, rbot64, {}, fused=0)
    reset_loop.assert_same(got, rbot64_singles)
    assert set(kernels) == {""}, kernels


def test_reset_bodies_leaves_every_other_body_alone(rbot64, monkeypatch):
    """two steps, then k of 64 bodies reset: the poses and histograms of the others are the same bits as before; those of
    the reset bodies are the poses handed in and the histograms of a fresh context started at that pose on that frame;
    and the next step moves the others exactly as in a context that never made the call"""
    set_knobs(monkeypatch, {})
    chosen = [3, 17, 40, 63]
    gt = reset_loop.ground_truth(rbot64, [(2, i, "a") for i in chosen])
    insts = [scenes.Instance(util.open_hip(), rbot64) for _ in range(2)]
    for inst in insts:
        inst.upload_frame(0)
        assert inst.tracker.StartModalities(0)
        for k in (1, 2):
            inst.upload_frame(k)
            assert inst.tracker.ExecuteTrackingStep(k)
    inst, twin = insts
    poses_before, hist_before = np.stack(inst.poses()), [r.histograms() for r in inst.region]
    assert inst.tracker.ResetBodies([inst.bodies[i] for i in chosen], [gt[2][i] for i in chosen], 0)
    poses_after, hist_after = np.stack(inst.poses()), [r.histograms() for r in inst.region]
    for i in range(rbot64.n_objects):
        if i in chosen:
            continue
        assert np.array_equal(poses_after[i], poses_before[i]), i
        assert np.array_equal(hist_after[i][0], hist_before[i][0]) and np.array_equal(hist_after[i][1], hist_before[i][1]), i
    for i in chosen:
        assert np.array_equal(poses_after[i], gt[2][i]), i
        fresh = scenes.Instance(util.open_hip(), sr.single_inputs(rbot64, i))
        fresh.bodies[0].set_body2world_pose(gt[2][i])
        fresh.color_cams[0].UpdateImage(rbot64.color[i][2])
        assert fresh.tracker.StartModalities(0)
        f, b = fresh.region[0].histograms()
        assert np.array_equal(hist_after[i][0], f) and np.array_equal(hist_after[i][1], b), i
        assert not np.array_equal(hist_after[i][0], hist_before[i][0]), i
    # poses == NULL: the poses stay, the histograms are initialised at them
    assert inst.tracker.ResetBodies([inst.bodies[5]], None, 0)
    again = np.stack(inst.poses())
    assert np.array_equal(again, poses_after)
    assert not np.array_equal(inst.region[5].histograms()[0], hist_after[5][0])
    for k in (3, 4):
        for x in insts:
            x.upload_frame(k)
            assert x.tracker.ExecuteTrackingStep(k)
        a, b = np.stack(inst.poses()), np.stack(twin.poses())
        for i in range(rbot64.n_objects):
            if i not in chosen and i != 5:
                assert np.array_equal(a[i], b[i]), (k, i)
    ha, hb = [r.histograms() for r in inst.region], [r.histograms() for r in twin.region]
    for i in range(rbot64.n_objects):
        if i not in chosen and i != 5:
            assert np.array_equal(ha[i][0], hb[i][0]) and np.array_equal(ha[i][1], hb[i][1]), i


@pytest.mark.parametrize("n_bins", [16, 64])
def test_both_histogram_placements(n_bins, monkeypatch):
    """the list-driven start with the count table in LDS (16 bins: the step kernel also stages the histograms in LDS)
    and with the 64-bin count table in HBM (262144 bins do not fit the LDS of a CU)"""
    inputs = scenes.Inputs(6, 7, n_divides=2)
    kw = dict(region_params=dict(util.syn.RBOT_REGION_PARAMS, n_histogram_bins=n_bins))
    got, kernels, _ = hip_loop(monkeypatch, inputs, {"M3T_HIP_NO_SPLIT": "1"}, instance_kw=kw)
    reset_loop.assert_same(got, expect(inputs, instance_kw=kw))
    assert got[2][0][0].size == n_bins ** 3
    assert all(k.startswith("tracking_step_") for k in kernels), kernels


# ---- ycb shape: 21 Region + Depth objects -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ycb21():
    return scenes.Inputs(21, 5, n_divides=4, n_models=6, with_depth=True)


@pytest.fixture(scope="module")
def ycb21_singles(ycb21):
    return expect(ycb21, instance_kw=dict(use_depth=True))


@pytest.mark.parametrize("case", ["split_pair", "lds_pair", "compact_wide"])
def test_ycb21_reset_bodies_match_the_single_runs(ycb21, ycb21_singles, case, monkeypatch):
    env, kernel = YCB_CASES[case]
    got, kernels, _ = hip_loop(monkeypatch, ycb21, env, instance_kw=dict(use_depth=True))
    reset_loop.assert_same(got, ycb21_singles)
    assert set(kernels) == {kernel}, kernels


# ---- mixed: Region + Depth, Region only, Depth only in one context ----------------------------------------------------
@pytest.fixture(scope="module")
def mixed_inputs():
    return scenes.Inputs(9, 5, n_divides=4, n_models=3, with_depth=True)


def test_mixed_batch_reset_bodies_match_the_single_runs(mixed_inputs, monkeypatch):
    kw = dict(kinds=["rd", "r", "d"] * 3)
    got, kernels, _ = hip_loop(monkeypatch, mixed_inputs, {}, instance_kw=kw)
    reset_loop.assert_same(got, expect(mixed_inputs, instance_kw=kw))
    assert {i for _, i in got[1]} >= {4, 8}  # a Region-only and a Depth-only body were reset
    assert set(kernels) == {"tracking_step_split_pair_kernel"}, kernels


def test_first_iteration_follows_the_reset_bodies_alone(mixed_inputs, monkeypatch):
    """Region + Depth with n_unoccluded_iterations = 2 and the restart's iteration = the frame index: a reset body
    tracks its next frame without the occlusion test (iteration - first_iteration = 1 < 2), every other body with it
    -- as each does in a context of its own; a batch-wide first_iteration would switch the test off for all"""
    kw = dict(use_depth=True, region_params=dict(util.syn.YCB_REGION_PARAMS, n_unoccluded_iterations=2))
    ref = expect(mixed_inputs, instance_kw=kw, iteration_is_frame=True)
    got, _, _ = hip_loop(monkeypatch, mixed_inputs, {}, instance_kw=kw, iteration_is_frame=True)
    reset_loop.assert_same(got, ref)


# ---- ROI ingest -------------------------------------------------------------------------------------------------------
def roi_loop(inputs, schedule, with_depth):
    """the batch loop in rectangle mode (ring of two slots, the rectangles of frame k + 1 enqueued behind step k, as
    test_gpu_reset_on_loss.roi_loop): ResetBodies is refused while the lost bodies' cameras hold rectangles, and runs
    once THEIR whole frames -- no other camera's -- are in the slot"""
    hip = util.open_hip()
    n = inputs.n_objects
    rings, kernels, refused = [], [], [0]

    def upload(slot, k):
        for _, ids, blocks in rings:
            b = blocks[k]
            hip.call("cameras_upload_batch_roi_async", ids, n, slot, b.ctypes.data_as(C.c_void_p), b.strides[0],
                     b.strides[1])

    def frame(inst, k):
        if k == 1:
            groups = [(inst.color_cams, inputs.color, 3, np.uint8)]
            if with_depth:
                groups.append((inst.depth_cams, inputs.depth, 1, np.uint16))
            for cams, frames, channels, dtype in groups:
                h, w = frames[0][0].shape[:2]
                blocks = []
                for j in range(inputs.n_frames):
                    b = np.zeros((n, h, w * channels), dtype)
                    for i in range(n):
                        b[i] = frames[i][j].reshape(h, w * channels)
                    inst.tracker.register_host_buffer(b)
                    blocks.append(b)
                ids = (C.c_int * n)(*[cam.id for cam in cams])
                hip.call("cameras_set_ring", ids, n, 2)
                rings.append((cams, ids, blocks))
            upload(1, 1)
        inst.tracker.select_slot(k % 2)

    def after_step(inst, k):
        kernels.append(kernel_of(hip))
        if k + 1 < inputs.n_frames:
            upload((k + 1) % 2, k + 1)

    def before_reset(inst, k, lost):
        if k == 1:  # (the frame of the first step went whole: no step had been recorded to cut rectangles from)
            return
        gt = reset_loop.ground_truth(inputs, schedule)
        before = np.stack(inst.poses())
        rc = raw_reset(hip, [inst.bodies[i].id for i in lost], [gt[k][i] for i in lost])
        assert rc == capi.M3T_ERR_UNSUPPORTED, rc
        assert "ROI ingest" in hip.last_error(), hip.last_error()
        assert np.array_equal(np.stack(inst.poses()), before)  # the refused call changed nothing
        refused[0] += 1
        for cams, _, blocks in rings:
            for i in lost:
                f = blocks[k][i]
                hip.call("camera_upload_slot", cams[i].id, k % 2, f.ctypes.data_as(C.c_void_p), f.strides[0])

    holder = {}

    def setup(inst):
        holder["inst"] = inst
        hip.call("set_roi_ingest", 1, C.c_float(24.0))

    got = sr.run_batch(hip, inputs, schedule, "bodies", instance_kw=dict(use_depth=with_depth), setup=setup, frame=frame,
                       after_step=after_step, before_reset=before_reset)
    holder["inst"].tracker.ingest_sync()
    bodies = (C.c_int * 64)()
    nu = C.c_int(0)
    hip.call("roi_get_unrecovered", bodies, 64, C.byref(nu))
    return got, sorted(set(bodies[:min(nu.value, 64)])), refused[0], kernels


@pytest.mark.parametrize("with_depth", [False, True])
def test_roi_ingest_with_reset_bodies(with_depth, monkeypatch):
    set_knobs(monkeypatch, {})
    inputs = scenes.Inputs(6, 6, n_divides=2, with_depth=True) if with_depth else scenes.Inputs(6, 7, n_divides=2)
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    ref = sr.expectation(inputs, schedule, instance_kw=dict(use_depth=with_depth))
    got, unrecovered, refused, kernels = roi_loop(inputs, schedule, with_depth)
    reset_loop.assert_same(got, ref)
    assert unrecovered == []
    assert all(k.endswith("_guard_kernel") for k in kernels[1:]), kernels  # the steps read rectangles
    assert refused == len({f for f, _ in got[1]} - {1}) and refused


# ---- refused calls ----------------------------------------------------------------------------------------------------
def _step_poses(inst, k):
    inst.upload_frame(k)
    assert inst.tracker.ExecuteTrackingStep(k)
    return np.stack(inst.poses())


def _build(api, inputs, variant):
    """three rigid bodies (scenes.Instance) and, beside them: "lone" a body without modalities; "chain" a structure
    of two links; "shared" a body whose RegionModality uses a shared ColorHistograms object"""
    host = util.host
    inst = scenes.Instance(api, inputs)
    rp = dict(util.syn.RBOT_REGION_PARAMS, measure_occlusions=0)
    if variant == "lone":
        inst.extra = host.Body(api, inputs.start[0])
    elif variant == "chain":
        bodies = [host.Body(api, inputs.start[i]) for i in range(2)]
        link_a = host.Link(api, body=bodies[0])
        link_b = host.Link(api, body=bodies[1], parent=link_a, free_directions=(0, 0, 1, 0, 0, 0))
        link_a.AddModality(host.RegionModality(api, bodies[0], inst.color_cams[0], inst.region_models[0], **rp))
        link_b.AddModality(host.RegionModality(api, bodies[1], inst.color_cams[1], inst.region_models[1], **rp))
        host.Optimizer(api, root_link=link_a)
        inst.extra = bodies[1]
    else:
        inst.extra = host.Body(api, inputs.start[2])
        shared = host.ColorHistograms(api, n_bins=32, learning_rate_f=0.3, learning_rate_b=0.1)
        modality = host.RegionModality(api, inst.extra, inst.color_cams[2], inst.region_models[2], **rp)
        modality.UseSharedColorHistograms(shared)
        host.Optimizer(api, body=inst.extra, modalities=[modality])
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    return inst


@pytest.mark.parametrize("variant", ["lone", "chain", "shared"])
def test_refused_calls_change_nothing(variant, monkeypatch):
    """every refused call returns its code and says why; the context then goes on exactly like a twin that never made
    the call"""
    set_knobs(monkeypatch, {})
    inputs = scenes.Inputs(3, 4, n_divides=2)
    pose = reset_loop.ground_truth(inputs, [(1, 0, "a")])[1][0]
    api = util.open_hip()
    inst, twin = _build(api, inputs, variant), _build(util.open_hip(), inputs, variant)
    assert np.array_equal(_step_poses(inst, 1), _step_poses(twin, 1))
    INVALID, UNSUPPORTED = capi.M3T_ERR_INVALID_ARGUMENT, capi.M3T_ERR_UNSUPPORTED
    n_bodies = len(inst.bodies) + (2 if variant == "chain" else 1)
    cases = {"lone": [("bad body id", INVALID, [0, n_bodies], None), ("bad body id", INVALID, [-1], None),
                      ("twice", INVALID, [0, 1, 0], None), ("negative", INVALID, [0], -1)],
             "chain": [("more than one link", UNSUPPORTED, [0, inst.extra.id], None)],
             "shared": [("shared ColorHistograms", UNSUPPORTED, [inst.extra.id, 1], None)]}[variant]
    for text, code, ids, n in cases:
        rc = raw_reset(api, ids, [pose] * len(ids), n=n)
        assert rc == code, (text, rc)
        assert text in api.last_error(), (text, api.last_error())
    assert raw_reset(api, [0], [pose], n=0) == 0  # nothing to do
    assert np.array_equal(np.stack(inst.poses()), np.stack(twin.poses()))
    for r, t in zip(inst.region, twin.region):
        assert np.array_equal(r.histograms()[0], t.histograms()[0]) and np.array_equal(r.histograms()[1], t.histograms()[1])
    assert np.array_equal(_step_poses(inst, 2), _step_poses(twin, 2))
    if variant == "lone":  # a body without modalities only gets its pose; everything else goes on as in the twin
        assert inst.tracker.ResetBodies([inst.extra], [pose], 0)
        assert np.array_equal(inst.extra.body2world_pose(), pose)
        assert np.array_equal(_step_poses(inst, 3), _step_poses(twin, 3))
        assert np.array_equal(inst.extra.body2world_pose(), pose)


# ---- the batched dataset evaluator ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    ev = util.pkg.evaluation
    n_frames = 8
    directory, external, names, model_parameters = sr.write_rbot_dataset(tmp_path_factory.mktemp("rbot_batched"), n_frames)
    args = (str(directory), str(external), names, ["a_regular"])
    kw = dict(n_frames=n_frames, model_parameters=model_parameters)
    return args, kw, ev.evaluate_rbot_dataset(util.open_oracle, *args, batch=1, **kw)


@pytest.mark.parametrize("batch", [4, 3])
def test_batched_dataset_evaluation_equals_one_context_per_run(dataset, batch):
    """four runs in one context (batch = 4), or three and one (batch = 3): `cat` is lost once and reset alone; per-run
    and overall results are the oracle's at one context per run, float for float"""
    ev = util.pkg.evaluation
    args, kw, (ref_results, ref_overall) = dataset
    titles = []
    results, overall = ev.evaluate_rbot_dataset(util.open_hip, *args, batch=batch, report=lambda t, r: titles.append(t),
                                                **kw)
    assert titles == ["a_regular_" + name for name in sr.DATASET_BODIES]
    assert list(results) == list(ref_results)
    for run in (results, ref_results):
        for (_, name), r in run.items():
            assert r["tracking_success"] == (0.875 if name == sr.DATASET_LOST_BODY else 1.0), (name, r)
    for key in ref_results:
        sr.same_results(results[key], ref_results[key])
    sr.same_results(overall, ref_overall)
