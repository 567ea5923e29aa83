"""The RBOT evaluator's reset-on-loss loop (tests/reset_loop.py) on the device against the oracle: bodies set far from
their tracked pose between two steps -- 20 cm off, turned by 30-40 degrees across the line of sight (out of the
neighbour row the device's view search starts from), half over the image border -- with the renderers and modalities
started again (restart) or with the histograms going on (pose-only).  Every launch shape, both modes: the same resets,
the poses after every frame and the final histograms bit for bit.  Then the same loop with ROI ingest (rectangles
cut from the poses before the reset), and the evaluator front-ends over the device context."""
import ctypes as C

import numpy as np
import pytest

import reset_loop
import scenes
import util

pytestmark = pytest.mark.gpu

KNOBS = ("M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_THREADS", "M3T_HIP_COMPACT", "M3T_HIP_COMPACT_TABLE",
         "M3T_HIP_COMPACT_TABLE_KB", "M3T_HIP_COMPACT_TABLE_CAP", "M3T_HIP_COMPACT_WIDE", "M3T_HIP_NO_PAIR")


def kernel_of(api):
    name = C.create_string_buffer(64)
    api.call("get_step_kernel", name, 64)
    return name.value.decode()


def shape_of(api):
    shape = (C.c_int * 4)()
    api.call("get_step_shape", shape)
    return list(shape)


def hip_loop(monkeypatch, inputs, mode, env, instance_kw=None, fused=None):
    """the loop on the device with the launch knobs `env` set for all of it; returns (result, kernel per step, shape)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    api = util.open_hip()
    if fused is not None:
        api.call("set_fused_step", fused)
    kernels = []
    out = reset_loop.run(api, inputs, reset_loop.default_schedule(inputs.n_objects, inputs.n_frames), mode,
                         instance_kw=instance_kw, after_step=lambda inst, k: kernels.append(kernel_of(api)))
    return out, kernels, shape_of(api)


def restarted_before(result, k):
    """did the loop restart the modalities between step k - 1 and step k (frames 1 ..)"""
    return any(f == k - 1 for f, _ in result[1])


# ---- the benchmarked batch: 64 Region objects, 18 models of 2562 views ------------------------------------------------
@pytest.fixture(scope="module")
def rbot64():
    import bench
    return scenes.Inputs(64, 8, n_divides=4, n_models=bench.CONFIGS["rbot64"]["models"])


@pytest.fixture(scope="module")
def rbot64_oracle(rbot64):
    return {mode: reset_loop.run(util.open_oracle(), rbot64, reset_loop.default_schedule(64, rbot64.n_frames), mode)
            for mode in ("restart", "pose-only")}


RBOT64_CASES = {
    "split": ({}, "tracking_step_split_kernel", [64, 4, 512, 1]),
    "one workgroup 512": ({"M3T_HIP_NO_SPLIT": "1"}, None, [64, 1, 512, 1]),
    "one workgroup 256": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "256"}, None, [64, 1, 256, 0]),
    "compact": ({"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT_TABLE": "0"},
                "tracking_step_compact_kernel", None),
    "compact_table": ({"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1"}, "tracking_step_compact_table_kernel", None),
    "compact_table overflow": ({"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT_TABLE_CAP": "64"},
                               None, None),
}


@pytest.mark.parametrize("mode", ["restart", "pose-only"])
@pytest.mark.parametrize("case", list(RBOT64_CASES))
def test_rbot64_resets_match_the_oracle(rbot64, rbot64_oracle, case, mode, monkeypatch):
    env, kernel, shape = RBOT64_CASES[case]
    got, kernels, got_shape = hip_loop(monkeypatch, rbot64, mode, env)
    reset_loop.assert_same(got, rbot64_oracle[mode])
    if kernel is not None:
        assert set(kernels) == {kernel}, kernels
    if shape is not None:
        assert got_shape == shape, got_shape
    if case.startswith("one workgroup"):
        assert all("split" not in k and "compact" not in k and k.startswith("tracking_step_") for k in kernels), kernels
    if case == "compact_table overflow":
        # overflow: the kernel without the table from the step after; StartModalities brings the table back
        assert kernels[0] == "tracking_step_compact_table_kernel", kernels
        if mode == "pose-only":
            assert kernels[-1] == "tracking_step_compact_kernel", kernels
        restarts = [k for k in range(2, rbot64.n_frames) if mode == "restart" and restarted_before(got, k)]
        assert restarts or mode == "pose-only"
        for k in restarts:
            assert kernels[k - 1] == "tracking_step_compact_table_kernel", (k, kernels)
    if case == "compact_table" and mode == "restart":
        assert any(restarted_before(got, k) for k in range(2, rbot64.n_frames))


def test_rbot64_table_overflow_between_restarts(rbot64, monkeypatch):
    """restart mode with restarts after the first two steps only: the steps in between let the histograms fill, the
    table overflows and the kernel without it takes over; a restart brings the table back.  (With the default schedule
    almost every step follows a restart, and fresh histograms stay within what the fallback waits for.)"""
    schedule = [(1, 0, "a"), (rbot64.n_frames - 1, 63, "a")]
    ref = reset_loop.run(util.open_oracle(), rbot64, schedule, "restart")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in {"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT_TABLE_CAP": "64"}.items():
        monkeypatch.setenv(k, v)
    api = util.open_hip()
    kernels = []
    got = reset_loop.run(api, rbot64, schedule, "restart", after_step=lambda inst, k: kernels.append(kernel_of(api)))
    reset_loop.assert_same(got, ref)
    assert got[1][:2] == [(1, 0), (2, 0)] and all(f > 3 for f, _ in got[1][2:]), got[1]
    assert kernels[:3] == ["tracking_step_compact_table_kernel"] * 3, kernels  # steps 1, 2 and 3 follow a (re)start
    for k in range(2, rbot64.n_frames):
        if restarted_before(got, k):
            assert kernels[k - 1] == "tracking_step_compact_table_kernel", (k, kernels)
    assert "tracking_step_compact_kernel" in kernels[3:], kernels


def test_rbot64_unfused_restart_matches_the_oracle(rbot64, rbot64_oracle, monkeypatch):
    """one launch per sub-step (set_fused_step 0): StartModalities between steps through the same entry points"""
    got, kernels, _ = hip_loop(monkeypatch, rbot64, "restart", {}, fused=0)
    reset_loop.assert_same(got, rbot64_oracle["restart"])
    assert set(kernels) == {""}, kernels  # no fused step kernel ran


# ---- ycb shape: 21 Region + Depth objects -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ycb21():
    return scenes.Inputs(21, 5, n_divides=4, n_models=6, with_depth=True)


@pytest.fixture(scope="module")
def ycb21_oracle(ycb21):
    return {mode: reset_loop.run(util.open_oracle(), ycb21, reset_loop.default_schedule(21, ycb21.n_frames), mode,
                                 instance_kw=dict(use_depth=True))
            for mode in ("restart", "pose-only")}


YCB_CASES = {
    "split_pair": ({}, "tracking_step_split_pair_kernel"),
    "split": ({"M3T_HIP_NO_PAIR": "1"}, "tracking_step_split_kernel"),
    "lds_pair": ({"M3T_HIP_NO_SPLIT": "1"}, "tracking_step_lds_pair_kernel"),
    "compact 256": ({"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT_WIDE": "0"},
                    "tracking_step_compact_kernel"),
    "compact_wide": ({"M3T_HIP_COMPACT": "1", "M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT_WIDE": "1"},
                     "tracking_step_compact_wide_kernel"),
}


@pytest.mark.parametrize("mode", ["restart", "pose-only"])
@pytest.mark.parametrize("case", list(YCB_CASES))
def test_ycb21_resets_match_the_oracle(ycb21, ycb21_oracle, case, mode, monkeypatch):
    env, kernel = YCB_CASES[case]
    got, kernels, shape = hip_loop(monkeypatch, ycb21, mode, env, instance_kw=dict(use_depth=True))
    reset_loop.assert_same(got, ycb21_oracle[mode])
    assert set(kernels) == {kernel}, kernels
    if case == "compact 256":
        assert shape[2] == 256, shape


# ---- mixed: Region + Depth, Region only, Depth only in one context ----------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    inputs = scenes.Inputs(9, 5, n_divides=4, n_models=3, with_depth=True)
    kw = dict(kinds=["rd", "r", "d"] * 3)
    return inputs, kw, {mode: reset_loop.run(util.open_oracle(), inputs, reset_loop.default_schedule(9, inputs.n_frames),
                                             mode, instance_kw=kw) for mode in ("restart", "pose-only")}


@pytest.mark.parametrize("mode", ["restart", "pose-only"])
@pytest.mark.parametrize("env,kernel", [({}, "tracking_step_split_pair_kernel"),
                                        ({"M3T_HIP_NO_SPLIT": "1"}, "tracking_step_lds_pair_kernel"),
                                        ({"M3T_HIP_NO_PAIR": "1"}, "tracking_step_split_kernel")])
def test_mixed_batch_resets_match_the_oracle(mixed, env, kernel, mode, monkeypatch):
    inputs, kw, ref = mixed
    got, kernels, _ = hip_loop(monkeypatch, inputs, mode, env, instance_kw=kw)
    reset_loop.assert_same(got, ref[mode])
    assert set(kernels) == {kernel}, kernels


# ---- ROI ingest: the rectangles of the next frame come from the poses before the reset ---------------------------------
def roi_status(hip):
    bodies = (C.c_int * 64)()
    n = C.c_int(0)
    pulls = C.c_longlong(0)
    hip.call("roi_get_status", bodies, 64, C.byref(n), C.byref(pulls))
    return n.value, sorted(set(bodies[:min(n.value, 64)])), pulls.value


def roi_loop(inputs, schedule, mode, with_depth):
    """reset_loop.run in rectangle mode, with the ring and pipelined upload of test_gpu_roi.run: select slot, step k,
    enqueue the rectangles of k + 1, read the poses, reset.  Restart mode: StartModalities on a rectangle slot is
    refused; the evaluator uploads the whole current frame into its slot first (which marks it whole).
    Returns (run() result, roi status, unrecovered bodies, restarts refused, kernel per step)."""
    hip = util.open_hip()
    n = inputs.n_objects
    rings, kernels, refused = [], [], [0]

    def upload(slot, k):
        for _, ids, blocks in rings:
            b = blocks[k]
            hip.call("cameras_upload_batch_roi_async", ids, n, slot, b.ctypes.data_as(C.c_void_p), b.strides[0],
                     b.strides[1])

    def frame(inst, k):
        if k == 1:  # (after StartModalities on frame 0: the rings, then frame 1 -- as whole frames, no step recorded yet)
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

    def restart(inst, k):
        rc = hip.raw("start_modalities", 0)
        if k == 1:  # (the frame of the first step went whole: no step had been recorded to cut rectangles from)
            assert rc == 0, hip.last_error()
            return
        assert rc == util.pkg._capi.M3T_ERR_UNSUPPORTED, rc
        assert "ROI ingest" in hip.last_error(), hip.last_error()
        refused[0] += 1
        for cams, _, blocks in rings:
            for i, cam in enumerate(cams):
                f = blocks[k][i]
                hip.call("camera_upload_slot", cam.id, k % 2, f.ctypes.data_as(C.c_void_p), f.strides[0])
        assert inst.tracker.StartModalities(0)

    holder = {}

    def setup(inst):
        holder["inst"] = inst
        hip.call("set_roi_ingest", 1, C.c_float(24.0))

    got = reset_loop.run(hip, inputs, schedule, mode, instance_kw=dict(use_depth=with_depth), setup=setup, frame=frame,
                         after_step=after_step, restart=restart)
    holder["inst"].tracker.ingest_sync()
    bodies = (C.c_int * 64)()
    nu = C.c_int(0)
    hip.call("roi_get_unrecovered", bodies, 64, C.byref(nu))
    return got, roi_status(hip), sorted(set(bodies[:min(nu.value, 64)])), refused[0], kernels


@pytest.fixture(scope="module")
def roi_inputs():
    return {False: scenes.Inputs(6, 7, n_divides=2), True: scenes.Inputs(6, 6, n_divides=2, with_depth=True)}


@pytest.fixture(scope="module")
def roi_oracle(roi_inputs):
    out = {}
    for depth, inputs in roi_inputs.items():
        schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
        for mode in ("restart", "pose-only"):
            out[depth, mode] = reset_loop.run(util.open_oracle(), inputs, schedule, mode,
                                              instance_kw=dict(use_depth=depth))
    return out


ROI_SHAPES = {"split": ({}, "tracking_step_split_guard_kernel"),
              "one workgroup": ({"M3T_HIP_NO_SPLIT": "1"}, None),
              "compact": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT": "1"}, "tracking_step_compact_guard_kernel")}


@pytest.mark.parametrize("with_depth", [False, True])
@pytest.mark.parametrize("shape", list(ROI_SHAPES))
def test_roi_ingest_with_resets(roi_inputs, roi_oracle, shape, with_depth, monkeypatch):
    """pose-only: the rectangles of the frame after a reset were cut around the old pose; the guarded kernel drops the
    reset bodies' steps and repeats them on whole frames -- the poses of whole frames bit for bit, every body a
    translation entry reset reported, no other body.  restart: StartModalities on a rectangle slot is refused; the
    whole frame uploaded into the slot, it runs and the whole loop equals the oracle's.  With depth cameras too: the
    colour and the depth cameras are two batches of scattered camera ids, and the repeat fetches the whole frames of
    both"""
    env, kernel = ROI_SHAPES[shape]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    inputs = roi_inputs[with_depth]
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    reset_bodies = {i for _, i, _ in schedule}
    translated = {i for f, i, kind in schedule if kind == "a" and f + 1 < inputs.n_frames}
    for mode in ("pose-only", "restart"):
        got, (misses, bodies, pulls), unrecovered, refused, kernels = roi_loop(inputs, schedule, mode, with_depth)
        reset_loop.assert_same(got, roi_oracle[with_depth, mode])
        assert unrecovered == [], (mode, unrecovered)
        assert all(k.endswith("_guard_kernel") for k in kernels[1:]), kernels  # the steps read rectangles
        assert pulls > 0
        assert set(bodies) <= reset_bodies, (mode, bodies)
        assert translated <= set(bodies), (mode, bodies, translated)
        if kernel is not None:
            assert set(kernels[1:]) == {kernel}, kernels
        assert refused == (len({f for f, _ in got[1]} - {1}) if mode == "restart" else 0) and (refused or mode != "restart")


# ---- the evaluator front-ends over the device context ----------------------------------------------------------------
def _same_results(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "complete_cycle":
            continue
        va, vb = a[key], b[key]
        if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
            assert np.array_equal(np.asarray(va), np.asarray(vb)), key
        else:
            assert va == vb, (key, va, vb)


def test_rbot_sequence_evaluator_on_the_device():
    """evaluate_rbot_sequence with a lost frame: the HIP context resets exactly where the oracle does, and every
    per-frame and average result is the same float"""
    ev = util.pkg.evaluation
    n_frames = 6
    inputs = scenes.Inputs(1, n_frames + 1)
    poses_gt = np.asarray(inputs.gt[0], np.float32).copy()
    poses_gt[3, :3, 3] += (0.2, 0.0, 0.0)
    runs = []
    for api in (util.open_hip(), util.open_oracle()):
        inst = scenes.Instance(api, inputs)
        runs.append(ev.evaluate_rbot_sequence(inst.tracker, inst.bodies[0], poses_gt, inst.upload_frame,
                                              n_frames=n_frames))
    (fa, aa), (fb, ab) = runs
    assert [f["tracking_success"] for f in fa] == [1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    for x, y in zip(fa, fb):
        _same_results(x, y)
    _same_results(aa, ab)


def test_rbot_dataset_evaluator_on_the_device(tmp_path):
    import test_evaluation as te
    ev = util.pkg.evaluation
    n_frames = 5
    dataset, external, names, model_parameters = te.write_rbot_dataset(tmp_path, n_frames)
    path = dataset / "poses_first.txt"
    lines = path.read_text().splitlines()
    row = [float(v) for v in lines[1 + 2].split("\t")]
    row[9] += 200.0  # frame 2 lies 20 cm off: the main body is lost there and reset
    lines[1 + 2] = "\t".join("%.9g" % v for v in row)
    path.write_text("\n".join(lines) + "\n")
    runs = [ev.evaluate_rbot_dataset(open_api, str(dataset), str(external), names, ["a_regular"], n_frames=n_frames,
                                     model_parameters=model_parameters) for open_api in (util.open_hip, util.open_oracle)]
    (ra, oa), (rb, ob) = runs
    assert ra.keys() == rb.keys()
    for key in ra:
        _same_results(ra[key], rb[key])
        assert ra[key]["tracking_success"] < 1.0  # the run did reset
    _same_results(oa, ob)


def test_ycb_dataset_evaluator_on_the_device(tmp_path):
    import test_evaluation as te
    ev = util.pkg.evaluation
    dataset, external, names, model_parameters = te.write_ycb_dataset(tmp_path)
    runs = [ev.evaluate_ycb_dataset(open_api, str(dataset), str(external), [0, 1], names, n_vertices_evaluation=4,
                                    model_parameters=model_parameters) for open_api in (util.open_hip, util.open_oracle)]
    (ra, oa), (rb, ob) = runs
    assert ra.keys() == rb.keys() and ra
    for key in ra:
        _same_results(ra[key], rb[key])
    _same_results(oa, ob)
