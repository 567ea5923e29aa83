"""Device-decided resets through start-modality renderers (m3t_hip_judge_set_reset_renderers) and reset targets
(m3t_hip_judge_set_reset_target) on the GPU: the reset of a renderer-fed body against the oracle, a frame without a loss
that leaves everything alone, several runs of a context with partial losses against the host-judged loop, the RBOT
modelled-occlusion loop with its two judgements (evaluation.evaluate_rbot_occlusion_sequences), the refused calls and
the dataset driver's fifth column."""
import numpy as np
import pytest

import golden_scene as gs
import occlusion_scenes as oc
import scenes
import selective_reset as sr
import util
from util import host

pytestmark = pytest.mark.gpu

capi = util.pkg._capi
ev = util.pkg.evaluation
F = np.float32
INVALID, UNSUPPORTED = capi.M3T_ERR_INVALID_ARGUMENT, capi.M3T_ERR_UNSUPPORTED


# ---- 1 / 2. one tracked body: the triangle with the bottle static in front of it ----------------------------------------
def _triangle_scene(api, region_checking):
    """depth and silhouette renderer of the colour camera are twins; the bottle stands in front of the triangle"""
    if api.is_hip:
        api.call("set_fused_step", 2)  # one launch per correspondence search, the line state written back
    f = gs.TrackerFixture(api, measure_occlusions=False, region_params=dict(n_unoccluded_iterations=0),
                          depth_params=dict(n_unoccluded_iterations=0))
    geometry, schauma = gs.fixture_renderer_geometry(api, f.body)
    depth = host.FocusedBasicDepthRenderer(api, geometry, f.color_camera, image_size=200)
    silhouette = host.FocusedSilhouetteRenderer(api, geometry, f.color_camera, id_type=1, image_size=200)
    for r in (depth, silhouette):
        r.AddReferencedBody(f.body)
    pose = schauma.body2world_pose()
    pose[:3, 3] = f.body.body2world_pose()[:3, 3] + np.array([0.01, 0.0, -0.15], F)
    schauma.set_body2world_pose(pose)
    f.region.ModelOcclusions(depth)
    renderers = [depth]
    if region_checking:
        f.region.UseRegionChecking(silhouette)
        renderers.append(silhouette)
    assert f.tracker.StartModalities(0)
    assert f.tracker.ExecuteTrackingStep(0)
    return f, renderers


def _off_by_20_cm(pose):
    p = np.asarray(pose, F).copy()
    p[2, 3] += F(0.2)  # along world z: lost by translation alone
    return p


@pytest.mark.parametrize("region_checking", [False, True])
def test_a_device_decided_reset_through_renderers_equals_the_oracle(region_checking):
    out = []
    for api in (util.open_hip(), util.open_oracle()):
        f, renderers = _triangle_scene(api, region_checking)
        gt = _off_by_20_cm(f.body.body2world_pose())
        if api.is_hip:
            judge = f.tracker.CreateJudge([f.body], 1)
            judge.set_reset_renderers(True)
            row = judge.read(judge.judge([gt], 0), 1)[0]
            assert row[0]["was_reset"] == 1 and row[0]["tracking_success"] == 0.0
        else:
            f.body.set_body2world_pose(gt)
            for r in renderers:
                r.StartRendering()
            assert f.tracker.StartModalities(0)
        after = f.body.body2world_pose(), f.region.histograms()
        assert f.tracker.ExecuteTrackingStep(1)
        out.append((gt, after, f.body.body2world_pose(), f.region.data_lines()["valid"].copy()))
    (gt_a, after_a, pose_a, valid_a), (gt_b, after_b, pose_b, valid_b) = out
    assert np.array_equal(gt_a, gt_b) and np.array_equal(after_a[0], gt_a) and np.array_equal(after_b[0], gt_b)
    assert np.array_equal(after_a[1][0], after_b[1][0]) and np.array_equal(after_a[1][1], after_b[1][1])
    assert np.array_equal(pose_a, pose_b)
    assert np.array_equal(valid_a, valid_b) and 0 < valid_a.sum()


def test_a_frame_without_a_loss_leaves_renderers_and_bodies_alone():
    (f, renderers), (twin, _) = (_triangle_scene(util.open_hip(), True) for _ in range(2))
    judge = f.tracker.CreateJudge([f.body], 1)
    judge.set_reset_renderers(True)
    before = f.body.body2world_pose(), f.region.histograms(), [r.images() for r in renderers]
    row = judge.read(judge.judge([before[0]], 0), 1)[0]
    assert row[0]["was_reset"] == 0 and row[0]["tracking_success"] == 1.0 and row[0]["translation_error"] == 0.0
    assert np.array_equal(f.body.body2world_pose(), before[0])
    assert np.array_equal(f.region.histograms()[0], before[1][0]) and np.array_equal(f.region.histograms()[1], before[1][1])
    for r, images in zip(renderers, before[2]):
        got = r.images()
        assert np.array_equal(got[0], images[0]) and got[2:] == images[2:]
        assert (got[1] is None and images[1] is None) or np.array_equal(got[1], images[1])
    assert (before[2][0][0] < 65535).sum() > 1000  # something had been drawn
    for g in (f, twin):
        assert g.tracker.ExecuteTrackingStep(1)
    assert np.array_equal(f.body.body2world_pose(), twin.body.body2world_pose())
    assert np.array_equal(f.region.data_lines()["valid"], twin.region.data_lines()["valid"])
    assert np.array_equal(f.region.histograms()[0], twin.region.histograms()[0])
    assert np.array_equal(f.region.histograms()[1], twin.region.histograms()[1])


# ---- 3. several runs in one context, partial losses --------------------------------------------------------------------
N_RUNS, N_FRAMES = 3, 5
IMAGE_SIZES = (64, 200, 64)
SCHEDULE = [(1, 0, "a"), (3, 0, "a"), (3, 2, "a")]  # main 0 alone, then mains 0 and 2 together (and each once more
EXPECTED_RESETS = [(1, 0), (2, 0), (3, 0), (3, 2), (4, 0), (4, 2)]  # the frame after: back from 20 cm off)


@pytest.fixture(scope="module")
def inputs():
    return scenes.Inputs(2 * N_RUNS, N_FRAMES, n_divides=2)


def test_partial_losses_in_a_batch_equal_the_host_judged_loop(inputs):
    gt = oc.main_ground_truth(inputs, N_RUNS, SCHEDULE)
    out = []
    for on_device in (False, True):
        pairs = oc.Pairs(util.open_hip(), inputs, range(N_RUNS), IMAGE_SIZES)
        pairs.upload_frame(0)
        assert pairs.tracker.StartModalities(0)
        if on_device:
            judge = pairs.tracker.CreateJudge(pairs.mains, N_FRAMES - 1)
            judge.set_reset_renderers(True)
        states, resets = [], []
        for k in range(1, N_FRAMES):
            pairs.upload_frame(k)
            assert pairs.tracker.ExecuteTrackingStep(k)
            if on_device:
                images = [r.images() for r in pairs.renderers]
                assert judge.judge(gt[k], 0) == k - 1
                lost = [p for p in range(N_RUNS) if judge.read(k - 1, 1)[0][p]["was_reset"]]
                for p, r in enumerate(pairs.renderers):  # a run without a loss keeps its rendering; a lost one's moves
                    if p in lost:
                        assert not np.array_equal(r.images()[0], images[p][0]), (k, p)
                    else:
                        oc.assert_same_images(r.images(), images[p])
            else:
                poses = pairs.poses()
                for p in range(N_RUNS):
                    oc.assert_clear_of_the_thresholds(poses[2 * p], gt[k][p])
                lost = sr.lost_bodies([poses[2 * p] for p in range(N_RUNS)], gt[k])
                if lost:
                    assert pairs.tracker.ResetBodies([pairs.mains[p] for p in lost], [gt[k][p] for p in lost], 0)
            resets += [(k, p) for p in lost]
            states.append(pairs.state())
        out.append((states, resets))
    (ref_states, ref_resets), (states, resets) = out
    assert ref_resets == EXPECTED_RESETS and resets == EXPECTED_RESETS
    for k, (a, b) in enumerate(zip(states, ref_states), start=1):
        oc.assert_same_state(a, b, k)


# ---- 4. the reset target: RBOT's loop with modelled occlusions ---------------------------------------------------------
def _occlusion_loop(pairs, inputs, runs, schedule_gt, on_device, own_pose=False):
    """evaluate_rbot_occlusion_sequences over `pairs`; the state after every frame's judgements is taken when the next
    frame is loaded, and after the last one"""
    first = [np.stack([schedule_gt[k][p] for k in range(inputs.n_frames)]) for p in runs]
    second = [np.stack([oc.occluder_pose(inputs.gt[2 * p][k]) for k in range(inputs.n_frames)]) for p in runs]
    states = []

    def load_images(k):
        if k >= 2:
            states.append(pairs.state())
        pairs.upload_frame(k)

    frames, averages = ev.evaluate_rbot_occlusion_sequences(pairs.tracker, pairs.mains, pairs.occluders, first, second,
                                                            load_images, inputs.n_frames - 1, judge_on_device=on_device,
                                                            judge_occluder_on_own_pose=own_pose)
    states.append(pairs.state())
    return frames, averages, states


@pytest.mark.parametrize("own_pose", [False, True])
def test_rbot_occlusion_loop_with_two_judges_equals_one_context_per_run(inputs, own_pose):
    """the loop of evaluate_rbot_occlusion_sequences in one context per run, host-judged (two ResetBodies calls per
    frame), against the batch of three runs judged on the device with two judges: poses and histograms of main body and
    occluder after every frame bit for bit, the kept rows within the bounds of the device-judged RBOT dataset test.
    (The oracle yardstick for one run: test_rbot_occlusion_loop_of_one_run_equals_the_oracle below.)"""
    gt = oc.main_ground_truth(inputs, N_RUNS, [(2, 1, "a")])
    singles = [_occlusion_loop(oc.Pairs(util.open_hip(), inputs, [p], [IMAGE_SIZES[p]]), inputs, [p], gt, False, own_pose)
               for p in range(N_RUNS)]
    batch = oc.Pairs(util.open_hip(), inputs, range(N_RUNS), IMAGE_SIZES)
    frames, averages, states = _occlusion_loop(batch, inputs, range(N_RUNS), gt, True, own_pose)
    assert len(states) == N_FRAMES - 1
    for k, state in enumerate(states):
        for p, (_, _, single_states) in enumerate(singles):
            ref = single_states[k]
            assert np.array_equal(state[0][2 * p:2 * p + 2], ref[0]), (k, p)
            oc.assert_same_state((ref[0], state[1][2 * p:2 * p + 2]), ref, (k, p))
    for p, ((ref_frames,), _, _) in enumerate(singles):  # (a single's results: those of its one run)
        success = [f["tracking_success"] for f in frames[p]]
        assert success == [f["tracking_success"] for f in ref_frames]
        assert success == ([1.0, 0.0, 0.0, 1.0] if p == 1 else [1.0] * 4), (p, success)
        for got, ref in zip(frames[p], ref_frames):
            print(p, got, ref)
            # the bounds of test_gpu_judge_bodies.test_rbot_dataset_judged_on_the_device, per frame
            assert abs(got["translation_error"] - ref["translation_error"]) <= 4 * 2.0 ** -23 * ref["translation_error"]
            assert abs(got["rotation_error"] - ref["rotation_error"]) <= 4e-6 / 2e-3 + 1e-6


def test_rbot_occlusion_loop_of_one_run_equals_the_oracle(inputs):
    """The oracle yardstick for the reset target: run 1 (its main body is lost at frame 2) in a two-body oracle context,
    judged by the host, against the same run judged on the device with two judges.  The oracle has no ResetBodies;
    "ResetBody of one body" is there: set the pose, StartRendering, save the other body's histograms,
    StartModalities(0) -- which starts both modalities again from the fresh rendering --, restore the saved histograms.
    Poses and histograms of both bodies after every frame, bit for bit."""
    p, n = 1, inputs.n_frames
    gt = oc.main_ground_truth(inputs, N_RUNS, [(2, p, "a")])
    first = [gt[k][p] for k in range(n)]
    second = [oc.occluder_pose(inputs.gt[2 * p][k]) for k in range(n)]
    ora = oc.Pairs(util.open_oracle(), inputs, [p], [IMAGE_SIZES[p]])

    def reset(which, pose):
        ora.bodies[which].set_body2world_pose(pose)
        ora.renderers[0].StartRendering()
        saved = ora.region[1 - which].histograms()
        assert ora.tracker.StartModalities(0)
        ora.region[1 - which].set_histograms(*saved)

    ora.upload_frame(0)
    reset(0, first[0])
    reset(1, second[0])
    ref_states, ref_success = [], []
    for i in range(n - 1):
        ora.upload_frame(i + 1)
        assert ora.tracker.ExecuteTrackingStep(i)
        pose = ora.mains[0].body2world_pose()
        oc.assert_clear_of_the_thresholds(pose, first[i + 1])
        ref_success.append(ev.rbot_pose_result(pose, first[i + 1])[2])
        if ref_success[-1] == 0.0:
            reset(0, first[i + 1])
        pose = ora.mains[0].body2world_pose()
        oc.assert_clear_of_the_thresholds(pose, second[i + 1])
        if ev.rbot_pose_result(pose, second[i + 1])[2] == 0.0:
            reset(1, second[i + 1])
        ref_states.append(ora.state())
    frames, _, states = _occlusion_loop(oc.Pairs(util.open_hip(), inputs, [p], [IMAGE_SIZES[p]]), inputs, [p], gt, True)
    assert [f["tracking_success"] for f in frames[0]] == ref_success == [1.0, 0.0, 0.0, 1.0]
    for k, (a, b) in enumerate(zip(states, ref_states), start=1):
        oc.assert_same_state(a, b, k)


def test_a_target_whose_entry_is_not_lost_keeps_its_bits(inputs):
    """two runs, a judge of the main bodies with the occluders as targets: entry 0 is lost, entry 1 is judged against
    its own pose.  Occluder 0 takes the ground truth and run 0's renderer is drawn again; occluder 1, its histograms
    and run 1's renderer keep their bits (the pair's readers are entries of the list, the flags are the targets')."""
    pairs = oc.Pairs(util.open_hip(), inputs, [0, 1], [64, 200])
    pairs.upload_frame(0)
    assert pairs.tracker.StartModalities(0)
    pairs.upload_frame(1)
    assert pairs.tracker.ExecuteTrackingStep(1)
    judge = pairs.tracker.CreateJudge(pairs.mains, 1)
    judge.set_reset_renderers(True)
    for i in range(2):
        judge.set_reset_target(i, pairs.occluders[i])
    before, images = pairs.state(), [r.images() for r in pairs.renderers]
    far = _off_by_20_cm(before[0][0])
    row = judge.read(judge.judge([far, before[0][2]], 0), 1)[0]
    assert row["was_reset"].tolist() == [1, 0] and row["tracking_success"].tolist() == [0.0, 1.0]
    after = pairs.state()
    assert np.array_equal(after[0][1], far)  # occluder 0
    for body in (0, 2, 3):                   # both main bodies and occluder 1
        assert np.array_equal(after[0][body], before[0][body]), body
    for modality in (0, 2, 3):
        assert np.array_equal(after[1][modality][0], before[1][modality][0]), modality
        assert np.array_equal(after[1][modality][1], before[1][modality][1]), modality
    assert not np.array_equal(after[1][1][0], before[1][1][0])  # occluder 0 was started again
    assert not np.array_equal(pairs.renderers[0].images()[0], images[0][0])
    oc.assert_same_images(pairs.renderers[1].images(), images[1])


def test_the_occluder_hides_lines_of_the_main_body(inputs):
    """the branch is live: with the occluder in front of its contour the main body's modality keeps fewer lines"""
    valid = []
    for model_occlusions in (True, False):
        api = util.open_hip()
        api.call("set_fused_step", 2)  # (the line state is written back)
        pairs = oc.Pairs(api, inputs, [0], [200], model_occlusions=model_occlusions)
        pairs.upload_frame(0)
        assert pairs.tracker.StartModalities(0)
        pairs.upload_frame(1)
        assert pairs.tracker.ExecuteTrackingStep(1)
        valid.append(int(pairs.region[0].data_lines()["valid"].sum()))
    print(valid)
    assert 0 < valid[0] < valid[1]


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["written twice", "rows exist", "chain", "image 333", "no lds raster"])
def test_refused_targets_and_renderers_change_nothing(inputs, variant, monkeypatch):
    """image 333: the work spread gives few renderers many bands of few rows, and a band of three rows of 333 pixels
    fits the LDS; the renderer is too large for the LDS form once its bands are few (the developer override
    M3T_HIP_RASTER_BANDS=2: 167 rows x 333 pixels x 4 bytes = 222 KB of the 160).  no lds raster: the LDS form switched
    off for the context (M3T_HIP_NO_LDS_RASTER)."""
    from test_gpu_reset_bodies import _build
    for knob in ("M3T_HIP_RASTER_BANDS", "M3T_HIP_RASTER_SLICES", "M3T_HIP_NO_LDS_RASTER"):
        monkeypatch.delenv(knob, raising=False)
    if variant == "image 333":
        monkeypatch.setenv("M3T_HIP_RASTER_BANDS", "2")
    if variant == "no lds raster":
        monkeypatch.setenv("M3T_HIP_NO_LDS_RASTER", "1")
    api = util.open_hip()
    if variant == "chain":
        small = scenes.Inputs(3, 4, n_divides=2)
        inst = _build(api, small, "chain")
        inst.upload_frame(1)
        assert inst.tracker.ExecuteTrackingStep(1)
        listed, state = [inst.bodies[0]], lambda: (np.stack(inst.poses()), [r.histograms() for r in inst.region])
        tracker, lost_gt = inst.tracker, [_off_by_20_cm(inst.poses()[0])]
    else:
        pairs = oc.Pairs(api, inputs, [0, 1], [333, 64] if variant == "image 333" else [64, 64])
        pairs.upload_frame(0)
        assert pairs.tracker.StartModalities(0)
        pairs.upload_frame(1)
        assert pairs.tracker.ExecuteTrackingStep(1)
        listed, state, tracker = pairs.mains, pairs.state, pairs.tracker
        lost_gt = [_off_by_20_cm(p) for p in pairs.poses()[0::2]]
    judge = tracker.CreateJudge(listed, 4)
    judge.set_reset_renderers(True)
    before = state()
    rows_before = 0
    if variant == "written twice":
        judge.set_reset_target(0, pairs.occluders[0])
        assert api.raw("judge_set_reset_target", judge.id, 1, pairs.occluders[0].id) == INVALID
        assert "two entries" in api.last_error(), api.last_error()
        assert api.raw("judge_set_reset_target", judge.id, 1, pairs.mains[0].id) == INVALID  # listed by entry 0
        assert "another entry" in api.last_error(), api.last_error()
        assert api.raw("judge_set_reset_target", judge.id, 1, 2 * len(pairs.bodies)) == INVALID
        assert "bad body id" in api.last_error(), api.last_error()
    elif variant == "rows exist":
        assert judge.judge(lost_gt, -1) == 0
        rows_before = 1
        assert api.raw("judge_set_reset_target", judge.id, 0, pairs.occluders[0].id) == INVALID
        assert "judge_clear" in api.last_error(), api.last_error()
    elif variant == "chain":
        judge.set_reset_target(0, inst.extra)
        rc, _ = judge.raw_judge(lost_gt, 0)
        assert rc == UNSUPPORTED and "more than one link" in api.last_error(), (rc, api.last_error())
    else:
        rc, _ = judge.raw_judge(lost_gt, 0)
        assert rc == UNSUPPORTED and "three-launch form" in api.last_error(), (rc, api.last_error())
        assert ("image size 333" if variant == "image 333" else "image size 64") in api.last_error(), api.last_error()
    oc.assert_same_state(state(), before, variant)
    # no row was consumed, and a judge-only call takes any body and ignores the targets
    assert judge.judge(lost_gt, -1) == rows_before
    row = judge.read(rows_before, 1)[0]
    assert not row["tracking_success"].any() and not row["was_reset"].any()
    oc.assert_same_state(state(), before, variant)
    if variant == "written twice":  # the refused targets left the accepted one in place: main 1 resets itself
        assert judge.judge(lost_gt, 0) == 1
        assert judge.read(1, 1)[0]["was_reset"].tolist() == [1, 1]
        after = pairs.poses()
        assert np.array_equal(after[0], before[0][0]) and np.array_equal(after[1], lost_gt[0])
        assert np.array_equal(after[2], lost_gt[1]) and np.array_equal(after[3], before[0][3])


# ---- 6. the dataset driver ---------------------------------------------------------------------------------------------
def test_rbot_dataset_fifth_column_judged_on_the_device(tmp_path):
    n_frames = 8
    directory, external, names, model_parameters = oc.write_rbot_occlusion_dataset(tmp_path, n_frames)
    args = (str(directory), str(external), names, ["a_regular"])
    kw = dict(n_frames=n_frames, model_parameters=model_parameters, batch=4, sequence_occlusions=[True])
    ref_results, ref_overall = ev.evaluate_rbot_dataset(util.open_hip, *args, **kw)
    results, overall = ev.evaluate_rbot_dataset(util.open_hip, *args, judge_on_device=True, **kw)
    assert list(results) == list(ref_results) == [("a_regular_modeled", name) for name in names]
    for key, ref in ref_results.items():
        got = results[key]
        print(key, got, ref)
        assert got["tracking_success"] == ref["tracking_success"]
        assert abs(got["translation_error"] - ref["translation_error"]) <= 4 * 2.0 ** -23 * ref["translation_error"]
        assert abs(got["rotation_error"] - ref["rotation_error"]) <= 4e-6 / 2e-3 + 1e-6
        assert got["complete_cycle"] > 0
    assert ref_results[("a_regular_modeled", sr.DATASET_LOST_BODY)]["tracking_success"] < 1.0
    assert overall["tracking_success"] == ref_overall["tracking_success"]


def test_rbot_dataset_without_occlusions_is_unchanged(tmp_path):
    n_frames = 3
    directory, external, names, model_parameters = sr.write_rbot_dataset(tmp_path, n_frames)
    args = (str(directory), str(external), names, ["a_regular"])
    kw = dict(n_frames=n_frames, model_parameters=model_parameters, batch=4)
    ref_results, ref_overall = ev.evaluate_rbot_dataset(util.open_hip, *args, **kw)
    results, overall = ev.evaluate_rbot_dataset(util.open_hip, *args, sequence_occlusions=[False], **kw)
    assert list(results) == list(ref_results)
    for key in ref_results:
        sr.same_results(results[key], ref_results[key])
    sr.same_results(overall, ref_overall)
