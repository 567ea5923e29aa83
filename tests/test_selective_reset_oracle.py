"""Why m3t_hip_reset_bodies exists, on the CPU oracle alone (tests/selective_reset.py): a batch whose lost bodies are
reset with the batch-wide StartModalities is NOT the set of independent trackers an evaluator of independent
sequences runs -- the histograms of every body are initialised again whenever one of them is lost.  These tests pin
the yardstick of tests/test_gpu_reset_bodies.py: each object in a context of its own."""
import numpy as np
import pytest

import reset_loop
import scenes
import selective_reset as sr
import util


@pytest.fixture(scope="module")
def inputs():
    return scenes.Inputs(6, 7, n_divides=2)


@pytest.fixture(scope="module")
def singles(inputs):
    schedule = reset_loop.default_schedule(6, 7)
    sr.check_schedule(schedule, 6, 7)
    return schedule, sr.expectation(inputs, schedule)


def test_without_a_loss_the_batch_is_its_single_runs(inputs):
    """no reset: the objects of a batch do not see each other, bit for bit"""
    gt = reset_loop.ground_truth(inputs, [])
    inst = scenes.Instance(util.open_oracle(), inputs)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    batch = []
    for k in range(1, inputs.n_frames):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
        batch.append(np.stack(inst.poses()))
        assert sr.lost_bodies(batch[-1], gt[k]) == []
    hist = [r.histograms() for r in inst.region]
    for i in range(inputs.n_objects):
        poses, resets, (single_hist,) = sr.run_single(util.open_oracle(), inputs, i, gt)
        assert resets == []
        for k, p in enumerate(poses):
            assert np.array_equal(p, batch[k][i]), (i, k + 1)
        assert np.array_equal(single_hist[0], hist[i][0]) and np.array_equal(single_hist[1], hist[i][1]), i


def test_batch_wide_restart_disturbs_a_body_that_is_never_lost(inputs, singles):
    """the schedule's losses, batch-wide StartModalities: object 1 is never lost and yet leaves its single run, from
    the first frame after a restart on; the decisions (who is reset when) are still the same"""
    schedule, (ref_poses, ref_resets, _) = singles
    poses, resets, _ = sr.run_batch(util.open_oracle(), inputs, schedule, reset="all")
    assert resets == ref_resets
    assert {(f, i) for f, i, _ in schedule} <= set(resets)  # every injected loss was judged one
    assert 1 not in {i for _, i in resets}
    differs = [k + 1 for k in range(len(poses)) if not np.array_equal(poses[k][1], ref_poses[k][1])]
    first_restart = min(f for f, _ in resets)
    assert differs and differs[0] == first_restart + 1, (differs, first_restart)
    assert np.array_equal(poses[first_restart - 1][1], ref_poses[first_restart - 1][1])
    # the bodies that were reset differ from their single runs too (their neighbours' losses restart them again)
    assert any(not np.array_equal(poses[-1][i], ref_poses[-1][i]) for i in {i for _, i in resets})


def test_the_loop_helpers_agree_with_reset_loop(inputs):
    """run_batch(reset="all") is reset_loop.run in restart mode: same poses, resets and histograms"""
    schedule = reset_loop.default_schedule(6, 7)
    got = sr.run_batch(util.open_oracle(), inputs, schedule, reset="all")
    reset_loop.assert_same(got, reset_loop.run(util.open_oracle(), inputs, schedule, "restart"))


def test_the_evaluator_dataset_loses_one_body_once(tmp_path):
    """the dataset of the batched evaluator test, through the oracle at batch = 1: `cat` is lost once mid-sequence,
    reset, and tracks on; the other three bodies are never lost"""
    ev = util.pkg.evaluation
    n_frames = 8
    dataset, external, names, model_parameters = sr.write_rbot_dataset(tmp_path, n_frames)
    results, overall = ev.evaluate_rbot_dataset(util.open_oracle, str(dataset), str(external), names, ["a_regular"],
                                                n_frames=n_frames, model_parameters=model_parameters)
    for name in names:
        expected = 0.875 if name == sr.DATASET_LOST_BODY else 1.0
        assert results[("a_regular", name)]["tracking_success"] == expected, (name, results[("a_regular", name)])
    # per frame: lost at cycle 2 (image 3), five good frames after the reset
    api = util.open_oracle()
    from util import host
    gen = util.pkg.generator
    body = gen.Body(api, "cat", str(dataset / "cat" / "cat.obj"), 0.001, True, False, np.eye(4, dtype=np.float32))
    model = host.RegionModel(api, path=str(external / "models" / "cat_model.bin"))
    camera = gen.LoaderColorCamera(api, str(dataset / "cat" / "frames"), ev.RBOT_INTRINSICS, "a_regular", 0, 4)
    modality = host.RegionModality(api, body, camera, model, **ev.RBOT_REGION_PARAMETERS)
    host.Optimizer(api, body=body, modalities=[modality])
    tracker = host.Tracker(api, 7, 2)

    def load_image(k):
        camera.set_load_index(k)
        assert camera.UpdateImage()

    frames, _ = ev.evaluate_rbot_sequence(tracker, body, ev.read_poses_rbot(str(dataset / "poses_first.txt"), n_frames),
                                          load_image, n_frames)
    assert [f["tracking_success"] for f in frames] == [1, 1, 0, 1, 1, 1, 1, 1]


def test_reset_bodies_is_not_part_of_the_oracle():
    """the oracle is frozen: the front-end says so instead of falling back to the batch-wide restart"""
    api = util.open_oracle()
    inst = scenes.Instance(api, scenes.Inputs(1, 2))
    with pytest.raises(util.pkg.M3TError):
        inst.tracker.ResetBodies([inst.bodies[0]])
