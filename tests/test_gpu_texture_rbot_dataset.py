"""evaluation.evaluate_rbot_dataset with use_texture_modality on the synthetic RBOT-layout dataset of
tests/selective_reset.py (four bodies, 8 frames, `cat` alone is lost): every run carries a region modality and a texture
modality with the built-in detector.  One context per run restarts a lost body with StartModalities; a batch of four
restarts `cat` alone with Tracker.ResetBodies, or -- judge_on_device -- with a judge that may run the renderers; all
three are to give the same results, float for float (selective_reset.same_results).

The test does not claim that these synthetic frames yield features: the plates of tests/test_gpu_texture_reset.py carry
the non-vacuity of the texture path.  What it shows is that a batch whose bodies carry texture modalities can be
evaluated at all -- the parent refuses the reset of `cat` -- and that the other bodies are left alone.

These runs are judged in the device judge's arithmetic on the host as well (evaluation.judge_pose_result, which
tests/test_rbot_texture_loop.py holds against tests/judge_reference.py bit for bit, as tests/test_gpu_judge_bodies.py
holds the device): that is what lets the host-judged and the device-judged loops agree float for float.  With
rbot_pose_result on the host the device-judged batch differed from the host-judged runs in the last digits of the mean
errors, tracking_success being equal (measured: rotation error of `ape` 0.010348516108933836 device-judged against
0.010345443472033367, translation error of `cat` 0.020147299248492345 against 0.020147298782831058)."""
import pytest

import selective_reset as sr
import util

pytestmark = pytest.mark.gpu
ev = util.pkg.evaluation


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    n_frames = 8
    directory, external, names, model_parameters = sr.write_rbot_dataset(tmp_path_factory.mktemp("rbot_texture"), n_frames)
    args = (str(directory), str(external), names, ["a_regular"])
    kw = dict(n_frames=n_frames, model_parameters=model_parameters, use_texture_modality=True,
              texture_parameters=dict(n_keyframes=2), detector_parameters=dict(n_features=300, fast_threshold=15))
    return args, kw, ev.evaluate_rbot_dataset(util.open_hip, *args, batch=1, **kw)


def test_one_context_per_run_resets_the_lost_body(dataset):
    _, _, (single, _) = dataset
    assert list(single) == [("a_regular", name) for name in sr.DATASET_BODIES]
    print(single)
    assert single[("a_regular", sr.DATASET_LOST_BODY)]["tracking_success"] < 1.0  # a reset ran


@pytest.mark.parametrize("more", [dict(batch=4), dict(batch=4, judge_on_device=True)], ids=["batch4", "batch4_judge_on_device"])
def test_a_batch_with_texture_modalities_equals_one_context_per_run(dataset, more):
    args, kw, (single, single_overall) = dataset
    results, overall = ev.evaluate_rbot_dataset(util.open_hip, *args, **more, **kw)
    assert list(results) == list(single)
    for key in single:
        print(more, key, "batch:", results[key], "one context per run:", single[key])
    print(more, "overall", overall, single_overall)
    for key in single:  # `cat` and, reset or not, every other body
        sr.same_results(results[key], single[key])
    sr.same_results(overall, single_overall)


def test_the_device_judged_batch_equals_a_device_judged_context_per_run(dataset):
    """the same judge on both sides: a batch of one with the device judge, and the batch of four"""
    args, kw, (single, single_overall) = dataset
    one, one_overall = ev.evaluate_rbot_dataset(util.open_hip, *args, batch=1, judge_on_device=True, **kw)
    four, four_overall = ev.evaluate_rbot_dataset(util.open_hip, *args, batch=4, judge_on_device=True, **kw)
    assert list(one) == list(four) == list(single)
    for key in single:
        sr.same_results(four[key], one[key])
        sr.same_results(one[key], single[key])
    sr.same_results(four_overall, one_overall)
    sr.same_results(one_overall, single_overall)
    assert four[("a_regular", sr.DATASET_LOST_BODY)]["tracking_success"] < 1.0
