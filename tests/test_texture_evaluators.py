"""The texture columns of the YCB and OPT evaluators (evaluation.evaluate_ycb_dataset / evaluate_opt_dataset,
use_texture_modality) without a GPU: the parameter tables restate the reference's examples, the oracle's context is
refused, and without the flag both evaluators return what they returned before the flag existed."""
import numpy as np
import pytest

import util
from test_evaluation import write_ycb_dataset
from test_opt_evaluator import write_opt_dataset

ev = util.pkg.evaluation
F = np.float32
TEN_DEGREES = float(F(10.0) * F(np.pi) / F(180.0))  # 10.0f * m3t::kPi / 180.0f


def test_ycb_texture_parameters_restate_the_example():
    """evaluate_ycb_dataset.cpp:77-107, the fields the modality has"""
    assert ev.YCB_TEXTURE_PARAMETERS == dict(
        focused_image_size=200, descriptor_distance_threshold=0.7, tukey_norm_constant=20.0,
        standard_deviations=[10.0, 10.0, 3.0], max_keyframe_rotation_difference=TEN_DEGREES, max_keyframe_age=1000,
        n_keyframes=1, measured_occlusion_radius=0.01, measured_occlusion_threshold=0.03)
    assert ev.YCB_DETECTOR_PARAMETERS == dict(n_features=300)  # orb_n_features; the FAST threshold is the built-in's own
    params = util.pkg._capi.TextureModalityParams(**ev.YCB_TEXTURE_PARAMETERS)  # every key is a field of the modality
    assert params.n_standard_deviations == 3 and params.max_keyframe_age == 1000
    detector = util.pkg._capi.TextureDetectorParams(**ev.YCB_DETECTOR_PARAMETERS)
    assert detector.n_features == 300 and detector.fast_threshold == util.pkg._capi.TextureDetectorParams().fast_threshold


def test_opt_texture_parameters_restate_the_example():
    """evaluate_opt_dataset.cpp:49-77: YCB's fields with other standard deviations, no measured occlusions"""
    assert ev.OPT_TEXTURE_PARAMETERS == dict(
        focused_image_size=200, descriptor_distance_threshold=0.7, tukey_norm_constant=20.0,
        standard_deviations=[5.0, 1.0, 0.5], max_keyframe_rotation_difference=TEN_DEGREES, max_keyframe_age=1000,
        n_keyframes=1)
    assert ev.OPT_DETECTOR_PARAMETERS == dict(n_features=300)
    rest = {k: v for k, v in ev.YCB_TEXTURE_PARAMETERS.items() if k in ev.OPT_TEXTURE_PARAMETERS and k != "standard_deviations"}
    assert rest == {k: v for k, v in ev.OPT_TEXTURE_PARAMETERS.items() if k != "standard_deviations"}
    util.pkg._capi.TextureModalityParams(**ev.OPT_TEXTURE_PARAMETERS)


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a if k != "complete_cycle")  # (a wall time)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def test_ycb_evaluator_refuses_the_oracle_and_is_unchanged_without_the_flag(tmp_path):
    dataset, external, names, model_parameters = write_ycb_dataset(tmp_path)
    kw = dict(n_vertices_evaluation=4, model_parameters=model_parameters)
    with pytest.raises(ValueError, match="use_texture_modality needs the HIP library"):
        ev.evaluate_ycb_dataset(util.open_oracle, str(dataset), str(external), [0, 1], names,
                                use_texture_modality=True, **kw)
    before = ev.evaluate_ycb_dataset(util.open_oracle, str(dataset), str(external), [0, 1], names, **kw)
    after = ev.evaluate_ycb_dataset(util.open_oracle, str(dataset), str(external), [0, 1], names,
                                    use_texture_modality=False, texture_parameters=dict(n_keyframes=3),
                                    detector_parameters=dict(n_features=100), measure_occlusions_texture=False, **kw)
    assert set(before[0]) == {("0000", names[0]), ("0001", names[1])}
    assert _same(before[0], after[0]) and _same(before[1], after[1])


def test_opt_evaluator_refuses_the_oracle_and_is_unchanged_without_the_flag(tmp_path):
    dataset, external, kw = write_opt_dataset(tmp_path)
    for batch in (1, 2):
        with pytest.raises(ValueError, match="use_texture_modality needs the HIP library"):
            ev.evaluate_opt_dataset(util.open_oracle, str(dataset), str(external), batch=batch,
                                    use_texture_modality=True, **kw)
    before = ev.evaluate_opt_dataset(util.open_oracle, str(dataset), str(external), batch=2, **kw)
    after = ev.evaluate_opt_dataset(util.open_oracle, str(dataset), str(external), batch=2, use_texture_modality=False,
                                    texture_parameters=dict(n_keyframes=3), detector_parameters=dict(n_features=100), **kw)
    assert set(before[0]) == {"so_tr_1_b", "so_zo_2_b", "ch_tr_1_b", "ch_zo_2_b"}
    assert _same(before[0], after[0]) and _same(before[1], after[1])
