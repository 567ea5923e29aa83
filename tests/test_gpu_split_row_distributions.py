"""The row pass of tracking_step_split_moments_kernel (region_distribution_rows, m3t_kernels.hip): raw distribution
products, normalisation, mean and variance of a line in one 16-lane row of one wave, in place of phases C1 and C2 and the
owner's moments.  The one-workgroup tracking_step_kernel keeps the phases (its code is untouched) and is the in-library
reference: poses after every frame, histograms, the whole line state (all distribution rows, mean, variance, flags) and g/H
are compared byte for byte (fused mode 2); the cases whose rows are not walked are compared with the oracle too.

Shapes: 1 - 3 objects, n_divides=2, 4 frames.  Every case asserts the launch shape and the variant name first."""
import os

import numpy as np
import pytest

import scenes
import util
from test_gpu_split_moments_first import NEW, OLD, _params, assert_same, run
from util import syn

pytestmark = pytest.mark.gpu

FRAMES = 4
KNOBS = ("M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_NO_MOMENTS_FIRST", "M3T_HIP_THREADS")


def run_device(inputs, parts, threads=None, **instance_kw):
    """parts = 0: one workgroup per object"""
    for k in KNOBS:
        os.environ.pop(k, None)
    if parts:
        os.environ["M3T_HIP_SPLIT_PARTS"] = str(parts)
    else:
        os.environ["M3T_HIP_NO_SPLIT"] = "1"
    if threads:
        os.environ["M3T_HIP_THREADS"] = str(threads)
    try:
        api = util.open_hip()
        api.call("set_fused_step", 2)
        return run(api, inputs, FRAMES, **instance_kw)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)


def check(inputs, parts, threads=512, ref=None, **kw):
    """the row pass in `parts` workgroups per object against one workgroup per object; returns (got, ref)"""
    got = run_device(inputs, parts, threads=None if threads == 512 else threads, **kw)
    assert got.shape[:3] == [inputs.n_objects, parts, threads], got.shape
    assert got.kernel == OLD and got.variant == NEW
    if ref is None:
        ref = run_device(inputs, 0, **kw)
    assert ref.shape[:2] == [inputs.n_objects, 1] and ref.kernel == ref.variant == "tracking_step_kernel"
    assert_same(got, ref)
    return got, ref


def assert_equals_oracle(got, inputs, **kw):
    ref = run(util.open_oracle(), inputs, FRAMES, **kw)
    assert np.array_equal(got.poses, ref.poses)
    for x, y in zip(got.hists, ref.hists):
        assert np.array_equal(x, y)


# dl = 16 fills a row (the row boundary), dl = 2 is the shortest chain, fl != 8 takes the general product
@pytest.mark.parametrize("fl,dl", [(8, 12), (16, 16), (4, 16), (10, 8), (1, 2)])
def test_distribution_and_function_lengths(fl, dl):
    kw = _params(region=dict(function_length=fl, distribution_length=dl, scales=[2, 1], standard_deviations=[7.0, 1.5]))
    got, _ = check(scenes.Inputs(2, FRAMES, n_divides=2), 4, **kw)
    assert all(n > 0 for n in got.n_lines)


# ---- lines per part that are no multiple of a wave's four rows or of a trip's 32 ------------------------------------
_one_object = {}


def one_object(n_lines_max):
    """inputs, parameters and the one-workgroup result for one object: computed once, shared, never changed"""
    if n_lines_max not in _one_object:
        inputs = scenes.Inputs(1, FRAMES, n_divides=2)
        kw = _params(region=dict(n_lines_max=n_lines_max))
        _one_object[n_lines_max] = (inputs, kw, run_device(inputs, 0, **kw))
    return _one_object[n_lines_max]


@pytest.mark.parametrize("n_lines_max,parts", [(200, 2), (200, 8), (200, 16), (100, 8)])
def test_lines_per_part(n_lines_max, parts):
    """200 lines: 100, 25 and 13 lines per part; 100 lines over 8 parts: 13 per part, the last part holds 9"""
    inputs, kw, ref = one_object(n_lines_max)
    assert syn.RBOT_REGION_PARAMS["n_lines_max"] == 200
    got, _ = check(inputs, parts, ref=ref, **kw)
    assert 0 < got.n_lines[0] <= n_lines_max


def test_256_thread_workgroups():
    """16 rows per trip: a part's 50 lines take four trips"""
    got, _ = check(scenes.Inputs(2, FRAMES, n_divides=2), 4, threads=256)
    assert all(n > 0 for n in got.n_lines)


# ---- rows that are not walked ----------------------------------------------------------------------------------------
def test_fewer_lines_than_rows():
    """adaptive coverage: most views have fewer lines than n_lines_max; the rows beyond them send what they hold"""
    inputs = scenes.Inputs(2, FRAMES, n_divides=2, n_points=120)
    kw = _params(region=dict(n_lines_max=100, use_adaptive_coverage=1))
    got, _ = check(inputs, 4, **kw)
    assert all(n > 0 for n in got.n_lines) and any(n < 100 for n in got.n_lines), got.n_lines
    assert_equals_oracle(got, inputs, **kw)


def test_ragged_and_empty_line_sets():
    """object 0 on the image border (invalid lines among the valid ones), object 1 outside the image and object 2 behind
    the camera: parts without a single valid line"""
    inputs = scenes.Inputs(3, FRAMES, n_divides=2)
    W = inputs.intr["width"]
    z = inputs.gt[0][0][2, 3]
    inputs.start[0] = inputs.gt[0][0].copy()
    inputs.start[0][0, 3] = (W - 1 - inputs.intr["ppu"]) * z / inputs.intr["fu"]
    inputs.start[1] = inputs.gt[1][0].copy()
    inputs.start[1][0, 3] += 3.0
    inputs.start[2] = inputs.gt[2][0].copy()
    inputs.start[2][2, 3] = -0.5
    got, _ = check(inputs, 4)
    assert 0 < got.n_lines[0] < 200 and got.n_lines[1] == 0 and got.n_lines[2] == 0, got.n_lines
    for i in (1, 2):  # zero g/H leaves the pose untouched
        assert np.array_equal(got.poses[-1][i], np.asarray(inputs.start[i], got.poses.dtype))
    assert_equals_oracle(got, inputs)


def test_three_newton_steps_one_global_iteration():
    """two local steps read the rows the pass wrote (own lines) and the rows that were collected lazily"""
    kw = _params(region=dict(n_global_iterations=1), tracker=dict(n_update_iterations=3))
    got, _ = check(scenes.Inputs(2, FRAMES, n_divides=2), 4, **kw)
    assert all(n > 0 for n in got.n_lines)
