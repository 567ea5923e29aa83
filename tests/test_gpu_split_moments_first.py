"""tracking_step_split_moments_kernel: the split kernel whose workgroups exchange their lines' means and variances
first and collect the distribution rows beside the first Newton step's chain and solve.  A line's moments are a pure
function of its distribution, so nothing may change: poses, histograms, the whole line state (all distribution rows,
mean, variance) and g/H are compared byte for byte (fused mode 2) with the one-workgroup kernel, one batch with the
oracle too; batches that do not qualify must keep tracking_step_split_kernel (or its _pair_ sibling).

m3t_hip_get_step_kernel keeps saying "tracking_step_split_kernel" for both instantiations (the launch-shape tables of the
other test modules are written in its names); m3t_hip_get_step_variant tells them apart."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import util
from util import syn

pytestmark = pytest.mark.gpu

OLD, NEW = "tracking_step_split_kernel", "tracking_step_split_moments_kernel"
OVERRIDES = ("M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_NO_MOMENTS_FIRST")


def _name(api, entry):
    buf = C.create_string_buffer(64)
    api.call(entry, buf, 64)
    return buf.value.decode()


class Result:
    pass


def run(api, inputs, n_frames, **instance_kw):
    """poses after every frame, histograms, line / point state and g/H after the last one, launch shape and kernel"""
    device = api.is_hip
    inst = scenes.Instance(api, inputs, **instance_kw)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    out = Result()
    poses = []
    for k in range(n_frames):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
        poses.append(np.stack(inst.poses()))
    out.poses = np.stack(poses)
    out.hists = [np.concatenate(r.histograms()) for r in inst.region]
    if device:
        shape = (C.c_int * 4)()
        api.call("get_step_shape", shape)
        out.shape = list(shape)
        out.kernel, out.variant = _name(api, "get_step_kernel"), _name(api, "get_step_variant")
        out.state = [r.data_lines().tobytes() for r in inst.region] + [d.data_points().tobytes() for d in inst.depth]
        out.state += [np.concatenate([m.gradient(), m.hessian().reshape(-1)]).tobytes() for m in inst.region + inst.depth]
        out.n_lines = [len(r.data_lines()) for r in inst.region]
    return out


def run_device(inputs, parts, n_frames, env=None, **instance_kw):
    """parts = 0: one workgroup per object"""
    for k in OVERRIDES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    if parts:
        os.environ["M3T_HIP_SPLIT_PARTS"] = str(parts)
    else:
        os.environ["M3T_HIP_NO_SPLIT"] = "1"
    try:
        api = util.open_hip()
        api.call("set_fused_step", 2)
        return run(api, inputs, n_frames, **instance_kw)
    finally:
        for k in OVERRIDES:
            os.environ.pop(k, None)


def assert_same(a, b):
    assert np.array_equal(a.poses, b.poses)
    for x, y in zip(a.hists, b.hists):
        assert np.array_equal(x, y)
    assert a.state == b.state


# ---- the default parameters: every batch shape of the issue against the one-workgroup kernel ---------------------------
FRAMES = 5
_inputs, _one_workgroup = {}, {}


def inputs_of(n_objects):
    if n_objects not in _inputs:
        _inputs[n_objects] = scenes.Inputs(n_objects, FRAMES, n_divides=2, n_models=min(n_objects, 2))
    return _inputs[n_objects]


def one_workgroup(n_objects):
    """the one-workgroup kernel's result for the batch: computed once, shared, never changed"""
    if n_objects not in _one_workgroup:
        ref = run_device(inputs_of(n_objects), 0, FRAMES)
        assert ref.shape[:2] == [n_objects, 1] and ref.kernel == ref.variant == "tracking_step_kernel"
        _one_workgroup[n_objects] = ref
    return _one_workgroup[n_objects]


@pytest.mark.parametrize("n_objects,parts", [(1, 4), (3, 4), (8, 4), (8, 8), (1, 16)])
def test_moments_first_is_bit_identical_to_one_workgroup_per_object(n_objects, parts):
    got = run_device(inputs_of(n_objects), parts, FRAMES)
    assert got.shape[:2] == [n_objects, parts] and got.shape[3] == 1
    assert got.kernel == OLD and got.variant == NEW
    assert_same(got, one_workgroup(n_objects))
    for i in range(n_objects):  # and it tracks
        e = syn.pose_errors(got.poses[-1][i], inputs_of(n_objects).gt[i][FRAMES - 1])
        assert e[0] < np.deg2rad(5) and e[1] < 0.05


def test_moments_first_equals_the_oracle():
    got = run_device(inputs_of(3), 4, FRAMES)
    assert got.variant == NEW
    ref = run(util.open_oracle(), inputs_of(3), FRAMES)
    assert np.array_equal(got.poses, ref.poses)
    for x, y in zip(got.hists, ref.hists):
        assert np.array_equal(x, y)


def test_the_override_keeps_the_old_exchange():
    got = run_device(inputs_of(3), 4, FRAMES, env={"M3T_HIP_NO_MOMENTS_FIRST": "1"})
    assert got.kernel == got.variant == OLD
    assert_same(got, one_workgroup(3))


# ---- parameter edges -------------------------------------------------------------------------------------------------
def _params(region=None, tracker=None):
    return dict(region_params=dict(syn.RBOT_REGION_PARAMS, **(region or {})),
                tracker_params=dict(syn.RBOT_TRACKER, **(tracker or {})))


EDGES = {
    # the rows are needed by the write-back alone and are collected beside the search's one solve
    "one-update": (dict(), _params(tracker=dict(n_update_iterations=1))),
    # two local steps read the lazily collected rows
    "three-updates": (dict(), _params(region=dict(n_global_iterations=1), tracker=dict(n_update_iterations=3))),
    # no Newton step reads the rows; they are still written back
    "two-global": (dict(), _params(region=dict(n_global_iterations=2), tracker=dict(n_update_iterations=2))),
    "one-search": (dict(), _params(tracker=dict(n_corr_iterations=1))),
    # fewer lines than n_lines_max in most views: the rows beyond them still send their granules
    "adaptive-100": (dict(n_points=120), _params(region=dict(n_lines_max=100, use_adaptive_coverage=1))),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_parameter_edges(edge):
    inputs_args, kw = EDGES[edge]
    inputs = scenes.Inputs(2, 4, n_divides=2, **inputs_args)
    got = run_device(inputs, 4, 4, **kw)
    ref = run_device(inputs, 0, 4, **kw)
    assert got.shape[:2] == [2, 4] and ref.shape[:2] == [2, 1]
    assert got.kernel == OLD and got.variant == NEW
    assert_same(got, ref)
    assert all(n > 0 for n in got.n_lines)
    if edge == "adaptive-100":
        assert any(n < 100 for n in got.n_lines), got.n_lines


# ---- batches that do not qualify keep today's kernels -----------------------------------------------------------------
def test_no_global_iteration_keeps_the_old_kernel():
    """n_global_iterations = 0: the first Newton step after a search reads the distribution rows"""
    kw = _params(region=dict(n_global_iterations=0))
    inputs = scenes.Inputs(2, 4, n_divides=2)
    got, ref = run_device(inputs, 4, 4, **kw), run_device(inputs, 0, 4, **kw)
    assert got.shape[:2] == [2, 4] and got.kernel == got.variant == OLD
    assert_same(got, ref)


def test_region_and_depth_keeps_the_pair_kernel():
    inputs = scenes.Inputs(2, 4, n_divides=2, with_depth=True)
    got, ref = run_device(inputs, 4, 4, use_depth=True), run_device(inputs, 0, 4, use_depth=True)
    assert got.shape[:2] == [2, 4] and got.kernel == got.variant == "tracking_step_split_pair_kernel"
    assert_same(got, ref)


def test_measured_occlusions_keep_the_old_kernel():
    """Region-only bodies that look at a depth camera for occlusions: the occlusion vote is deferred behind the exchange"""
    inputs = scenes.Inputs(2, 4, n_divides=2, with_depth=True)
    assert syn.YCB_REGION_PARAMS["measure_occlusions"] == 1
    got, ref = run_device(inputs, 4, 4, kinds=["r", "r"]), run_device(inputs, 0, 4, kinds=["r", "r"])
    assert got.shape[:2] == [2, 4] and got.kernel == got.variant == OLD
    assert_same(got, ref)
