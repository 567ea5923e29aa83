"""tracking_step_split_moments_kernel at 512 threads: per search, threads 0-255 form what the first Newton step's products
need of the pose alone (region_products_head) while threads 256-511 collect the other parts' means and variances; the
rows are stored behind the collect's barrier (region_products_tail).  The expressions are those of region_products on the
same bits, so nothing may change: poses, histograms, the whole line state and g/H are compared byte for byte (fused
mode 2) with the one-workgroup tracking_step_kernel of the same batch, one batch with the oracle too."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import util
from test_gpu_split_moments_first import NEW, _params
from test_gpu_split_row_distributions import FRAMES, assert_equals_oracle, check, run_device

pytestmark = pytest.mark.gpu

assert FRAMES == 4

_batches = {}


def batch(n_objects):
    """inputs and the one-workgroup result of a batch with the default parameters: computed once, shared, never changed"""
    if n_objects not in _batches:
        inputs = scenes.Inputs(n_objects, FRAMES, n_divides=2)
        _batches[n_objects] = (inputs, run_device(inputs, 0))
    return _batches[n_objects]


# 50, 25, 13 and 100 lines per part; 13 is no multiple of a wave's rows, 16 parts leave part 15 with 5 lines
@pytest.mark.parametrize("n_objects,parts", [(1, 4), (3, 4), (2, 8), (1, 16), (2, 2)])
def test_batch_shapes(n_objects, parts):
    inputs, ref = batch(n_objects)
    got, _ = check(inputs, parts, ref=ref)
    assert all(n > 0 for n in got.n_lines)


def test_equals_the_oracle():
    inputs, ref = batch(3)
    got, _ = check(inputs, 4, ref=ref)
    assert_equals_oracle(got, inputs)


EDGES = {
    # the early head's step is the search's only one
    "one-update": (dict(), 4, _params(tracker=dict(n_update_iterations=1))),
    # u = 1, 2 are local steps: region_products as before, behind an early head and tail
    "three-updates": (dict(), 4, _params(region=dict(n_global_iterations=1), tracker=dict(n_update_iterations=3))),
    # u = 1 is a global step too, but not an early one: region_products as before
    "two-global": (dict(), 4, _params(region=dict(n_global_iterations=2), tracker=dict(n_update_iterations=2))),
    "one-search": (dict(), 4, _params(tracker=dict(n_corr_iterations=1))),
    # head threads whose slot lies beyond the view's lines: zero rows
    "adaptive-100": (dict(n_points=120), 4, _params(region=dict(n_lines_max=100, use_adaptive_coverage=1))),
    # 5 lines per part, 48 slots: most head threads have no line
    "40-lines-8-parts": (dict(), 8, _params(region=dict(n_lines_max=40))),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_parameter_edges(edge):
    inputs_args, parts, kw = EDGES[edge]
    got, _ = check(scenes.Inputs(2, FRAMES, n_divides=2, **inputs_args), parts, **kw)
    assert all(n > 0 for n in got.n_lines)
    if edge == "adaptive-100":
        assert any(n < 100 for n in got.n_lines), got.n_lines
    if edge == "40-lines-8-parts":
        assert all(n <= 40 for n in got.n_lines), got.n_lines


def _moved(inputs, edit):
    out = copy.copy(inputs)  # (the generated inputs are shared: the start poses are this copy's own)
    out.start = [p.copy() for p in inputs.start]
    edit(out)
    return out


def test_a_body_partly_out_of_the_image():
    """object 0 centred on the right image border: the lines beyond it are invalid (ok == false, zero rows)"""
    inputs, ref = batch(2)

    def edit(x):
        W, z = x.intr["width"], x.gt[0][0][2, 3]
        x.start[0] = x.gt[0][0].copy()
        x.start[0][0, 3] = (W - 1 - x.intr["ppu"]) * z / x.intr["fu"]

    got, _ = check(_moved(inputs, edit), 4)
    print("valid lines:", got.n_lines, "in the image:", ref.n_lines)
    assert 0 < got.n_lines[0] < ref.n_lines[0]
    assert got.n_lines[1] == ref.n_lines[1]


def test_a_body_wholly_out_of_the_image():
    """object 1 far outside: no valid line, H = 0, the solve's serial fall-back; its pose stays where it started"""
    inputs, ref = batch(2)

    def edit(x):
        x.start[1] = x.gt[1][0].copy()
        x.start[1][0, 3] += 3.0

    moved = _moved(inputs, edit)
    got, _ = check(moved, 4)
    assert got.n_lines[0] > 0 and got.n_lines[1] == 0, got.n_lines
    g_h = np.frombuffer(got.state[-1], np.float32)  # (the state ends with every modality's gradient and Hessian)
    assert g_h.size == 42 and not g_h.any()
    assert all(np.array_equal(p[1], moved.start[1].astype(np.float32)) for p in got.poses)


def test_256_threads_keep_the_old_order():
    """M3T_HIP_THREADS=256: every thread collects, then region_products as before"""
    inputs, ref = batch(3)
    check(inputs, 4, threads=256, ref=ref)


def test_two_contexts_stepped_alternately():
    """two contexts of one process, a frame of the one after a frame of the other: each object's exchange tags and
    granules are its context's own"""
    batches = [batch(2), batch(3)]
    os.environ["M3T_HIP_SPLIT_PARTS"] = "4"
    try:
        apis = [util.open_hip() for _ in batches]
        insts = []
        for api, (inputs, _) in zip(apis, batches):
            api.call("set_fused_step", 2)
            inst = scenes.Instance(api, inputs)
            inst.upload_frame(0)
            assert inst.tracker.StartModalities(0)
            insts.append(inst)
        poses = [[], []]
        for k in range(FRAMES):
            for t, inst in enumerate(insts):
                inst.upload_frame(k)
                assert inst.tracker.ExecuteTrackingStep(k)
            for t, inst in enumerate(insts):
                poses[t].append(np.stack(inst.poses()))
        for t, (api, (inputs, ref)) in enumerate(zip(apis, batches)):
            name = C.create_string_buffer(64)
            api.call("get_step_variant", name, 64)
            assert name.value.decode() == NEW
            assert np.array_equal(np.stack(poses[t]), ref.poses)
            for got, want in zip([np.concatenate(r.histograms()) for r in insts[t].region], ref.hists):
                assert np.array_equal(got, want)
            region = insts[t].region  # line state and g/H after the last frame, as run() collects them
            state = [r.data_lines().tobytes() for r in region]
            state += [np.concatenate([m.gradient(), m.hessian().reshape(-1)]).tobytes() for m in region]
            assert state == ref.state
    finally:
        os.environ.pop("M3T_HIP_SPLIT_PARTS", None)
