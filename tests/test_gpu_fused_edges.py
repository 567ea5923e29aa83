"""Every case of tests/fused_edges.py through every fused launch shape, free running over the case's frames, against the
oracle: body2world of every object after every frame and both histograms of every RegionModality after the last frame
are np.array_equal -- there is no tolerance in this module --, and the kernel and launch shape the host chose are the
ones the case table derives from the host's eligibility rules.  Where a shape is not eligible for a case (a scale of
10, other function / distribution lengths, more than 256 lines, 2 histogram bins) the expectation is the kernel the
library must fall back to, and the poses still equal the oracle's.  A modality whose working set does not fit the LDS is
answered with M3T_ERR_UNSUPPORTED in every shape.

The matrix: Region-only cases x 9 shapes (split with the library's choice of parts, 16 and 2 parts; one workgroup with
512, 256, 128 threads; compact, compact with the LDS pair table, compact with a table of 64 entries) + Region + Depth cases x 9
shapes (the three split shapes and split without pairing; the three one-workgroup sizes; compact with 256 and with 512
threads).  tests/test_fused_edge_cases.py checks on the CPU that the cases are live and what the table covers."""
import numpy as np
import pytest

import fused_edges as fe
import scenes
import util

pytestmark = pytest.mark.gpu

assert len(fe.PAIRS) == len(fe.CASES) * 9 + len(fe.CASES_DEPTH) * 9

_oracle = {}  # case id -> Run: the oracle's trajectory and histograms, computed once per case


def _reference(case):
    if case.id not in _oracle:
        _oracle[case.id] = fe.oracle_run(case)
    return _oracle[case.id]


def _assert_clean_refusal(api, case, inputs, ref):
    inst = scenes.Instance(api, inputs, **case.instance_kw())
    inst.upload_frame(0)
    for call in ("start_modalities", "execute_tracking_step"):
        assert api.raw(call, 0) == fe.M3T_ERR_UNSUPPORTED, call
        assert "LDS" in api.last_error()
    assert np.array_equal(np.stack(inst.poses()), ref.start)  # nothing was launched


def _assert_equals_oracle(api, case, shape, inputs, ref):
    kernel, parts, threads = case.expect[shape]
    got = fe.run(api, case, inputs, device=True)
    assert got.started
    for k in range(inputs.n_frames):
        assert np.array_equal(got.poses[k], ref.poses[k]), k
    for (fa, ba), (fb, bb) in zip(got.hist, ref.hist):
        assert np.array_equal(fa, fb) and np.array_equal(ba, bb)
    for i in range(case.n_objects):
        if not case.moves[i]:
            assert all(np.array_equal(p[i], got.start[i]) for p in got.poses), i
    for i in case.empty:  # no valid line: the histograms stay what StartModalities left
        assert np.array_equal(got.hist[i][0], got.hist_start[i][0]) and np.array_equal(got.hist[i][1], got.hist_start[i][1])
    assert got.kernels[0] == kernel, got.kernels
    assert got.shapes[0][:3] == [case.n_objects, parts, threads], got.shapes
    if shape == "compact_cap64" and kernel == "tracking_step_compact_table_kernel":
        # the table of 64 entries: the walks of the objects with more mixed bins read the global table (table->fits ==
        # false) and report it, and the host goes back to the kernel without the table -- when the oracle's histograms
        # say so (tests/test_fused_edge_cases.py: in every 32-bin case but the two with 5 and 10 lines, after frame 0)
        assert got.kernels == fe.table_kernels(ref, inputs.n_frames), got.kernels
    else:
        assert got.kernels == [kernel] * inputs.n_frames, got.kernels
    assert all(s[:3] == got.shapes[0][:3] for s in got.shapes), got.shapes


@pytest.mark.parametrize("case,shape", fe.PAIRS, ids=["%s-%s" % (c.id, s) for c, s in fe.PAIRS])
def test_fused_step_equals_the_oracle(case, shape, monkeypatch):
    for k in fe.OVERRIDES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.shapes[shape][0].items():
        monkeypatch.setenv(k, v)
    inputs = fe.inputs_of(case)
    ref = _reference(case)
    assert ref.started
    api = util.open_hip()
    if case.unsupported:
        _assert_clean_refusal(api, case, inputs, ref)
    else:
        _assert_equals_oracle(api, case, shape, inputs, ref)
