"""Every case of tests/structure_edges.py, TRACK_CASES, through every launch shape of the structure step -- the library's
choice, at most two parts and one part per tracked link (M3T_HIP_TREE_PARTS), per-sub-step launches
(M3T_HIP_NO_TREE_FUSION) and the one-launch-per-Newton-step path of a structure spread over processes, at world size 1
behind a reduce callback that leaves the sums as they are -- free running over two frames against the oracle: body2world
of every body and joint2parent of every link after every frame and both histograms of every RegionModality are
np.array_equal -- there is no tolerance in this module --, and the kernel, the launch shape and the number of reductions
are the ones the case table derives from the host's eligibility rules.  tests/test_structure_edge_cases.py checks on the
CPU that the cases are live and what the table covers."""
import numpy as np
import pytest

import fused_edges
import structure_edges as se
import util

pytestmark = pytest.mark.gpu

_oracle = {}  # case id -> TrackRun of the oracle, computed once per case


def _reference(case):
    if case.id not in _oracle:
        _oracle[case.id] = se.oracle_track_run(case)
    return _oracle[case.id]


@pytest.mark.parametrize("case,shape", se.TRACK_PAIRS, ids=["%s-%s" % (c.id, s) for c, s in se.TRACK_PAIRS])
def test_structure_step_equals_the_oracle(case, shape, monkeypatch):
    for k in fused_edges.OVERRIDES + se.TREE_VARIABLES:
        monkeypatch.delenv(k, raising=False)
    overrides, kind, _ = se.SHAPES[shape]
    for k, v in overrides.items():
        monkeypatch.setenv(k, v)
    ref = _reference(case)
    got = se.track_run(util.open_hip(), case, device=True, segment=kind == "segment")
    assert np.array_equal(got.start, ref.start)
    for k in range(se.N_FRAMES):
        assert np.array_equal(got.states[k], ref.states[k]), k
    assert len(got.hist) == len(ref.hist) == len(case.tracked_links)
    for mine, theirs in ((got.hist_start, ref.hist_start), (got.hist, ref.hist)):
        for (fa, ba), (fb, bb) in zip(mine, theirs):
            assert np.array_equal(fa, fb) and np.array_equal(ba, bb)
    for m in case.empty:  # no valid line: the histograms stay what StartModalities left
        assert np.array_equal(got.hist[m][0], got.hist_start[m][0]) and np.array_equal(got.hist[m][1], got.hist_start[m][1])
    kernel, launch = case.expect[shape]
    assert got.kernels == [kernel] * se.N_FRAMES, got.kernels
    if launch is not None:
        assert [s[:3] for s in got.shapes] == [launch] * se.N_FRAMES, got.shapes
    # one reduction per Newton step wherever a communicator or callback is set, whichever launches the step takes
    assert got.reductions == (case.newton_steps * se.N_FRAMES if kind == "segment" else 0)
