"""The case tables of tests/structure_edges.py against the oracle alone (no GPU): every case is *live* -- finite poses,
the structures and bodies that must move do, those that must not keep their start bit for bit, the off-screen leaf has
no valid line --, the tables cover what tests/test_gpu_structure_solves.py and tests/test_gpu_structure_edges.py claim
to cover, and the oracle's own LdltSolve / OptimizerEnd, which no reference golden reaches at these sizes, equal a
float64 restatement of the same step (numpy.linalg.solve) within a bound a dropped term could not hide under."""
import numpy as np
import pytest

import structure_edges as se
import util
from test_step_plan import NAMES
from util import syn

_solve_runs, _track_runs = {}, {}


def _solve(case):
    if case.id not in _solve_runs:
        _solve_runs[case.id] = se.solve_run(util.open_oracle(), case)
    return _solve_runs[case.id]


def _track(case):
    if case.id not in _track_runs:
        _track_runs[case.id] = se.oracle_track_run(case)
    return _track_runs[case.id]


# ---- liveness ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", se.SOLVE_CASES, ids=repr)
def test_solve_case_is_live_in_the_oracle(case):
    run = _solve(case)
    for k, st in enumerate(case.structures):
        states = [s[k] for s in run.states]
        assert all(np.isfinite(s).all() for s in states)
        moved = float(np.max(np.abs(states[-1].astype(np.float64) - run.start[k])))
        print(case.id, "structure", k, "n", st.size, "moved", moved)
        if case.moves[k]:
            assert 1e-4 < moved < 10.0
            assert not np.array_equal(states[0], run.start[k]) and not np.array_equal(states[1], states[0])
        else:
            assert all(np.array_equal(s, run.start[k]) for s in states)
    if case.id.startswith("zero-pivot"):  # the links above the leaf still move
        st = case.structures[0]
        others = [i for i in range(st.n_links) if i != st.leaf and st.links[i].dof]
        assert all(not np.array_equal(run.states[0][0][i, 1], run.start[0][i, 1]) for i in others if st.links[i].parent >= 0)


@pytest.mark.parametrize("case", se.TRACK_CASES, ids=repr)
def test_track_case_is_live_in_the_oracle(case):
    run = _track(case)
    assert len(run.states) == se.N_FRAMES and all(np.isfinite(s).all() for s in run.states)
    n = len(case.body_links)
    for b, (s, i) in enumerate(case.body_links):
        moved = float(np.max(np.abs(run.states[-1][b].astype(np.float64) - run.start[b])))
        print(case.id, "body", b, "moved", moved)
        assert (moved > 1e-4) == case.moves[b], (b, moved)
        if case.tracks:
            body = case.structures[s].links[i].body
            rot, trans = syn.pose_errors(run.states[-1][b], run.gt[-1][0][body])[:2]
            assert rot < np.deg2rad(5) and trans < 0.05, (b, rot, trans)
    assert len(run.n_lines) == len(case.tracked_links)
    print(case.id, "lines", run.n_lines)
    for m in range(len(case.tracked_links)):
        if m in case.empty:  # no valid line: the histograms stay as started, the body still follows its parent
            assert run.n_lines[m] == 0
            assert all(np.array_equal(x, y) for x, y in zip(run.hist[m], run.hist_start[m]))
            assert case.moves[case.body_links.index(case.tracked_links[m])]
        else:
            assert run.n_lines[m] > 0
    assert n <= 8


def test_padding_leaves_the_plain_chains_poses():
    """body-less links behind the leaf add Tikhonov rows only: the bodies end where the plain chain's end, bit for bit"""
    by_id = {c.id: c for c in se.TRACK_CASES}
    plain = _track(by_id["plain-bins64"]).states
    padded = [c for c in se.TRACK_CASES if c.group == "limits" and c.id not in ("plain-bins64", "links-16-bins32")]
    assert len(padded) >= 6
    for case in padded:
        for a, b in zip(_track(case).states, plain):
            assert np.array_equal(a[:3], b[:3]), case.id
    for a, b in zip(_track(by_id["links-16-bins32"]).states, _track(by_id["joints-1dof-n8"]).states):
        assert np.array_equal(a[:3], b[:3])


# ---- what the tables cover --------------------------------------------------------------------------------------------
def test_tables_are_well_formed():
    for cases in (se.SOLVE_CASES, se.TRACK_CASES):
        ids = [c.id for c in cases]
        assert len(ids) == len(set(ids))
    for case in se.SOLVE_CASES:
        assert len(case.modes) == len(case.moves) == len(case.structures)
        assert case.sums(0).shape == (42 * case.n_links,) and not np.array_equal(case.sums(0), case.sums(1))
    for case in se.TRACK_CASES:
        assert set(case.expect) == set(se.SHAPES) and len(case.tracked_links) <= 8
        for kernel, shape in case.expect.values():
            assert kernel in NAMES  # m3t_step::StepKernelName
            assert (shape is None) == (kernel == "")
            if shape is not None:
                assert kernel.startswith("tracking_step_tree_") and shape[0] == len(case.tracked_links)
                assert shape[1] in (1, 2, 8) and shape[2] == 512
                assert (shape[1] > 1) == (kernel == "tracking_step_tree_split_kernel")
    assert {c.group for c in se.TRACK_CASES} == {"solve-size", "limits", "host-rules", "topology", "geometry", "parameters",
                                                "constrained", "depth"}
    assert len(se.TRACK_PAIRS) == 5 * len(se.TRACK_CASES)


def test_every_branch_of_the_solve_dispatch_has_a_case():
    """ldlt_solve_any: n <= 8, 9..13, 14..16 and above, in the MODE 0 kernels through both entries, with open trees and
    with constraint rows, and inside the one-launch kernels; the equal-diagonal, all-zero, zero-pivot and NaN paths"""
    def branches(cases):
        return {se.ldlt_branch(n) for c in cases for n in c.sizes}

    everything = {"rows8", "rows13", "rows16", "wave"}
    sums = [c for c in se.SOLVE_CASES if c.entry == "sums"]
    assert branches(c for c in sums if c.group == "size") == everything
    assert {n for c in sums if c.group == "size" for n in c.sizes} >= {1, 6, 7, 8, 9, 13, 14, 15, 16, 17, 32, 64, 65}
    assert branches(c for c in sums if c.group == "constraint") == everything
    assert {n for c in sums if c.group == "constraint" for n in c.sizes} >= {8, 9, 13, 14, 16, 17}
    assert branches(c for c in se.SOLVE_CASES if c.entry == "plain") == {"rows13", "rows16", "wave"}
    assert {n for c in sums if c.group == "joint-shape" for n in c.sizes} >= {14, 16, 18}
    modes = {(m, se.ldlt_branch(st.size), st.tikhonov == se.TIKHONOV)
             for c in se.SOLVE_CASES for st, m in zip(c.structures, c.modes)}
    assert {("zero", b, True) for b in ("rows8", "rows13", "rows16")} <= modes  # two diagonal values: ties
    assert {("coupled-ties", b, True) for b in ("rows8", "rows13", "rows16")} <= modes  # ... with entries beside them
    assert ("zero", "rows8", False) in modes                                       # an all-zero diagonal
    assert ("leaf-zero", "rows13", False) in modes and ("leaf-zero", "wave", False) in modes  # a zero pivot on the way
    assert ("nan", "rows13", True) in modes and ("nan", "wave", True) in modes and ("nan-h", "rows13", True) in modes
    for c in se.SOLVE_CASES:  # a NaN structure keeps its poses, its healthy neighbour moves
        if "nan" in c.modes or "nan-h" in c.modes:
            assert [m.startswith("nan") for m in c.modes] == [not mv for mv in c.moves] and any(c.moves)
    assert any(len({st.size for st in c.structures}) >= 3 and c.work_in_lds for c in se.SOLVE_CASES)
    assert any(len(c.structures) >= 2 and not c.work_in_lds for c in se.SOLVE_CASES)
    tracked = {se.ldlt_branch(st.size) for c in se.TRACK_CASES for st in c.structures
               if c.expect["auto"][0].startswith("tracking_step_tree")}
    assert tracked == everything
    constrained = {se.ldlt_branch(st.size) for c in se.TRACK_CASES for st in c.structures
                   if c.expect["auto"][0] == "tracking_step_tree_constrained_kernel" and st.n_rows}
    assert constrained == {"rows13", "wave"}


def test_both_sides_of_the_work_array_limit_have_a_case():
    """the count of the issue, checked: a fixed body-less root and N one-dof links need 35 722 floats at N = 27 and 38 988
    at N = 28; the LDS holds 38 912"""
    assert se.LDS_WORK_LIMIT_FLOATS == 38912
    assert se.lds_limit_pair() == (27, 28)
    assert se.tree_work_floats(28, 27, 0) == 35722 and se.tree_work_floats(29, 28, 0) == 38988
    by_id = {c.id: c for c in se.SOLVE_CASES}
    lo, hi = by_id["work-arrays-n27"], by_id["work-arrays-n28"]
    assert (lo.structures[0].n_links, lo.structures[0].dof, lo.work_in_lds) == (28, 27, True)
    assert (hi.structures[0].n_links, hi.structures[0].dof, hi.work_in_lds) == (29, 28, False)
    assert lo.structures[0].work_floats == 35722 and hi.structures[0].work_floats == 38988


def test_both_sides_of_the_one_launch_limits_have_a_case():
    e = {c.id: c for c in se.TRACK_CASES}
    tree = "tracking_step_tree_split_kernel"
    # 16 / 17 links
    assert (e["links-16"].structures[0].n_links, e["links-17"].structures[0].n_links) == (16, 17)
    assert e["links-16"].expect["auto"][0] == tree and e["links-16"].expect["segment"][0] == "tracking_step_tree_segment_kernel"
    assert set(k for k, _ in e["links-17"].expect.values()) == {""}
    assert e["links-17"].lds <= se.CU_LDS_BYTES  # (the link count refuses it, not the LDS)
    # sizes 64 / 65: the structure copy of 64 unknowns needs at least eleven links and does not fit the LDS next to the
    # tracking state -- the size limit of 64 is behind the LDS rule, whose own two sides are the padded-n38 / -n44 pair
    assert (e["padded-n64"].structures[0].size, e["padded-n65"].structures[0].size) == (64, 65)
    assert e["padded-n64"].structures[0].n_links <= se.FUSED_MAX_LINKS and e["padded-n64"].lds > se.CU_LDS_BYTES
    assert set(k for k, _ in e["padded-n64"].expect.values()) == {""} == set(k for k, _ in e["padded-n65"].expect.values())
    lo, hi = e["padded-n38"], e["padded-n44"]
    assert lo.lds <= se.CU_LDS_BYTES < hi.lds and hi.structures[0].size <= se.FUSED_MAX_SIZE
    assert lo.expect["auto"][0] == tree and set(k for k, _ in hi.expect.values()) == {""}
    assert e["links-16-bins32"].lds > se.CU_LDS_BYTES and e["links-16-bins32"].expect["auto"][0] == ""
    # 62 / 63 Newton steps
    assert (e["newton-31x2"].newton_steps, e["newton-9x7"].newton_steps) == (62, 63)
    assert e["newton-31x2"].expect["auto"][0] == tree and e["newton-9x7"].expect["auto"][0] == ""
    assert e["newton-9x7"].expect["segment"][0] == "tracking_step_tree_segment_kernel"
    assert e["newton-1x1"].newton_steps == 1 and e["newton-3x3"].newton_steps % 2 == 1
    # histogram bins: up to 16 the pair table is staged in LDS and no tree kernel runs (which leaves the split kernel's
    # own "at least 4 bins" nothing to refuse); 32 and 64 bins run them
    assert set(k for c in ("bins-2", "bins-16") for k, _ in e[c].expect.values()) == {""}
    assert e["bins-64"].expect["auto"] == (tree, [3, 8, 512])
    # more than 256 lines: one workgroup per link
    assert e["points300-lines257"].expect["auto"] == ("tracking_step_tree_kernel", [3, 1, 512])
    for c in se.TRACK_CASES:
        if c.constrained:
            assert all(c.expect[s] == ("tracking_step_tree_constrained_kernel", [3, 1, 512])
                       for s in ("auto", "parts2", "parts1"))
            assert c.expect["segment"][0] == "tracking_step_tree_segment_constrained_kernel"
    assert e["two-structures"].expect["auto"][1][0] == 6 and e["middle-untracked"].expect["auto"][1][0] == 2


# ---- the oracle against float64 ---------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _adjoint(pose):
    """Link::Adjoint, link.cpp:341-348"""
    r, t = pose[:3, :3], pose[:3, 3]
    out = np.zeros((6, 6))
    out[:3, :3] = r
    out[3:, :3] = _skew(t) @ r
    out[3:, 3:] = r
    return out


def _exp_so3(w):
    a = np.linalg.norm(w)
    k = _skew(w)
    if a < 1e-12:
        return np.eye(3) + k
    return np.eye(3) + np.sin(a) / a * k + (1.0 - np.cos(a)) / (a * a) * (k @ k)


def optimizer_end_f64(st, start, sums):
    """Optimizer::CalculateOptimization of an open tree in float64: the Jacobians of link.cpp:159-182, the projection
    sum J^T H J / sum J^T g (optimizer.cpp:309-321), the Tikhonov diagonal, numpy.linalg.solve, Link::UpdatePoses
    (link.cpp:205-241).  start: link_state of the structure; sums: [link in depth-first order][42].  Returns the new
    link_state."""
    assert st.open
    state = np.array(start, np.float64)
    l2w, j2p, b2j = state[:, 0], state[:, 1], state[:, 2]
    jac = {}
    a, b = np.zeros((st.dof, st.dof)), np.zeros(st.dof)
    for k, i in enumerate(st.order):
        link = st.links[i]
        j = np.zeros((6, st.dof))
        if link.parent >= 0:
            j = _adjoint(np.linalg.inv(j2p[i] @ b2j[i])) @ jac[link.parent]
        own = _adjoint(np.linalg.inv(b2j[i]))
        idx = st.first[i]
        for d in range(6):
            if link.free[d]:
                j[:, idx] = own[:, d]
                a[idx, idx] += st.tikhonov[0] if d < 3 else st.tikhonov[1]
                idx += 1
        jac[i] = j
        g = sums[k, :6].astype(np.float64)
        h = sums[k, 6:].astype(np.float64).reshape(6, 6).T  # (column-major)
        a -= j.T @ h @ j
        b += j.T @ g
    theta = np.linalg.solve(a, b)
    for i in st.order:
        link = st.links[i]
        th = np.zeros(6)
        idx = st.first[i]
        for d in range(6):
            if link.free[d]:
                th[d] = theta[idx]
                idx += 1
        var = np.eye(4)
        var[:3, :3] = _exp_so3(th[:3])
        var[:3, 3] = th[3:]
        if link.parent >= 0:
            if link.fixed_body2joint:
                j2p[i] = j2p[i] @ var
            else:
                b2j[i] = var @ b2j[i]
            l2w[i] = l2w[link.parent] @ j2p[i] @ b2j[i]
        else:
            l2w[i] = l2w[i] @ np.linalg.inv(b2j[i]) @ var @ b2j[i]
    return state


# Largest |pose entry of the oracle - float64| over every compared case after one round, as measured: 4.68e-7 (chain-n32;
# the smallest is 5.3e-8).  The assertion allows four times that.  It could not hide a dropped term: the smallest pose
# change of any compared case, 2.66e-3, is more than a thousand bounds away (a hundred are asserted below).
F64_MEASURED = 4.68e-7
F64_BOUND = 4 * F64_MEASURED
F64_CASES = [c for c in se.SOLVE_CASES if c.f64]


def test_the_f64_check_sees_every_open_tree_case():
    assert len(F64_CASES) >= 25
    assert {se.ldlt_branch(n) for c in F64_CASES for n in c.sizes} == {"rows8", "rows13", "rows16", "wave"}
    assert {n for c in F64_CASES for n in c.sizes} >= {1, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18, 32, 64, 65}
    assert all(c.f64 == (c.entry == "sums" and c.group in ("size", "lds-limit", "joint-shape", "mixed") or
                         c.id.startswith(("ties", "coupled-ties"))) for c in se.SOLVE_CASES)


@pytest.mark.parametrize("case", F64_CASES, ids=repr)
def test_oracle_step_equals_float64(case):
    run = _solve(case)
    sums = case.sums(0).reshape(-1, 42)
    first = 0
    for k, st in enumerate(case.structures):
        want = optimizer_end_f64(st, run.start[k], sums[first:first + st.n_links])
        first += st.n_links
        got = run.states[0][k].astype(np.float64)
        err = float(np.max(np.abs(got - want)))
        moved = float(np.max(np.abs(want - run.start[k])))
        print("f64 %s structure %d n %d: error %.3g moved %.3g" % (case.id, k, st.size, err, moved))
        assert err <= F64_BOUND
        assert moved >= 100 * F64_BOUND
