"""The case table of tests/fused_edges.py against the oracle alone (no GPU): every case is *live* -- finite poses, the
objects that must move do and the empty ones keep their start pose bit for bit, the valid-line / valid-point counts lie
in the bracket the case states -- and the table covers what tests/test_gpu_fused_edges.py claims to cover.  This is the
guard against a device matrix that is green because its cases are degenerate."""
import numpy as np
import pytest

import fused_edges as fe
import scenes
import util
from util import syn

_runs = {}


def _oracle(case):
    if case.id not in _runs:
        _runs[case.id] = fe.oracle_run(case)
    return _runs[case.id]


@pytest.mark.parametrize("case", fe.ALL_CASES, ids=repr)
def test_case_is_live_in_the_oracle(case):
    ref = _oracle(case)
    assert ref.started and len(ref.poses) == 3
    assert all(np.isfinite(p).all() for p in ref.poses)
    print(case.id, "lines", ref.n_lines, "points", ref.n_points)
    for i in range(case.n_objects):
        moved = not np.array_equal(ref.poses[-1][i], ref.start[i])
        assert moved == case.moves[i], (i, moved)
        if not case.moves[i]:
            assert all(np.array_equal(p[i], ref.start[i]) for p in ref.poses), i
    if case.has_region:
        assert len(ref.n_lines) == case.n_objects
        for i, (lo, hi) in enumerate(case.lines):
            assert lo <= ref.n_lines[i] <= hi, (i, ref.n_lines[i], lo, hi)
        for i in case.empty:
            assert ref.n_lines[i] == 0 and not case.moves[i]
            for a, b in zip(ref.hist[i], ref.hist_start[i]):
                assert np.array_equal(a, b)
    if case.with_depth:
        assert len(ref.n_points) == case.n_objects
        for i, (lo, hi) in enumerate(case.points):
            assert lo <= ref.n_points[i] <= hi, (i, ref.n_points[i], lo, hi)


def test_scale_reaches_the_walk():
    """the nine scale lists end in nine different poses"""
    cases = [c for c in fe.CASES if c.group == "scale"]
    assert sorted(c.first_scale for c in cases) == list(range(1, 10))
    final = [_oracle(c).poses[-1] for c in cases]
    for i in range(len(final)):
        for j in range(i):
            assert not np.array_equal(final[i], final[j]), (cases[i].id, cases[j].id)


def test_compact_line_limit_needs_the_300_point_model():
    """with the default 200-point models n_lines_max 256 and 257 both clamp to 200 lines (region_modality.cpp:426-430):
    only the 300-point model makes 256 / 257 a boundary of the compact kernel"""
    inputs = scenes.Inputs(2, 3, n_divides=2)
    for n_lines_max in (256, 257):
        inst = scenes.Instance(util.open_oracle(), inputs, region_params=dict(syn.RBOT_REGION_PARAMS, n_lines_max=n_lines_max))
        inst.upload_frame(0)
        assert inst.tracker.StartModalities(0) and inst.tracker.ExecuteTrackingStep(0)
        assert [len(r.data_lines()) for r in inst.region] == [200, 200]


def test_the_small_table_overflows_where_the_matrix_says_so():
    """the "compact_cap64" shape: in every 32-bin case that takes the table kernel the first walk already meets more
    than 64 + 32 mixed bins in some object (the walk with table->fits == false runs, the host leaves the table after
    frame 0) -- except with 5 and 10 lines, whose histograms never hold 64 mixed bins: there the small table fits"""
    seen = 0
    for case in fe.CASES:
        if case.unsupported or case.expect["compact_cap64"][0] != "tracking_step_compact_table_kernel":
            continue
        ref = _oracle(case)
        mixed = [[fe.mixed_bins(f, b) for f, b in frame] for frame in ref.hist_frames]
        print(case.id, mixed)
        kernels = fe.table_kernels(ref, 3)
        assert kernels[0] == "tracking_step_compact_table_kernel"
        if case.small_histograms:
            assert max(max(m) for m in mixed) <= fe.TABLE_CAP and kernels == [kernels[0]] * 3
        elif case.region_params["n_histogram_bins"] == 32:
            assert max(mixed[0]) > fe.TABLE_CAP + fe.TABLE_CAP // 2
            assert kernels[1:] == ["tracking_step_compact_kernel"] * 2
            seen += 1
    assert seen >= 9 + 6  # the nine first scales among them


def test_table_is_well_formed():
    ids = [c.id for c in fe.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert len(fe.SHAPES_REGION) == 9 and len(fe.SHAPES_DEPTH) == 9
    assert len(fe.PAIRS) == len(fe.CASES) * 9 + len(fe.CASES_DEPTH) * 9
    for case in fe.ALL_CASES:
        assert case.n_objects <= 8  # 16 parts per object still fit the GPU
        assert set(case.expect) == set(case.shapes)
        for kernel, parts, threads in case.expect.values():
            assert kernel.startswith("tracking_step_") and kernel.endswith("_kernel")
            assert parts in (1, 2, 8, 16) and threads in (128, 256, 512)
        assert len(case.moves) == len(case.lines) == len(case.points) == case.n_objects
    groups = {c.group for c in fe.ALL_CASES}
    assert groups == {"scale", "refused-scale", "lengths", "bins", "few-lines", "compact-limit", "many-lines", "ragged",
                      "image", "depth"}


def test_coverage_of_the_scale_templates():
    """every first scale 1..9 is walked by the compact kernel, by the table kernel with the table fitting and with the
    table too small; every first scale 1..9, 10 and 12 by a split kernel and by a one-workgroup kernel"""
    def kernels(shape):
        return {c.first_scale: c.expect[shape][0] for c in fe.CASES if c.group in ("scale", "refused-scale")}

    for s in range(1, 10):
        assert kernels("compact")[s] == "tracking_step_compact_kernel"
        assert kernels("compact_table")[s] == "tracking_step_compact_table_kernel"
        assert kernels("compact_cap64")[s] == "tracking_step_compact_table_kernel"
    for s in list(range(1, 10)) + [10, 12]:
        for shape in ("split", "split16", "split2"):
            assert kernels(shape)[s] == "tracking_step_split_kernel"
        for shape in ("wg512", "wg256", "wg128"):
            assert kernels(shape)[s] == "tracking_step_kernel"
    for s in (10, 12):  # refused: the one-workgroup kernel in every compact shape
        for shape in ("compact", "compact_table", "compact_cap64"):
            assert kernels(shape)[s] == "tracking_step_kernel"


def test_eligibility_rules_as_the_table_states_them():
    """the rows of the ineligibility group, spelled out (parity section)"""
    e = {c.id: c.expect for c in fe.ALL_CASES}
    for cid in ("lengths-6-10", "lengths-4-16", "lengths-10-8", "lengths-16-16", "lengths-1-2", "points300-lines257"):
        for shape in ("compact", "compact_table", "compact_cap64"):
            assert e[cid][shape] == ("tracking_step_kernel", 1, 512), (cid, shape)
    assert e["lengths-8-12"]["compact"][0] == "tracking_step_compact_kernel"
    assert e["points300-lines256"]["compact"] == ("tracking_step_compact_kernel", 1, 256)
    assert e["points300-lines256"]["split16"] == ("tracking_step_split_kernel", 16, 512)
    for shape in ("split", "split16", "split2"):
        assert e["points300-lines257"][shape] == ("tracking_step_kernel", 1, 512)
        assert e["bins-2"][shape] == ("tracking_step_lds_kernel", 1, 512)
        assert e["bins-4"][shape][0] == "tracking_step_split_kernel"
    table = {b: e["bins-%d" % b]["compact_table"][0] for b in (2, 4, 8, 16, 32, 64)}
    assert table == {2: "tracking_step_compact_kernel", 4: "tracking_step_compact_kernel", 8: "tracking_step_compact_kernel",
                     16: "tracking_step_compact_table_kernel", 32: "tracking_step_compact_table_kernel",
                     64: "tracking_step_compact_kernel"}
    staged = {b: e["bins-%d" % b]["wg512"][0] for b in (2, 4, 8, 16, 32, 64)}
    assert staged == {2: "tracking_step_lds_kernel", 4: "tracking_step_lds_kernel", 8: "tracking_step_lds_kernel",
                      16: "tracking_step_lds_kernel", 32: "tracking_step_kernel", 64: "tracking_step_kernel"}
    assert [c.id for c in fe.ALL_CASES if c.unsupported] == ["points600-lines513", "points600-lines600"]
    d = e["depth-points-200"]
    assert d["split"] == ("tracking_step_split_pair_kernel", 8, 512) and d["split_nopair"][0] == "tracking_step_split_kernel"
    assert d["wg256"] == ("tracking_step_lds_pair_kernel", 1, 256)
    assert d["compact"] == ("tracking_step_compact_kernel", 1, 256) and d["compact_wide"] == ("tracking_step_compact_wide_kernel", 1, 512)
    only = e["depth-only-zero-frames"]  # no RegionModality in the batch: nothing to pair, no table to stage
    assert only["split"][0] == "tracking_step_split_kernel" and only["wg512"][0] == "tracking_step_kernel"
