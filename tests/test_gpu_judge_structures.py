"""The structure judgement of m3t_hip_judge_* (RTBEvaluator::CalculatePoseResults, examples/rtb_evaluator.cpp:930-989)
on the device: the structure rows against tests/structure_reference.py applied to the judge's own per-body rows, bit
for bit, with bodies in one workgroup, split over two and beyond a vertex tile; the per-body rows against
tests/judge_reference.py; evaluate_rtb_sequences judged on the device against the host-judged run, with sequences of
unequal length (ResetStructures mid-batch) and nothing read before the end; the refused calls."""
import numpy as np
import pytest

import judge_reference as jr
import structure_reference as sref
import structure_scenes as ss
import util
from test_structure_reference import JudgeEvaluation, rtb_sequences, rtb_structure
from util import host, syn

pytestmark = pytest.mark.gpu

capi = util.pkg._capi
ev = util.pkg.evaluation
F = np.float32
INVALID = capi.M3T_ERR_INVALID_ARGUMENT
VERTEX_COUNTS = (5, 257, 1025, 257)  # one workgroup; split over two; beyond M3T_JUDGE_TILE; the second structure's body
STRUCTURES = [[[0, 1], [2]], [[3]]]  # a two-body group plus a one-body group; a single group
THRESHOLDS = [0.05, 0.02]


def test_structure_rows_follow_the_body_rows_bit_for_bit():
    rng = np.random.default_rng(31)
    vertices = [rng.uniform(-0.05, 0.05, (n, 3)).astype(F) for n in VERTEX_COUNTS]
    poses = [syn.make_pose(syn.rot_vec(rng.normal(size=3) * 0.5), [0.1 * i, 0.0, 0.6]).astype(F) for i in range(4)]
    api = util.open_hip()
    bodies = [host.Body(api, p) for p in poses]
    tracker = host.Tracker(api)
    judge = tracker.CreateJudge(bodies, 3)
    # a group's body without vertices is refused; so is a list that does not start at 0
    judge.set_vertices(0, vertices[0])
    first_group, first_index, listed = np.asarray([0, 2, 3], np.int32), np.asarray([0, 2, 3, 4], np.int32), np.asarray([0, 1, 2, 3], np.int32)
    thr = np.asarray(THRESHOLDS, F)
    args = (capi.iptr(first_group), capi.iptr(first_index), capi.iptr(listed), capi.fptr(thr))
    assert api.raw("judge_set_structures", judge.id, 2, *args) == INVALID and "vertices" in api.last_error()
    for i in range(1, 4):
        judge.set_vertices(i, vertices[i])
    assert api.raw("judge_set_structures", judge.id, 2, capi.iptr(np.asarray([1, 2, 3], np.int32)), *args[1:]) == INVALID
    assert api.raw("judge_set_structures", judge.id, 0, *args) == INVALID
    assert api.raw("judge_read_structures", judge.id, 0, 0, None) == INVALID  # no structures set yet
    judge.set_structures(STRUCTURES, THRESHOLDS)
    # three frames of rows: the pose itself (error 0), small deltas around the thresholds, a delta beyond them
    scales = [0.0, 0.012, 0.2]
    gts = []
    for scale in scales:
        gt = []
        for i, p in enumerate(poses):
            delta = syn.make_pose(syn.rot_vec(rng.normal(size=3) * scale), rng.normal(size=3) * scale * (0.5 + i))
            gt.append((p.astype(np.float64) @ delta).astype(F) if scale else p.copy())
        gts.append(gt)
        judge.judge(gt, -1)
    rows, srows = judge.read(0, 3), judge.read_structures(0, 3)
    for k in range(3):
        for i in range(4):  # the per-body rows, as tests/test_gpu_judge_bodies.py holds them
            t_err, r_err, cosine, success = jr.pose_errors(poses[i], gts[k][i])
            assert rows[k, i]["translation_error"].tobytes() == t_err.tobytes()
            assert rows[k, i]["rotation_cosine"].tobytes() == cosine.tobytes()
            add, adds = jr.add_adds(vertices[i], poses[i], gts[k][i])
            print(k, i, rows[k, i]["add_error"], add, rows[k, i]["adds_error"], adds)
            assert abs(float(rows[k, i]["add_error"]) - float(add)) <= 2e-5 * abs(float(add)) + 1e-7
            assert abs(float(rows[k, i]["adds_error"]) - float(adds)) <= 2e-5 * abs(float(adds)) + 1e-7
        for s, groups in enumerate(STRUCTURES):
            want = sref.structure_judgement(rows[k]["add_error"], rows[k]["adds_error"], groups, F(THRESHOLDS[s]))
            got = srows[k, s]
            print(k, s, got, want)
            assert got["add_auc"].tobytes() == want[0].tobytes() and got["adds_auc"].tobytes() == want[1].tobytes()
            assert (int(got["add_curve_zeros"]), int(got["adds_curve_zeros"])) == want[2:]
    # (frame 0: delta = pose^-1 * pose is the identity up to the rounding of a rotation that is orthonormal in f32 only,
    # so the errors are ~1e-8, not 0; the exact closed forms are in tests/test_structure_reference.py)
    assert all(a > 0.9999 for a in srows[0]["add_auc"]) and srows[0]["add_curve_zeros"].tolist() == [100, 100]
    assert srows[2]["add_auc"].tolist() == [0.0, 0.0] and srows[2]["add_curve_zeros"].tolist() == [0, 0]
    assert 0.0 < srows[1, 0]["add_auc"] < 1.0 and 0 < srows[1, 0]["add_curve_zeros"] < 100
    # rows that have not been judged, and a change of the structures while rows are held
    assert api.raw("judge_read_structures", judge.id, 0, 4, None) == INVALID
    assert api.raw("judge_set_structures", judge.id, 2, *args) == INVALID and "judge_clear" in api.last_error()
    judge.clear()
    judge.set_structures([[[3], [0]]], [0.1])
    judge.judge(gts[1], -1)
    again = judge.read(0, 1)[0]
    assert again.tobytes() == rows[1].tobytes()  # the per-body rows do not depend on the structures
    want = sref.structure_judgement(again["add_error"], again["adds_error"], [[3], [0]], F(0.1))
    got = judge.read_structures(0, 1)[0, 0]
    assert got["add_auc"].tobytes() == want[0].tobytes() and int(got["adds_curve_zeros"]) == want[3]


def test_evaluate_rtb_sequences_judged_on_the_device(monkeypatch):
    """two chains in one context, sequences of 3 + 3 and of 4 images: the first structure is put on its second sequence
    with ResetStructures while the second keeps tracking.  The device-judged run equals the host-judged one field for
    field, and its loop reads nothing: no Sync, no pose, one read of the rows at the end."""
    inputs, joint2parent, gt = ss.chain_inputs(5)
    poses = [(a.astype(F), b.astype(F)) for a, b, _ in gt]
    angles = [angle for _, _, angle in gt]
    vertices = [inputs.vertices[0][:257], inputs.vertices[1][:40]]
    sequences = [rtb_sequences(poses, [3, 3]), rtb_sequences(poses, [4])]
    first_image = [[0, 2], [0]]
    runs = {}
    for on_device in (False, True):
        api = util.open_hip()
        chains = [ss.two_body_chain(api, inputs, joint2parent, poses[0][0], angles[0]) for _ in range(2)]
        structures = [rtb_structure(chains[0], vertices, groups=((0, 1),)),
                      rtb_structure(chains[1], vertices, groups=((0,), (1,)), error_threshold=0.03)]
        resets, reads = [], []
        reset_structures = host.Tracker.ResetStructures
        monkeypatch.setattr(host.Tracker, "ResetStructures",
                            lambda self, opts, *a: resets.append([o.id for o in opts]) or reset_structures(self, opts, *a))
        if on_device:
            def refuse(*a, **kw):
                raise AssertionError("the device-judged loop reads nothing")
            monkeypatch.setattr(host.Tracker, "Sync", refuse)
            monkeypatch.setattr(host.Body, "body2world_pose", refuse)
            monkeypatch.setattr(host.Judge, "read", refuse)
            read_structures = host.Judge.read_structures
            monkeypatch.setattr(host.Judge, "read_structures",
                                lambda self, *a: reads.append(a) or read_structures(self, *a))
        runs[on_device] = ev.evaluate_rtb_sequences(
            chains[0].tracker, structures, sequences,
            lambda s, q, k: ss.upload(chains[s], inputs, first_image[s][q] + k), judge_on_device=on_device)
        monkeypatch.undo()
        assert resets == [[chains[0].optimizer.id, chains[1].optimizer.id], [chains[0].optimizer.id]], resets
        if on_device:
            assert len(reads) == 1, reads
    host_run, device_run = runs[False], runs[True]
    assert [[len(q) for q in s] for s in host_run] == [[2, 2], [3]]
    for s in range(2):
        for q in range(len(host_run[s])):
            for a, b in zip(host_run[s][q], device_run[s][q]):
                import selective_reset
                selective_reset.same_results(a, b)
    assert 0.0 < host_run[0][1][0]["add_auc"] < 1.0
