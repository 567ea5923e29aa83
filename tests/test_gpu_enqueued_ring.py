"""The ring of mapped argument blocks behind m3t_hip_reset_bodies, m3t_hip_reset_structures (one ring of four blocks per
context) and m3t_hip_judge_bodies (one per judge): more calls than the ring has blocks, queued without a wait in
between, so that a block comes round again while earlier calls may still be reading theirs -- and, for the resets, has
to be replaced by a larger one.  Against a twin context that makes the same calls with a Sync after every one: poses,
histograms and judgement rows bit for bit."""
import numpy as np
import pytest

import scenes
import structure_scenes as ss
import util
from test_gpu_reset_on_loss import KNOBS
from util import syn

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS + ("M3T_HIP_TREE_PARTS",):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def inputs():
    """4 Region bodies (the first four of the judge tests' six)"""
    return scenes.subset(scenes.Inputs(6, 7, n_divides=2), [0, 1, 2, 3])


def started(inputs):
    """a context with every frame staged in device-side rings: a new frame is a slot switch, nothing waits"""
    inst = scenes.Instance(util.open_hip(), inputs)
    scenes.stage_frames(inst.api, inst, inputs, inputs.n_frames)
    inst.tracker.select_slot(0)
    assert inst.tracker.StartModalities(0)
    return inst


def final_state(inst):
    assert inst.tracker.Sync()
    return [np.stack(inst.poses())] + [h for r in inst.region for h in r.histograms()]


def same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), i


def test_reset_bodies_reuses_and_regrows_its_blocks(inputs):
    """lists of 1 1 1 1 4 4 4 4 1 bodies: a call for one body (one region modality) needs 16 + 64 = 80 bytes, so every
    block is first allocated at 160; the calls for four need 32 + 256 = 288 and replace each of them; the ninth takes
    the first block a third time.  A tracking step behind every call."""
    lengths = [1, 1, 1, 1, 4, 4, 4, 4, 1]

    def run(sync):
        inst = started(inputs)
        for c, n in enumerate(lengths):
            k = 1 + c % (inputs.n_frames - 1)
            ids = [(c + i) % 4 for i in range(n)]
            inst.tracker.select_slot(k)
            assert inst.tracker.ResetBodies([inst.bodies[i] for i in ids], [np.asarray(inputs.gt[i][k], F) for i in ids], 0)
            if sync:
                assert inst.tracker.Sync()
            assert inst.tracker.ExecuteTrackingStep(k)
            if sync:
                assert inst.tracker.Sync()
        return final_state(inst)

    queued, synced = run(False), run(True)
    same(queued, synced)
    assert not np.array_equal(queued[0][0], np.asarray(inputs.start[0], F))  # (the bodies moved)


def test_judge_bodies_reuses_its_blocks(inputs):
    """six judgements with reset on loss queued back to back behind one tracking step, no read in between: the fifth
    and sixth take the blocks of the first and second.  Every second call judges two bodies against ground truth 0.2 m
    away, so bodies are found lost and reset from the block's poses."""
    def run(sync):
        inst = started(inputs)
        inst.tracker.select_slot(1)
        assert inst.tracker.ExecuteTrackingStep(1)
        judge = inst.tracker.CreateJudge(inst.bodies, 6)
        for c in range(6):
            gt = [np.asarray(inputs.gt[i][1], F).copy() for i in range(4)]
            if c % 2:
                gt[c % 4][0, 3] += F(0.2)
                gt[(c + 1) % 4][1, 3] -= F(0.2)
            assert judge.judge(gt, 0) == c
            if sync:
                assert inst.tracker.Sync()
        rows = judge.read(0, 6)
        return rows, final_state(inst)

    (rows_q, state_q), (rows_s, state_s) = run(False), run(True)
    assert rows_q.tobytes() == rows_s.tobytes()
    same(state_q, state_s)
    # an odd call finds the two bodies lost whose ground truth it moved and puts them there; the even call behind it
    # judges against the unmoved ground truth, finds the same two lost and puts them back
    lost = [set()] + [{c % 4, (c + 1) % 4} if c % 2 else {(c - 1) % 4, c % 4} for c in range(1, 6)]
    assert [set(np.flatnonzero(r["was_reset"])) for r in rows_q] == lost


def test_reset_structures_reuses_its_blocks():
    """five calls on two chains of two links, one and two listed structures in turn (176 and 352 bytes: the blocks
    allocated for one structure, at twice their size, hold two exactly), a tracking step behind every call"""
    chain_inputs, joint2parent, gt = ss.chain_inputs(3)
    gt_poses = [(a.astype(F), b.astype(F)) for a, b, _ in gt]
    angle = gt[0][2]

    def run(sync):
        api = util.open_hip()
        structures = []
        for s in range(2):
            start_a = syn.perturb_pose(gt_poses[0][0], np.random.default_rng(5 + s), rot_deg=0.5, trans=0.001)
            structures.append(ss.two_body_chain(api, chain_inputs, joint2parent, start_a, angle + 0.01))
        tracker = structures[0].tracker
        for st in structures:
            ss.upload(st, chain_inputs, 0)
        assert tracker.StartModalities(0)
        for c in range(5):
            due = [c // 2 % 2] if c % 2 == 0 else [0, 1]
            poses = [p for s in due for p in ss.reset_poses(gt_poses[c % 3], 10 * c + s)]
            assert tracker.ResetStructures([structures[s].optimizer for s in due], poses, 0, 0)
            if sync:
                assert tracker.Sync()
            assert tracker.ExecuteTrackingStep(c)
            if sync:
                assert tracker.Sync()
        assert tracker.Sync()
        return [x for st in structures for x in st.state()]

    same(run(False), run(True))
