"""m3t_hip_reset_structures (RTBEvaluator::SetBodyAndJointPoses + StartModalities for the listed structures of a batch,
and for no other) on the device: three two-body chains in ONE HIP context, reset on a fixed schedule, against each
structure tracked in an oracle context of its own where the harness sets the body poses and the joints of
tests/structure_reference.py and calls StartModalities(0) -- body poses, joint poses and histograms after every step,
bit for bit, in every step kernel; that the call leaves the other structures alone; a joint whose body2joint tracking
has moved; the constrained mode; Region + Depth links; shared ColorHistograms; single links; the refused calls."""
import numpy as np
import pytest

import scenes
import structure_reference as sref
import structure_scenes as ss
import util
from test_gpu_reset_on_loss import KNOBS, kernel_of
from util import host, syn

pytestmark = pytest.mark.gpu

capi = util.pkg._capi
fptr, iptr, pose_arg = capi.fptr, capi.iptr, capi.pose_arg
F = np.float32
INVALID, UNSUPPORTED = capi.M3T_ERR_INVALID_ARGUMENT, capi.M3T_ERR_UNSUPPORTED
N_FRAMES = 4


def set_knobs(monkeypatch, env):
    for k in KNOBS + ("M3T_HIP_TREE_PARTS",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def raw_reset(api, optimizers, poses, mode=0, iteration=0, n=None):
    ids = np.asarray([o if isinstance(o, int) else o.id for o in optimizers], np.int32)
    flat = np.ascontiguousarray(np.concatenate([pose_arg(p) for p in poses]) if len(poses) else np.zeros(16, F), F)
    return api.raw("reset_structures", iptr(ids), len(ids) if n is None else n, fptr(flat), mode, iteration)


@pytest.fixture(scope="module")
def chain():
    inputs, joint2parent, gt = ss.chain_inputs(N_FRAMES)
    return inputs, joint2parent, [(a.astype(F), b.astype(F)) for a, b, _ in gt], [angle for _, _, angle in gt]


def chain_builder(chain, **kw):
    inputs, joint2parent, gt, angles = chain

    def build(api, s):
        start_a = syn.perturb_pose(gt[0][0], np.random.default_rng(5 + s), rot_deg=0.5, trans=0.001)
        return ss.two_body_chain(api, inputs, joint2parent, start_a, angles[0] + 0.01, **kw)
    return build


@pytest.fixture(scope="module")
def chain_singles(chain):
    """the expectation, computed once: every structure of the batch in an oracle context of its own"""
    return [ss.run_single(util.open_oracle(), chain_builder(chain), s, chain[0], chain[2]) for s in range(3)]


def assert_batch_equals_singles(states, singles):
    for k, frame in enumerate(states):
        for s, state in enumerate(frame):
            ss.same_state(state, singles[s][k])


# ---- 1. the schedule in every step kernel -----------------------------------------------------------------------------
CASES = {
    "one-launch tree kernel": ({"M3T_HIP_TREE_PARTS": "1"}, None, "tracking_step_tree_kernel"),
    "split tree kernel": ({"M3T_HIP_TREE_PARTS": "4"}, None, "tracking_step_tree_split_kernel"),
    "unfused sub-steps": ({}, 0, ""),
}


@pytest.mark.parametrize("case", list(CASES))
def test_three_chains_reset_on_schedule_match_the_single_runs(chain, chain_singles, case, monkeypatch):
    env, fused, kernel = CASES[case]
    set_knobs(monkeypatch, env)
    kernels = []
    states = ss.run_batch(util.open_hip(), chain_builder(chain), 3, chain[0], chain[2],
                          setup=(lambda api: api.call("set_fused_step", fused)) if fused is not None else None,
                          after_step=lambda api: kernels.append(kernel_of(api)))
    assert set(kernels) == {kernel}, kernels
    assert_batch_equals_singles(states, chain_singles)
    # the resets did something: a reset structure's pose before the step differs from the free-running one
    assert not np.array_equal(states[2][1][0], states[2][0][0])


# ---- 2. neighbours ----------------------------------------------------------------------------------------------------
def test_reset_structures_leaves_every_other_structure_alone(chain, monkeypatch):
    set_knobs(monkeypatch, {})
    inputs, _, gt, _ = chain
    contexts = []
    for _ in range(2):
        api = util.open_hip()
        structures = [chain_builder(chain)(api, s) for s in range(3)]
        for st in structures:
            ss.upload(st, inputs, 0)
        assert structures[0].tracker.StartModalities(0)
        for k in (0, 1):
            for st in structures:
                ss.upload(st, inputs, k)
            assert structures[0].tracker.ExecuteTrackingStep(k)
        contexts.append(structures)
    inst, twin = contexts
    before = [st.state() for st in inst]
    poses = ss.reset_poses(gt[2], 1)
    assert inst[0].tracker.ResetStructures([inst[1].optimizer], poses, 0, 0)
    after = [st.state() for st in inst]
    for s in (0, 2):
        ss.same_state(after[s], before[s])
    assert np.array_equal(after[1][0], poses[0]) and np.array_equal(after[1][1], poses[1])
    expected_joint = sref.joint2parent_pose(poses[0], poses[1], before[1][3])
    assert np.array_equal(after[1][2], expected_joint) and np.array_equal(after[1][3], before[1][3])
    assert not np.array_equal(after[1][4], before[1][4])  # histograms started again
    for k in (2, 3):
        for structures in contexts:
            for st in structures:
                ss.upload(st, inputs, k)
            assert structures[0].tracker.ExecuteTrackingStep(k)
        for s in (0, 2):
            ss.same_state(inst[s].state(), twin[s].state())
        assert not np.array_equal(inst[1].state()[0], twin[1].state()[0])


# ---- 3. a joint whose body2joint tracking has moved -------------------------------------------------------------------
def three_link_chain(api, inputs, start):
    """A free -- B on a revolute joint with fixed_body2joint_pose = 0 and a non-identity body2joint -- C revolute"""
    rp = dict(syn.RBOT_REGION_PARAMS)
    models = [host.RegionModel(api, data_points=m[0], orientations=m[1], contour_lengths=m[2]) for m in inputs.region_models]
    bodies = [host.Body(api, np.eye(4)) for _ in range(3)]
    cams = [host.ColorCamera(api, **inputs.intr) for _ in range(3)]
    mods = [host.RegionModality(api, bodies[i], cams[i], models[i], **rp) for i in range(3)]
    b2j = syn.make_pose(syn.rot_vec([0.1, -0.2, 0.15]), [0.01, -0.02, 0.005])
    la = host.Link(api, body=bodies[0])
    lb = host.Link(api, body=bodies[1], parent=la, body2joint_pose=b2j, free_directions=(0, 0, 1, 0, 0, 0),
                   joint2parent_pose=syn.make_pose(syn.rot_vec([0.2, -0.1, 0.3]), [0.05, 0.01, 0.0]),
                   fixed_body2joint_pose=False)
    lc = host.Link(api, body=bodies[2], parent=lb, free_directions=(0, 0, 1, 0, 0, 0),
                   joint2parent_pose=syn.make_pose(syn.rot_vec([-0.1, 0.25, 0.05]), [0.04, -0.02, 0.01]))
    for link, mod in zip((la, lb, lc), mods):
        link.AddModality(mod)
    opt = host.Optimizer(api, root_link=la)
    st = ss.Structure(opt, [(la, bodies[0], -1), (lb, bodies[1], 0), (lc, bodies[2], 1)], cams, mods)
    st.tracker = host.Tracker(api, 7, 2)
    bodies[0].set_body2world_pose(start)
    assert st.tracker.CalculateConsistentPoses()
    return st


def test_a_moved_body2joint_is_read_from_the_device(monkeypatch):
    """two tracked frames move body2joint of the middle link on the device; the reset's joint2parent follows from THAT
    value (the oracle's own, read back at the reset), not from the pose the link was created with"""
    set_knobs(monkeypatch, {})
    inputs = scenes.Inputs(3, 4, n_divides=2)
    start = inputs.gt[0][0]
    target = [syn.perturb_pose(inputs.gt[i][2], np.random.default_rng(40 + i), rot_deg=1.0, trans=0.002).astype(F) for i in range(3)]
    results = {}
    for name, api in (("hip", util.open_hip()), ("oracle", util.open_oracle())):
        st = three_link_chain(api, inputs, start)
        created = st.links[1][0].body2joint_pose()
        ss.upload(st, inputs, 0)
        assert st.tracker.StartModalities(0)
        for k in (0, 1):
            ss.upload(st, inputs, k)
            assert st.tracker.ExecuteTrackingStep(k)
        if name == "hip":
            assert st.tracker.ResetStructures([st.optimizer], target, 0, 0)
        else:
            assert not np.array_equal(st.links[1][0].body2joint_pose(), created)  # tracking did move it
            st.reset_on_host(st.tracker, target)
            assert st.tracker.StartModalities(0)
        out = [st.state()]
        ss.upload(st, inputs, 2)
        assert st.tracker.ExecuteTrackingStep(2)
        out.append(st.state())
        results[name] = out
    for a, b in zip(results["hip"], results["oracle"]):
        ss.same_state(a, b)


# ---- 4. the constrained mode: a body-less root, two children, one hard constraint -----------------------------------
def constrained_pair(api, inputs, start):
    rp = dict(syn.RBOT_REGION_PARAMS)
    models = [host.RegionModel(api, data_points=m[0], orientations=m[1], contour_lengths=m[2]) for m in inputs.region_models]
    bodies = [host.Body(api, np.eye(4)) for _ in range(2)]
    cams = [host.ColorCamera(api, **inputs.intr) for _ in range(2)]
    mods = [host.RegionModality(api, bodies[i], cams[i], models[i], **rp) for i in range(2)]
    root = host.Link(api)
    la = host.Link(api, body=bodies[0], parent=root, joint2parent_pose=start[0])
    lb = host.Link(api, body=bodies[1], parent=root, joint2parent_pose=start[1])
    la.AddModality(mods[0])
    lb.AddModality(mods[1])
    opt = host.Optimizer(api, root_link=root)
    a_t_b = np.linalg.inv(start[0].astype(np.float64)) @ start[1].astype(np.float64)
    host.Constraint(api, opt, la, lb, body12joint1_pose=np.linalg.inv(a_t_b), body22joint2_pose=np.eye(4),
                    constraint_directions=(0, 0, 0, 1, 1, 1))
    st = ss.Structure(opt, [(root, None, -1), (la, bodies[0], 0), (lb, bodies[1], 0)], cams, mods, mode=1)
    st.tracker = host.Tracker(api, 7, 2)
    assert st.tracker.CalculateConsistentPoses()
    return st


def test_constrained_mode_on_a_bodyless_root(monkeypatch):
    set_knobs(monkeypatch, {})
    inputs = scenes.Inputs(2, 4, n_divides=2)
    start = [inputs.gt[0][i].astype(F) for i in range(2)]
    target = [syn.perturb_pose(inputs.gt[i][2], np.random.default_rng(60 + i), rot_deg=0.5, trans=0.001).astype(F) for i in range(2)]
    results = {}
    for name, api in (("hip", util.open_hip()), ("oracle", util.open_oracle())):
        st = constrained_pair(api, inputs, start)
        ss.upload(st, inputs, 0)
        assert st.tracker.StartModalities(0)
        for k in (0, 1):
            ss.upload(st, inputs, k)
            assert st.tracker.ExecuteTrackingStep(k)
        root_before = st.links[0][0].link2world_pose()
        if name == "hip":
            assert raw_reset(api, [st.optimizer], target, mode=0) == UNSUPPORTED  # the root has no body
            assert st.tracker.ResetStructures([st.optimizer], target, 1, 0)
            assert np.array_equal(st.links[1][0].joint2parent_pose(), target[0])
            assert np.array_equal(st.links[2][0].joint2parent_pose(), target[1])
            assert np.array_equal(st.links[0][0].link2world_pose(), root_before)
        else:
            st.reset_on_host(st.tracker, target)
            assert st.tracker.StartModalities(0)
        out = [st.state()]
        for k in (2, 3):
            ss.upload(st, inputs, k)
            assert st.tracker.ExecuteTrackingStep(k)
            out.append(st.state())
        results[name] = out
    for a, b in zip(results["hip"], results["oracle"]):
        ss.same_state(a, b)


# ---- 4b. Region + Depth links ------------------------------------------------------------------------------------------
def depth_chain(api, inputs, joint2parent, start_a, start_angle):
    """test_gpu_multibody.DepthChain with its modalities kept: a RegionModality (measured occlusions) and a
    DepthModality on each of the two links, YCB parameters"""
    rp, dp = dict(syn.YCB_REGION_PARAMS, n_histogram_bins=32), dict(syn.YCB_DEPTH_PARAMS)
    bodies = [host.Body(api, np.eye(4)), host.Body(api, np.eye(4))]
    cams = [host.ColorCamera(api, **inputs.intr) for _ in range(2)]
    dcams = [host.DepthCamera(api, depth_scale=inputs.depth_scale, **inputs.intr) for _ in range(2)]
    rmodels = [host.RegionModel(api, data_points=m[0], orientations=m[1], contour_lengths=m[2]) for m in inputs.region_models]
    dmodels = [host.DepthModel(api, data_points=m[0], orientations=m[1], surface_areas=m[2]) for m in inputs.depth_models]
    la = host.Link(api, body=bodies[0])
    lb = host.Link(api, body=bodies[1], parent=la, free_directions=(0, 0, 1, 0, 0, 0),
                   joint2parent_pose=joint2parent @ syn.make_pose(syn.rot_vec([0, 0, start_angle]), [0, 0, 0]))
    region = []
    for i, link in enumerate((la, lb)):
        region.append(host.RegionModality(api, bodies[i], cams[i], rmodels[i], depth_camera=dcams[i], **rp))
        link.AddModality(region[-1])
        link.AddModality(host.DepthModality(api, bodies[i], dcams[i], dmodels[i], **dp))
    st = ss.Structure(host.Optimizer(api, root_link=la), [(la, bodies[0], -1), (lb, bodies[1], 0)], list(zip(cams, dcams)), region)
    st.tracker = host.Tracker(api, 4, 2)
    bodies[0].set_body2world_pose(start_a)
    assert st.tracker.CalculateConsistentPoses()
    return st


def test_region_and_depth_links(monkeypatch):
    """two DepthChain structures in one context, the second reset before frame 2, against the single runs"""
    set_knobs(monkeypatch, {})
    inputs = scenes.Inputs(2, 1, n_divides=2, with_depth=True)
    rng = np.random.default_rng(11)
    joint2parent = syn.make_pose(syn.rot_vec([0.3, -0.2, 0.1]), [0.16, 0.02, 0.0])
    pose_a, angle, gt, angles = inputs.gt[0][0].copy(), 0.2, [], []
    inputs.frames = [[], []]
    for k in range(3):
        pose_a = syn.perturb_pose(pose_a, rng, rot_deg=0.7, trans=0.002)
        angle += rng.uniform(-0.03, 0.03)
        pose_b = pose_a @ joint2parent @ syn.make_pose(syn.rot_vec([0, 0, angle]), [0, 0, 0])
        gt.append((pose_a.astype(F), pose_b.astype(F)))
        angles.append(angle)
        inputs.frames[0].append(inputs.scenes[0].render(pose_a))
        inputs.frames[1].append(inputs.scenes[1].render(pose_b))

    def build(api, s):
        start_a = syn.perturb_pose(gt[0][0], np.random.default_rng(5 + s), rot_deg=0.5, trans=0.001)
        return depth_chain(api, inputs, joint2parent, start_a, angles[0] + 0.01)
    schedule = {1: 2}
    singles = [ss.run_single(util.open_oracle(), build, s, inputs, gt, schedule) for s in range(2)]
    states = ss.run_batch(util.open_hip(), build, 2, inputs, gt, schedule)
    assert_batch_equals_singles(states, singles)


# ---- 5. shared ColorHistograms ----------------------------------------------------------------------------------------
def test_histograms_shared_inside_a_structure_follow_it(chain, monkeypatch):
    """two chains that each share one ColorHistograms object among their own two modalities: accepted, and each equals
    its single-structure context"""
    set_knobs(monkeypatch, {})
    build = chain_builder(chain, shared_histograms=True)
    schedule = {1: 2}
    singles = [ss.run_single(util.open_oracle(), build, s, chain[0], chain[2], schedule) for s in range(2)]
    states = ss.run_batch(util.open_hip(), build, 2, chain[0], chain[2], schedule)
    assert_batch_equals_singles(states, singles)


def test_histograms_shared_across_structures_are_refused(chain, monkeypatch):
    set_knobs(monkeypatch, {})
    inputs, _, gt, _ = chain
    contexts = []
    for _ in range(2):
        api = util.open_hip()
        structures = [chain_builder(chain)(api, s) for s in range(2)]
        shared = host.ColorHistograms(api, n_bins=structures[0].region[0].n_bins)
        structures[0].region[1].UseSharedColorHistograms(shared)
        structures[1].region[0].UseSharedColorHistograms(shared)
        for st in structures:
            ss.upload(st, inputs, 0)
        assert structures[0].tracker.StartModalities(0)
        contexts.append((api, structures))
    (api, inst), (_, twin) = contexts
    before = [st.state() for st in inst]
    assert raw_reset(api, [inst[0].optimizer], ss.reset_poses(gt[1], 0)) == UNSUPPORTED
    assert "shared" in api.last_error()
    for st, b in zip(inst, before):
        ss.same_state(st.state(), b)
    # both listed: every user of the object is restarted, as start_modalities would
    assert inst[0].tracker.ResetStructures([inst[0].optimizer, inst[1].optimizer],
                                           ss.reset_poses(gt[1], 0) + ss.reset_poses(gt[1], 1), 0, 0)
    for s, st in enumerate(twin):
        st.reset_on_host(st.tracker, ss.reset_poses(gt[1], s))
    assert twin[0].tracker.StartModalities(0)
    for a, b in zip(inst, twin):
        ss.same_state(a.state(), b.state())


# ---- 6. single links ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree_context", [False, True])
def test_a_single_link_structure_is_reset_like_its_body(chain, tree_context, monkeypatch):
    """optimizer_create_rigid bodies, alone in the context (no link table on the device) or next to a chain: mode 0 gives
    the bits of ResetBodies"""
    set_knobs(monkeypatch, {})
    small = scenes.Inputs(3, 3, n_divides=2)
    target = [syn.perturb_pose(small.gt[i][1], np.random.default_rng(70 + i), rot_deg=0.5, trans=0.001).astype(F) for i in (0, 2)]
    states = []
    for how in ("structures", "bodies"):
        api = util.open_hip()
        inst = scenes.Instance(api, small)
        if tree_context:
            st = chain_builder(chain)(api, 0)
            ss.upload(st, chain[0], 0)
        inst.upload_frame(0)
        assert inst.tracker.StartModalities(0)
        inst.upload_frame(1)
        assert inst.tracker.ExecuteTrackingStep(1)
        if how == "structures":
            assert raw_reset(api, [0, 2], target) == 0, api.last_error()  # (optimizer i tracks body i)
        else:
            assert inst.tracker.ResetBodies([inst.bodies[0], inst.bodies[2]], target, 0)
        out = [np.stack(inst.poses())] + [h for r in inst.region for h in r.histograms()]
        inst.upload_frame(2)
        assert inst.tracker.ExecuteTrackingStep(2)
        states.append(out + [np.stack(inst.poses())])
    ss.same_state(*states)
    assert np.array_equal(states[0][0][0], target[0]) and np.array_equal(states[0][0][2], target[1])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(chain, monkeypatch):
    set_knobs(monkeypatch, {})
    inputs, _, gt, _ = chain
    contexts = []
    for _ in range(2):
        api = util.open_hip()
        structures = [chain_builder(chain)(api, s) for s in range(2)]
        for st in structures:
            ss.upload(st, inputs, 0)
        assert structures[0].tracker.StartModalities(0)
        ss.upload(structures[0], inputs, 0)
        assert structures[0].tracker.ExecuteTrackingStep(0)
        contexts.append((api, structures))
    (api, inst), (_, twin) = contexts
    poses = ss.reset_poses(gt[1], 0)
    before = [st.state() for st in inst]
    assert raw_reset(api, [], [], n=0) == 0
    assert raw_reset(api, [inst[0].optimizer], poses, n=-1) == INVALID
    assert raw_reset(api, [7], poses) == INVALID
    assert raw_reset(api, [-1], poses) == INVALID
    assert raw_reset(api, [inst[0].optimizer, inst[0].optimizer], poses + poses) == INVALID
    assert raw_reset(api, [inst[0].optimizer], poses, mode=2) == INVALID
    assert raw_reset(api, [inst[0].optimizer], poses, mode=-1) == INVALID
    assert raw_reset(api, [inst[0].optimizer], poses, mode=1) == INVALID  # the root has a body
    api.call("comm_set_reduce_callback", capi.REDUCE_FN(lambda *a: 0), None)  # "spread over ranks"
    assert raw_reset(api, [inst[0].optimizer], poses) == UNSUPPORTED
    api.call("comm_set_reduce_callback", None, None)
    for st, b in zip(inst, before):
        ss.same_state(st.state(), b)
    for structures in (inst, twin):
        for st in structures:
            ss.upload(st, inputs, 1)
        assert structures[0].tracker.ExecuteTrackingStep(1)
    for a, b in zip(inst, twin):
        ss.same_state(a.state(), b.state())


def test_rectangle_only_slots_are_refused(monkeypatch):
    """ROI ingest: the loop of test_gpu_reset_bodies.roi_loop over six single-link structures, its probe of the refusal
    made with reset_structures -- M3T_ERR_UNSUPPORTED while the listed bodies' cameras hold rectangles only, nothing
    changed (the loop goes on to the poses and histograms of the whole-frame expectation)"""
    import reset_loop
    import selective_reset as sr
    import test_gpu_reset_bodies as rb
    set_knobs(monkeypatch, {})
    probes = []

    def probe(api, ids, poses=None, n=None, iteration=0):
        probes.append(list(ids))
        return raw_reset(api, [int(i) for i in ids], poses)  # (optimizer i tracks body i)
    monkeypatch.setattr(rb, "raw_reset", probe)
    inputs = scenes.Inputs(6, 7, n_divides=2)
    schedule = reset_loop.default_schedule(inputs.n_objects, inputs.n_frames)
    got, unrecovered, refused, _ = rb.roi_loop(inputs, schedule, False)
    assert refused and len(probes) == refused and unrecovered == []
    reset_loop.assert_same(got, sr.expectation(inputs, schedule))


def test_partial_ownership_and_bodyless_links_are_refused(chain, monkeypatch):
    set_knobs(monkeypatch, {})
    inputs, joint2parent, gt, angles = chain
    from test_gpu_multibody import Chain
    api = util.open_hip()
    ch = Chain(api, inputs, joint2parent, gt[0][0], angles[0], owned=(0,))  # body B's modality lives elsewhere
    ch.cams[0].UpdateImage(inputs.color[0][0])
    assert ch.tracker.StartModalities(0)
    assert raw_reset(api, [ch.opt], list(gt[1])) == UNSUPPORTED
    assert "rank" in api.last_error()
