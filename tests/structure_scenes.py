"""Scenes of the m3t_hip_reset_structures / structure-judgement tests: the kinematic structures of
tests/test_gpu_multibody.py (Chain, DepthChain) re-instantiated several times in one context, a three-link chain whose
middle joint moves body2joint, a body-less root with two children and a hard constraint, and the loop that resets
structures on a fixed schedule -- in ONE HIP context with Tracker.ResetStructures, or each structure in a context of
its own (the CPU oracle) where the harness sets the body poses and the joints of tests/structure_reference.py and calls
StartModalities(0): the reference's one tracker per sequence."""
import numpy as np

import scenes
import structure_reference as sref
import util
from util import host, syn

F = np.float32


class Structure:
    """one kinematic structure in a context: optimizer, links in depth-first order as (Link, Body or None, parent
    index), cameras in upload order, region modalities"""

    def __init__(self, optimizer, links, cams, region, mode=0):
        self.optimizer, self.links, self.cams, self.region, self.mode = optimizer, links, cams, region, mode
        self.bodies = [b for _, b, _ in links if b is not None]

    def state(self):
        """body poses, joint poses of every link below the root, histograms"""
        out = [b.body2world_pose() for b in self.bodies]
        for link, _, parent in self.links:
            if parent >= 0:
                out += [link.joint2parent_pose(), link.body2joint_pose()]
        for r in self.region:
            out += list(r.histograms())
        return out

    def reference_links(self):
        """the links as tests/structure_reference.set_body_and_joint_poses takes them, body2joint read from the engine"""
        return [(parent, body is not None, link.body2joint_pose()) for link, body, parent in self.links]

    def reset_on_host(self, tracker, poses):
        """what ResetStructures does, through the engine's setters (any library), minus the restart"""
        body_pose, joint = sref.set_body_and_joint_poses(self.reference_links(), poses, self.mode)
        for (link, body, _), p, j in zip(self.links, body_pose, joint):
            if p is not None:
                body.set_body2world_pose(p)
            if j is not None:
                link.set_joint2parent_pose(j)


def same_state(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), i


def chain_inputs(n_frames=4):
    from test_gpu_multibody import chain_inputs as make
    return make(n_frames)


def two_body_chain(api, inputs, joint2parent, start_a, start_angle, shared_histograms=False):
    """test_gpu_multibody.Chain (A free, B on a revolute joint), optionally with one ColorHistograms object shared by
    its two modalities"""
    from test_gpu_multibody import Chain
    ch = Chain(api, inputs, joint2parent, start_a, start_angle)
    if shared_histograms:
        shared = host.ColorHistograms(api, n_bins=ch.mods[0].n_bins)
        for m in ch.mods.values():
            m.UseSharedColorHistograms(shared)
    s = Structure(ch.opt, [(ch.link_a, ch.bodies[0], -1), (ch.link_b, ch.bodies[1], 0)], ch.cams, [ch.mods[0], ch.mods[1]])
    s.tracker = ch.tracker
    return s


def upload(structure, inputs, k):
    """image k into the structure's cameras: inputs.color[camera][k], or (Region + Depth links: `cams` holds (colour,
    depth) camera pairs) inputs.frames[camera][k] = (colour image, depth image)"""
    for i, cam in enumerate(structure.cams):
        if isinstance(cam, tuple):
            cam[0].UpdateImage(inputs.frames[i][k][0])
            cam[1].UpdateImage(inputs.frames[i][k][1])
        else:
            cam.UpdateImage(inputs.color[i][k])


def reset_poses(gt_k, seed):
    """the poses a structure is put on before frame k: the frame's ground truth of both bodies, moved a little per
    structure so that no two structures of a batch get the same bits"""
    rng = np.random.default_rng(100 + seed)
    return [syn.perturb_pose(p, rng, rot_deg=0.3, trans=0.001).astype(F) for p in gt_k]


# structure -> frame before which it is reset
SCHEDULE = {1: 2, 0: 3, 2: 3}


def run_batch(api, build, n_structures, inputs, gt_poses, schedule=SCHEDULE, setup=None, after_step=None):
    """n structures in one context, reset on `schedule` with Tracker.ResetStructures; state of every structure after
    every step"""
    structures = [build(api, s) for s in range(n_structures)]
    tracker = structures[0].tracker
    if setup:
        setup(api)
    for st in structures:
        upload(st, inputs, 0)
    assert tracker.StartModalities(0)
    states = []
    for k in range(len(gt_poses)):
        due = [s for s in range(n_structures) if schedule.get(s) == k]
        if due:
            poses = [p for s in due for p in reset_poses(gt_poses[k], s)]
            assert tracker.ResetStructures([structures[s].optimizer for s in due], poses, structures[due[0]].mode, 0)
        for st in structures:
            upload(st, inputs, k)
        assert tracker.ExecuteTrackingStep(k)
        if after_step:
            after_step(api)
        states.append([st.state() for st in structures])
    return states


def run_single(api, build, s, inputs, gt_poses, schedule=SCHEDULE):
    """structure s of the batch in a context of its own: at its reset the harness sets poses and joints and calls
    StartModalities(0)"""
    st = build(api, s)
    upload(st, inputs, 0)
    assert st.tracker.StartModalities(0)
    states = []
    for k in range(len(gt_poses)):
        if schedule.get(s) == k:
            st.reset_on_host(st.tracker, reset_poses(gt_poses[k], s))
            assert st.tracker.StartModalities(0)
        upload(st, inputs, k)
        assert st.tracker.ExecuteTrackingStep(k)
        states.append(st.state())
    return states
