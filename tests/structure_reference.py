"""The arithmetic of m3t_hip_reset_structures and of the structure judgement (csrc/m3t_structures.hip) restated in
scalar np.float32, one rounding per operation in the kernels' order:
  - inverse3 / inverse_pose / mul_pose of csrc/m3t_kernels.hip (Eigen's Transform3fA inverse and product),
  - the two modes of RTBEvaluator::SetBodyAndJointPoses (examples/rtb_evaluator.cpp:809-858),
  - RTBEvaluator::CalculatePoseResults' combination of per-body errors and its curve count (:935-988, :20-24).
The GPU tests compare the device with this bit for bit; tests/test_structure_reference.py checks this file itself."""
import numpy as np

F = np.float32
N_CURVE_VALUES = 100


def _cofactor3(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return F(F(m[i1, j1] * m[i2, j2]) - F(m[i1, j2] * m[i2, j1]))


def inverse3(m):
    """Eigen compute_inverse_size3: cofactors / determinant"""
    m = np.asarray(m, F)
    c00, c10, c20 = _cofactor3(m, 0, 0), _cofactor3(m, 1, 0), _cofactor3(m, 2, 0)
    det = F(F(F(c00 * m[0, 0]) + F(c10 * m[1, 0])) + F(c20 * m[2, 0]))
    invdet = F(F(1.0) / det)
    r = np.zeros((3, 3), F)
    for rr in range(3):
        for cc in range(3):
            r[rr, cc] = F(_cofactor3(m, cc, rr) * invdet)
    return r


def inverse_pose(a):
    a = np.asarray(a, F)
    r = np.zeros((4, 4), F)
    r[3, 3] = 1.0
    r[:3, :3] = inverse3(a[:3, :3])
    for k in range(3):
        r[k, 3] = -F(F(F(r[k, 0] * a[0, 3]) + F(r[k, 1] * a[1, 3])) + F(r[k, 2] * a[2, 3]))
    return r


def mul_pose(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    r = np.zeros((4, 4), F)
    r[3, 3] = 1.0
    for c in range(3):
        for k in range(3):
            r[k, c] = F(F(F(a[k, 0] * b[0, c]) + F(a[k, 1] * b[1, c])) + F(a[k, 2] * b[2, c]))
    for k in range(3):
        r[k, 3] = F(F(F(F(a[k, 0] * b[0, 3]) + F(a[k, 1] * b[1, 3])) + F(a[k, 2] * b[2, 3])) + a[k, 3])
    return r


def joint2parent_pose(parent_body2world, body2world, body2joint):
    """:836-838, left to right: (parent world2body * body2world) * body2joint^-1"""
    return mul_pose(mul_pose(inverse_pose(parent_body2world), body2world), inverse_pose(body2joint))


def set_body_and_joint_poses(links, poses, mode=0):
    """links: the structure's links in depth-first order as (parent index or -1, has_body, body2joint); poses: one per
    link with a body, in that order.  Returns (body2world per link or None, joint2parent per link or None = unchanged).
    mode 0: :823-844; mode 1: :846-858 (the body-less root stays, its children's joint2parent is their pose)."""
    body_pose, joint, k = [None] * len(links), [None] * len(links), 0
    for index, (parent, has_body, body2joint) in enumerate(links):
        if mode == 1 and index == 0:
            assert not has_body
            continue
        assert has_body
        pose = np.array(poses[k], F)
        k += 1
        body_pose[index] = pose
        if parent < 0:
            continue
        if mode == 1 and parent == 0:
            joint[index] = pose.copy()
        else:
            joint[index] = joint2parent_pose(body_pose[parent], pose, body2joint)
    assert k == len(poses)
    return body_pose, joint


def thresholds():
    step = F(F(1.0) / F(N_CURVE_VALUES))
    return [F(step * F(F(0.5) + F(i))) for i in range(N_CURVE_VALUES)]


def curve_zeros(auc):
    """the leading curve entries the reference sets to 0: the first i with auc < thresholds[i], 100 if there is none"""
    auc = F(auc)
    for i, t in enumerate(thresholds()):
        if auc < t:
            return i
    return N_CURVE_VALUES


def combine(errors, groups, threshold):
    """errors[i]: one body's error (np.float32); groups: lists of i.  Returns the structure's auc as np.float32."""
    auc = F(0.0)
    for group in groups:
        err = F(0.0)
        for i in group:
            err = F(err + F(errors[i]))
        err = F(err / F(len(group)))
        q = F(err / F(threshold))
        auc = F(auc + F(F(1.0) - (q if q < F(1.0) else F(1.0))))  # fminf(q, 1)
    return F(auc / F(len(groups)))


def structure_judgement(add_errors, adds_errors, groups, threshold):
    """(add_auc, adds_auc, add_curve_zeros, adds_curve_zeros) of one structure"""
    add_auc, adds_auc = combine(add_errors, groups, threshold), combine(adds_errors, groups, threshold)
    return add_auc, adds_auc, curve_zeros(add_auc), curve_zeros(adds_auc)
