"""The arithmetic of judge_bodies_kernel (csrc/m3t_judge.hip) restated in scalar np.float32, operation by operation in
the kernel's order: RBOTEvaluator::CalculatePoseResults (rbot_evaluator.cpp:416-433) and YCBEvaluator::
CalculatePoseResults (ycb_evaluator.cpp:803-848).  The GPU tests compare the device with this bit for bit (pose errors)
and tests/test_judge_reference.py compares this with the host evaluators of 3dobjecttracking_amd/evaluation.py."""
import numpy as np

F = np.float32
D = np.float64
THRESHOLD_TRANSLATION = F(0.05)                    # rbot_evaluator.h:192
THRESHOLD_ROTATION = F(5.0) * F(np.pi) / F(180.0)  # rbot_evaluator.h:193, in float like the header


def pose_errors(pose, gt, thr_t=THRESHOLD_TRANSLATION, thr_r=THRESHOLD_ROTATION):
    """(translation_error, rotation_error, rotation_cosine, tracking_success) as np.float32 scalars"""
    p, g = np.asarray(pose, F), np.asarray(gt, F)
    dx, dy, dz = F(p[0, 3] - g[0, 3]), F(p[1, 3] - g[1, 3]), F(p[2, 3] - g[2, 3])
    t_err = F(np.sqrt(F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))))
    d = []
    for j in range(3):  # the rotation columns
        d.append(F(F(F(p[0, j] * g[0, j]) + F(p[1, j] * g[1, j])) + F(p[2, j] * g[2, j])))
    tr = F(F(d[0] + d[1]) + d[2])
    c = F(F(tr - F(1.0)) * F(0.5))
    with np.errstate(invalid="ignore"):
        r_err = F(np.arccos(D(c)))
    lost = bool(t_err > F(thr_t)) or bool(r_err > F(thr_r))  # a NaN error is "not lost"
    return t_err, r_err, c, F(0.0 if lost else 1.0)


def delta_pose(pose, gt):
    """body2world^-1 * gt with the rigid inverse [R^T | -R^T t], f64 left to right, rounded to f32: 3 x 4"""
    p, g = np.asarray(pose, F).astype(D), np.asarray(gt, F).astype(D)
    delta = np.zeros((3, 4), F)
    for r in range(3):
        i0, i1, i2 = p[0, r], p[1, r], p[2, r]
        i3 = -((i0 * p[0, 3] + i1 * p[1, 3]) + i2 * p[2, 3])
        for c in range(4):
            delta[r, c] = F(((i0 * g[0, c] + i1 * g[1, c]) + i2 * g[2, c]) + i3 * g[3, c])
    return delta


def add_adds(vertices, pose, gt, chunk=512):
    """(ADD, ADD-S) as np.float32: v' = delta v in f32 left to right, |v - v'|, the nearest vertex by exhaustive search
    over the squared distance (dx dx + dy dy) + dz dz with one sqrt per query, f64 sums, the mean rounded to f32.
    (Elementwise numpy f32 operations round like the scalar ones; the f64 sums differ from the kernel's order by
    parts in 1e16.)"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    d = delta_pose(pose, gt)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    moved = [((d[r, 0] * x + d[r, 1] * y) + d[r, 2] * z) + d[r, 3] for r in range(3)]
    assert all(m.dtype == F for m in moved)
    ex, ey, ez = x - moved[0], y - moved[1], z - moved[2]
    add = np.sqrt((ex * ex + ey * ey) + ez * ez).astype(D).sum() / D(len(v))
    best = np.empty(len(v), F)
    for first in range(0, len(v), chunk):
        q = slice(first, first + chunk)
        tx = x[None, :] - moved[0][q, None]
        ty = y[None, :] - moved[1][q, None]
        tz = z[None, :] - moved[2][q, None]
        best[q] = ((tx * tx + ty * ty) + tz * tz).min(axis=1)
    adds = np.sqrt(best).astype(D).sum() / D(len(v))
    return F(add), F(adds)


def ulps(a, b):
    """distance of two finite float32 values in units in the last place"""
    ia = np.asarray(a, F).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)
