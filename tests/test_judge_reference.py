"""tests/judge_reference.py (the kernel's arithmetic in scalar float32) against the host evaluators it replaces on the
device: evaluation.rbot_pose_result and YCBBodyEvaluation.errors, on seeded random pose pairs with errors from 1e-4 to
0.3 m / rad and the identical pair."""
import numpy as np

import judge_reference as jr
import reset_loop
import util

ev = util.pkg.evaluation
F = np.float32


def random_pose(rng):
    p = np.eye(4, dtype=F)
    p[:3, :3] = reset_loop.rotation(rng.normal(size=3), rng.uniform(0.0, np.pi))
    p[:3, 3] = rng.uniform(-0.5, 0.5, 3) + (0.0, 0.0, 0.8)
    return p


def pose_pairs(seed=5, n=60):
    """(pose, ground truth): translation / rotation errors log-spaced over 1e-4 .. 0.3, and the identical pair"""
    rng = np.random.default_rng(seed)
    sizes = np.geomspace(1e-4, 0.3, n)
    pairs = []
    for k in range(n):
        gt = random_pose(rng)
        p = gt.astype(np.float64)
        direction = rng.normal(size=3)
        p[:3, 3] += sizes[k] * direction / np.linalg.norm(direction)
        p[:3, :3] = reset_loop.rotation(rng.normal(size=3), sizes[(k * 7) % n]) @ p[:3, :3]
        pairs.append((p.astype(F), gt))
    same = random_pose(rng)
    pairs.append((same, same.copy()))
    return pairs


def test_pose_errors_match_the_host_evaluator():
    thr_t, thr_r = 0.05, 5.0 * np.pi / 180.0
    seen = set()
    for p, gt in pose_pairs():
        t_host, r_host, ok_host = ev.rbot_pose_result(p, gt)
        t, r, c, ok = jr.pose_errors(p, gt)
        assert jr.ulps(t, F(t_host)) <= 4, (t, t_host)
        assert np.isnan(r) == np.isnan(r_host)
        if not np.isnan(r_host):
            # the host's matmul forms the cosine in an unspecified order: eighteen roundings of terms <= 3 bound the
            # cosines' difference by about 4e-6, and dr = dcos / sin r
            assert abs(float(r) - r_host) <= 4e-6 / max(np.sin(r_host), 2e-3) + 1e-6, (r, r_host)
        clear = abs(t_host - thr_t) > 1e-4 and (np.isnan(r_host) or abs(r_host - thr_r) > 1e-4)
        if clear:
            assert float(ok) == ok_host, (t_host, r_host)
            seen.add(ok_host)
        assert all(isinstance(x, F) for x in (t, r, c, ok))
    assert seen == {0.0, 1.0}
    # the identical pair: no translation error; the rotation error is 0, tiny or NaN as the cosine rounds
    p, gt = pose_pairs()[-1]
    t, r, c, ok = jr.pose_errors(p, gt)
    assert t == 0.0 and ok == 1.0
    assert np.isnan(r) == (c > 1.0)


def test_add_and_adds_match_the_host_evaluator():
    rng = np.random.default_rng(9)
    all_vertices = rng.uniform(-0.05, 0.05, (700, 3)).astype(F)
    for vertices in (all_vertices, ev.reduce_vertices(all_vertices, 300), all_vertices[:1]):
        body = ev.YCBBodyEvaluation(vertices)
        for p, gt in pose_pairs(seed=6, n=12):
            add_host, adds_host = body.errors(p, gt)
            add, adds = jr.add_adds(body.vertices, p, gt)
            assert abs(float(add) - add_host) <= 2e-5 * abs(add_host) + 1e-7, (add, add_host)
            assert abs(float(adds) - adds_host) <= 2e-5 * abs(adds_host) + 1e-7, (adds, adds_host)
    # a symmetry of the cube: ADD sees the rotation, ADD-S does not
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F) * F(0.05)
    turned = np.eye(4, dtype=F)
    turned[:3, :3] = reset_loop.rotation((0, 0, 1), np.pi / 2)
    add, adds = jr.add_adds(cube, turned, np.eye(4, dtype=F))
    assert abs(float(add) - 0.1) <= 1e-6 and abs(float(adds)) <= 1e-6


def test_delta_is_the_host_evaluators():
    for p, gt in pose_pairs(seed=7, n=10):
        pd, gd = p.astype(np.float64), gt.astype(np.float64)
        inverse = np.eye(4)
        inverse[:3, :3] = pd[:3, :3].T
        inverse[:3, 3] = -pd[:3, :3].T @ pd[:3, 3]
        host = (inverse @ gd).astype(F)[:3]
        assert np.all(jr.ulps(jr.delta_pose(p, gt), host) <= 1) or np.allclose(jr.delta_pose(p, gt), host, rtol=0, atol=1e-7)
