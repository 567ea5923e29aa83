"""tests/texture_reference.py -- the scalar np.float32 restatement of the texture modality the GPU tests compare the
device with -- against independent formulations: Hamming distances through np.unpackbits and the best two through a
stable argsort; g/H against a float64 evaluation of the same formula (1e-4 relative on the largest element: a sanity
bound on the restatement, not on the kernel); the rotation block of the Jacobian against a finite difference of the
projection."""
import numpy as np

import texture_reference as T

F = np.float32


def _scene(seed, n):
    rng = np.random.default_rng(seed)
    cam = T.Camera(650.0, 651.0, 320.5, 239.25, 640, 480)
    angle = 0.3
    pose = np.eye(4, dtype=F)
    pose[:3, :3] = np.array([[np.cos(angle), 0, np.sin(angle)], [0, 1, 0], [-np.sin(angle), 0, np.cos(angle)]], F)
    pose[:3, 3] = [0.02, -0.03, 0.6]
    points = []
    for _ in range(n):
        p = {"center_f_body": rng.uniform(-0.05, 0.05, 3).astype(F)}
        T.project(p, pose, cam)
        p["correspondence_center"] = (p["center"] + rng.uniform(-8, 8, 2)).astype(F)
        points.append(p)
    return cam, pose, points


def test_hamming_and_best_two_against_unpackbits_and_stable_argsort():
    rng = np.random.default_rng(5)
    for n_bytes in (32, 64):
        train = rng.integers(0, 256, (37, n_bytes), dtype=np.uint8)
        queries = rng.integers(0, 256, (19, n_bytes), dtype=np.uint8)
        train[20] = train[3]              # duplicates: ties
        queries[4] = train[3]             # distance 0 twice
        queries[5] = train[7] ^ np.uint8(1)
        matches = T.knn_match2_sequential(queries, train)
        assert matches == T.knn_match2(queries, train)
        assert np.array_equal(T.hamming_matrix(queries, train), [T.hamming_row(q, train) for q in queries])
        for q in range(len(queries)):
            bits = np.unpackbits(queries[q][None, :] ^ train, axis=1)
            d = bits.sum(axis=1)
            assert np.array_equal(d, T.hamming_row(queries[q], train))
            order = np.argsort(d, kind="stable")
            assert matches[q] == (int(d[order[0]]), int(d[order[1]]), int(order[0]))
        assert matches[4] == (0, 0, 3)
        assert T.knn_match2(queries, train[:1]) == [None] * len(queries) == T.knn_match2_sequential(queries, train[:0])


def test_ratio_test_keeps_nan_and_rejects_at_the_threshold():
    assert T.ratio_keeps(0, 0, 0.7)           # NaN >= x is false
    assert not T.ratio_keeps(3, 4, 0.75)      # exactly at the threshold
    assert T.ratio_keeps(2, 4, 0.75)
    assert not T.ratio_keeps(7, 10, 0.7)      # f32: 0.7f is below 7 / 10
    assert not T.ratio_keeps(5, 0, 0.7)       # +inf


def test_gradient_hessian_against_float64():
    cam, pose, points = _scene(11, 40)
    # (no point with error == 0 here: the reference's weight jumps there -- 1 / variance at 0, the Tukey limit
    # 0.5 / variance beside it -- and f64 lands beside it; tests/cpp/texture_check.cpp and the GPU test hold that point)
    points[5]["correspondence_center"] = (points[5]["center"] + F(40.0)).astype(F)  # error > c
    c, variance = F(20.0), F(25.0)
    g, h = T.gradient_hessian(points, pose, cam, c, variance)
    assert np.array_equal(h, h.T)
    g64, h64 = np.zeros(6), np.zeros((6, 6))
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    fu, fv, ppu, ppv = (np.float64(v) for v in (cam.fu, cam.fv, cam.ppu, cam.ppv))
    for p in points:
        cb = p["center_f_body"].astype(np.float64)
        x, y, z = R @ cb + t
        diff = np.array([x * fu / z + ppu, y * fv / z + ppv]) - p["correspondence_center"].astype(np.float64)
        e2 = diff @ diff
        e = np.sqrt(e2)
        w = 1.0 / 25.0
        if e > np.finfo(np.float32).tiny:
            tukey = 400.0 / 6.0 * (1.0 - (1.0 - (e / 20.0) ** 2) ** 3) if e <= 20.0 else 400.0 / 6.0
            w = tukey / e2 / 25.0
        dx_dX = np.array([[fu / z, 0, -x * fu / z ** 2], [0, fv / z, -y * fv / z ** 2]])
        dt = dx_dX @ R
        skew = np.array([[0, -cb[2], cb[1]], [cb[2], 0, -cb[0]], [-cb[1], cb[0], 0]])
        J = np.hstack([-dt @ skew, dt])
        g64 -= w * diff @ J
        h64 -= w * J.T @ J
    assert np.abs(g - g64).max() <= 1e-4 * np.abs(g64).max()
    assert np.abs(h - h64).max() <= 1e-4 * np.abs(h64).max()
    assert np.abs(g64).max() > 0 and np.abs(h64).max() > 0


def test_rotation_block_against_a_finite_difference_of_the_projection():
    """dx / dtheta for body2camera * exp(theta) (the variation Link applies to the body frame): the first three columns
    of dx_dtheta are -dx_dtranslation * skew(center_f_body)"""
    cam, pose, points = _scene(3, 6)
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    fu, fv, ppu, ppv = (np.float64(v) for v in (cam.fu, cam.fv, cam.ppu, cam.ppv))

    def proj(cb, theta, d):
        skew = np.array([[0, -theta[2], theta[1]], [theta[2], 0, -theta[0]], [-theta[1], theta[0], 0]])
        x, y, z = R @ ((np.eye(3) + skew) @ cb + d) + t
        return np.array([x * fu / z + ppu, y * fv / z + ppv])

    eps = 1e-6
    for p in points:
        J = T.point_jacobian(p, pose, cam).astype(np.float64)
        cb = p["center_f_body"].astype(np.float64)
        for k in range(6):
            step = np.zeros(6)
            step[k] = eps
            numeric = (proj(cb, step[:3], step[3:]) - proj(cb, -step[:3], -step[3:])) / (2 * eps)
            assert np.abs(numeric - J[:, k]).max() <= 1e-3 * max(1.0, np.abs(J[:, k]).max()), (k, numeric, J[:, k])


def test_region_of_interest_refusals_and_focus_offset():
    cam = T.Camera(650.0, 651.0, 320.5, 239.25, 640, 480)
    assert T.region_of_interest((0.0, 0.0, 0.11), 0.08, cam, 200) is None      # z < 1.5 r
    assert T.region_of_interest((-0.5, 0.0, 0.6), 0.08, cam, 200) is None      # empty rectangle
    roi, scale = T.region_of_interest((0.02, -0.01, 0.6), 0.08, cam, 200)
    assert roi == (244, 131, 196, 195) and scale == F(1.1377981)
    full = T.focused_to_full(roi, scale, [[10.0, 20.0]])
    assert full[0, 0] == F(244) + F(10.0) / scale and full[0, 1] == F(131) + F(20.0) / scale


def test_tukey_norm_special_points():
    c = F(20.0)
    assert T.tukey_norm(F(0.0), c) == 0 and T.tukey_norm(c, c) == F(F(400.0) / F(6.0)) == T.tukey_norm(F(25.0), c)
    assert T.weight(F(0.0), F(0.0), c, F(225.0)) == F(F(1.0) / F(225.0)) == T.weight(T.FLT_MIN, F(0.0), c, F(225.0))
