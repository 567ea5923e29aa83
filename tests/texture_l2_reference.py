"""The L2-norm matcher of TextureModality (cv::BFMatcher(cv::NORM_L2) for SIFT and DAISY, texture_modality.cpp:794-796;
line numbers are that file's) restated in scalar np.float32, as include/m3t_hip.h pins it: the squared distance is the
sequential sum s = s + (q[k] - t[k]) * (q[k] - t[k]) over ascending k, one rounding per operation; the distance is its
correctly rounded square root; the best two are compared by their distances.  The GPU tests compare the device
(csrc/m3t_texture_l2.hip) with this bit for bit; tests/test_texture_l2_reference.py checks this file against independent
formulations.  Keyframes, g/H and renewal are those of tests/texture_reference.py."""
import numpy as np

import texture_reference as T

F = np.float32


def l2_squared(q, t):
    s = F(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(len(q)):
            e = F(F(q[k]) - F(t[k]))
            s = F(s + F(e * e))
    return s


def l2_distance(q, t):
    with np.errstate(invalid="ignore"):
        return F(np.sqrt(l2_squared(q, t)))  # (np.sqrt of a float32 is the correctly rounded f32 root)


def l2_squared_rows(query, train):
    """l2_squared of one query against every train row: the same chain, all rows at once (elementwise float32
    operations round like the scalar ones)"""
    train = np.asarray(train, F)
    s = np.zeros(len(train), F)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(train.shape[1]):
            e = F(query[k]) - train[:, k]
            s = s + e * e
    return s


def knn_match2_l2_sequential(queries, train):
    """per query: (d0, d1, index of the best), or None with fewer than two entries.  Candidates in ascending index; a
    candidate displaces an entry only if its distance is strictly smaller; a NaN distance satisfies no `<` and never
    enters"""
    out = []
    for q in range(len(queries)):
        with np.errstate(invalid="ignore"):
            d = np.sqrt(l2_squared_rows(queries[q], train)) if len(train) else np.zeros(0, F)
        d0 = d1 = None
        i0 = -1
        for i in range(len(d)):
            if np.isnan(d[i]):
                continue
            if d0 is None or d[i] < d0:
                d0, d1, i0 = d[i], d0, i
            elif d1 is None or d[i] < d1:
                d1 = d[i]
        out.append(None if d1 is None else (F(d0), F(d1), i0))
    return out


def ratio_keeps_l2(d0, d1, threshold):
    """:365-367: kept iff NOT d0 / d1 >= threshold in f32 (0 / 0 and inf / inf: NaN, kept)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return not bool(F(F(d0) / F(d1)) >= F(threshold))


def seeded_rows(rng, n, n_floats, integer):
    """descriptors for the tests: integers 0 .. 255 as floats (what OpenCV's SIFT writes) or uniform floats in [0, 1)"""
    if integer:
        return rng.integers(0, 256, (n, n_floats)).astype(F)
    return rng.random((n, n_floats), dtype=F)


class TextureStateL2(T.TextureState):
    """TextureState with descriptors of floats and the L2 matcher"""

    def set_features(self, keypoints, descriptors):
        self.keypoints = np.asarray(keypoints, F).reshape(-1, 2)
        descriptors = np.asarray(descriptors, F)
        self.descriptors = descriptors.reshape(len(self.keypoints), descriptors.shape[-1] if descriptors.ndim == 2 else -1)

    def calculate_correspondences(self, body2world, cam, corr_iteration):
        """:324-387"""
        if corr_iteration == 0:
            self.data_points = []
            for points, descriptors in zip(self.points_keyframes, self.descriptors_keyframes):
                if len(descriptors) == 0 or len(self.descriptors) == 0:
                    continue
                for q, best in enumerate(knn_match2_l2_sequential(descriptors, self.descriptors)):
                    if best is None or not ratio_keeps_l2(best[0], best[1], self.threshold):
                        continue
                    self.data_points.append({"center_f_body": points[q].copy(),
                                             "correspondence_center": self.keypoints[best[2]].copy()})
        body2camera = T.mul_pose(cam.world2camera, body2world)
        for p in self.data_points:
            T.project(p, body2camera, cam)
