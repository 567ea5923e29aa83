"""TextureModality (M3T/src/texture_modality.cpp; line numbers below are that file's) behind its feature detector,
restated in scalar np.float32: one rounding per operation, left to right, no contraction, int() truncating.  The GPU
tests compare the device (csrc/m3t_texture.hip) with this bit for bit; tests/test_texture_reference.py checks this file
against independent formulations.  Poses are 4 x 4 np.float32 matrices; Transform products and inverses are the
library's restatement of Eigen's (tests/structure_reference.py), rotation() is taken as linear()."""
import numpy as np

from structure_reference import inverse3, inverse_pose, mul_pose

F = np.float32
FLT_MIN = F(np.finfo(np.float32).tiny)
MAX_FEATURES = 4096
ROI_MARGIN = 10          # kRegionOfInterestMargin, texture_modality.h:132
MAX_N_OCCLUSION_STRIDES = 5  # kMaxNOcclusionStrides, texture_modality.h:133


def f2i(v):
    """int(float): truncation"""
    return int(np.trunc(np.float64(v)))


def apply_pose(a, p):
    """Transform * Vector3f: t + L v"""
    return np.array([F(a[k, 3] + F(F(F(a[k, 0] * p[0]) + F(a[k, 1] * p[1])) + F(a[k, 2] * p[2]))) for k in range(3)], F)


class Camera:
    def __init__(self, fu, fv, ppu, ppv, width, height, world2camera=np.eye(4), depth_scale=0.0):
        self.fu, self.fv, self.ppu, self.ppv = F(fu), F(fv), F(ppu), F(ppv)
        self.width, self.height = int(width), int(height)
        self.world2camera = np.asarray(world2camera, F)
        self.depth_scale = F(depth_scale)


class Rendering:
    """what renderer_get_images returns of a focused renderer, with its depth range"""

    def __init__(self, depth, silhouette, corner_u, corner_v, scale, visible, z_min, z_max):
        self.depth, self.silhouette = depth, silhouette
        self.corner_u, self.corner_v, self.scale = F(corner_u), F(corner_v), F(scale)
        self.visible = bool(visible)
        self.image_size = depth.shape[0]
        z_min, z_max = F(z_min), F(z_max)
        # renderer.cpp:567-570
        self.term_a = F(F(F(z_max * z_min) * F(65535.0)) / F(z_max - z_min))
        self.term_b = F(F(z_max * F(65535.0)) / F(z_max - z_min))

    def Depth(self, value):
        return F(self.term_a / F(self.term_b - F(value)))


def maximum_body_diameter(vertices, geometry2body):
    """Body::CalculateMaximumBodyDiameter (body.cpp:244-250) as m3t_hip_body_set_geometry takes it: twice the largest
    norm of geometry2body * vertex, t + ((l0 x + l1 y) + l2 z), norm sqrt(x x + (y y + z z))"""
    v, m = np.asarray(vertices, F), np.asarray(geometry2body, F)
    q = [m[k, 3] + ((m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2]) for k in range(3)]
    return F(F(2.0) * np.sqrt(q[0] * q[0] + (q[1] * q[1] + q[2] * q[2])).max())


# ---- CalculateScaleAndRegionOfInterest :890-931 ----------------------------------------------------------------------
def region_of_interest(translation, radius, cam, focused_image_size):
    """((x, y, width, height), scale) or None"""
    x, y, z = (F(v) for v in translation)
    r = F(radius)
    if z < F(r * F(1.5)):
        return None
    abs_x, abs_y = F(abs(x)), F(abs(y))
    x2, y2, z2, r2, rz = F(x * x), F(y * y), F(z * z), F(r * r), F(r * z)
    z2_r2 = F(z2 - r2)
    z3_zr2 = F(z2_r2 * z)
    r_u = F(F(cam.fu * F(F(abs_x * r2) + F(rz * np.sqrt(F(z2_r2 + x2))))) / z3_zr2)
    r_v = F(F(cam.fv * F(F(abs_y * r2) + F(rz * np.sqrt(F(z2_r2 + y2))))) / z3_zr2)
    center_u = F(F(F(x * cam.fu) / z) + cam.ppu)
    center_v = F(F(F(y * cam.fv) / z) + cam.ppv)
    m, h = F(ROI_MARGIN), F(0.5)
    u_min = max(f2i(F(F(F(center_u - r_u) - m) + h)), 0)
    u_max = min(f2i(F(F(F(center_u + r_u) + m) + h)), cam.width - 1)
    v_min = max(f2i(F(F(F(center_v - r_v) - m) + h)), 0)
    v_max = min(f2i(F(F(F(center_v + r_v) + m) + h)), cam.height - 1)
    if u_min >= u_max or v_min >= v_max:
        return None
    du, dv = F(F(2.0) * r_u), F(F(2.0) * r_v)
    scale = F(F(focused_image_size) / (dv if du < dv else du))
    return (u_min, v_min, u_max - u_min, v_max - v_min), scale


def focused_to_full(roi, scale, focused_keypoints):
    """:884-887"""
    pts = np.asarray(focused_keypoints, F).reshape(-1, 2)
    out = np.empty_like(pts)
    out[:, 0] = F(roi[0]) + pts[:, 0] / F(scale)
    out[:, 1] = F(roi[1]) + pts[:, 1] / F(scale)
    return out


# ---- keyframes :933-1127 ---------------------------------------------------------------------------------------------
def orientation(body2camera):
    """rotation().inverse() * translation().normalized() :988-990"""
    t = body2camera[:3, 3]
    tn = np.sqrt(F(F(F(t[0] * t[0]) + F(t[1] * t[1])) + F(t[2] * t[2])))
    if tn == 0:
        return np.zeros(3, F)
    n = [F(t[k] / tn) for k in range(3)]
    ri = inverse3(body2camera[:3, :3])
    return np.array([F(F(F(ri[k, 0] * n[0]) + F(ri[k, 1] * n[1])) + F(ri[k, 2] * n[2])) for k in range(3)], F)


def reconstruct_3d_point(center, body_id, cam, sil, camera2body):
    """:994-1023"""
    cx, cy = F(center[0]), F(center[1])
    u = f2i(F(F(F(cx - sil.corner_u) * sil.scale) + F(0.5)))
    v = f2i(F(F(F(cy - sil.corner_v) * sil.scale) + F(0.5)))
    if u < 0 or u > sil.image_size - 1 or v < 0 or v > sil.image_size - 1:
        return None
    if int(sil.silhouette[v, u]) != body_id:
        return None
    depth = sil.Depth(sil.depth[v, u])
    p = [F(F(depth * F(cx - cam.ppu)) / cam.fu), F(F(depth * F(cy - cam.ppv)) / cam.fv), depth]
    return apply_pose(camera2body, p)


def _window(center_u, center_v, diameter, width_minus_1, height_minus_1):
    stride = f2i(F(F(diameter / F(MAX_N_OCCLUSION_STRIDES)) + F(1.0)))
    n_strides = f2i(F(F(diameter / F(stride)) + F(0.5)))
    rounded_diameter = n_strides * stride
    rounded_radius = F(F(0.5) * F(rounded_diameter))
    u_min = f2i(F(F(center_u - rounded_radius) + F(0.5)))
    v_min = f2i(F(F(center_v - rounded_radius) + F(0.5)))
    u_max, v_max = u_min + rounded_diameter, v_min + rounded_diameter
    return max(u_min, 0), max(v_min, 0), min(u_max, width_minus_1), min(v_max, height_minus_1), stride


def is_point_unoccluded_measured(center_f_body, body2depth_camera, dcam, depth_image, radius, threshold):
    """:1035-1081"""
    x, y, z = apply_pose(body2depth_camera, center_f_body)
    center_u = F(F(F(x * dcam.fu) / z) + dcam.ppu)
    center_v = F(F(F(y * dcam.fv) / z) + dcam.ppv)
    meter_to_pixel = F(dcam.fu / z)
    diameter = F(F(F(2.0) * F(radius)) * meter_to_pixel)
    if not diameter >= 0:  # (no window: the point is kept, m3t_texture.hip)
        return True
    u_min, v_min, u_max, v_max, stride = _window(center_u, center_v, diameter, dcam.width - 1, dcam.height - 1)
    min_depth = f2i(F(F(z - F(threshold)) / dcam.depth_scale)) & 0xffff
    for v in range(v_min, v_max + 1, stride):
        for u in range(u_min, u_max + 1, stride):
            d = int(depth_image[v, u])
            if 0 < d < min_depth:
                return False
    return True


def is_point_unoccluded_modeled(center_f_body, body2camera, cam, rend, radius, threshold):
    """:1083-1127"""
    x, y, z = apply_pose(body2camera, center_f_body)
    meter_to_pixel = F(F(cam.fu / z) * rend.scale)
    diameter = F(F(F(2.0) * F(radius)) * meter_to_pixel)
    center_u = F(F(F(x * cam.fu) / z) + cam.ppu)
    center_v = F(F(F(y * cam.fv) / z) + cam.ppv)
    if not diameter >= 0:
        return True
    focused_u = F(F(center_u - rend.corner_u) * rend.scale)
    focused_v = F(F(center_v - rend.corner_v) * rend.scale)
    u_min, v_min, u_max, v_max, stride = _window(focused_u, focused_v, diameter, rend.image_size - 1, rend.image_size - 1)
    min_value = 65535
    for v in range(v_min, v_max + 1, stride):
        for u in range(u_min, u_max + 1, stride):
            min_value = min(min_value, int(rend.depth[v, u]))
    return bool(rend.Depth(min_value) > F(z - F(threshold)))


class TextureState:
    """what a TextureModality carries from call to call"""

    def __init__(self, n_keyframes=1, descriptor_distance_threshold=0.7, tukey_norm_constant=20.0,
                 standard_deviations=(15.0, 5.0), max_keyframe_rotation_difference=None, max_keyframe_age=100,
                 measure_occlusions=False, measured_occlusion_radius=0.01, measured_occlusion_threshold=0.03,
                 modeled_occlusion_radius=0.01, modeled_occlusion_threshold=0.03):
        self.n_keyframes = n_keyframes
        self.threshold = F(descriptor_distance_threshold)
        self.tukey_norm_constant = F(tukey_norm_constant)
        self.standard_deviations = [F(s) for s in standard_deviations]
        self.max_keyframe_rotation_difference = (F(F(F(10.0) * F(np.pi)) / F(180.0))
                                                 if max_keyframe_rotation_difference is None
                                                 else F(max_keyframe_rotation_difference))
        self.max_keyframe_age = max_keyframe_age
        self.measure_occlusions = measure_occlusions
        self.measured_occlusion_radius, self.measured_occlusion_threshold = measured_occlusion_radius, measured_occlusion_threshold
        self.modeled_occlusion_radius, self.modeled_occlusion_threshold = modeled_occlusion_radius, modeled_occlusion_threshold
        self.points_keyframes = []       # list of (k x 3) arrays, oldest first
        self.descriptors_keyframes = []  # list of (k x bytes) arrays
        self.orientation_last_keyframe = np.zeros(3, F)
        self.keyframe_age = 0
        self.keypoints = np.zeros((0, 2), F)
        self.descriptors = np.zeros((0, 32), np.uint8)
        self.data_points = []  # dicts: center_f_body, correspondence_center, center_f_camera, center

    def set_features(self, keypoints, descriptors):
        self.keypoints = np.asarray(keypoints, F).reshape(-1, 2)
        descriptors = np.asarray(descriptors, np.uint8)
        self.descriptors = descriptors.reshape(len(self.keypoints), descriptors.shape[-1] if descriptors.ndim == 2 else -1)

    def compute_keyframe_data(self, body2world, cam, body_id, sil, depth_rendering=None, dcam=None, depth_image=None):
        """:933-992.  depth_rendering: the focused depth renderer's Rendering when model_occlusions, else None"""
        if len(self.points_keyframes) >= self.n_keyframes:
            self.points_keyframes.pop(0)
            self.descriptors_keyframes.pop(0)
        if not sil.visible:
            return
        body2camera = mul_pose(cam.world2camera, body2world)
        camera2body = inverse_pose(body2camera)
        modeled = depth_rendering is not None and depth_rendering.visible
        points, indexes = [], []
        for i in range(len(self.keypoints)):
            p = reconstruct_3d_point(self.keypoints[i], body_id, cam, sil, camera2body)
            if p is None:
                continue
            if self.measure_occlusions and not is_point_unoccluded_measured(
                    p, mul_pose(dcam.world2camera, body2world), dcam, depth_image, self.measured_occlusion_radius,
                    self.measured_occlusion_threshold):
                continue
            if modeled and not is_point_unoccluded_modeled(p, body2camera, cam, depth_rendering,
                                                           self.modeled_occlusion_radius, self.modeled_occlusion_threshold):
                continue
            points.append(p)
            indexes.append(i)
        self.points_keyframes.append(np.array(points, F).reshape(-1, 3))
        self.descriptors_keyframes.append(self.descriptors[np.asarray(indexes, np.int64)])
        self.orientation_last_keyframe = orientation(body2camera)
        self.keyframe_age = 0

    def calculate_correspondences(self, body2world, cam, corr_iteration):
        """:324-387"""
        if corr_iteration == 0:
            self.data_points = []
            for points, descriptors in zip(self.points_keyframes, self.descriptors_keyframes):
                if len(descriptors) == 0 or len(self.descriptors) == 0:
                    continue
                for q, best in enumerate(knn_match2(descriptors, self.descriptors)):
                    if best is None or not ratio_keeps(best[0], best[1], self.threshold):
                        continue
                    self.data_points.append({"center_f_body": points[q].copy(),
                                             "correspondence_center": self.keypoints[best[2]].copy()})
        body2camera = mul_pose(cam.world2camera, body2world)
        for p in self.data_points:
            project(p, body2camera, cam)

    def variance(self, corr_iteration):
        sd = self.standard_deviations[min(corr_iteration, len(self.standard_deviations) - 1)]  # LastValidValue
        return F(sd * sd)

    def gradient_hessian(self, body2world, cam, corr_iteration):
        """:397-444 -> (gradient[6], hessian[6, 6])"""
        return gradient_hessian(self.data_points, mul_pose(cam.world2camera, body2world), cam, self.tukey_norm_constant,
                                self.variance(corr_iteration))

    def renewal_due(self, body2world, cam):
        """CalculateResults :456-472 up to the decision; counts the age"""
        o = orientation(mul_pose(cam.world2camera, body2world))
        l = self.orientation_last_keyframe
        dot = F(F(F(o[0] * l[0]) + F(o[1] * l[1])) + F(o[2] * l[2]))
        with np.errstate(invalid="ignore"):
            rotation_difference = F(np.arccos(np.float64(dot)))
        self.keyframe_age += 1
        return bool(rotation_difference > self.max_keyframe_rotation_difference) or self.keyframe_age > self.max_keyframe_age


# ---- matcher :349-367 ------------------------------------------------------------------------------------------------
_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming_row(query, train):
    """distances of one query descriptor to all train descriptors"""
    return _POPCOUNT[np.bitwise_xor(train, query[None, :])].sum(axis=1)


def hamming_matrix(queries, train):
    """all distances at once: bits_q . (1 - bits_t) + (1 - bits_q) . bits_t, integers below 2^24: exact in f32"""
    q = np.unpackbits(np.ascontiguousarray(queries), axis=1).astype(np.float32)
    t = np.unpackbits(np.ascontiguousarray(train), axis=1).astype(np.float32)
    return (q @ (1.0 - t).T + (1.0 - q) @ t.T).astype(np.int32)


def knn_match2_sequential(queries, train):
    """per query: (d0, d1, index of the best) with the lower index first among equal distances -- candidates in
    ascending index, a candidate only displaces an entry it is strictly smaller than (cv::BFMatcher::knnMatch(k = 2)) --
    or None with fewer than two train descriptors"""
    out = []
    for q in range(len(queries)):
        if len(train) < 2:
            out.append(None)
            continue
        d = hamming_row(queries[q], train)
        d0 = d1 = None
        i0 = -1
        for i in range(len(d)):
            if d0 is None or d[i] < d0:
                d0, d1, i0 = int(d[i]), d0, i
            elif d1 is None or d[i] < d1:
                d1 = int(d[i])
        out.append((d0, d1, i0))
    return out


def knn_match2(queries, train):
    """knn_match2_sequential for all queries at once: the best is the first minimum, the second the minimum of the
    rest (what the strict < leaves there)"""
    if len(train) < 2:
        return [None] * len(queries)
    out = []
    for lo in range(0, len(queries), 512):
        d = hamming_matrix(queries[lo:lo + 512], train)
        i0 = d.argmin(axis=1)
        rows = np.arange(len(d))
        d0 = d[rows, i0].copy()
        d[rows, i0] = np.iinfo(np.int32).max
        d1 = d.min(axis=1)
        out += [(int(a), int(b), int(i)) for a, b, i in zip(d0, d1, i0)]
    return out


def ratio_keeps(d0, d1, threshold):
    """:365-367: kept iff NOT d0 / d1 >= threshold in f32 (0 / 0: NaN, kept)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return not bool(F(F(d0) / F(d1)) >= F(threshold))


# ---- projection and g/H :380-385, 397-444 ----------------------------------------------------------------------------
def project(p, body2camera, cam):
    c = apply_pose(body2camera, p["center_f_body"])
    p["center_f_camera"] = c
    p["center"] = np.array([F(F(F(c[0] * cam.fu) / c[2]) + cam.ppu), F(F(F(c[1] * cam.fv) / c[2]) + cam.ppv)], F)


def tukey_norm(error, c):
    """:1231-1237: powf(c, 2) = c * c; the cube is the f32 nearest to the f64 product"""
    error, c = F(error), F(c)
    c2_6 = F(F(c * c) / F(6.0))
    if abs(error) <= c:
        q = F(error / c)
        t = np.float64(F(F(1.0) - F(q * q)))
        cube = F((t * t) * t)
        return F(c2_6 * F(F(1.0) - cube))
    return c2_6


def weight(error, squared_error, c, variance):
    """:424-427"""
    if error > FLT_MIN:
        return F(F(tukey_norm(error, c) / squared_error) / variance)
    return F(F(1.0) / variance)


def point_jacobian(p, body2camera, cam):
    """dx_dtheta (2 x 6) :429-435 at the point's current center_f_camera"""
    x, y, z = p["center_f_camera"]
    cb = p["center_f_body"]
    R = body2camera[:3, :3]
    z2 = F(z * z)
    zero = F(0.0)
    dx_dX = [[F(cam.fu / z), zero, F(F(F(-x) * cam.fu) / z2)], [zero, F(cam.fv / z), F(F(F(-y) * cam.fv) / z2)]]
    T = [[F(F(F(dx_dX[i][0] * R[0, k]) + F(dx_dX[i][1] * R[1, k])) + F(dx_dX[i][2] * R[2, k])) for k in range(3)]
         for i in range(2)]
    J = np.zeros((2, 6), F)
    for i in range(2):
        t0, t1, t2 = F(-T[i][0]), F(-T[i][1]), F(-T[i][2])
        J[i, 0] = F(F(t1 * cb[2]) + F(t2 * F(-cb[1])))
        J[i, 1] = F(F(t0 * F(-cb[2])) + F(t2 * cb[0]))
        J[i, 2] = F(F(t0 * cb[1]) + F(t1 * F(-cb[0])))
        J[i, 3:] = T[i]
    return J


def gradient_hessian(data_points, body2camera, cam, tukey_norm_constant, variance):
    g = np.zeros(6, F)
    h = np.zeros((6, 6), F)
    for p in data_points:
        project(p, body2camera, cam)
        d0 = F(p["center"][0] - p["correspondence_center"][0])
        d1 = F(p["center"][1] - p["correspondence_center"][1])
        squared_error = F(F(d0 * d0) + F(d1 * d1))
        error = np.sqrt(squared_error)
        w = weight(error, squared_error, tukey_norm_constant, F(variance))
        J = point_jacobian(p, body2camera, cam)
        wd0, wd1 = F(w * d0), F(w * d1)
        for k in range(6):
            g[k] = F(g[k] - F(F(wd0 * J[0, k]) + F(wd1 * J[1, k])))
        for c in range(6):
            for r in range(c, 6):
                h[r, c] = F(h[r, c] - F(F(F(w * J[0, r]) * J[0, c]) + F(F(w * J[1, r]) * J[1, c])))
    for c in range(6):
        for r in range(c):
            h[r, c] = h[c, r]
    return g, h
