"""The texture modality on the device (csrc/m3t_texture.hip behind m3t_hip_texture_modality_*) against its scalar
np.float32 restatement (tests/texture_reference.py), bit for bit: the matcher with the ratio test, keyframe
reconstruction with the two occlusion tests, the Tukey-weighted g/H, the Newton update through the link kernels (against
the oracle's optimizer fed with the restated g/H), a free-running sequence with keyframe renewal, a batch against
single contexts, and the refusals.  Scenes: the triangle and the bottle of tests/test_gpu_renderer.py; descriptors from a
seeded generator -- no detector, no OpenCV."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_scene as gs
import texture_reference as T
import util
from util import host

pytestmark = pytest.mark.gpu
mtv = gs.mtv
F = np.float32
BODY_ID = 150  # the triangle's, tests/golden_scene.py
Z_MIN, Z_MAX = 0.02, 10.0


def _header_constant(name):
    text = open(os.path.join(util.ROOT, "3dobjecttracking_amd", "csrc", "m3t_texture.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


TILE = _header_constant("M3T_TEXTURE_TRAIN_TILE")
CHUNK = _header_constant("M3T_TEXTURE_GH_CHUNK")
THREADS = _header_constant("M3T_TEXTURE_MATCH_THREADS")


class Scene:
    """the triangle in front of the colour camera, a focused silhouette renderer (ids of bodies) over the triangle and
    the bottle, optionally a focused depth renderer and a depth camera; with a texture modality on a HIP context"""

    def __init__(self, api, texture=True, depth_renderer=False, depth_image=None, optimizer=True, body2world=None,
                 bottle_offset=None, **params):
        self.api = api
        self.body = host.Body(api, mtv.body2world() if body2world is None else body2world)
        self.color_camera = host.ColorCamera(api, **mtv.COLOR_INTRINSICS)
        self.cam = T.Camera(**mtv.COLOR_INTRINSICS)
        geometry, self.bottle = gs.fixture_renderer_geometry(api, self.body)
        if bottle_offset is not None:
            pose = self.bottle.body2world_pose()
            pose[:3, 3] = mtv.body2world()[:3, 3] + np.asarray(bottle_offset, F)
            self.bottle.set_body2world_pose(pose)
        self.sil = host.FocusedSilhouetteRenderer(api, geometry, self.color_camera, id_type=0, image_size=200,
                                                  z_min=Z_MIN, z_max=Z_MAX)
        self.sil.AddReferencedBody(self.body)
        self.dep = None
        if depth_renderer:
            self.dep = host.FocusedBasicDepthRenderer(api, geometry, self.color_camera, image_size=200, z_min=Z_MIN,
                                                      z_max=Z_MAX)
            self.dep.AddReferencedBody(self.body)
        self.depth_camera, self.dcam, self.depth_image = None, None, depth_image
        if depth_image is not None:
            w2c = np.linalg.inv(mtv.DEPTH_CAMERA2WORLD).astype(F)
            self.depth_camera = host.DepthCamera(api, depth_scale=mtv.DEPTH_SCALE, world2camera_pose=w2c,
                                                 **mtv.DEPTH_INTRINSICS)
            self.depth_camera.UpdateImage(depth_image)
            self.dcam = T.Camera(world2camera=w2c, depth_scale=mtv.DEPTH_SCALE, **mtv.DEPTH_INTRINSICS)
            params["measure_occlusions"] = 1
        self.texture = None
        if texture:
            self.texture = host.TextureModality(api, self.body, self.color_camera, self.sil,
                                                depth_camera=self.depth_camera, **params)
            if self.dep is not None:
                self.texture.ModelOcclusions(self.dep)
            if optimizer:
                self.optimizer = host.Optimizer(api, body=self.body, modalities=[self.texture])
        self.tracker = host.Tracker(api)

    @staticmethod
    def rendering(renderer):
        depth, sil, corner_u, corner_v, scale, n_visible = renderer.images()
        return T.Rendering(depth, sil, corner_u, corner_v, scale, n_visible > 0, Z_MIN, Z_MAX)

    def on_body_keypoints(self, n, seed=0):
        """n keypoints (full-image coordinates) that land on distinct silhouette pixels of the body"""
        self.sil.StartRendering()
        r = self.rendering(self.sil)
        vs, us = np.nonzero(r.silhouette == BODY_ID)
        assert len(vs) >= n, len(vs)
        pick = np.random.default_rng(seed).permutation(len(vs))[:n]
        xy = np.stack([r.corner_u + us[pick].astype(F) / r.scale, r.corner_v + vs[pick].astype(F) / r.scale], axis=1)
        return xy.astype(F)

    def state(self, **kw):
        p = self.texture.params
        defaults = dict(n_keyframes=p.n_keyframes, descriptor_distance_threshold=p.descriptor_distance_threshold,
                        tukey_norm_constant=p.tukey_norm_constant,
                        standard_deviations=list(p.standard_deviations)[:p.n_standard_deviations],
                        max_keyframe_rotation_difference=p.max_keyframe_rotation_difference,
                        max_keyframe_age=p.max_keyframe_age, measure_occlusions=bool(p.measure_occlusions),
                        measured_occlusion_radius=p.measured_occlusion_radius,
                        measured_occlusion_threshold=p.measured_occlusion_threshold,
                        modeled_occlusion_radius=p.modeled_occlusion_radius,
                        modeled_occlusion_threshold=p.modeled_occlusion_threshold)
        defaults.update(kw)
        return T.TextureState(**defaults)

    def reference_keyframe(self, state, pose=None):
        """ComputeKeyframeData of the restatement on the renderings the device holds"""
        state.compute_keyframe_data(self.body.body2world_pose() if pose is None else pose, self.cam, BODY_ID,
                                    self.rendering(self.sil),
                                    depth_rendering=self.rendering(self.dep) if self.dep is not None else None,
                                    dcam=self.dcam, depth_image=self.depth_image)


def _points_equal(device, reference):
    assert len(device) == len(reference)
    if len(reference) == 0:
        return
    for name in ("center_f_body", "correspondence_center", "center_f_camera", "center"):
        expected = np.array([p[name] for p in reference], F).reshape(len(reference), -1)
        assert np.array_equal(device[name].reshape(len(device), -1).view(np.uint32), expected.view(np.uint32)), name


def _keyframes_equal(texture, state):
    age, keyframes = texture.keyframes()
    assert age == state.keyframe_age and len(keyframes) == len(state.points_keyframes)
    for a, b in zip(keyframes, state.points_keyframes):
        assert np.array_equal(a.view(np.uint32), np.asarray(b, F).reshape(-1, 3).view(np.uint32))


def _descriptors(rng, n_query, n_train, n_bytes, planted=True):
    """train rows at random; queries: even ones a train row with one bit flipped (kept by the ratio test), odd ones
    random (rejected: two random rows are about equally far).  Planted where the sizes allow it: a train row duplicated
    across a tile boundary and a query equal to both (tie rule: the lower index; 0 / 0: kept), and a ratio exactly at
    the threshold 0.75 (rejected)."""
    train = rng.integers(0, 256, (n_train, n_bytes), dtype=np.uint8)
    queries = rng.integers(0, 256, (n_query, n_bytes), dtype=np.uint8)
    tie = planted and n_train > TILE + 2 and n_query >= 6
    ratio = planted and n_train >= 2 and n_query >= 6
    if tie:
        train[TILE + 1] = train[TILE - 2]
    if ratio:  # rows 0 and 1 differ in one bit
        train[0] = 0
        train[1] = 0
        train[1, 0] = 0x01
    for q in range(0, n_query, 2):
        if n_train:
            queries[q] = train[(q * 7) % n_train]
            queries[q, (q + 5) % n_bytes] ^= np.uint8(1 << (q % 8))
    if tie:
        queries[2] = train[TILE - 2]   # distance 0 to rows TILE - 2 and TILE + 1
    if ratio:
        queries[4] = 0
        queries[4, 1] = 0x07           # 3 bits from row 0, 4 bits from row 1, far from every random row
    return queries, train


# ---- 1. matcher --------------------------------------------------------------------------------------------------------
SIZES = sorted({0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, THREADS + 1})


@pytest.mark.parametrize("n_bytes", [32, 64])
def test_matcher_equals_the_restatement_at_every_size(n_bytes):
    api = util.open_hip()
    s = Scene(api, descriptor_bytes=n_bytes, descriptor_distance_threshold=0.75)
    keypoints = s.on_body_keypoints(max(SIZES), seed=1)
    rng = np.random.default_rng(n_bytes)
    for n_query in SIZES:
        for n_train in SIZES:
            queries, train = _descriptors(rng, n_query, n_train, n_bytes)
            train_xy = rng.uniform(0, 900, (n_train, 2)).astype(F)
            state = s.state()
            s.texture.SetFeatures(keypoints[:n_query], queries)
            state.set_features(keypoints[:n_query], queries)
            assert s.tracker.StartModalities(0)
            s.reference_keyframe(state)
            assert [len(k) for k in state.points_keyframes] == [n_query]  # every keypoint is on the body
            s.texture.SetFeatures(train_xy, train)
            state.set_features(train_xy, train)
            assert s.tracker.CalculateCorrespondences(0, 0)
            state.calculate_correspondences(s.body.body2world_pose(), s.cam, 0)
            if n_query >= 2 and n_train >= 2:  # not vacuous: the restatement alone keeps some and rejects some
                assert 0 < len(state.data_points) < n_query, (n_query, n_train)
            else:  # degenerate: a single query, or fewer than two train descriptors (no match at all)
                assert n_train >= 2 or len(state.data_points) == 0
            _points_equal(s.texture.points(), state.data_points)
            _keyframes_equal(s.texture, state)


@pytest.mark.parametrize("n_bytes", [32, 64])
def test_matcher_with_three_keyframes_and_at_full_size(n_bytes):
    api = util.open_hip()
    s = Scene(api, descriptor_bytes=n_bytes, n_keyframes=3)
    n = T.MAX_FEATURES
    keypoints = s.on_body_keypoints(n, seed=2)
    rng = np.random.default_rng(100 + n_bytes)
    state = s.state()
    # three keyframes of 4096, 65 and TILE + 1 points, then 4096 current features
    for n_query in (n, 65, TILE + 1):
        queries, _ = _descriptors(rng, n_query, 0, n_bytes, planted=False)
        s.texture.SetFeatures(keypoints[:n_query], queries)
        state.set_features(keypoints[:n_query], queries)
        assert s.tracker.StartModalities(0)
        s.reference_keyframe(state)
    assert [len(k) for k in state.points_keyframes] == [n, 65, TILE + 1]
    train = rng.integers(0, 256, (n, n_bytes), dtype=np.uint8)
    for k, descriptors in enumerate(state.descriptors_keyframes):  # every third query has a near twin among the train rows
        for q in range(0, len(descriptors), 3):
            train[(q * 5 + k) % n] = descriptors[q]
            train[(q * 5 + k) % n, 3] ^= np.uint8(16)
    train_xy = rng.uniform(0, 900, (n, 2)).astype(F)
    s.texture.SetFeatures(train_xy, train)
    state.set_features(train_xy, train)
    assert s.tracker.CalculateCorrespondences(0, 0)
    state.calculate_correspondences(s.body.body2world_pose(), s.cam, 0)
    assert 1000 < len(state.data_points) < n + 65 + TILE + 1
    _points_equal(s.texture.points(), state.data_points)
    _keyframes_equal(s.texture, state)
    # 4097 features are refused before anything changes
    too_many = np.zeros((n + 1, 2), F)
    rc = api.raw("texture_modality_set_features", s.texture.id, util.pkg._capi.fptr(too_many),
                 np.zeros((n + 1, n_bytes), np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), n + 1)
    assert rc == util.pkg._capi.M3T_ERR_INVALID_ARGUMENT
    assert s.tracker.CalculateCorrespondences(0, 0)
    _points_equal(s.texture.points(), state.data_points)
    # a fourth keyframe pops the oldest; later correspondence iterations only project
    s.texture.SetFeatures(keypoints[:63], train[:63])
    state.set_features(keypoints[:63], train[:63])
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    assert [len(k) for k in state.points_keyframes] == [65, TILE + 1, 63]
    _keyframes_equal(s.texture, state)
    pose = s.body.body2world_pose()
    pose[:3, 3] += np.array([0.002, -0.001, 0.003], F)
    s.body.set_body2world_pose(pose)
    assert s.tracker.CalculateCorrespondences(0, 1)
    state.calculate_correspondences(pose, s.cam, 1)
    _points_equal(s.texture.points(), state.data_points)


# ---- 2. keyframe data --------------------------------------------------------------------------------------------------
def _grid(scene):
    """keypoints on a grid over the focused rectangle and its surroundings, finer around the body"""
    scene.sil.StartRendering()
    r = scene.rendering(scene.sil)
    size = F(r.image_size) / r.scale
    coarse = np.arange(-0.25 * size, 1.25 * size, 6.0, dtype=np.float64)
    vs, us = np.nonzero(r.silhouette == BODY_ID)
    lo_u, hi_u, lo_v, hi_v = us.min() / r.scale, us.max() / r.scale, vs.min() / r.scale, vs.max() / r.scale
    pad_u, pad_v = 0.1 * (hi_u - lo_u), 0.1 * (hi_v - lo_v)
    fine_u = np.arange(lo_u - pad_u, hi_u + pad_u, 1.3, dtype=np.float64)
    fine_v = np.arange(lo_v - pad_v, hi_v + pad_v, 1.3, dtype=np.float64)
    grids = [np.meshgrid(coarse, coarse), np.meshgrid(fine_u, fine_v)]
    xy = np.concatenate([np.stack([r.corner_u + u.ravel(), r.corner_v + v.ravel()], axis=1) for u, v in grids])
    return xy.astype(F), r


def _near_plane_depth_image(scene_pose):
    """a depth frame with a plane 0.2 m in front of the camera over the left half of the body, nothing elsewhere"""
    intr = mtv.DEPTH_INTRINSICS
    w2c = np.linalg.inv(mtv.DEPTH_CAMERA2WORLD).astype(F)
    t = T.mul_pose(w2c, scene_pose)[:3, 3]
    split = int(t[0] * F(intr["fu"]) / t[2] + F(intr["ppu"]))
    image = np.zeros((intr["height"], intr["width"]), np.uint16)
    image[:, :split] = 200
    return image


@pytest.mark.parametrize("occlusions", ["none", "measured", "modeled"])
def test_keyframe_data_equals_the_restatement(occlusions):
    api = util.open_hip()
    kw = {}
    if occlusions == "measured":
        kw["depth_image"] = _near_plane_depth_image(mtv.body2world())
    if occlusions == "modeled":
        kw.update(depth_renderer=True, bottle_offset=[0.06, 0.0, -0.15])
    s = Scene(api, **kw)
    keypoints, r = _grid(s)
    assert len(keypoints) <= T.MAX_FEATURES
    descriptors = np.random.default_rng(7).integers(0, 256, (len(keypoints), 32), dtype=np.uint8)
    # asserted on the restatement's side: the grid covers the body, its surroundings and the outside of the rendering
    u = np.floor((keypoints[:, 0] - r.corner_u) * r.scale + F(0.5))
    v = np.floor((keypoints[:, 1] - r.corner_v) * r.scale + F(0.5))
    inside = (u >= 0) & (u < r.image_size) & (v >= 0) & (v < r.image_size)
    on_body = np.zeros(len(keypoints), bool)
    on_body[inside] = r.silhouette[v[inside].astype(int), u[inside].astype(int)] == BODY_ID
    assert (~inside).sum() > 0
    assert on_body.sum() * 4 >= len(keypoints) and (~on_body).sum() * 4 >= len(keypoints)
    plain = s.state(measure_occlusions=False)
    plain.set_features(keypoints, descriptors)
    plain.compute_keyframe_data(s.body.body2world_pose(), s.cam, BODY_ID, r)
    assert len(plain.points_keyframes[0]) == on_body.sum()
    state = s.state()
    state.set_features(keypoints, descriptors)
    s.texture.SetFeatures(keypoints, descriptors)
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    if occlusions != "none":  # the occlusion test removes at least one point and keeps at least one
        assert 0 < len(state.points_keyframes[0]) < len(plain.points_keyframes[0])
    _keyframes_equal(s.texture, state)
    # the descriptors went with the points: matching the keyframe against the same features finds every point at
    # distance 0 (second distance > 0 for random rows: kept), in feature order
    assert s.tracker.CalculateCorrespondences(0, 0)
    state.calculate_correspondences(s.body.body2world_pose(), s.cam, 0)
    assert len(state.data_points) == len(state.points_keyframes[0])
    _points_equal(s.texture.points(), state.data_points)


def test_keyframe_of_a_body_the_renderer_does_not_see():
    api = util.open_hip()
    s = Scene(api, n_keyframes=2)
    keypoints = s.on_body_keypoints(70, seed=3)
    descriptors = np.random.default_rng(8).integers(0, 256, (70, 32), dtype=np.uint8)
    state = s.state()
    s.texture.SetFeatures(keypoints, descriptors)
    state.set_features(keypoints, descriptors)
    for n in (70, 40):
        s.texture.SetFeatures(keypoints[:n], descriptors[:n])
        state.set_features(keypoints[:n], descriptors[:n])
        assert s.tracker.StartModalities(0)
        s.reference_keyframe(state)
    assert [len(k) for k in state.points_keyframes] == [70, 40]
    before = state.orientation_last_keyframe.copy()
    hidden = mtv.body2world()
    hidden[:3, 3] = [0.0, 0.0, -1.0]  # behind the camera
    s.body.set_body2world_pose(hidden)
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    assert not s.rendering(s.sil).visible
    assert [len(k) for k in state.points_keyframes] == [40]  # popped, nothing pushed
    assert np.array_equal(state.orientation_last_keyframe, before) and state.keyframe_age == 0
    _keyframes_equal(s.texture, state)
    # the device kept its orientation too: back at the first pose CalculateResults sees no rotation and renews nothing;
    # had the orientation of the hidden pose been stored, the difference would be far above the threshold
    away = T.orientation(T.mul_pose(s.cam.world2camera, hidden))
    assert np.arccos(np.float64(away @ before)) > 2 * state.max_keyframe_rotation_difference
    s.body.set_body2world_pose(mtv.body2world())
    assert s.tracker.CalculateResults(0)
    assert not state.renewal_due(mtv.body2world(), s.cam)
    assert [len(k) for k in state.points_keyframes] == [40] and state.keyframe_age == 1
    _keyframes_equal(s.texture, state)


def test_region_of_interest_equals_the_restatement():
    """m3t_hip_texture_modality_get_region_of_interest composes body2camera, half the body's maximum diameter and the
    camera's intrinsics on the host: against CalculateScaleAndRegionOfInterest of the restatement, inside the image, at
    its borders, too close and outside"""
    api = util.open_hip()
    s = Scene(api, focused_image_size=160)
    vertices, _ = util.pkg.config.load_obj(os.path.join(util.GOLDEN, "_body", "triangle.obj"))
    radius = F(0.5) * T.maximum_body_diameter(vertices, np.asarray(mtv.GEOMETRY2BODY, F))
    seen = set()
    for translation in ([-0.08187602, -0.00546734, 0.618302], [0.3, 0.0, 0.5], [-0.4, 0.0, 0.6], [0.0, -0.2, 0.6],
                        [0.0, 0.19, 0.5], [0.0, 0.0, 0.05], [0.9, 0.0, 0.6], [0.0, 0.0, float(radius) * 1.6]):
        pose = mtv.body2world()
        pose[:3, 3] = translation
        s.body.set_body2world_pose(pose)
        expected = T.region_of_interest(T.mul_pose(s.cam.world2camera, pose)[:3, 3], radius, s.cam, 160)
        got = s.texture.RegionOfInterest()
        if expected is None:
            assert got is None
            seen.add("refused")
            continue
        assert got is not None and got[0] == expected[0] and got[1].tobytes() == expected[1].tobytes(), translation
        x, y, w, h = expected[0]
        seen.add("border" if x == 0 or y == 0 or x + w == s.cam.width - 1 or y + h == s.cam.height - 1 else "inside")
    assert seen == {"refused", "border", "inside"}


# ---- 3. g/H ------------------------------------------------------------------------------------------------------------
def _planted_matches(s, state, n, seed, bytes_per_row=32, pose=None):
    """a keyframe of n points whose descriptors all reappear among the current features (every query is kept), with
    correspondences a few pixels beside the projections at `pose` (the body is moved there behind the keyframe; None:
    it stays); point 0 with error == 0 exactly at that pose, point 1 with error > c"""
    rng = np.random.default_rng(seed)
    keypoints = s.on_body_keypoints(n, seed=seed)
    descriptors = rng.integers(0, 256, (n, bytes_per_row), dtype=np.uint8)
    s.texture.SetFeatures(keypoints, descriptors)
    state.set_features(keypoints, descriptors)
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    assert len(state.points_keyframes[-1]) == n
    if pose is not None:
        s.body.set_body2world_pose(pose)
    assert s.tracker.CalculateCorrespondences(0, 0)
    centers = s.texture.points()["center"].copy()
    assert len(centers) == (n if n >= 2 else 0)  # (a single current feature matches nothing)
    order = rng.permutation(n)  # the current features arrive in another order than the keyframe's points
    moved = (keypoints + rng.uniform(-6, 6, (n, 2))).astype(F)
    if n >= 2:
        moved[0] = centers[0]
        moved[1] = centers[1] + F(30.0)
    s.texture.SetFeatures(moved[order], descriptors[order])
    state.set_features(moved[order], descriptors[order])


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_gradient_hessian_equals_the_restatement(n):
    api = util.open_hip()
    s = Scene(api)
    state = s.state()
    pose = s.body.body2world_pose()
    pose[:3, 3] += np.array([0.001, 0.002, -0.002], F)  # the points have moved since the keyframe
    _planted_matches(s, state, n, seed=20 + n, pose=pose)
    for corr_iteration in (0, 1, 2):
        assert s.tracker.CalculateCorrespondences(0, corr_iteration)
        state.calculate_correspondences(pose, s.cam, corr_iteration)
        assert len(state.data_points) == (n if n >= 2 else 0)
        assert s.tracker.CalculateGradientAndHessian(0, corr_iteration, 0)
        g, h = state.gradient_hessian(pose, s.cam, corr_iteration)
        dg, dh = s.texture.gradient_hessian()
        assert np.array_equal(dg.view(np.uint32), g.view(np.uint32))
        assert np.array_equal(dh.view(np.uint32), h.view(np.uint32))
        _points_equal(s.texture.points(), state.data_points)
    if n >= 2:
        # one point with error == 0 exactly (the weight's 1 / variance branch) and one beyond the Tukey constant
        errors = [np.sqrt(F(np.sum((p["center"] - p["correspondence_center"]) ** 2, dtype=F))) for p in state.data_points]
        assert min(errors) == 0.0 and max(errors) > s.texture.params.tukey_norm_constant and np.abs(h).max() > 0


# ---- 4. Newton update --------------------------------------------------------------------------------------------------
def _oracle_stand_in(region_first=None):
    """the oracle's optimizer over a stand-in modality that takes the restated g/H (and, with region_first set, the
    oracle's own region modality before or behind it)"""
    ora = util.open_oracle()
    f = gs.RegionFixture.__new__(gs.RegionFixture)
    v = gs.views()
    f.api = ora
    f.model = host.RegionModel(ora, data_points=v["region_points"], orientations=v["region_orientations"],
                               contour_lengths=v["region_contour_lengths"])
    f.body = host.Body(ora, mtv.body2world())
    f.camera = host.ColorCamera(ora, **mtv.COLOR_INTRINSICS)
    f.camera.UpdateImage(gs.load_png("_sequence/color_camera_image_200.png"))
    f.stand_in = host.RegionModality(ora, f.body, f.camera, f.model)
    f.region = host.RegionModality(ora, f.body, f.camera, f.model) if region_first is not None else None
    modalities = [f.stand_in] if f.region is None else ([f.region, f.stand_in] if region_first else [f.stand_in, f.region])
    f.optimizer = host.Optimizer(ora, body=f.body, modalities=modalities)
    f.tracker = host.Tracker(ora)
    return f


def test_newton_update_of_a_texture_only_body_equals_the_oracle():
    api = util.open_hip()
    s = Scene(api)
    state = s.state()
    _planted_matches(s, state, 120, seed=5)
    ora = _oracle_stand_in()
    pose = s.body.body2world_pose()
    for corr_iteration in range(2):
        assert s.tracker.CalculateCorrespondences(0, corr_iteration)
        state.calculate_correspondences(pose, s.cam, corr_iteration)
        for update_iteration in range(2):
            assert s.tracker.CalculateGradientAndHessian(0, corr_iteration, update_iteration)
            assert s.tracker.CalculateOptimization(0, corr_iteration, update_iteration)
            g, h = state.gradient_hessian(pose, s.cam, corr_iteration)
            ora.stand_in.set_gradient_hessian(g, h)
            assert ora.tracker.CalculateOptimization(0, corr_iteration, update_iteration)
            new_pose = ora.body.body2world_pose()
            assert not np.array_equal(new_pose, pose)
            pose = new_pose
            assert np.array_equal(s.body.body2world_pose().view(np.uint32), pose.view(np.uint32))


@pytest.mark.parametrize("region_first", [True, False])
def test_newton_update_of_a_region_and_texture_body_follows_the_order_of_the_link(region_first):
    api = util.open_hip()
    s = Scene(api, optimizer=False)
    v = gs.views()
    model = host.RegionModel(api, data_points=v["region_points"], orientations=v["region_orientations"],
                             contour_lengths=v["region_contour_lengths"])
    s.color_camera.UpdateImage(gs.load_png("_sequence/color_camera_image_200.png"))
    region = host.RegionModality(api, s.body, s.color_camera, model)
    host.Optimizer(api, body=s.body, modalities=[region, s.texture] if region_first else [s.texture, region])
    ora = _oracle_stand_in(region_first=region_first)
    state = s.state()
    assert ora.tracker.StartModalities(0)
    _planted_matches(s, state, 90, seed=6)  # (StartModalities on the device: histograms and the keyframe)
    pose = s.body.body2world_pose()
    assert s.tracker.CalculateCorrespondences(0, 0) and ora.tracker.CalculateCorrespondences(0, 0)
    state.calculate_correspondences(pose, s.cam, 0)
    for update_iteration in range(2):
        assert s.tracker.CalculateGradientAndHessian(0, 0, update_iteration)
        assert ora.tracker.CalculateGradientAndHessian(0, 0, update_iteration)
        rg, rh = ora.region.gradient_hessian()
        dg, dh = region.gradient_hessian()
        assert np.array_equal(rg, dg) and np.array_equal(rh, dh) and np.abs(rh).max() > 0
        g, h = state.gradient_hessian(pose, s.cam, 0)
        ora.stand_in.set_gradient_hessian(g, h)
        assert s.tracker.CalculateOptimization(0, 0, update_iteration)
        assert ora.tracker.CalculateOptimization(0, 0, update_iteration)
        pose = ora.body.body2world_pose()
        assert np.array_equal(s.body.body2world_pose().view(np.uint32), pose.view(np.uint32))


# ---- 5. sequence -------------------------------------------------------------------------------------------------------
def _rotated(pose, degrees):
    a = np.deg2rad(degrees)
    r = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float64)
    out = pose.copy()
    out[:3, :3] = (pose[:3, :3].astype(np.float64) @ r).astype(F)
    return out


def test_sequence_with_keyframe_renewal_equals_a_restatement_driven_loop():
    api = util.open_hip()
    s = Scene(api, n_keyframes=2, max_keyframe_age=1)
    ora = _oracle_stand_in()
    s.tracker = host.Tracker(api, 3, 2)
    state = s.state()
    rng = np.random.default_rng(9)
    n = 150
    base = s.on_body_keypoints(n, seed=9)
    descriptors = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s.texture.SetFeatures(base, descriptors)
    state.set_features(base, descriptors)
    assert s.tracker.StartModalities(0)
    s.reference_keyframe(state)
    renewals = []
    for frame in range(6):
        # frame 4: the body turns by 12 degrees and the detector finds nothing (n = 0: no data points, the pose stays
        # where it was put): renewal by angle in a frame in which the age alone (every other frame) would not renew
        if frame == 4:
            pose = _rotated(s.body.body2world_pose(), 12.0)
            s.body.set_body2world_pose(pose)
            ora.body.set_body2world_pose(pose)
        count = n - 10 * frame if frame != 4 else 0  # another number of features in every frame
        order = rng.permutation(n)[:count]
        xy = (base[order] + rng.uniform(-2, 2, (count, 2))).astype(F)
        s.texture.SetFeatures(xy, descriptors[order])
        state.set_features(xy, descriptors[order])
        assert s.tracker.ExecuteTrackingStep(frame)
        pose = ora.body.body2world_pose()
        for corr_iteration in range(3):
            state.calculate_correspondences(pose, s.cam, corr_iteration)
            for update_iteration in range(2):
                g, h = state.gradient_hessian(pose, s.cam, corr_iteration)
                ora.stand_in.set_gradient_hessian(g, h)
                assert ora.tracker.CalculateOptimization(frame, corr_iteration, update_iteration)
                pose = ora.body.body2world_pose()
        assert len(state.data_points) > 20 or frame == 4
        assert np.array_equal(s.body.body2world_pose().view(np.uint32), pose.view(np.uint32)), frame
        _points_equal(s.texture.points(), state.data_points)
        due = state.renewal_due(pose, s.cam)
        renewals.append(due)
        if due:
            s.reference_keyframe(state, pose)  # (the renderings the device's CalculateResults used)
        _keyframes_equal(s.texture, state)
    assert renewals == [False, True, False, True, True, False], renewals  # by age, by age, by angle
    assert len(state.points_keyframes) == 2  # the ring popped


# ---- 6. batch = singles ------------------------------------------------------------------------------------------------
def test_three_bodies_in_one_context_equal_each_body_alone():
    counts = (40, 97, 300)

    def run(api, which):
        # StartModalities builds the keyframe of EVERY texture modality of the context from its current features, so
        # all bodies get their keyframe features first, one StartModalities follows, then the features of the frame
        scenes, later, poses = [], [], []
        for k in which:
            s = Scene(api, n_keyframes=1)
            rng = np.random.default_rng(30 + k)
            keypoints = s.on_body_keypoints(counts[k], seed=30 + k)
            descriptors = rng.integers(0, 256, (counts[k], 32), dtype=np.uint8)
            s.texture.SetFeatures(keypoints, descriptors)
            order = rng.permutation(counts[k])
            later.append(((keypoints + rng.uniform(-6, 6, keypoints.shape)).astype(F)[order], descriptors[order]))
            scenes.append(s)
        tracker = host.Tracker(api, 2, 2)
        assert tracker.StartModalities(0)
        for s, (keypoints, descriptors) in zip(scenes, later):
            s.texture.SetFeatures(keypoints, descriptors)
        assert tracker.ExecuteTrackingStep(0)
        for s, n in zip(scenes, [counts[k] for k in which]):
            assert len(s.texture.points()) == n  # every keyframe point found its feature
            poses.append(s.body.body2world_pose())
        return poses

    batch = run(util.open_hip(), (0, 1, 2))
    for k in range(3):
        single = run(util.open_hip(), (k,))[0]
        assert np.array_equal(batch[k].view(np.uint32), single.view(np.uint32)), k
        assert not np.array_equal(batch[k], mtv.body2world())


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone():
    capi = util.pkg._capi
    api = util.open_hip()
    s = Scene(api)
    state = s.state()
    _planted_matches(s, state, 50, seed=11)
    assert s.tracker.CalculateCorrespondences(0, 0)
    points, pose = s.texture.points().copy(), s.body.body2world_pose()
    ids = np.array([s.body.id], np.int32)
    poses = capi.pose_arg(np.eye(4)).copy()
    opt = np.array([0], np.int32)
    row = C.c_int()
    judge = host.Judge(api, [s.body], 4)
    unique_id = (C.c_char * 128)()
    refused = [
        api.raw("reset_bodies", capi.iptr(ids), capi.fptr(poses), 1, 0),
        api.raw("reset_structures", capi.iptr(opt), 1, capi.fptr(poses), 0, 0),
        api.raw("judge_bodies", judge.id, capi.fptr(poses), 0, C.byref(row)),
        api.raw("set_roi_ingest", 1, 4.0),
        api.raw("comm_set_reduce_callback", KEEP_CALLBACK, None),
        # a communicator: the host's own (any non-null handle is refused before the collective library is opened) and
        # the library's own (well-formed arguments, refused before a communicator is made)
        api.raw("comm_set", C.c_void_p(8)),
        api.raw("comm_init_rank", C.cast(unique_id, C.c_void_p), 128, 1, 0),
    ]
    assert refused == [capi.M3T_ERR_UNSUPPORTED] * len(refused), refused
    assert "texture modality" in api.last_error()
    assert api.raw("judge_bodies", judge.id, capi.fptr(poses), -1, C.byref(row)) == 0  # judge-only calls take it
    assert np.array_equal(s.body.body2world_pose(), pose)
    assert s.tracker.CalculateCorrespondences(0, 1)
    assert np.array_equal(s.texture.points(), points)
    rank_count = C.c_int(-1)
    api.call("comm_get_rank_count", C.byref(rank_count))
    assert rank_count.value == 0  # no communicator was kept
    # a silhouette renderer with REGION ids, a depth renderer, an L2 descriptor's size
    geometry = host.RendererGeometry(api)
    geometry.AddBody(s.body)
    wrong = host.FocusedSilhouetteRenderer(api, geometry, s.color_camera, id_type=1)
    wrong.AddReferencedBody(s.body)
    with pytest.raises(capi.M3TError) as e:
        host.TextureModality(api, s.body, s.color_camera, wrong)
    assert e.value.code == capi.M3T_ERR_INVALID_ARGUMENT and "BODY" in str(e.value)
    depth = host.FocusedBasicDepthRenderer(api, geometry, s.color_camera)
    depth.AddReferencedBody(s.body)
    with pytest.raises(capi.M3TError):
        host.TextureModality(api, s.body, s.color_camera, depth)
    with pytest.raises(capi.M3TError):
        host.TextureModality(api, s.body, s.color_camera, s.sil, descriptor_bytes=128)  # an L2 descriptor's size
    assert np.array_equal(s.body.body2world_pose(), pose) and s.tracker.CalculateCorrespondences(0, 1)
    assert np.array_equal(s.texture.points(), points)
    # more than M3T_MAX_LINK_MODALITIES (4) modalities on a link, a texture modality among them: refused where the
    # link table is built, before anything runs -- no keyframe, the pose as it was
    crowded = util.open_hip()
    c = Scene(crowded, optimizer=False)
    few = c.on_body_keypoints(10, seed=1)  # (rendered while the context can still build its tables)
    link = host.Link(crowded, c.body)
    link.AddModality(c.texture)
    for _ in range(4):
        link.AddModality(host.TextureModality(crowded, c.body, c.color_camera, c.sil))
    host.Optimizer(crowded, link)
    c.texture.SetFeatures(few, np.zeros((10, 32), np.uint8))
    assert crowded.raw("start_modalities", 0) == capi.M3T_ERR_UNSUPPORTED
    assert "too many modalities per link" in crowded.last_error()
    assert crowded.raw("execute_tracking_step", 0) == capi.M3T_ERR_UNSUPPORTED
    assert c.texture.keyframes() == (0, []) and len(c.texture.points()) == 0
    assert np.array_equal(c.body.body2world_pose(), mtv.body2world())
    # ROI ingest or a reduce callback first: the modality is refused
    for setup in (lambda a: a.call("set_roi_ingest", 1, 4.0),
                  lambda a: a.call("comm_set_reduce_callback", KEEP_CALLBACK, None)):
        other = util.open_hip()
        setup(other)
        with pytest.raises(capi.M3TError) as e:
            Scene(other)
        assert e.value.code == capi.M3T_ERR_UNSUPPORTED


KEEP_CALLBACK = util.pkg._capi.REDUCE_FN(lambda *a: 0)


def test_a_context_with_a_texture_modality_steps_by_sub_steps_and_one_without_keeps_its_kernel():
    name = C.create_string_buffer(64)
    api = util.open_hip()
    s = Scene(api)
    _planted_matches(s, s.state(), 30, seed=12)
    assert s.tracker.ExecuteTrackingStep(0)
    api.call("get_step_kernel", name, 64)
    assert name.value == b""
    # the 64-object batch of tests/test_gpu_benchmark_shape.py (its inputs, one frame): launch choice and launch shape
    # are the ones that test pins for contexts without a texture modality
    import bench
    import scenes
    inputs = scenes.Inputs(64, 6, n_divides=4, n_models=bench.CONFIGS["rbot64"]["models"])
    plain = util.open_hip()
    batch = scenes.Instance(plain, inputs)
    batch.upload_frame(0)
    assert batch.tracker.StartModalities(0) and batch.tracker.ExecuteTrackingStep(0)
    plain.call("get_step_kernel", name, 64)
    shape = (C.c_int * 4)()
    plain.call("get_step_shape", shape)
    assert name.value == b"tracking_step_split_kernel" and list(shape) == [64, 4, 512, 1]
