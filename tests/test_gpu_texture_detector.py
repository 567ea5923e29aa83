"""The built-in feature detector of the texture modality on the device (csrc/m3t_features.hip behind
m3t_hip_texture_modality_set_detector) against its integer restatement (tests/feature_reference.py), bit for bit: the
focused image, the keypoints and the descriptors of get_focused_image / get_features; then the modality driven by the
built-in detector against the same modality fed with the restatement's output through SetFeatures.

Scenes: a 160 x 120 colour frame and a flat plate in front of the camera.  The "unit" scene is built so that the scale
of the focused image is exactly 1 (z = 1.25, radius 0.75: z^2 - r^2 = 1, r_u = 48 pixels, focused_image_size 96): the
focused image is then the grey of a 116 x 116 crop of the frame, and corners can be drawn at exact focused pixels."""
import ctypes as C

import numpy as np
import pytest

import feature_reference as FR
import feature_scenes as FS
import texture_reference as T
import util
from util import host

pytestmark = pytest.mark.gpu
capi = util.pkg._capi
F = np.float32
WIDTH, HEIGHT = 160, 120
BAND = FR.BAND


def _pose(x, y, z):
    pose = np.eye(4, dtype=F)
    pose[:3, 3] = [x, y, z]
    return pose


class Plate:
    """a diamond-shaped plate (vertices at distance `radius` on the body's x and y axes) facing the camera, with a
    focused silhouette renderer and a texture modality; cameras and images are shared through `frame`"""

    def __init__(self, api, frame, pose, radius, builtin=True, focused_image_size=64, n_features=500, fast_threshold=20,
                 body_id=150, optimizer=True, **params):
        self.api, self.frame = api, frame
        self.radius = F(radius)
        r = float(radius)
        self.vertices = np.array([[r, 0, 0], [0, r, 0], [-r, 0, 0], [0, -r, 0]], F)
        self.body = host.Body(api, pose)
        self.body.set_geometry(self.vertices, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.eye(4, dtype=F),
                               geometry_enable_culling=False, body_id=body_id, region_id=body_id)
        assert T.maximum_body_diameter(self.vertices, np.eye(4)) == F(2.0) * self.radius
        geometry = host.RendererGeometry(api)
        geometry.AddBody(self.body)
        self.sil = host.FocusedSilhouetteRenderer(api, geometry, frame.camera, id_type=0)
        self.sil.AddReferencedBody(self.body)
        self.focused_image_size = focused_image_size
        self.texture = host.TextureModality(api, self.body, frame.camera, self.sil,
                                            focused_image_size=focused_image_size, **params)
        self.n_features, self.fast_threshold = n_features, fast_threshold
        if builtin:
            self.texture.SetDetector(n_features=n_features, fast_threshold=fast_threshold)
        if optimizer:
            host.Optimizer(api, body=self.body, modalities=[self.texture])

    def reference(self, image=None, pose=None):
        """the restatement's detection at the body's pose (world2camera is the identity: the translation is the
        pose's) on the frame the camera holds"""
        pose = self.body.body2world_pose() if pose is None else pose
        return FR.detect(self.frame.image if image is None else image, pose[:3, 3], self.radius, self.frame.cam,
                         self.focused_image_size, self.n_features, self.fast_threshold)

    def feed(self, detection):
        self.texture.SetFeatures(detection.keypoints, detection.descriptors)

    def equals(self, detection):
        focused = self.texture.focused_image()
        if detection.focused is None:
            assert focused is None
        else:
            assert focused is not None and focused.shape == detection.focused.shape, (focused, detection.focused.shape)
            assert np.array_equal(focused, detection.focused)
        keypoints, descriptors = self.texture.features()
        assert len(keypoints) == len(detection.keypoints), (len(keypoints), len(detection.keypoints))
        assert np.array_equal(keypoints.view(np.uint32), detection.keypoints.view(np.uint32))
        assert np.array_equal(descriptors, detection.descriptors)


class Frame:
    def __init__(self, api, fu=200.0, fv=200.0, ppu=79.5, ppv=59.5):
        intrinsics = dict(fu=fu, fv=fv, ppu=ppu, ppv=ppv, width=WIDTH, height=HEIGHT)
        self.camera = host.ColorCamera(api, **intrinsics)
        self.cam = T.Camera(**intrinsics)
        self.image = None

    def show(self, image):
        self.image = np.ascontiguousarray(image, np.uint8)
        self.camera.UpdateImage(self.image)


# ---- the unit scene: focused pixel (x, y) is frame pixel (22 + x, 2 + y) -----------------------------------------------
UNIT_SIDE, UNIT_X, UNIT_Y = 116, 22, 2


def _unit(api, **kw):
    frame = Frame(api, fu=64.0, fv=64.0)
    plate = Plate(api, frame, _pose(0.0, 0.0, 1.25), 0.75, focused_image_size=96, **kw)
    return frame, plate


def _unit_frame(focused_grey):
    """the colour frame whose focused image in the unit scene is the given 116 x 116 grey image"""
    assert focused_grey.shape == (UNIT_SIDE, UNIT_SIDE)
    image = np.full((HEIGHT, WIDTH, 3), 90, np.uint8)
    image[UNIT_Y:UNIT_Y + UNIT_SIDE, UNIT_X:UNIT_X + UNIT_SIDE] = FS.as_bgr(focused_grey)
    return image


def _detect_once(frame, plate, image):
    frame.show(image)
    assert host.Tracker(plate.api).StartModalities(0)
    detection = plate.reference()
    plate.equals(detection)
    return detection


def _dots(points, ground=60, values=250):
    """isolated one-pixel dots: each is a corner of score 16 * (value - ground - threshold), and nothing else is"""
    image = np.full((UNIT_SIDE, UNIT_SIDE), ground, np.uint8)
    values = [values] * len(points) if np.isscalar(values) else values
    for (x, y), v in zip(points, values):
        image[y, x] = v
    return image


def _found(detection):
    return [(int(x), int(y)) for x, y in detection.xy]


def test_unit_scene_focuses_without_resampling():
    api = util.open_hip()
    frame, plate = _unit(api)
    grey = FS.blocks(UNIT_SIDE, UNIT_SIDE, seed=3)[..., 0]
    detection = _detect_once(frame, plate, _unit_frame(grey))
    assert detection.roi == (UNIT_X, UNIT_Y, UNIT_SIDE, UNIT_SIDE) and detection.scale == F(1.0)
    assert np.array_equal(detection.focused, grey) and len(detection.xy) > 20
    assert UNIT_SIDE % 16 != 0 and UNIT_SIDE % BAND != 0


# ---- focus -------------------------------------------------------------------------------------------------------------
# (pose, radius, focused_image_size): scale below and above 1, sides that are no multiples of 16; a region of interest
# clipped by the left and top edges of the frame
FOCUS_CASES = {
    "below_1": (_pose(0.0, 0.0, 0.3), 0.05, 56),
    "above_1": (_pose(0.01, -0.005, 0.5), 0.05, 50),
    "clipped": (_pose(-0.17, -0.12, 0.5), 0.06, 84),
}


@pytest.mark.parametrize("case", sorted(FOCUS_CASES))
def test_focused_image_and_features_equal_the_restatement(case):
    pose, radius, size = FOCUS_CASES[case]
    api = util.open_hip()
    frame = Frame(api)
    plate = Plate(api, frame, pose, radius, focused_image_size=size, fast_threshold=15)
    detection = _detect_once(frame, plate, FS.blocks(HEIGHT, WIDTH, seed=11, n=260, low=3, high=10))
    fh, fw = detection.focused.shape
    assert 64 <= max(fw, fh) <= 96 and (fw % 16 or fh % 16) and (fw % BAND or fh % BAND), (fw, fh)
    assert len(detection.xy) >= 10, len(detection.xy)
    if case == "below_1":
        assert detection.scale < 1
    else:
        assert detection.scale > 1
    if case == "clipped":
        assert detection.roi[0] == 0 and detection.roi[1] == 0
    else:
        assert detection.roi[0] > 0 and detection.roi[1] > 0


def test_invalid_region_of_interest_leaves_no_features_and_the_next_frame_detects_again():
    api = util.open_hip()
    frame = Frame(api)
    plate = Plate(api, frame, _pose(0.0, 0.0, 0.5), 0.05, focused_image_size=70)
    tracker = host.Tracker(api)
    image = FS.blocks(HEIGHT, WIDTH, seed=12, n=260, low=3, high=10)
    first = _detect_once(frame, plate, image)
    assert len(first.xy) > 0
    plate.body.set_body2world_pose(_pose(0.0, 0.0, 0.07))  # z < 1.5 r
    assert tracker.StartModalities(0)
    nothing = plate.reference()
    assert nothing.roi is None and len(nothing.keypoints) == 0
    plate.equals(nothing)
    plate.body.set_body2world_pose(_pose(0.0, 0.0, 0.5))
    assert tracker.StartModalities(0)
    plate.equals(first)


def _pose_with_focused_side(cam, radius, size, side):
    """a pose on the optical axis whose focused image has the given larger side"""
    for z in np.linspace(0.2, 0.6, 4001):
        found = T.region_of_interest([0.0, 0.0, z], radius, cam, size)
        if found is None:
            continue
        roi, scale = found
        if max(FR.focused_side(roi[2], scale), FR.focused_side(roi[3], scale)) == side:
            return _pose(0.0, 0.0, z)
    raise AssertionError("no pose gives a focused side of %d" % side)


@pytest.mark.parametrize("side", [FR.FOCUSED_MAX, FR.FOCUSED_MAX + 1])
def test_focused_side_at_the_cap_detects_and_one_above_leaves_no_features(side):
    api = util.open_hip()
    frame = Frame(api)
    radius, size = 0.05, 400
    pose = _pose_with_focused_side(frame.cam, radius, size, side)
    plate = Plate(api, frame, pose, radius, focused_image_size=size, n_features=50)
    detection = _detect_once(frame, plate, FS.blocks(HEIGHT, WIDTH, seed=13, n=260, low=3, high=10))
    if side > FR.FOCUSED_MAX:
        assert detection.roi is not None and detection.focused is None and len(detection.keypoints) == 0
    else:
        assert max(detection.focused.shape) == FR.FOCUSED_MAX and len(detection.keypoints) == 50


# ---- FAST and suppression ----------------------------------------------------------------------------------------------
def test_border_band_boundaries_and_suppression():
    api = util.open_hip()
    frame, plate = _unit(api)
    last = UNIT_SIDE - FR.BORDER - 1
    kept = [(16, 16), (last, last), (16, last), (last, 16),           # at distance 16 from the edges
            (30, 2 * BAND - 1), (40, 2 * BAND), (60, 3 * BAND - 1), (70, 3 * BAND), (50, 4 * BAND)]  # around band boundaries
    dropped = [(15, 40), (40, 15), (last + 1, 60), (60, last + 1),    # at distance 15
               (50, 50), (51, 50),                                    # adjacent, equal score: both vanish
               (80, 2 * BAND - 1), (80, 2 * BAND),                    # adjacent across a band boundary
               (90, 5 * BAND - 1), (91, 5 * BAND)]                    # diagonal neighbours across a band boundary
    detection = _detect_once(frame, plate, _unit_frame(_dots(kept + dropped)))
    assert sorted(_found(detection)) == sorted(kept)
    assert set(detection.scores) == {16 * (250 - 60 - 20)}
    # the stronger of two neighbours across a band boundary survives, from either side
    pairs = [(30, 2 * BAND - 1), (30, 2 * BAND), (60, 3 * BAND), (61, 3 * BAND - 1)]
    detection = _detect_once(frame, plate, _unit_frame(_dots(pairs, values=[250, 240, 250, 240])))
    assert sorted(_found(detection)) == [(30, 2 * BAND - 1), (60, 3 * BAND)]


def test_constant_image_has_no_features():
    api = util.open_hip()
    frame, plate = _unit(api)
    detection = _detect_once(frame, plate, np.full((HEIGHT, WIDTH, 3), 123, np.uint8))
    assert detection.focused is not None and len(detection.keypoints) == 0


# ---- selection ---------------------------------------------------------------------------------------------------------
def _grid(step=7, first=18):
    return [(x, y) for y in range(first, UNIT_SIDE - FR.BORDER, step) for x in range(first, UNIT_SIDE - FR.BORDER, step)]


@pytest.mark.parametrize("n_features", [1, 12, 40, 144, 145, 4096])
def test_selection_keeps_the_best_and_the_first_in_raster_order_among_equals(n_features):
    """144 dots on a 12 x 12 grid in three strengths: 20 strong ones, 24 middle ones, 100 weak ones.  n = 12: the cut
    is among the strong ones; n = 40: four more than the strong ones, 24 tied at the cut; 144: exactly all; more: all"""
    points = _grid()
    assert len(points) == 144
    rng = np.random.default_rng(5)
    strength = np.full(144, 200)
    order = rng.permutation(144)
    strength[order[:20]] = 250
    strength[order[20:44]] = 225
    api = util.open_hip()
    frame, plate = _unit(api, n_features=n_features)
    detection = _detect_once(frame, plate, _unit_frame(_dots(points, values=list(strength))))
    score_map = FR.suppress(FR.fast_scores(detection.focused, 20))
    assert sorted(set(score_map[score_map > 0])) == [16 * 120, 16 * 145, 16 * 170]  # really equal within a strength
    raster = [p for p in points]  # _grid is in raster order
    by_strength = {v: [p for p, s in zip(raster, strength) if s == v] for v in (250, 225, 200)}
    expected = {1: by_strength[250][:1], 12: by_strength[250][:12], 40: by_strength[250] + by_strength[225][:20],
                144: raster, 145: raster, 4096: raster}[n_features]
    assert _found(detection) == sorted(expected, key=lambda p: (p[1], p[0]))


# ---- descriptor --------------------------------------------------------------------------------------------------------
def test_direction_tie_takes_the_lowest_bin():
    """a ground that brightens downwards and does not change along x: m10 = 0 exactly and m01 > 0, so bins 7 and 8
    (S = 16294 both, C = 1713 and -1713) tie; a dot on it is the keypoint"""
    ground = np.repeat((40 + np.arange(UNIT_SIDE))[:, None], UNIT_SIDE, axis=1).astype(np.uint8)
    ground[58, 58] = 255
    api = util.open_hip()
    frame, plate = _unit(api)
    detection = _detect_once(frame, plate, _unit_frame(ground))
    assert _found(detection) == [(58, 58)]
    m10, m01 = FR.moments(detection.focused, 58, 58)
    values = m10 * FR.COS + m01 * FR.SIN
    assert m10 == 0 and m01 > 0 and values[7] == values[8] == values.max()
    assert list(detection.bins) == [7]


def test_all_thirty_directions_occur_in_one_seeded_image():
    api = util.open_hip()
    frame, plate = _unit(api, fast_threshold=10)
    grey = FS.blocks(UNIT_SIDE, UNIT_SIDE, seed=14, n=400, low=2, high=8)[..., 0]
    detection = _detect_once(frame, plate, _unit_frame(grey))
    assert set(detection.bins) == set(range(FR.N_DIRECTIONS)), sorted(set(detection.bins))


# ---- integration -------------------------------------------------------------------------------------------------------
def _points_equal(a, b):
    assert len(a) == len(b)
    for name in ("center_f_body", "correspondence_center", "center_f_camera", "center"):
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def _state_equal(a, b):
    assert np.array_equal(a.body.body2world_pose().view(np.uint32), b.body.body2world_pose().view(np.uint32))
    _points_equal(a.texture.points(), b.texture.points())
    (age_a, frames_a), (age_b, frames_b) = a.texture.keyframes(), b.texture.keyframes()
    assert age_a == age_b and len(frames_a) == len(frames_b)
    for x, y in zip(frames_a, frames_b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


PLATES = [(_pose(0.0, 0.0, 0.5), 0.06, 60), (_pose(-0.1, 0.03, 0.55), 0.05, 54), (_pose(0.11, -0.04, 0.45), 0.045, 64)]
SEQUENCE_IMAGE = FS.blocks(HEIGHT, WIDTH, seed=21, n=300, low=3, high=9)


def _sequence(which, builtin):
    """StartModalities and three tracking steps over frames that move by a pixel or two: the poses, data points and
    keyframes after every call.  builtin[k]: plate k detects on the device, else it is fed the restatement's features
    for its own region of interest in front of every call (generator.Tracker.DetectFeatures)"""
    api = util.open_hip()
    frame = Frame(api)
    plates = [Plate(api, frame, *PLATES[k][:2], builtin=b, focused_image_size=PLATES[k][2], fast_threshold=15,
                    body_id=100 + k, n_keyframes=2, max_keyframe_age=2) for k, b in zip(which, builtin)]
    tracker = host.Tracker(api, 2, 2)
    history = []
    for step, shift in enumerate([(0, 0), (1, 0), (1, 1), (2, 1)]):
        frame.show(np.roll(SEQUENCE_IMAGE, (shift[1], shift[0]), axis=(0, 1)))
        for plate, b in zip(plates, builtin):
            if not b:
                plate.feed(plate.reference())
        assert tracker.StartModalities(0) if step == 0 else tracker.ExecuteTrackingStep(step)
        history.append([(p.body.body2world_pose(), p.texture.points(), p.texture.keyframes()) for p in plates])
    return plates, history


def _histories_equal(a, b):
    assert len(a) == len(b)
    for step, (sa, sb) in enumerate(zip(a, b)):
        for (pose_a, points_a, keys_a), (pose_b, points_b, keys_b) in zip(sa, sb):
            assert np.array_equal(pose_a.view(np.uint32), pose_b.view(np.uint32)), step
            _points_equal(points_a, points_b)
            assert keys_a[0] == keys_b[0] and len(keys_a[1]) == len(keys_b[1]), step
            for x, y in zip(keys_a[1], keys_b[1]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), step


def test_sequence_with_keyframe_renewal_equals_the_modality_fed_with_the_restatement():
    _, device = _sequence([0], [True])
    plates, fed = _sequence([0], [False])
    _histories_equal(device, fed)
    # not vacuous: data points in every step, the pose moves, one renewal by age (a second keyframe is held)
    assert all(len(step[0][1]) > 10 for step in fed[1:])
    assert not np.array_equal(fed[3][0][0], PLATES[0][0])
    assert [len(step[0][2][1]) for step in fed] == [1, 1, 1, 2]


def test_three_bodies_one_of_them_caller_fed_equal_three_caller_fed_bodies():
    _, mixed = _sequence([0, 1, 2], [True, False, True])
    _, fed = _sequence([0, 1, 2], [False, False, False])
    _histories_equal(mixed, fed)
    assert all(len(points) > 5 for _, points, _ in fed[1])


def test_one_step_follows_a_plate_shifted_by_three_and_two_pixels():
    """the unit scene: a pixel is 1.25 / 64 m at the plate.  The whole frame moves by (3, 2) pixels between the keyframe
    and the next frame; one tracking step has to reduce the error of the translation in x and in y.  Observed (written
    down, not bounded): 0.05859 / 0.03906 m before, 0.03844 / 0.02566 m after the step"""
    api = util.open_hip()
    frame, plate = _unit(api, fast_threshold=15)
    grey = FS.blocks(UNIT_SIDE, UNIT_SIDE, seed=31, n=120, low=3, high=9)[..., 0]
    tracker = host.Tracker(api, 4, 2)
    frame.show(_unit_frame(grey))
    assert tracker.StartModalities(0)
    frame.show(np.roll(_unit_frame(grey), (2, 3), axis=(0, 1)))
    assert tracker.ExecuteTrackingStep(1)
    assert len(plate.texture.points()) > 20
    metre = 1.25 / 64.0
    target = np.array([3 * metre, 2 * metre])
    after = plate.body.body2world_pose()[:2, 3].astype(np.float64)
    residual = np.abs(after - target)
    print("translation error before:", target, "after one step:", residual)
    assert residual[0] < target[0] and residual[1] < target[1]


def test_generated_tracker_with_the_builtin_detector_equals_one_driven_by_the_restatement(tmp_path):
    from test_generator import reference_tree
    from test_gpu_texture_generator import CONFIG
    import golden_scene as gs
    root = reference_tree(tmp_path)
    config = root / "tracker_test" / "texture_config.yaml"
    config.write_text(CONFIG)
    (root / "tracker_test" / "texture_modality.yaml").write_text(
        '%YAML:1.2\ndescriptor_type: "ORB"\nn_keyframes: 2\norb_n_features: 300\n')
    generator = util.pkg.generator
    calls = []

    def restatement(image, roi, scale):
        focused = FR.focus(image, roi, scale)
        xy, _, _, descriptors = FR.detect_focused(focused, 300, 20)
        calls.append(len(xy))
        return xy.astype(F), descriptors

    trackers = [generator.GenerateConfiguredTracker(util.open_hip(), str(config), feature_detector=d)
                for d in ("builtin", restatement)]
    for tracker in trackers:
        tracker.objects["Body"]["triangle"].set_body2world_pose(gs.mtv.body2world())
        assert tracker.SetUp() and tracker.StartModalities(0)
        assert tracker.ExecuteTrackingStep(0) and tracker.ExecuteTrackingStep(1)
    assert len(calls) == 3 and min(calls) > 50, calls
    a, b = (t.objects["TextureModality"]["triangle_texture_modality"] for t in trackers)
    assert a.detector is not None and a.detector.n_features == 300 and b.detector is None
    pose_a, pose_b = (t.objects["Body"]["triangle"].body2world_pose() for t in trackers)
    assert np.array_equal(pose_a.view(np.uint32), pose_b.view(np.uint32))
    _points_equal(a.points(), b.points())
    assert len(b.points()) > 20
    for x, y in zip(a.keyframes()[1], b.keyframes()[1]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    with pytest.raises(ValueError, match="needs the caller's feature detector"):
        generator.GenerateConfiguredTracker(util.open_hip(), str(config))


# ---- boundary ----------------------------------------------------------------------------------------------------------
def test_set_features_is_refused_while_the_detector_is_set_and_null_hands_them_back():
    api = util.open_hip()
    frame, plate = _unit(api)
    grey = FS.blocks(UNIT_SIDE, UNIT_SIDE, seed=3)[..., 0]
    detection = _detect_once(frame, plate, _unit_frame(grey))
    tracker = host.Tracker(api, 2, 2)
    assert tracker.CalculateCorrespondences(0, 0)
    points, keyframes = plate.texture.points().copy(), plate.texture.keyframes()
    assert len(points) > 5
    xy = np.array([[50.0, 50.0], [60.0, 61.0]], F)
    rows = np.zeros((2, 32), np.uint8)
    rc = api.raw("texture_modality_set_features", plate.texture.id, capi.fptr(xy),
                 rows.ctypes.data_as(C.POINTER(C.c_uint8)), 2)
    assert rc == capi.M3T_ERR_UNSUPPORTED and "detects its features itself" in api.last_error()
    plate.equals(detection)
    assert tracker.CalculateCorrespondences(0, 1)
    assert np.array_equal(plate.texture.points(), points) and plate.texture.keyframes()[0] == keyframes[0]
    # NULL: the caller's features again -- nothing is detected, what set_features brings is what the modality holds
    plate.texture.SetDetector(builtin=False)
    plate.texture.SetFeatures(xy, rows)
    assert tracker.CalculateCorrespondences(0, 0)
    held_xy, held_rows = plate.texture.features()
    assert np.array_equal(held_xy, xy) and np.array_equal(held_rows, rows)
    # and the detector again
    plate.texture.SetDetector(n_features=500, fast_threshold=20)
    assert tracker.CalculateCorrespondences(0, 0)
    plate.equals(detection)


def test_refused_detector_parameters_and_a_context_without_a_detector():
    api = util.open_hip()
    frame = Frame(api)
    plate = Plate(api, frame, _pose(0.0, 0.0, 0.5), 0.05, builtin=False)
    for bad in (dict(n_features=0), dict(n_features=4097), dict(fast_threshold=256), dict(fast_threshold=-1), dict(type=7)):
        params = capi.TextureDetectorParams(**bad)
        assert api.raw("texture_modality_set_detector", plate.texture.id, C.byref(params)) == capi.M3T_ERR_INVALID_ARGUMENT, bad
    assert api.raw("texture_modality_set_detector", 99, C.byref(capi.TextureDetectorParams())) == capi.M3T_ERR_INVALID_ARGUMENT
    long_rows = Plate(api, frame, _pose(0.0, 0.0, 0.5), 0.05, builtin=False, descriptor_bytes=64, body_id=151)
    too_large = Plate(api, frame, _pose(0.0, 0.0, 0.5), 0.05, builtin=False, focused_image_size=FR.FOCUSED_MAX + 1,
                      body_id=152)
    for refused in (long_rows, too_large):
        assert api.raw("texture_modality_set_detector", refused.texture.id,
                       C.byref(capi.TextureDetectorParams())) == capi.M3T_ERR_UNSUPPORTED
    # nothing above set a detector: the context runs what it ran before -- no detection state exists, the features are
    # the caller's, and the step is the sub-step path of every context with a texture modality
    frame.show(FS.blocks(HEIGHT, WIDTH, seed=11, n=260, low=3, high=10))
    for p in (plate, long_rows, too_large):
        p.texture.SetFeatures(np.zeros((0, 2), F), np.zeros((0, p.texture.params.descriptor_bytes), np.uint8))
    tracker = host.Tracker(api, 2, 2)
    assert tracker.StartModalities(0) and tracker.ExecuteTrackingStep(0)
    width, height = C.c_int(), C.c_int()
    assert api.raw("texture_modality_get_focused_image", plate.texture.id, None, 0, C.byref(width),
                   C.byref(height)) == capi.M3T_ERR_NOT_SET_UP
    assert len(plate.texture.features()[0]) == 0
    name = C.create_string_buffer(64)
    api.call("get_step_kernel", name, 64)
    assert name.value == b""
