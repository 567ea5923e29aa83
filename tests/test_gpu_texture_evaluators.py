"""The texture columns of the YCB and OPT evaluators on the device (evaluation.evaluate_ycb_dataset /
evaluate_opt_dataset with use_texture_modality) on small datasets of thin textured plates: two bodies in the YCB layout,
two in the OPT layout, 4 to 6 frames each.  A plate faces the camera and moves in its own plane by whole pixels, so a
frame is one textured image shifted by those pixels with the plate brighter than the ground, and its depth image holds
the plate's front face.  Each evaluator equals, float for float, a loop written out here with host objects in the
reference's construction order (ycb_evaluator.cpp:476-492, :625; opt_evaluator.cpp:314-326); the loop also shows that
the texture modality has data points in every tracked frame and that the column differs from the Region + Depth one."""
import os

import numpy as np
import pytest

import feature_scenes as FS
import util
from util import host

pytestmark = pytest.mark.gpu
ev = util.pkg.evaluation
generator = util.pkg.generator
F = np.float32
INTRINSICS = ev.YCB_INTRINSICS  # (evaluate_ycb_dataset has no other; the OPT dataset brings the same small frames)
FU, FV, PPU, PPV, WIDTH, HEIGHT = INTRINSICS
RADIUS, HALF_THICKNESS, DISTANCE = 0.06, 0.01, 0.8  # of a plate: metres
MODEL_PARAMETERS = dict(n_divides=2, n_points=200, image_size=400)
DETECTOR = dict(n_features=300, fast_threshold=15)


def write_plate_obj(path):
    """a diamond-shaped prism: vertices at RADIUS on the body's x and y axes, faces at z = -+HALF_THICKNESS, outward
    counter-clockwise triangles"""
    r, h = RADIUS, HALF_THICKNESS
    corners = [(r, 0), (0, r), (-r, 0), (0, -r)]
    vertices = [(x, y, -h) for x, y in corners] + [(x, y, h) for x, y in corners]
    faces = [(0, 3, 2), (0, 2, 1), (4, 5, 6), (4, 6, 7)]
    for i in range(4):
        j = (i + 1) % 4
        faces += [(i, j, 4 + j), (i, 4 + j, 4 + i)]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.writelines("v %.9g %.9g %.9g\n" % v for v in vertices)
        f.writelines("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in faces)


def plate_frames(seed, shifts, depth_scale):
    """[(pose, colour image BGR, depth image u16)]: the plate's front face at DISTANCE, its centre `shift` pixels from
    the principal point"""
    base = FS.blocks(HEIGHT, WIDTH, seed=seed, n=1500, low=4, high=12).astype(np.int32)
    ys, xs = np.mgrid[0:HEIGHT, 0:WIDTH]
    out = []
    for dx, dy in shifts:
        pose = np.eye(4, dtype=F)
        pose[:3, 3] = [dx * DISTANCE / FU, dy * DISTANCE / FV, DISTANCE + HALF_THICKNESS]
        moved = np.roll(base, (dy, dx), axis=(0, 1))
        on_plate = (np.abs(xs - (PPU + dx)) * (DISTANCE / FU) + np.abs(ys - (PPV + dy)) * (DISTANCE / FV)) <= RADIUS
        color = np.where(on_plate[..., None], moved // 2 + 120, moved // 2).astype(np.uint8)
        depth = np.where(on_plate, DISTANCE, 1.5) / depth_scale
        out.append((pose, color, depth.astype(np.uint16)))
    return out


SHIFTS = {"first": [(0, 0), (2, 1), (3, 3), (5, 4), (6, 6), (8, 7)], "second": [(-20, 10), (-22, 11), (-23, 13), (-25, 14)],
          "third": [(15, -12), (16, -14), (18, -15), (19, -17), (21, -18)]}


def _save(path, image):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(image).save(path)


def _pose_line(p):
    return "1 0 0 0 %.9g %.9g %.9g" % (p[0, 3], p[1, 3], p[2, 3])  # the plates do not turn


@pytest.fixture(scope="module")
def ycb(tmp_path_factory):
    """sequence 0000 with 002_master_chef_can (6 frames), 0001 with 003_cracker_box (4 frames), every frame a keyframe"""
    root = tmp_path_factory.mktemp("ycb_plates")
    dataset, external = root / "YCB-Video", root / "external"
    names = ["002_master_chef_can", "003_cracker_box"]
    os.makedirs(dataset / "image_sets")
    os.makedirs(external / "models")
    keyframe_lines = []
    for index, (sequence, name, shifts) in enumerate((("0000", names[0], SHIFTS["first"]), ("0001", names[1], SHIFTS["second"]))):
        write_plate_obj(str(dataset / "models" / name / "textured.obj"))
        frames = plate_frames(40 + index, shifts, 1e-4)
        for k, (pose, color, depth) in enumerate(frames, 1):
            _save(str(dataset / "data" / sequence / ("%06d-color.png" % k)), np.ascontiguousarray(color[:, :, ::-1]))
            _save(str(dataset / "data" / sequence / ("%06d-depth.png" % k)), depth)
            (dataset / "data" / sequence / ("%06d-box.txt" % k)).write_text("%s 10.0 20.0 110.0 120.0\n" % name)
            keyframe_lines.append("%s/%06d\n" % (sequence, k))
        os.makedirs(external / "poses" / "ground_truth", exist_ok=True)
        (external / "poses" / "ground_truth" / ("%s_%s.txt" % (sequence, name))).write_text(
            "".join(_pose_line(pose) + "\n" for pose, _, _ in frames))
    (dataset / "image_sets" / "keyframe.txt").write_text("".join(keyframe_lines))
    kw = dict(n_vertices_evaluation=8, model_parameters=MODEL_PARAMETERS, detector_parameters=DETECTOR)
    return str(dataset), str(external), names, kw


def _ycb_twin(dataset, external, sequence, name, kw, judge_on_device, use_texture=True):
    """the run of one (sequence, body) written out: returns (per-frame results, final pose, points per tracked frame)"""
    api = util.open_hip()
    model_parameters = dict(ev.YCB_MODEL_PARAMETERS, **kw["model_parameters"])
    body = generator.Body(api, name, os.path.join(dataset, "models", name, "textured.obj"), 1.0, True, True,
                          np.eye(4, dtype=F))
    assert util.pkg.config.model_bin_matches(os.path.join(external, "models", name + "_region_model.bin"), True,
                                             model_parameters, body.body_data())  # (the evaluator wrote them)
    region_model = host.RegionModel(api, path=os.path.join(external, "models", name + "_region_model.bin"))
    depth_model = host.DepthModel(api, path=os.path.join(external, "models", name + "_depth_model.bin"))
    directory = os.path.join(dataset, "data", sequence)
    color = generator.LoaderColorCamera(api, directory, ev.YCB_INTRINSICS, "", 1, 6, "-color")
    depth = generator.LoaderDepthCamera(api, directory, ev.YCB_INTRINSICS, 0.0001, "", 1, 6, "-depth")
    modalities = [host.RegionModality(api, body, color, region_model, depth_camera=depth, measure_occlusions=1,
                                      **ev.YCB_REGION_PARAMETERS),
                  host.DepthModality(api, body, depth, depth_model, measure_occlusions=1, **ev.YCB_DEPTH_PARAMETERS)]
    texture = None
    if use_texture:
        geometry = host.RendererGeometry(api)
        geometry.AddBody(body)
        silhouette = host.FocusedSilhouetteRenderer(api, geometry, color, id_type=0, image_size=200)
        silhouette.AddReferencedBody(body)
        texture = host.TextureModality(api, body, color, silhouette, depth_camera=depth, measure_occlusions=1,
                                       **ev.YCB_TEXTURE_PARAMETERS)
        texture.SetDetector(**kw["detector_parameters"])
        modalities.append(texture)  # behind the region and the depth modality: modality_ptrs()[2]
    host.Optimizer(api, body=body, modalities=modalities, tikhonov_parameter_rotation=1000.0,
                   tikhonov_parameter_translation=30000.0)
    tracker = host.Tracker(api, 4, 2)
    keyframes = ev.ycb_keyframes(dataset, sequence)
    gt = ev.read_matlab_poses_ycb(os.path.join(external, "poses", "ground_truth", sequence + "_" + name + ".txt"))
    evaluation = ev.YCBBodyEvaluation(body.vertices, kw["n_vertices_evaluation"])

    def update(frame):
        for camera in (color, depth):
            camera.set_load_index(frame)
            assert camera.UpdateImage()

    body.set_body2world_pose(gt[0])
    update(keyframes[0])
    assert tracker.StartModalities(0)
    results, n_points = [], []
    judge = None
    if judge_on_device:
        judge = tracker.CreateJudge([body], len(keyframes))
        judge.set_vertices(0, evaluation.vertices)
    for i, frame in enumerate(keyframes):
        update(frame)
        assert tracker.ExecuteTrackingStep(i)
        if judge is not None:
            judge.judge([gt[i]], -1)
        else:
            assert tracker.Sync()
            results.append(evaluation.result(body.body2world_pose(), gt[i]))
            if texture is not None:
                n_points.append(len(texture.points()))
    if judge is not None:
        rows = judge.read(0, len(keyframes))
        results = [evaluation.result_of_errors(float(rows[i, 0]["add_error"]), float(rows[i, 0]["adds_error"]))
                   for i in range(len(keyframes))]
    return results, body.body2world_pose(), n_points


@pytest.mark.parametrize("judge_on_device", [False, True], ids=["host_judge", "device_judge"])
def test_ycb_texture_column_equals_the_loop_written_out(ycb, judge_on_device, monkeypatch):
    dataset, external, names, kw = ycb
    per_form = {}
    for form in ("tiled", "one"):
        monkeypatch.setenv("M3T_HIP_TEXTURE_MATCH", form)  # (the library's developer override: looked at by every new context)
        results, overall = ev.evaluate_ycb_dataset(util.open_hip, dataset, external, [0, 1], names,
                                                   use_texture_modality=True, judge_on_device=judge_on_device, **kw)
        monkeypatch.delenv("M3T_HIP_TEXTURE_MATCH")
        assert set(results) == {("0000", names[0]), ("0001", names[1])}
        per_form[form] = (results, overall)
    for (sequence, name), average in per_form["tiled"][0].items():
        frames, pose, n_points = _ycb_twin(dataset, external, sequence, name, kw, judge_on_device)
        print(sequence, name, "points per frame:", n_points, "add auc:", average["add_auc"])
        assert average["add_auc"] == float(np.mean([r["add_auc"] for r in frames]))
        assert average["adds_auc"] == float(np.mean([r["adds_auc"] for r in frames]))
        assert np.array_equal(average["add_curve"], np.mean([r["add_curve"] for r in frames], axis=0))
        one = per_form["one"][0][(sequence, name)]  # the two forms of the matcher: identical results
        assert (one["add_auc"], one["adds_auc"]) == (average["add_auc"], average["adds_auc"])
        assert np.array_equal(one["adds_curve"], average["adds_curve"])
        if not judge_on_device:
            assert len(n_points) == len(frames) and min(n_points) > 0  # texture.points() is non-empty in every frame
            _, plain_pose, _ = _ycb_twin(dataset, external, sequence, name, kw, False, use_texture=False)
            assert not np.array_equal(pose, plain_pose)  # the texture column is not the Region + Depth column
    assert per_form["one"][1]["add_auc"] == per_form["tiled"][1]["add_auc"]


# ---- OPT -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def opt(tmp_path_factory):
    """soda with two sequences of 6 and 4 images, chest with one of 5: sequences of unequal length"""
    root = tmp_path_factory.mktemp("opt_plates")
    dataset, external = root / "OPT", root / "external"
    os.makedirs(dataset / "3D" / "poses")
    os.makedirs(external / "models")
    plan = {"soda": [("tr_1", SHIFTS["first"]), ("zo_2", SHIFTS["second"])],
            "chest": [("tr_1", SHIFTS["third"]), ("zo_2", SHIFTS["second"][::-1])]}
    for index, (name, sequences) in enumerate(plan.items()):
        write_plate_obj(str(dataset / "Model3D" / name / (name + ".obj")))
        for pattern, shifts in sequences:
            sequence = ev.opt_sequence_name(name, "b", pattern)
            lines = []
            for k, (pose, color, depth) in enumerate(plate_frames(60 + index, shifts, ev.OPT_DEPTH_SCALE), 1):
                # the file holds geometry2world; the frames show the geometry (the plate) at `pose`
                _save(str(dataset / "3D" / sequence / "color" / ("%04d.png" % k)), np.ascontiguousarray(color[:, :, ::-1]))
                _save(str(dataset / "3D" / sequence / "depth" / ("%04d.png" % k)), depth)
                m = pose.astype(np.float64)
                lines.append(" ".join("%.9g" % m[j, i] for i in range(4) for j in range(3)) + "\n")
            (dataset / "3D" / "poses" / (sequence + ".txt")).write_text("".join(lines))
    kw = dict(body_names=list(plan), body_orientations=["b"], motion_patterns=["tr_1", "zo_2"],
              model_parameters=MODEL_PARAMETERS, intrinsics=INTRINSICS, depth2color_pose=np.eye(4, dtype=F),
              n_vertices_evaluation=8, detector_parameters=DETECTOR)
    return str(dataset), str(external), kw


def _same_opt(a, b):
    assert list(a[0]) == list(b[0]) and set(a[1]) == set(b[1])
    for key in a[0]:
        assert a[0][key]["area_under_curve"] == b[0][key]["area_under_curve"], key
        assert np.array_equal(a[0][key]["curve_values"], b[0][key]["curve_values"]), key
    for key in a[1]:
        assert a[1][key]["area_under_curve"] == b[1][key]["area_under_curve"], key


def _opt_twin(dataset, external, name, sequence, kw, use_texture=True):
    """one body, one sequence, written out (opt_evaluator.cpp:204-251, :314-326): (per-cycle results, final pose,
    points per cycle)"""
    api = util.open_hip()
    geometry2body = ev.opt_geometry2body_pose(name)
    body = generator.Body(api, name, os.path.join(dataset, "Model3D", name, name + ".obj"), 1.0, True, True, geometry2body)
    region_model = host.RegionModel(api, path=os.path.join(external, "models", name + "_region_model.bin"))
    depth_model = host.DepthModel(api, path=os.path.join(external, "models", name + "_depth_model.bin"))
    directory = os.path.join(dataset, "3D", sequence)
    color = generator.LoaderColorCamera(api, os.path.join(directory, "color"), kw["intrinsics"], "", 1, 4)
    depth = generator.LoaderDepthCamera(api, os.path.join(directory, "depth"), kw["intrinsics"], ev.OPT_DEPTH_SCALE, "", 1, 4,
                                        camera2world_pose=kw["depth2color_pose"])
    modalities = [host.RegionModality(api, body, color, region_model, **ev.OPT_REGION_PARAMETERS),
                  host.DepthModality(api, body, depth, depth_model, **ev.OPT_DEPTH_PARAMETERS)]
    texture = None
    if use_texture:
        geometry = host.RendererGeometry(api)
        geometry.AddBody(body)
        silhouette = host.FocusedSilhouetteRenderer(api, geometry, color, id_type=0, image_size=200)
        silhouette.AddReferencedBody(body)
        texture = host.TextureModality(api, body, color, silhouette, **ev.OPT_TEXTURE_PARAMETERS)
        texture.SetDetector(**kw["detector_parameters"])
        modalities.append(texture)
    host.Optimizer(api, body=body, modalities=modalities, tikhonov_parameter_rotation=ev.OPT_TIKHONOV_PARAMETER_ROTATION,
                   tikhonov_parameter_translation=ev.OPT_TIKHONOV_PARAMETER_TRANSLATION)
    diameter = ev.vertices_diameter(api, body.vertices)
    evaluation = ev.OPTBodyEvaluation(body.vertices, geometry2body, diameter, kw["n_vertices_evaluation"])
    gt = ev.read_poses_opt(os.path.join(dataset, "3D", "poses", sequence + ".txt"), geometry2body)
    tracker = host.Tracker(api, ev.OPT_N_CORR_ITERATIONS, ev.OPT_N_UPDATE_ITERATIONS)

    def load(k):
        for camera in (color, depth):
            camera.set_load_index(1 + k)
            assert camera.UpdateImage()

    load(0)
    body.set_body2world_pose(gt[0])
    assert tracker.StartModalities(0)
    results, n_points = [], []
    for i in range(len(gt) - 1):
        load(i + 1)
        assert tracker.ExecuteTrackingStep(i) and tracker.Sync()
        results.append(evaluation.result(body.body2world_pose(), gt[i + 1]))
        if texture is not None:
            n_points.append(len(texture.points()))
    return results, body.body2world_pose(), n_points


def test_opt_texture_column_equals_the_loop_written_out_in_a_batch_and_alone(opt, monkeypatch):
    dataset, external, kw = opt
    single = ev.evaluate_opt_dataset(util.open_hip, dataset, external, batch=1, use_texture_modality=True, **kw)
    assert list(single[0]) == ["so_tr_1_b", "so_zo_2_b", "ch_tr_1_b", "ch_zo_2_b"]
    # the batch of two: its bodies' sequences have unequal lengths, so one is restarted by ResetBodies while the other
    # tracks; both forms of the matcher; the device judge with set_add_only against itself alone
    batch = ev.evaluate_opt_dataset(util.open_hip, dataset, external, batch=2, use_texture_modality=True, **kw)
    _same_opt(batch, single)
    for form in ("tiled", "one"):
        monkeypatch.setenv("M3T_HIP_TEXTURE_MATCH", form)  # (the library's developer override)
        _same_opt(ev.evaluate_opt_dataset(util.open_hip, dataset, external, batch=2, use_texture_modality=True, **kw), single)
        monkeypatch.delenv("M3T_HIP_TEXTURE_MATCH")
    judged = [ev.evaluate_opt_dataset(util.open_hip, dataset, external, batch=b, use_texture_modality=True,
                                      judge_on_device=True, **kw) for b in (1, 2)]
    _same_opt(judged[0], judged[1])
    for key in single[0]:
        assert abs(judged[0][0][key]["area_under_curve"] - single[0][key]["area_under_curve"]) < 1e-3, key
    for name, sequence in (("soda", "so_tr_1_b"), ("soda", "so_zo_2_b"), ("chest", "ch_tr_1_b"), ("chest", "ch_zo_2_b")):
        frames, pose, n_points = _opt_twin(dataset, external, name, sequence, kw)
        print(sequence, "points per cycle:", n_points, "auc:", single[0][sequence]["area_under_curve"])
        want = ev.opt_average_result(frames)
        assert single[0][sequence]["area_under_curve"] == want["area_under_curve"]
        assert np.array_equal(single[0][sequence]["curve_values"], want["curve_values"])
        assert len(n_points) == len(frames) and min(n_points) > 0
        _, plain_pose, _ = _opt_twin(dataset, external, name, sequence, kw, use_texture=False)
        assert not np.array_equal(pose, plain_pose)
