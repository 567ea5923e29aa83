"""GenerateConfiguredTracker with a TextureModality and the caller's feature detector: a tracker from a YAML
configuration (the reference's triangle fixture) with a stub detector that returns planted features does, in one
StartModalities + ExecuteTrackingStep, what the hand-built context does with the same features; without the callable
the class is refused with a message that says what is missing."""
import numpy as np
import pytest

import golden_scene as gs
import util
from test_generator import reference_tree
from util import host

pytestmark = pytest.mark.gpu
generator = util.pkg.generator
mtv = gs.mtv
F = np.float32

CONFIG = """%YAML:1.2
LoaderColorCamera:
  - name: "color_camera"
    metafile_path: "../_sequence/color_camera.yaml"

RendererGeometry:
  - name: "renderer_geometry"
    bodies: ["triangle"]

Body:
  - name: "triangle"
    metafile_path: "../_body/triangle.yaml"

FocusedSilhouetteRenderer:
  - name: "silhouette_renderer"
    renderer_geometry: "renderer_geometry"
    camera: "color_camera"
    referenced_bodies: ["triangle"]

TextureModality:
  - name: "triangle_texture_modality"
    metafile_path: "texture_modality.yaml"
    body: "triangle"
    color_camera: "color_camera"
    focused_silhouette_renderer: "silhouette_renderer"

Link:
  - name: "triangle_link"
    body: "triangle"
    modalities: ["triangle_texture_modality"]

Optimizer:
  - name: "triangle_optimizer"
    root_link: "triangle_link"

Tracker:
  - name: "tracker"
    optimizers: ["triangle_optimizer"]
"""
METAFILE = '%YAML:1.2\ndescriptor_type: "BRISK"\nn_keyframes: 2\nbrisk_threshold: 25\norb_n_features: 300\ntukey_norm_constant: 15.0\n'


def _hand_built(api):
    body = host.Body(api)
    tv, tf = util.pkg.config.load_obj(util.GOLDEN + "/_body/triangle.obj")
    body.set_geometry(tv, tf, np.asarray(mtv.GEOMETRY2BODY, F), body_id=150, region_id=150)
    camera = host.ColorCamera(api, **mtv.COLOR_INTRINSICS)
    geometry = host.RendererGeometry(api)
    geometry.AddBody(body)
    renderer = host.FocusedSilhouetteRenderer(api, geometry, camera, id_type=0)
    renderer.AddReferencedBody(body)
    texture = host.TextureModality(api, body, camera, renderer, descriptor_bytes=64, n_keyframes=2,
                                   tukey_norm_constant=15.0)
    link = host.Link(api, body)
    link.AddModality(texture)
    host.Optimizer(api, link)
    body.set_body2world_pose(mtv.body2world())  # (as the generated tracker's body gets its pose: after the set-up)
    return body, renderer, texture, host.Tracker(api)


def test_generated_tracker_with_a_stub_detector_equals_the_hand_built_context(tmp_path):
    root = reference_tree(tmp_path)
    config = root / "tracker_test" / "texture_config.yaml"
    config.write_text(CONFIG)
    (root / "tracker_test" / "texture_modality.yaml").write_text(METAFILE)
    # planted features: pixels of the body in the focused image of the region of interest, moved a little for the step
    hand_api = util.open_hip()
    body, renderer, texture, hand_tracker = _hand_built(hand_api)
    roi, scale = texture.RegionOfInterest()
    renderer.StartRendering()
    _, silhouette, corner_u, corner_v, render_scale, _ = renderer.images()
    vs, us = np.nonzero(silhouette == 150)
    rng = np.random.default_rng(4)
    pick = rng.permutation(len(vs))[:200]
    full = np.stack([F(corner_u) + us[pick].astype(F) / F(render_scale), F(corner_v) + vs[pick].astype(F) / F(render_scale)], 1)
    focused = ((full - np.array(roi[:2], F)) * scale).astype(F)
    descriptors = rng.integers(0, 256, (200, 64), dtype=np.uint8)
    planted = [(focused, descriptors), ((focused[:150] + rng.uniform(-3, 3, (150, 2))).astype(F), descriptors[:150])]
    calls = []

    def detector(image, roi, scale, params):
        assert image.shape == (540, 960, 3) and params == {"descriptor_type": "BRISK", "brisk_threshold": 25,
                                                           "orb_n_features": 300}
        calls.append((roi, scale))
        return planted[len(calls) - 1]

    api = util.open_hip()
    tracker = generator.GenerateConfiguredTracker(api, str(config), feature_detector=detector, pass_detector_params=True)
    tracker.objects["Body"]["triangle"].set_body2world_pose(mtv.body2world())
    assert tracker.SetUp() and tracker.StartModalities(0) and tracker.ExecuteTrackingStep(0)
    assert len(calls) == 2 and calls[0] == (roi, scale)
    generated = tracker.objects["TextureModality"]["triangle_texture_modality"]
    assert generated.params.descriptor_bytes == 64 and generated.params.n_keyframes == 2
    # the hand-built context with the same features
    for step, (keypoints, rows) in enumerate(planted):
        texture.SetFocusedFeatures(*texture.RegionOfInterest(), keypoints, rows)
        assert hand_tracker.StartModalities(0) if step == 0 else hand_tracker.ExecuteTrackingStep(0)
    pose = body.body2world_pose()
    assert np.array_equal(tracker.objects["Body"]["triangle"].body2world_pose().view(np.uint32), pose.view(np.uint32))
    assert not np.array_equal(pose, mtv.body2world())
    points = texture.points()
    assert len(points) > 100 and np.array_equal(generated.points(), points)
    assert generated.keyframes()[0] == texture.keyframes()[0]
    assert all(np.array_equal(a, b) for a, b in zip(generated.keyframes()[1], texture.keyframes()[1]))


def test_texture_modality_without_a_detector_or_with_an_l2_descriptor_is_refused(tmp_path):
    root = reference_tree(tmp_path)
    config = root / "tracker_test" / "texture_config.yaml"
    config.write_text(CONFIG)
    (root / "tracker_test" / "texture_modality.yaml").write_text(METAFILE)
    with pytest.raises(ValueError, match="needs the caller's feature detector"):
        generator.GenerateConfiguredTracker(util.open_hip(), str(config))
    (root / "tracker_test" / "texture_modality.yaml").write_text('%YAML:1.2\ndescriptor_type: "SIFT"\n')
    with pytest.raises(ValueError, match="not a Hamming-norm descriptor"):
        generator.GenerateConfiguredTracker(util.open_hip(), str(config), feature_detector=lambda i, r, s: ([], []))
