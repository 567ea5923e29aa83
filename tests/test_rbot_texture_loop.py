"""The RBOT dataset driver with use_texture_modality on the host, against recording stand-ins for the classes it
instantiates (no device): per run a RendererGeometry with the body, a FocusedSilhouetteRenderer on the run's camera
that references it, a TextureModality(body, camera, silhouette) with the built-in detector, behind the region modality
in the optimizer's list (rbot_evaluator.cpp:244-249, :262-283); that the default builds what it built before the
argument existed; the device judge's set_reset_renderers; the two refusals; and the judgement of these runs in the
device judge's arithmetic on the host (evaluation.judge_pose_result against tests/judge_reference.py, bit for bit)."""
import numpy as np
import pytest

import test_rbot_occlusion_loop as base
import util
from test_rbot_occlusion_loop import FakeBody, FakeTracker, Made, Recorder, _plain_run, pose

ev = util.pkg.evaluation
F = np.float32
KINDS = ("RegionModel", "RegionModality", "Optimizer", "Tracker", "RendererGeometry", "FocusedBasicDepthRenderer",
         "FocusedSilhouetteRenderer", "TextureModality")


class TextureRecorder(Recorder):
    """the keyword arguments of the texture modality and its renderer are part of the record"""

    def __call__(self, *args, **kw):
        obj = super().__call__(*args, **kw)
        if self.kind == "TextureModality":
            self.log[-1] = self.log[-1][:3] + (dict(kw),)
        return obj


class DetectingMade(Made):
    def __getattr__(self, method):
        if method != "SetDetector":
            return super().__getattr__(method)

        def call(*args, **kw):
            self.log.append((self.name + ".SetDetector", list(args), dict(kw)))
        return call


def _drive(monkeypatch, tmp_path, api="api", **kw):
    log = []
    generator, host, cfg = util.pkg.generator, util.pkg.host, util.pkg.config
    monkeypatch.setattr(generator, "Body", Recorder(log, "Body"))
    monkeypatch.setattr(generator, "LoaderColorCamera", Recorder(log, "Camera"))
    for kind in KINDS:
        monkeypatch.setattr(host, kind, TextureRecorder(log, kind))
    monkeypatch.setattr(base, "Made", DetectingMade)  # (what a Recorder makes: SetDetector takes keywords)
    monkeypatch.setattr(cfg, "model_bin_matches", lambda *a: True)
    monkeypatch.setattr(ev, "read_poses_rbot", lambda path, n: "poses of " + str(path).split("/")[-1])
    average = dict(translation_error=0.0, rotation_error=0.0, tracking_success=1.0, complete_cycle=1.0)

    def single(tracker, body, poses, load_image, n_frames=None, reset_renderers=(), **more):
        log.append(("evaluate_rbot_sequence", body.name, poses, list(reset_renderers)) + ((more,) if more else ()))
        return None, dict(average)

    def plain(tracker, bodies, poses, load_images, n_frames, judge_on_device=False, **more):
        log.append(("evaluate_rbot_sequences", [b.name for b in bodies], poses, judge_on_device) + ((more,) if more else ()))
        return None, [dict(average) for _ in bodies]

    monkeypatch.setattr(ev, "evaluate_rbot_sequence", single)
    monkeypatch.setattr(ev, "evaluate_rbot_sequences", plain)
    results, _ = ev.evaluate_rbot_dataset(lambda: api, str(tmp_path), str(tmp_path), ["ape", "cat"], n_frames=2,
                                          sequence_names=["a_regular"], **kw)
    return log, results


def _texture_run(n, name, texture_kw=None, detector_kw=None):
    body, camera = "Body%d" % n, "Camera%d" % n
    plain = _plain_run(n, name, "a_regular")
    return plain[:4] + [
        ("RendererGeometry", "RendererGeometry%d" % n, [], {}),
        ("RendererGeometry%d.AddBody" % n, [body]),
        ("FocusedSilhouetteRenderer", "FocusedSilhouetteRenderer%d" % n, ["RendererGeometry%d" % n, camera],
         {"image_size": 200}),
        ("FocusedSilhouetteRenderer%d.AddReferencedBody" % n, [body]),
        ("TextureModality", "TextureModality%d" % n, [body, camera, "FocusedSilhouetteRenderer%d" % n],
         dict(texture_kw or {})),
        ("TextureModality%d.SetDetector" % n, [], dict(detector_kw or {})),
        ("Optimizer", "Optimizer%d" % n, [], {"body": body, "modalities": ["RegionModality%d" % n, "TextureModality%d" % n]})]


def test_a_texture_run_is_wired_like_the_reference_in_a_batch(monkeypatch, tmp_path):
    texture_kw, detector_kw = dict(n_keyframes=2, focused_image_size=120), dict(n_features=300, fast_threshold=15)
    log, results = _drive(monkeypatch, tmp_path, batch=2, use_texture_modality=True, texture_parameters=texture_kw,
                          detector_parameters=detector_kw)
    expected = (_texture_run(1, "ape", texture_kw, detector_kw) + _texture_run(2, "cat", texture_kw, detector_kw) +
                [("Tracker", "Tracker1", [], {}),
                 ("evaluate_rbot_sequences", ["Body1", "Body2"], ["poses of poses_first.txt"] * 2, False,
                  {"reset_renderers": True, "pose_result": ev.judge_pose_result})])
    assert log == expected
    assert list(results) == [("a_regular", "ape"), ("a_regular", "cat")]


def test_a_texture_run_with_a_context_of_its_own_and_on_the_device_judge(monkeypatch, tmp_path):
    log, _ = _drive(monkeypatch, tmp_path, batch=1, use_texture_modality=True)
    run = _texture_run(1, "ape") + [("Tracker", "Tracker1", [], {}),
                                    ("evaluate_rbot_sequence", "Body1", "poses of poses_first.txt", [],
                                     {"pose_result": ev.judge_pose_result})]
    assert log[:len(run)] == run and len(log) == 2 * len(run)
    log, _ = _drive(monkeypatch, tmp_path, batch=2, judge_on_device=True, use_texture_modality=True)
    assert log[-1] == ("evaluate_rbot_sequences", ["Body1", "Body2"], ["poses of poses_first.txt"] * 2, True,
                       {"reset_renderers": True, "pose_result": ev.judge_pose_result})


def test_the_default_builds_what_it_built(monkeypatch, tmp_path):
    batched = (_plain_run(1, "ape", "a_regular") + _plain_run(2, "cat", "a_regular") + [("Tracker", "Tracker1", [], {})] +
               [("evaluate_rbot_sequences", ["Body1", "Body2"], ["poses of poses_first.txt"] * 2, False)])
    for kw in (dict(), dict(use_texture_modality=False),
               dict(use_texture_modality=False, texture_parameters=dict(n_keyframes=2), detector_parameters=dict(n_features=9))):
        log, _ = _drive(monkeypatch, tmp_path, batch=2, **kw)
        assert log == batched, kw
        log, _ = _drive(monkeypatch, tmp_path, batch=1, **kw)
        single = _plain_run(1, "ape", "a_regular") + [("Tracker", "Tracker1", [], {}),
                                                      ("evaluate_rbot_sequence", "Body1", "poses of poses_first.txt", [])]
        assert log[:len(single)] == single and len(log) == 2 * len(single), kw
        assert not [entry for entry in log if "Texture" in entry[0] or "Silhouette" in entry[0]]


def test_the_two_refusals(monkeypatch, tmp_path):
    class OracleApi:
        is_hip = False

    for batch in (1, 2):
        with pytest.raises(ValueError, match="oracle"):
            _drive(monkeypatch, tmp_path, api=OracleApi(), batch=batch, use_texture_modality=True)
        with pytest.raises(ValueError, match="sequence_occlusions"):
            _drive(monkeypatch, tmp_path, batch=batch, use_texture_modality=True, sequence_occlusions=[True])
    # without the texture modality the oracle's context builds what it built
    log, _ = _drive(monkeypatch, tmp_path, api=OracleApi(), batch=1)
    assert [entry[0] for entry in log[:5]] == ["Body", "RegionModel", "Camera", "RegionModality", "Optimizer"]


# ---- the loop: the device judge of a batch with texture modalities may run the renderers -------------------------------
class LoopJudge:
    def __init__(self, log, bodies, n_rows):
        self.log, self.n = log, len(bodies)
        log.append(("judge_create", [b.name for b in bodies], n_rows))

    def set_reset_renderers(self, enable):
        self.log.append(("set_reset_renderers", enable))

    def judge(self, gt, reset_iteration):
        self.log.append(("judge", [float(g[0, 3]) for g in gt], reset_iteration))

    def read(self, first, n):
        return np.zeros((n, self.n), util.pkg._capi.BODY_JUDGEMENT_DTYPE)


class LoopTracker(FakeTracker):
    def StartModalities(self, iteration):
        self.log.append(("start", iteration))
        return True

    def CreateJudge(self, bodies, n_rows):
        return LoopJudge(self.log, bodies, n_rows)


@pytest.mark.parametrize("reset_renderers", [None, False, True])
def test_the_device_judged_loop_opts_into_the_renderers_only_when_asked(reset_renderers):
    log = []
    bodies = [FakeBody(log, "a", None), FakeBody(log, "b", None)]
    for b in bodies:
        b.set_body2world_pose = lambda p, b=b: log.append(("pose", b.name, float(p[0, 3])))
    gt = [np.stack([pose(1.0 + k) for k in range(2)]), np.stack([pose(11.0 + k) for k in range(2)])]
    kw = {} if reset_renderers is None else dict(reset_renderers=reset_renderers)
    ev.evaluate_rbot_sequences(LoopTracker(log), bodies, gt, lambda k: log.append(("load", k)), 1, judge_on_device=True, **kw)
    opt_in = [("set_reset_renderers", True)] if reset_renderers else []
    assert log == ([("pose", "a", 1.0), ("pose", "b", 11.0), ("load", 0), ("start", 0), ("judge_create", ["a", "b"], 1)] +
                   opt_in + [("load", 1), ("step", 0), ("judge", [2.0, 12.0], 0)])


# ---- the judgement of a texture run on the host is the device judge's, float for float --------------------------------
def test_judge_pose_result_is_the_restated_judge_bit_for_bit():
    import judge_reference as jr
    from test_judge_reference import pose_pairs
    seen = set()
    for p, gt in pose_pairs() + pose_pairs(seed=8, n=40):
        t, r, c, ok = jr.pose_errors(p, gt)
        t_host, r_host, ok_host = ev.judge_pose_result(p, gt)
        assert isinstance(t_host, float) and isinstance(r_host, float)
        assert F(t_host).view(np.uint32) == t.view(np.uint32) and t_host == float(t)
        assert (np.isnan(r_host) and np.isnan(r)) or (r_host == float(r) and F(r_host).view(np.uint32) == r.view(np.uint32))
        assert ok_host == float(ok)
        seen.add(ok_host)
    assert seen == {0.0, 1.0}
    # the thresholds are the judge's f32 values: an error of exactly the threshold is not lost, the next float is
    at = np.eye(4, dtype=F)
    at[0, 3] = F(0.05)
    assert ev.judge_pose_result(at, np.eye(4, dtype=F)) == (float(F(0.05)), 0.0, 1.0)
    at[0, 3] = np.nextafter(F(0.05), F(1.0))
    assert ev.judge_pose_result(at, np.eye(4, dtype=F))[2] == 0.0


def test_the_host_judged_loops_take_the_judgement_they_are_given():
    log = []
    calls = []

    def judgement(pose, gt):
        calls.append((float(pose[0, 3]), float(gt[0, 3])))
        return 0.25, 0.5, 1.0

    bodies = [FakeBody(log, "a", lambda b: pose(7.0)), FakeBody(log, "b", lambda b: pose(8.0))]
    for b in bodies:
        b.set_body2world_pose = lambda p: None
    gt = [np.stack([pose(1.0 + k) for k in range(2)]), np.stack([pose(11.0 + k) for k in range(2)])]
    frames, _ = ev.evaluate_rbot_sequences(LoopTracker(log), bodies, gt, lambda k: None, 1, pose_result=judgement)
    assert calls == [(7.0, 2.0), (8.0, 12.0)] and frames[0][0]["translation_error"] == 0.25
    del calls[:]
    frames, _ = ev.evaluate_rbot_sequence(LoopTracker(log), bodies[0], gt[0], lambda k: None, 1, pose_result=judgement)
    assert calls == [(7.0, 2.0)] and frames[0]["rotation_error"] == 0.5
