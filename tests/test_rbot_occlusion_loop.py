"""The RBOT evaluator's modelled-occlusion runs on the host, against recording fakes (no device): the order of the two
judgements of evaluation.evaluate_rbot_occlusion_sequences -- which body is judged against which pose file, which body
is reset -- on the host-judged and on the device-judged path, the wiring of an occlusion run in the dataset driver
(rbot_evaluator.cpp:213-332 without the texture modality), and that sequence_occlusions=None makes the calls it made
before the argument existed."""
import numpy as np

import util

ev = util.pkg.evaluation
F = np.float32


def pose(x):
    p = np.eye(4, dtype=F)
    p[0, 3] = x
    return p


class FakeBody:
    def __init__(self, log, name, script):
        self.log, self.name, self.script, self.reads = log, name, script, 0

    def body2world_pose(self):
        self.log.append(("read", self.name))
        return self.script(self)


class FakeJudge:
    def __init__(self, log, name, bodies, n_rows):
        self.log, self.name, self.n = log, name, len(bodies)
        log.append(("judge_create", name, [b.name for b in bodies], n_rows))
        self.rows = 0

    def set_reset_renderers(self, enable):
        self.log.append(("set_reset_renderers", self.name, enable))

    def set_reset_target(self, index, target):
        self.log.append(("set_reset_target", self.name, index, target.name))

    def judge(self, gt, reset_iteration):
        self.log.append(("judge", self.name, [float(g[0, 3]) for g in gt], reset_iteration))
        self.rows += 1
        return self.rows - 1

    def read(self, first, n):
        self.log.append(("judge_read", self.name, first, n))
        return np.zeros((n, self.n), util.pkg._capi.BODY_JUDGEMENT_DTYPE)


class FakeTracker:
    def __init__(self, log):
        self.log, self.judges = log, 0

    def ExecuteTrackingStep(self, i):
        self.log.append(("step", i))
        return True

    def Sync(self):
        return True

    def ResetBodies(self, bodies, poses, iteration):
        self.log.append(("reset", [b.name for b in bodies], [float(p[0, 3]) for p in poses], iteration))
        for b, p in zip(bodies, poses):
            b.pose = np.asarray(p, F)
        return True

    def CreateJudge(self, bodies, n_rows):
        self.judges += 1
        return FakeJudge(self.log, "judge%d" % self.judges, bodies, n_rows)


def _run(own_pose, on_device):
    """two runs, two frames.  poses_first: x = 1, 2 ... per frame (run 1: 10 + that); poses_second: 100 + ...; the main
    body of run 0 stays at its start, so it is lost at every frame; run 1's main follows its ground truth"""
    log = []
    first = [np.stack([pose(1.0 + k) for k in range(3)]), np.stack([pose(11.0 + k) for k in range(3)])]
    second = [np.stack([pose(101.0 + k) for k in range(3)]), np.stack([pose(111.0 + k) for k in range(3)])]
    frame = [0]
    mains = [FakeBody(log, "main0", lambda b: b.pose), FakeBody(log, "main1", lambda b: first[1][frame[0]])]
    occluders = [FakeBody(log, "occ0", lambda b: b.pose), FakeBody(log, "occ1", lambda b: second[1][frame[0]])]

    def load_images(k):
        frame[0] = k
        log.append(("load", k))

    frames, averages = ev.evaluate_rbot_occlusion_sequences(FakeTracker(log), mains, occluders, first, second, load_images,
                                                            2, judge_on_device=on_device,
                                                            judge_occluder_on_own_pose=own_pose)
    assert len(frames) == 2 and all(len(f) == 2 for f in frames) and len(averages) == 2
    return log, frames


def test_host_loop_judges_the_main_pose_twice_and_resets_the_occluder():
    log, frames = _run(own_pose=False, on_device=False)
    assert log == [
        ("load", 0), ("reset", ["main0", "main1"], [1.0, 11.0], 0), ("reset", ["occ0", "occ1"], [101.0, 111.0], 0),
        # frame 1: main0 stayed at x = 1 (lost against 2), main1 follows; then the MAIN poses against poses_second
        ("load", 1), ("step", 0), ("read", "main0"), ("read", "main1"), ("reset", ["main0"], [2.0], 0),
        ("read", "main0"), ("read", "main1"), ("reset", ["occ0", "occ1"], [102.0, 112.0], 0),
        ("load", 2), ("step", 1), ("read", "main0"), ("read", "main1"), ("reset", ["main0"], [3.0], 0),
        ("read", "main0"), ("read", "main1"), ("reset", ["occ0", "occ1"], [103.0, 113.0], 0)]
    assert [f["tracking_success"] for f in frames[0]] == [0.0, 0.0]
    assert [f["tracking_success"] for f in frames[1]] == [1.0, 1.0]
    assert [f["translation_error"] for f in frames[0]] == [1.0, 1.0]  # judged before the reset, against poses_first


def test_host_loop_on_the_occluders_own_pose():
    log, _ = _run(own_pose=True, on_device=False)
    # occ0 stays where its last reset put it (lost at every frame), occ1 follows poses_second
    assert log[3:11] == [("load", 1), ("step", 0), ("read", "main0"), ("read", "main1"), ("reset", ["main0"], [2.0], 0),
                         ("read", "occ0"), ("read", "occ1"), ("reset", ["occ0"], [102.0], 0)]


def test_device_loop_uses_two_judges_and_targets():
    log, _ = _run(own_pose=False, on_device=True)
    assert log == [
        ("load", 0), ("reset", ["main0", "main1"], [1.0, 11.0], 0), ("reset", ["occ0", "occ1"], [101.0, 111.0], 0),
        ("judge_create", "judge1", ["main0", "main1"], 2), ("set_reset_renderers", "judge1", True),
        ("judge_create", "judge2", ["main0", "main1"], 2), ("set_reset_renderers", "judge2", True),
        ("set_reset_target", "judge2", 0, "occ0"), ("set_reset_target", "judge2", 1, "occ1"),
        ("load", 1), ("step", 0), ("judge", "judge1", [2.0, 12.0], 0), ("judge", "judge2", [102.0, 112.0], 0),
        ("load", 2), ("step", 1), ("judge", "judge1", [3.0, 13.0], 0), ("judge", "judge2", [103.0, 113.0], 0),
        ("judge_read", "judge1", 0, 2), ("judge_read", "judge2", 1, 1)]
    log, _ = _run(own_pose=True, on_device=True)
    assert ("judge_create", "judge2", ["occ0", "occ1"], 2) in log
    assert not [entry for entry in log if entry[0] == "set_reset_target"]


# ---- the dataset driver's wiring ---------------------------------------------------------------------------------------
class Recorder:
    """stands in for the classes the driver instantiates: every construction and every method call is logged"""

    def __init__(self, log, kind):
        self.log, self.kind, self.count = log, kind, 0

    def __call__(self, *args, **kw):
        self.count += 1
        obj = Made(self.log, "%s%d" % (self.kind, self.count))
        named = [a.name if isinstance(a, Made) else a for a in args[1:]]  # (args[0]: the api)
        if self.kind == "Body":
            obj.body_name = args[1]
            named = [args[1]]
        elif self.kind == "Camera":
            named = [args[3]]
        elif self.kind in ("RegionModel", "Tracker"):
            named = []
        self.log.append((self.kind, obj.name, named, {k: (v.name if isinstance(v, Made) else
                                                        [m.name for m in v] if isinstance(v, list) else v)
                                                    for k, v in kw.items() if k in ("body", "modalities", "image_size")}))
        return obj


class Made:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def body_data(self):
        return None

    def __getattr__(self, method):
        def call(*args):
            self.log.append((self.name + "." + method, [a.name if isinstance(a, Made) else a for a in args]))
            return True
        return call


def _drive(monkeypatch, tmp_path, **kw):
    log = []
    generator, host, cfg = util.pkg.generator, util.pkg.host, util.pkg.config
    monkeypatch.setattr(generator, "Body", Recorder(log, "Body"))
    monkeypatch.setattr(generator, "LoaderColorCamera", Recorder(log, "Camera"))
    for kind in ("RegionModel", "RegionModality", "Optimizer", "Tracker", "RendererGeometry", "FocusedBasicDepthRenderer"):
        monkeypatch.setattr(host, kind, Recorder(log, kind))
    monkeypatch.setattr(cfg, "model_bin_matches", lambda *a: True)
    monkeypatch.setattr(ev, "read_poses_rbot", lambda path, n: "poses of " + str(path).split("/")[-1])
    average = dict(translation_error=0.0, rotation_error=0.0, tracking_success=1.0, complete_cycle=1.0)

    def plain(tracker, bodies, poses, load_images, n_frames, judge_on_device=False):
        log.append(("evaluate_rbot_sequences", [b.name for b in bodies], poses, judge_on_device))
        return None, [dict(average) for _ in bodies]

    def occluded(tracker, bodies, occluders, first, second, load_images, n_frames, judge_on_device=False,
                 judge_occluder_on_own_pose=False):
        log.append(("evaluate_rbot_occlusion_sequences", [b.name for b in bodies], [b.name for b in occluders], first,
                    second, judge_on_device, judge_occluder_on_own_pose))
        return None, [dict(average) for _ in bodies]

    monkeypatch.setattr(ev, "evaluate_rbot_sequences", plain)
    monkeypatch.setattr(ev, "evaluate_rbot_occlusion_sequences", occluded)
    results, _ = ev.evaluate_rbot_dataset(lambda: "api", str(tmp_path), str(tmp_path), ["ape", "cat"], n_frames=2, **kw)
    return log, results


def _plain_run(n, name, sequence):
    return [("Body", "Body%d" % n, [name], {}), ("RegionModel", "RegionModel%d" % n, [], {}),
            ("Camera", "Camera%d" % n, [sequence], {}),
            ("RegionModality", "RegionModality%d" % n, ["Body%d" % n, "Camera%d" % n, "RegionModel%d" % n], {}),
            ("Optimizer", "Optimizer%d" % n, [], {"body": "Body%d" % n, "modalities": ["RegionModality%d" % n]})]


def test_without_sequence_occlusions_the_driver_makes_the_calls_it_made(monkeypatch, tmp_path):
    expected = (_plain_run(1, "ape", "a_regular") + _plain_run(2, "cat", "a_regular") + [("Tracker", "Tracker1", [], {})] +
                [("evaluate_rbot_sequences", ["Body1", "Body2"], ["poses of poses_first.txt"] * 2, False)])
    for kw in (dict(), dict(sequence_occlusions=None), dict(sequence_occlusions=[False])):
        log, results = _drive(monkeypatch, tmp_path, sequence_names=["a_regular"], batch=2, **kw)
        assert log == expected, kw
        assert list(results) == [("a_regular", "ape"), ("a_regular", "cat")]


def test_an_occlusion_run_is_wired_like_the_reference(monkeypatch, tmp_path):
    log, results = _drive(monkeypatch, tmp_path, sequence_names=["d_occlusion"], batch=1, sequence_occlusions=[True],
                          judge_occluder_on_own_pose=True)
    run = [("Body", "Body1", ["ape"], {}), ("RegionModel", "RegionModel1", [], {}), ("Camera", "Camera1", ["d_occlusion"], {}),
           ("RegionModality", "RegionModality1", ["Body1", "Camera1", "RegionModel1"], {}),
           ("Body", "Body2", ["squirrel_small"], {}), ("RegionModel", "RegionModel2", [], {}),
           ("RendererGeometry", "RendererGeometry1", [], {}),
           ("RendererGeometry1.AddBody", ["Body1"]), ("RendererGeometry1.AddBody", ["Body2"]),
           ("FocusedBasicDepthRenderer", "FocusedBasicDepthRenderer1", ["RendererGeometry1", "Camera1"], {"image_size": 200}),
           ("FocusedBasicDepthRenderer1.AddReferencedBody", ["Body1"]),
           ("FocusedBasicDepthRenderer1.AddReferencedBody", ["Body2"]),
           ("RegionModality1.ModelOcclusions", ["FocusedBasicDepthRenderer1"]),
           ("Optimizer", "Optimizer1", [], {"body": "Body1", "modalities": ["RegionModality1"]}),
           ("RegionModality", "RegionModality2", ["Body2", "Camera1", "RegionModel2"], {}),
           ("RegionModality2.ModelOcclusions", ["FocusedBasicDepthRenderer1"]),
           ("Optimizer", "Optimizer2", [], {"body": "Body2", "modalities": ["RegionModality2"]}),
           ("Tracker", "Tracker1", [], {}),
           ("evaluate_rbot_occlusion_sequences", ["Body1"], ["Body2"], ["poses of poses_first.txt"],
            ["poses of poses_second.txt"], False, True)]
    assert log[:len(run)] == run
    assert len(log) == 2 * len(run)  # the second body's run: a context of its own (batch = 1)
    assert list(results) == [("d_occlusion_modeled", "ape"), ("d_occlusion_modeled", "cat")]


def test_the_occluders_of_a_context_share_one_model(monkeypatch, tmp_path):
    log, _ = _drive(monkeypatch, tmp_path, sequence_names=["d_occlusion"], batch=2, sequence_occlusions=[True])
    made = [entry for entry in log if entry[0] in ("Body", "RegionModel", "RegionModality", "Tracker")]
    assert [e[2] for e in made if e[0] == "Body"] == [["ape"], ["squirrel_small"], ["cat"], ["squirrel_small"]]
    assert len([e for e in made if e[0] == "RegionModel"]) == 3 and len([e for e in made if e[0] == "Tracker"]) == 1
    # both occluders' modalities read the second model made: squirrel_small's
    assert [e[2][2] for e in made if e[0] == "RegionModality"] == ["RegionModel1", "RegionModel2", "RegionModel3", "RegionModel2"]
