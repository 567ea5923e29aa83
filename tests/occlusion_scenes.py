"""Modelled-occlusion runs for the tests of the device-decided renderer runs (m3t_hip_judge_set_reset_renderers,
m3t_hip_judge_set_reset_target): run p of `inputs` tracks a main body (object 2 p of scenes.Inputs, on that object's
frames) and an occluding body in front of it, both with the octahedron mesh of selective_reset.write_rbot_dataset, one
RendererGeometry, one FocusedBasicDepthRenderer on the run's camera referencing both, ModelOcclusions on both region
modalities, two rigid optimizers -- RBOTEvaluator::SetUpTracker (rbot_evaluator.cpp:213-332) without the texture
modality.  Also the synthetic RBOT-layout dataset with squirrel_small and poses_second.txt."""
import numpy as np

import reset_loop
import selective_reset as sr
import util
from util import host, pkg, syn

ev = pkg.evaluation
F = np.float32
OCTAHEDRON = np.array([(60, 0, 0), (-60, 0, 0), (0, 50, 0), (0, -50, 0), (0, 0, 40), (0, 0, -40)], F) * F(0.001)
FACES = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], np.int32)
OCCLUDER_OFFSET = (0.03, 0.0, -0.1)  # from the main body: beside it and nearer to the camera (which looks along +z)


def occluder_pose(main_pose):
    p = np.asarray(main_pose, F).copy()
    p[:3, 3] += np.asarray(OCCLUDER_OFFSET, F)
    return p


class Pairs:
    """runs `runs` of `inputs` behind one context; bodies in the order main, occluder, main, occluder, ..."""

    def __init__(self, api, inputs, runs, image_sizes=None, model_occlusions=True):
        self.api, self.inputs, self.runs = api, inputs, list(runs)
        rp = dict(syn.RBOT_REGION_PARAMS, measure_occlusions=0, n_unoccluded_iterations=0)
        tp = syn.RBOT_TRACKER
        models = {}
        self.mains, self.occluders, self.cams, self.renderers, self.region = [], [], [], [], []
        for at, p in enumerate(self.runs):
            for i in (2 * p, 2 * p + 1):
                m = inputs.model_of[i]
                if m not in models:
                    d = inputs.region_models[m]
                    models[m] = host.RegionModel(api, data_points=d[0], orientations=d[1], contour_lengths=d[2])
            cam = host.ColorCamera(api, **inputs.intr)
            main = host.Body(api, inputs.start[2 * p])
            occluder = host.Body(api, occluder_pose(inputs.start[2 * p]))
            geometry = host.RendererGeometry(api)
            for body in (main, occluder):
                body.set_geometry(OCTAHEDRON, FACES)
                geometry.AddBody(body)
            size = image_sizes[at] if image_sizes else 200
            renderer = host.FocusedBasicDepthRenderer(api, geometry, cam, image_size=size)
            for body, i in ((main, 2 * p), (occluder, 2 * p + 1)):
                renderer.AddReferencedBody(body)
                modality = host.RegionModality(api, body, cam, models[inputs.model_of[i]], **rp)
                if model_occlusions:
                    modality.ModelOcclusions(renderer)
                host.Optimizer(api, body=body, modalities=[modality],
                               tikhonov_parameter_rotation=tp["tikhonov_parameter_rotation"],
                               tikhonov_parameter_translation=tp["tikhonov_parameter_translation"])
                self.region.append(modality)
            self.mains.append(main)
            self.occluders.append(occluder)
            self.cams.append(cam)
            self.renderers.append(renderer)
        self.bodies = [b for pair in zip(self.mains, self.occluders) for b in pair]
        self.tracker = host.Tracker(api, tp["n_corr_iterations"], tp["n_update_iterations"])

    def upload_frame(self, k):
        for cam, p in zip(self.cams, self.runs):
            cam.UpdateImage(self.inputs.color[2 * p][k])

    def poses(self):
        return np.stack([b.body2world_pose() for b in self.bodies])

    def histograms(self):
        return [r.histograms() for r in self.region]

    def state(self):
        return self.poses(), self.histograms()


def assert_same_state(a, b, what=""):
    assert np.array_equal(a[0], b[0]), what
    assert len(a[1]) == len(b[1])
    for (fa, ba), (fb, bb) in zip(a[1], b[1]):
        assert np.array_equal(fa, fb) and np.array_equal(ba, bb), what


def assert_same_images(a, b):
    assert np.array_equal(a[0], b[0]) and a[2:] == b[2:]


def main_ground_truth(inputs, n_runs, schedule):
    """[frame][run]: the main bodies' ground truth with the schedule's offsets ((frame, run, kind) entries)"""
    gt = reset_loop.ground_truth(inputs, [(frame, 2 * run, kind) for frame, run, kind in schedule])
    return [[gt[k][2 * p] for p in range(n_runs)] for k in range(inputs.n_frames)]


def assert_clear_of_the_thresholds(pose, gt):
    """the condition under which the device's judgement has to agree with the host's"""
    t_err, r_err, _ = ev.rbot_pose_result(pose, gt)
    assert abs(t_err - 0.05) > 1e-4 and (np.isnan(r_err) or abs(r_err - 5.0 * np.pi / 180.0) > 1e-4), (t_err, r_err)


# ---- the dataset with the occluding body ------------------------------------------------------------------------------
def write_rbot_occlusion_dataset(tmp_path, n_frames=8):
    """selective_reset.write_rbot_dataset and, beside its four bodies, squirrel_small (the octahedron again, its model
    written with the same parameters) and poses_second.txt: poses_first.txt moved by OCCLUDER_OFFSET"""
    cfg = pkg.config
    dataset, external, names, model_parameters = sr.write_rbot_dataset(tmp_path, n_frames)
    name = ev.RBOT_OCCLUSION_BODY
    (dataset / name).mkdir()
    source = dataset / names[0] / (names[0] + ".obj")
    (dataset / name / (name + ".obj")).write_text(source.read_text())
    with open(dataset / "poses_first.txt") as f:
        lines = f.read().split("\n")
    with open(dataset / "poses_second.txt", "w") as f:
        f.write(lines[0] + "\n")
        for line in lines[1:]:
            if not line:
                continue
            v = [float(x) for x in line.split("\t")]
            for c in range(3):
                v[9 + c] += 1000.0 * OCCLUDER_OFFSET[c]
            f.write("\t".join("%.9g" % x for x in v) + "\n")
    scene = util.syn.Scene(len(names), intr=dict(zip(("fu", "fv", "ppu", "ppv", "width", "height"), ev.RBOT_INTRINSICS)))
    points, orientations, lengths = util.syn.make_region_model(scene.body, n_divides=2, n_points=200)
    vertices, _ = cfg.load_obj(str(dataset / name / (name + ".obj")), 0.001)
    data = cfg.BodyData(str(dataset / name / (name + ".obj")), 0.001, True, False, cfg.maximum_body_diameter(vertices),
                        np.eye(4))
    cfg.write_model_bin(str(external / "models" / (name + "_model.bin")), True, model_parameters, data, points,
                        orientations, lengths)
    return dataset, external, names, model_parameters
