"""Evaluator front-ends of the reference's dataset benchmarks, over the batched tracker.

RBOT (M3T/examples/rbot_evaluator.cpp): ground-truth pose file reader, the 5 cm / 5 degree success criterion,
the frame loop with reset-on-loss.  YCB-Video (M3T/examples/ycb_evaluator.cpp): ground-truth reader, ADD /
ADD-S per frame, the tracking-loss curves and the area under curve, reduced evaluation vertices.  The
datasets themselves are external downloads; the loops take a frame source, so that synthetic sequences and
the real datasets run through the same code.  OPT (M3T/examples/opt_evaluator.cpp): ground-truth reader, ADD per frame
against the body's diameter, computed diameters, N sequences of different lengths in one context.
"""
import time

import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------
# RBOT
# ---------------------------------------------------------------------------------------------------------
def read_poses_rbot(path, n_frames=1000):
    """RBOTEvaluator::ReadPosesRBOTDataset (rbot_evaluator.cpp:558-585): one header line, then per frame
    nine rotation entries (row-major) and a translation in millimetres, tab separated; n_frames + 1 poses."""
    poses = np.zeros((n_frames + 1, 4, 4), F)
    with open(path) as f:
        f.readline()
        for i in range(n_frames + 1):
            t = f.readline().split("\t")
            if len(t) < 12:
                raise ValueError("Could not read pose %d from %s" % (i, path))
            v = [F(x) for x in t[:12]]
            poses[i, :3, :3] = np.asarray(v[:9], F).reshape(3, 3)
            poses[i, :3, 3] = np.asarray(v[9:12], F) * F(0.001)
            poses[i, 3, 3] = 1.0
    return poses


def rbot_pose_result(body2world_pose, body2world_pose_gt, translation_error_threshold=0.05,
                     rotation_error_threshold=5.0 * np.pi / 180.0):
    """RBOTEvaluator::CalculatePoseResults (rbot_evaluator.cpp:416-433): (translation error [m], rotation error
    [rad], tracking success 0/1).  Thresholds: rbot_evaluator.h:192-193."""
    p, g = np.asarray(body2world_pose, F), np.asarray(body2world_pose_gt, F)
    t_err = float(np.linalg.norm((p[:3, 3] - g[:3, 3]).astype(F)))
    c = (np.trace((p[:3, :3].T @ g[:3, :3]).astype(F)) - F(1.0)) / F(2.0)
    r_err = float(np.arccos(c))  # NaN for |c| > 1 exactly like acos(); the comparisons below are then false
    lost = t_err > translation_error_threshold or r_err > rotation_error_threshold
    return t_err, r_err, 0.0 if lost else 1.0


def judge_pose_result(body2world_pose, body2world_pose_gt, translation_error_threshold=F(0.05),
                      rotation_error_threshold=F(5.0) * F(np.pi) / F(180.0)):
    """rbot_pose_result in the arithmetic of the device judge (m3t_hip_judge_bodies, csrc/m3t_judge.hip), operation by
    operation: f32 throughout, sums left to right, the cosine from the dot products of the rotation columns, acos in
    double rounded to f32, the thresholds in f32.  rbot_pose_result leaves the order of its sums to numpy and differs
    from the judge in the last digits; a loop judged on the host with this function reports what the same loop reports
    when the device judges it, float for float."""
    p, g = np.asarray(body2world_pose, F), np.asarray(body2world_pose_gt, F)
    dx, dy, dz = F(p[0, 3] - g[0, 3]), F(p[1, 3] - g[1, 3]), F(p[2, 3] - g[2, 3])
    t_err = F(np.sqrt(F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))))
    d = [F(F(F(p[0, j] * g[0, j]) + F(p[1, j] * g[1, j])) + F(p[2, j] * g[2, j])) for j in range(3)]
    c = F(F(F(F(d[0] + d[1]) + d[2]) - F(1.0)) * F(0.5))
    with np.errstate(invalid="ignore"):
        r_err = F(np.arccos(np.float64(c)))  # NaN for |c| > 1: the comparisons below are then false
    lost = bool(t_err > F(translation_error_threshold)) or bool(r_err > F(rotation_error_threshold))
    return float(t_err), float(r_err), 0.0 if lost else 1.0


def evaluate_rbot_sequence(tracker, body, poses_gt, load_image, n_frames=None, reset_renderers=(),
                           pose_result=rbot_pose_result):
    """RBOTEvaluator::EvaluateRunConfiguration (rbot_evaluator.cpp:174-210) for the main body: start on image 0
    at its ground truth, then cycle i tracks image i + 1 (the loader camera advances once per UpdateCameras),
    compares with the ground truth of image i + 1 and resets the body to it (ResetBody :334-342) whenever
    tracking is lost.  `load_image(k)` makes image k the cameras' current image.
    Returns the per-frame results and their average (CalculateAverageResult :435-470).
    pose_result: the judgement, rbot_pose_result or judge_pose_result."""
    n_frames = len(poses_gt) - 1 if n_frames is None else n_frames

    def reset(i):
        body.set_body2world_pose(poses_gt[i])
        for r in reset_renderers:
            r.StartRendering()
        # (refused, e.g., while a frame slot holds an ROI rectangle only: the loop must not go on with stale histograms)
        if not tracker.StartModalities(0):
            raise RuntimeError("StartModalities failed")

    load_image(0)
    reset(0)
    frames = []
    for i in range(n_frames):
        load_image(i + 1)
        t0 = time.perf_counter()
        ok = tracker.ExecuteTrackingStep(i) and tracker.Sync()
        dt = (time.perf_counter() - t0) * 1e6
        if not ok:
            raise RuntimeError("tracking step %d failed" % i)
        t_err, r_err, success = pose_result(body.body2world_pose(), poses_gt[i + 1])
        frames.append(dict(frame_index=i, translation_error=t_err, rotation_error=r_err,
                           tracking_success=success, complete_cycle=dt))
        if success == 0.0:
            reset(i + 1)
    avg = {k: float(np.mean([f[k] for f in frames])) for k in
           ("translation_error", "rotation_error", "tracking_success", "complete_cycle")}
    return frames, avg


def evaluate_rbot_sequences(tracker, bodies, poses_gt_per_body, load_images, n_frames, judge_on_device=False,
                            reset_renderers=False, pose_result=rbot_pose_result):
    """The loop of evaluate_rbot_sequence for N independent bodies in ONE context (HIP library): every body starts on
    image 0 at its own ground truth, cycle i tracks image i + 1 of all of them in one step, every body is judged
    against its own ground truth, and the lost ones -- those alone -- are reset with one Tracker.ResetBodies call
    (ResetBody :334-342 per body: its pose, StartModality(0, 0) of its modalities), so that each body's results are
    those of a tracker of its own.  `load_images(k)` makes image k current in every body's camera.
    Returns (per-body lists of per-frame results, per-body averages); complete_cycle is the time of the batch's step.
    judge_on_device (HIP library): the judgement and the reset are the device's (Tracker.CreateJudge, judge(gt, 0)
    behind every step): the loop makes no Sync() and reads no pose per frame, and the rows are read once after the last
    frame.  complete_cycle is then the loop's wall time, the final read included, divided by its frames.
    reset_renderers: the bodies' modalities read start-modality renderers (a texture modality's silhouette renderer):
    the device judge may run them (Judge.set_reset_renderers); Tracker.ResetBodies runs them anyway.
    pose_result: the host's judgement, rbot_pose_result or judge_pose_result (the device judge's arithmetic)."""
    for body, poses_gt in zip(bodies, poses_gt_per_body):
        body.set_body2world_pose(poses_gt[0])
    load_images(0)
    if not tracker.StartModalities(0):
        raise RuntimeError("StartModalities failed")
    frames = [[] for _ in bodies]
    keys = ("translation_error", "rotation_error", "tracking_success", "complete_cycle")
    if judge_on_device:
        judge = tracker.CreateJudge(bodies, max(1, n_frames))
        if reset_renderers:
            judge.set_reset_renderers(True)
        t0 = time.perf_counter()
        for i in range(n_frames):
            load_images(i + 1)
            if not tracker.ExecuteTrackingStep(i):
                raise RuntimeError("tracking step %d failed" % i)
            judge.judge([poses_gt[i + 1] for poses_gt in poses_gt_per_body], 0)
        rows = judge.read(0, n_frames)
        dt = (time.perf_counter() - t0) * 1e6 / max(1, n_frames)
        for i in range(n_frames):
            for j in range(len(bodies)):
                r = rows[i, j]
                frames[j].append(dict(frame_index=i, translation_error=float(r["translation_error"]),
                                      rotation_error=float(r["rotation_error"]),
                                      tracking_success=float(r["tracking_success"]), complete_cycle=dt))
        averages = [{k: float(np.mean([f[k] for f in fs])) for k in keys} for fs in frames]
        return frames, averages
    for i in range(n_frames):
        load_images(i + 1)
        t0 = time.perf_counter()
        ok = tracker.ExecuteTrackingStep(i) and tracker.Sync()
        dt = (time.perf_counter() - t0) * 1e6
        if not ok:
            raise RuntimeError("tracking step %d failed" % i)
        lost = []
        for j, (body, poses_gt) in enumerate(zip(bodies, poses_gt_per_body)):
            t_err, r_err, success = pose_result(body.body2world_pose(), poses_gt[i + 1])
            frames[j].append(dict(frame_index=i, translation_error=t_err, rotation_error=r_err,
                                  tracking_success=success, complete_cycle=dt))
            if success == 0.0:
                lost.append(j)
        if lost and not tracker.ResetBodies([bodies[j] for j in lost], [poses_gt_per_body[j][i + 1] for j in lost], 0):
            raise RuntimeError("ResetBodies failed")
    averages = [{k: float(np.mean([f[k] for f in fs])) for k in keys} for fs in frames]
    return frames, averages


def evaluate_rbot_occlusion_sequences(tracker, bodies, occluders, poses_first_per_run, poses_second_per_run,
                                      load_images, n_frames, judge_on_device=False,
                                      judge_occluder_on_own_pose=False):
    """RBOTEvaluator::EvaluateRunConfiguration (rbot_evaluator.cpp:174-210) with run_configuration.occlusions for N
    independent runs in ONE context (HIP library): run j tracks bodies[j] and occluders[j], whose region modalities
    read one FocusedBasicDepthRenderer (ModelOcclusions).  Start: ResetBody(0), then ResetOcclusionBody(0) (:184-185).
    Cycle i, to the letter of :189-208:
      1. the tracking step on image i + 1;
      2. the main body is judged against poses_first[i + 1]; lost: ResetBody -- its pose, the start-modality
         renderers, StartModality(0, 0) of its modalities;
      3. the MAIN body's pose, as it then is, is judged against poses_second[i + 1] (:204 passes body_ptr, not the
         occluding body); lost: ResetOcclusionBody -- the occluder's pose, the renderers, its modalities.
    judge_occluder_on_own_pose: step 3 judges the occluder's own pose instead (the evident intent; not the reference).
    The lost bodies of a frame take ONE Tracker.ResetBodies call per step 2 and 3 (every run has a renderer of its own,
    so each run sees what a tracker of its own would).  Only the main bodies' results are kept.
    judge_on_device: two judges per context, called one after the other behind the step, both with
    set_reset_renderers: the first lists the main bodies, the second the main bodies with the occluders as reset targets
    (judge_occluder_on_own_pose: the occluders themselves); no Sync() and no pose read per frame, the first judge's
    rows are read once after the last frame.  Returns (per-run lists of per-frame results, per-run averages)."""
    n = len(bodies)
    keys = ("translation_error", "rotation_error", "tracking_success", "complete_cycle")
    load_images(0)
    if not tracker.ResetBodies(bodies, [poses[0] for poses in poses_first_per_run], 0):
        raise RuntimeError("ResetBodies failed")
    if not tracker.ResetBodies(occluders, [poses[0] for poses in poses_second_per_run], 0):
        raise RuntimeError("ResetBodies failed")
    frames = [[] for _ in bodies]
    if judge_on_device:
        judge_main = tracker.CreateJudge(bodies, max(1, n_frames))
        judge_main.set_reset_renderers(True)
        judge_occluder = tracker.CreateJudge(occluders if judge_occluder_on_own_pose else bodies, max(1, n_frames))
        judge_occluder.set_reset_renderers(True)
        if not judge_occluder_on_own_pose:
            for j in range(n):
                judge_occluder.set_reset_target(j, occluders[j])
        t0 = time.perf_counter()
        for i in range(n_frames):
            load_images(i + 1)
            if not tracker.ExecuteTrackingStep(i):
                raise RuntimeError("tracking step %d failed" % i)
            judge_main.judge([poses[i + 1] for poses in poses_first_per_run], 0)
            judge_occluder.judge([poses[i + 1] for poses in poses_second_per_run], 0)
        rows = judge_main.read(0, n_frames)
        if n_frames:
            judge_occluder.read(n_frames - 1, 1)  # (the loop's time includes its last launches)
        dt = (time.perf_counter() - t0) * 1e6 / max(1, n_frames)
        for i in range(n_frames):
            for j in range(n):
                r = rows[i, j]
                frames[j].append(dict(frame_index=i, translation_error=float(r["translation_error"]),
                                      rotation_error=float(r["rotation_error"]),
                                      tracking_success=float(r["tracking_success"]), complete_cycle=dt))
        averages = [{k: float(np.mean([f[k] for f in fs])) for k in keys} for fs in frames]
        return frames, averages
    for i in range(n_frames):
        load_images(i + 1)
        t0 = time.perf_counter()
        ok = tracker.ExecuteTrackingStep(i) and tracker.Sync()
        dt = (time.perf_counter() - t0) * 1e6
        if not ok:
            raise RuntimeError("tracking step %d failed" % i)
        lost = []
        for j in range(n):
            t_err, r_err, success = rbot_pose_result(bodies[j].body2world_pose(), poses_first_per_run[j][i + 1])
            frames[j].append(dict(frame_index=i, translation_error=t_err, rotation_error=r_err,
                                  tracking_success=success, complete_cycle=dt))
            if success == 0.0:
                lost.append(j)
        if lost and not tracker.ResetBodies([bodies[j] for j in lost], [poses_first_per_run[j][i + 1] for j in lost], 0):
            raise RuntimeError("ResetBodies failed")
        judged = occluders if judge_occluder_on_own_pose else bodies
        lost = [j for j in range(n)
                if rbot_pose_result(judged[j].body2world_pose(), poses_second_per_run[j][i + 1])[2] == 0.0]
        if lost and not tracker.ResetBodies([occluders[j] for j in lost], [poses_second_per_run[j][i + 1] for j in lost], 0):
            raise RuntimeError("ResetBodies failed")
    averages = [{k: float(np.mean([f[k] for f in fs])) for k in keys} for fs in frames]
    return frames, averages


# ---------------------------------------------------------------------------------------------------------
# YCB-Video
# ---------------------------------------------------------------------------------------------------------
K_N_CURVE_VALUES = 100   # ycb_evaluator.h:45
K_THRESHOLD_MAX = 0.1    # ycb_evaluator.h:46


def ycb_thresholds():
    """ycb_evaluator.cpp:18-22"""
    step = F(K_THRESHOLD_MAX) / F(K_N_CURVE_VALUES)
    return (step * (F(0.5) + np.arange(K_N_CURVE_VALUES, dtype=F))).astype(F)


def _quaternion_pose(w, x, y, z, tx, ty, tz):
    q = np.asarray([w, x, y, z], F)
    q = q / F(np.sqrt((q * q).sum(dtype=F)))
    w, x, y, z = [float(v) for v in q]
    pose = np.eye(4, dtype=F)
    pose[:3, :3] = np.asarray([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                               [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                               [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F)
    pose[:3, 3] = (tx, ty, tz)
    return pose


def read_poses_ycb(path, pose_begin, n_frames, keyframes):
    """YCBEvaluator::LoadGTPoses (ycb_evaluator.cpp:850-901): the per-body pose file holds one line
    'qw qx qy qz tx ty tz' per frame of every sequence; skip `pose_begin` lines, then keep the lines whose
    1-based frame index is a keyframe.  Quaternions are normalised, pose = translation * rotation."""
    keyframes = list(keyframes)
    poses = []
    with open(path) as f:
        for _ in range(pose_begin):
            f.readline()
        k = 0
        for idx in range(1, n_frames + 1):
            if k >= len(keyframes):
                break
            line = f.readline()
            if idx == keyframes[k]:
                v = [float(x) for x in line.split(" ")[:7]]
                poses.append(_quaternion_pose(*v))
                k += 1
    return np.asarray(poses, F)


def reduce_vertices(vertices, n_vertices_evaluation):
    """YCBEvaluator::GenderateReducedVertices (ycb_evaluator.cpp:1222-1248): all vertices, or
    n_vertices_evaluation draws `mt19937{7}() % n` with repetition"""
    vertices = np.asarray(vertices, F)
    n = len(vertices)
    if n_vertices_evaluation <= 0 or n_vertices_evaluation >= n:
        return vertices
    raw = np.random.RandomState(7)._bit_generator.random_raw(n_vertices_evaluation)  # == std::mt19937{7}
    return vertices[(raw % n).astype(np.int64)]


class YCBBodyEvaluation:
    """the per-body data of YCBEvaluator::CalculatePoseResults (ycb_evaluator.cpp:803-848): reduced vertices
    and a nearest-neighbour index over them (nanoflann there, scipy's k-d tree here: both exact)"""

    def __init__(self, vertices, n_vertices_evaluation=-1):
        from scipy.spatial import cKDTree
        self.vertices = reduce_vertices(vertices, n_vertices_evaluation)
        self.tree = cKDTree(self.vertices.astype(np.float64))
        self.thresholds = ycb_thresholds()

    def errors(self, body2world_pose, gt_body2world_pose):
        """(ADD, ADD-S) in metres: delta = body2world^-1 * gt; mean |v - delta v| and mean nearest-vertex
        distance of delta v"""
        p = np.asarray(body2world_pose, np.float64)
        g = np.asarray(gt_body2world_pose, np.float64)
        pi = np.eye(4)
        pi[:3, :3] = p[:3, :3].T
        pi[:3, 3] = -p[:3, :3].T @ p[:3, 3]
        delta = (pi @ g).astype(F)
        v = (self.vertices @ delta[:3, :3].T + delta[:3, 3]).astype(F)
        add = float(np.sqrt(((self.vertices - v) ** 2).sum(axis=1, dtype=F)).mean(dtype=F))
        dist, _ = self.tree.query(v.astype(np.float64), k=1)
        adds = float(dist.astype(F).mean(dtype=F))
        return add, adds

    def result(self, body2world_pose, gt_body2world_pose):
        return self.result_of_errors(*self.errors(body2world_pose, gt_body2world_pose))

    def result_of_errors(self, add, adds):
        """errors, curves and AUC from ADD / ADD-S in metres (judged here or on the device)"""
        out = dict(add_error=add, adds_error=adds)
        for key, err in (("add", add), ("adds", adds)):
            curve = np.ones(K_N_CURVE_VALUES, F)
            for i in range(K_N_CURVE_VALUES):  # the curve is 0 below the error, 1 from the first threshold above
                if err < self.thresholds[i]:
                    break
                curve[i] = 0.0
            out[key + "_curve"] = curve
            out[key + "_auc"] = float(F(1.0) - min(F(err) / F(K_THRESHOLD_MAX), F(1.0)))
        return out


def evaluate_ycb_sequence(tracker, bodies, evaluations, gt_body2world_poses, keyframes, update_cameras,
                          judge_on_device=False):
    """YCBEvaluator::EvaluateRunConfiguration without refinement (ycb_evaluator.cpp:333-372): bodies start at
    the ground truth of the first keyframe, StartModalities once, then one tracking step per keyframe and the
    ADD / ADD-S results of every evaluated body.  bodies / evaluations / gt poses are dicts by body name.
    judge_on_device (HIP library): ADD / ADD-S of the evaluated bodies are formed on the device over the evaluations'
    vertices (Tracker.CreateJudge, judge(gt, -1) behind every step); the loop makes no Sync() and reads no pose per
    frame, the rows are read once after the last keyframe and the curves and AUC are formed from them by
    YCBBodyEvaluation.result's code.  complete_cycle is then the loop's wall time, the final read included, divided by
    its keyframes."""
    for name, body in bodies.items():
        body.set_body2world_pose(gt_body2world_poses[name][0])
    update_cameras(keyframes[0])
    if not tracker.StartModalities(0):
        raise RuntimeError("StartModalities failed")
    results = {name: [] for name in evaluations}
    if judge_on_device:
        names = list(evaluations)
        judge = tracker.CreateJudge([bodies[name] for name in names], max(1, len(keyframes)))
        for j, name in enumerate(names):
            judge.set_vertices(j, evaluations[name].vertices)
        t0 = time.perf_counter()
        for i, frame in enumerate(keyframes):
            update_cameras(frame)
            if not tracker.ExecuteTrackingStep(i):
                raise RuntimeError("tracking step %d failed" % i)
            judge.judge([gt_body2world_poses[name][i] for name in names], -1)
        rows = judge.read(0, len(keyframes))
        dt = (time.perf_counter() - t0) * 1e6 / max(1, len(keyframes))
        for i in range(len(keyframes)):
            for j, name in enumerate(names):
                r = evaluations[name].result_of_errors(float(rows[i, j]["add_error"]), float(rows[i, j]["adds_error"]))
                r.update(frame_index=i, complete_cycle=dt)
                results[name].append(r)
    else:
        for i, frame in enumerate(keyframes):
            update_cameras(frame)
            t0 = time.perf_counter()
            if not (tracker.ExecuteTrackingStep(i) and tracker.Sync()):
                raise RuntimeError("tracking step %d failed" % i)
            dt = (time.perf_counter() - t0) * 1e6
            for name, ev in evaluations.items():
                r = ev.result(bodies[name].body2world_pose(), gt_body2world_poses[name][i])
                r.update(frame_index=i, complete_cycle=dt)
                results[name].append(r)
    average = {}
    for name, rs in results.items():
        average[name] = dict(add_auc=float(np.mean([r["add_auc"] for r in rs])),
                             adds_auc=float(np.mean([r["adds_auc"] for r in rs])),
                             add_curve=np.mean([r["add_curve"] for r in rs], axis=0),
                             adds_curve=np.mean([r["adds_curve"] for r in rs], axis=0),
                             complete_cycle=float(np.mean([r["complete_cycle"] for r in rs])))
    return results, average


# ---------------------------------------------------------------------------------------------------------
# RTB (M3T/examples/rtb_evaluator.cpp): kinematic structures
# ---------------------------------------------------------------------------------------------------------
RTB_N_CURVE_VALUES = 100  # rtb_evaluator.h kNCurveValues


def rtb_thresholds():
    """rtb_evaluator.cpp:20-24"""
    step = F(1.0) / F(RTB_N_CURVE_VALUES)
    return np.asarray([step * (F(0.5) + F(i)) for i in range(RTB_N_CURVE_VALUES)], F)


def rtb_pose_result(errors_per_body, groups, error_threshold):
    """RTBEvaluator::CalculatePoseResults (rtb_evaluator.cpp:935-988) from the per-body (ADD, ADD-S) errors, in f32 op
    by op: per group of combined bodies the members' errors summed in listed order and divided by their number, per
    structure 1 - min(err / threshold, 1) summed over the groups and divided by their number; the curves are 0 up to
    the first threshold above the auc.  `errors_per_body[i]` = (add, adds) of body i, `groups` lists of such i.
    The host twin of m3t_hip_judge_set_structures."""
    thresholds = rtb_thresholds()
    out = {}
    for key, which in (("add", 0), ("adds", 1)):
        auc = F(0.0)
        for group in groups:
            err = F(0.0)
            for i in group:
                err = F(err + F(errors_per_body[i][which]))
            err = F(err / F(len(group)))
            auc = F(auc + F(F(1.0) - min(F(err / F(error_threshold)), F(1.0))))
        auc = F(auc / F(len(groups)))
        curve = np.ones(RTB_N_CURVE_VALUES, F)
        zeros = 0
        while zeros < RTB_N_CURVE_VALUES and not auc < thresholds[zeros]:
            curve[zeros] = 0.0
            zeros += 1
        out[key + "_auc"] = float(auc)
        out[key + "_curve"] = curve
        out[key + "_curve_zeros"] = zeros
    return out


class RTBStructure:
    """What evaluate_rtb_sequences needs of one kinematic structure: its optimizer, its links in depth-first order as
    (Link, Body or None, index of the parent link in this list or -1), the evaluation of every body (an object with
    .vertices and .errors(pose, gt) such as YCBBodyEvaluation) in the order of the links that have one, RTB's combined
    bodies as lists of indices into that order, the error threshold and the evaluation mode (0 independent /
    projected, 1 constrained: body-less root)."""

    def __init__(self, optimizer, links, evaluations, groups, error_threshold, mode=0):
        self.optimizer, self.links, self.evaluations, self.groups = optimizer, list(links), list(evaluations), groups
        self.error_threshold, self.mode = float(error_threshold), int(mode)
        self.bodies = [body for _, body, _ in self.links if body is not None]
        assert len(self.bodies) == len(self.evaluations)


def _mul_pose_f32(a, b):
    """Transform3fA * Transform3fA in f32, one rounding per operation, sums left to right"""
    r = np.zeros((4, 4), F)
    r[3, 3] = 1.0
    for c in range(3):
        for k in range(3):
            r[k, c] = F(F(F(a[k, 0] * b[0, c]) + F(a[k, 1] * b[1, c])) + F(a[k, 2] * b[2, c]))
    for k in range(3):
        r[k, 3] = F(F(F(F(a[k, 0] * b[0, 3]) + F(a[k, 1] * b[1, 3])) + F(a[k, 2] * b[2, 3])) + a[k, 3])
    return r


def _inverse_pose_f32(a):
    """Transform3fA::inverse() (Affine): the cofactor inverse of the linear part, t' = -(L^-1 t)"""
    m = a[:3, :3]

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return F(F(m[i1, j1] * m[i2, j2]) - F(m[i1, j2] * m[i2, j1]))

    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = F(F(F(c00 * m[0, 0]) + F(c10 * m[1, 0])) + F(c20 * m[2, 0]))
    invdet = F(F(1.0) / det)
    r = np.zeros((4, 4), F)
    r[3, 3] = 1.0
    for rr in range(3):
        for cc in range(3):
            r[rr, cc] = F(cof(cc, rr) * invdet)
    for k in range(3):
        r[k, 3] = -F(F(F(r[k, 0] * a[0, 3]) + F(r[k, 1] * a[1, 3])) + F(r[k, 2] * a[2, 3]))
    return r


def set_body_and_joint_poses(structure, poses):
    """RTBEvaluator::SetBodyAndJointPoses (rtb_evaluator.cpp:809-858) on the host objects of one structure (any
    library): what Tracker.ResetStructures does on the device, minus the restart of the modalities"""
    pose_of, k = {}, 0
    for index, (link, body, parent) in enumerate(structure.links):
        if body is None:
            assert structure.mode == 1 and index == 0, "only the root of mode 1 may have no body"
            continue
        pose = np.asarray(poses[k], F)
        pose_of[index] = pose
        k += 1
        body.set_body2world_pose(pose)
        if parent < 0:
            continue
        if structure.mode == 1 and parent == 0:
            link.set_joint2parent_pose(pose)
        else:
            link.set_joint2parent_pose(_mul_pose_f32(_mul_pose_f32(_inverse_pose_f32(pose_of[parent]), pose),
                                                     _inverse_pose_f32(np.asarray(link.body2joint_pose(), F))))


def evaluate_rtb_sequences(tracker, structures, gt_poses_per_structure, load_images, judge_on_device=False):
    """The loop of RTBEvaluator::EvaluateRunConfiguration (rtb_evaluator.cpp:465-495) for S kinematic structures in ONE
    context, each with a list of sequences of its own: gt_poses_per_structure[s][q][k][b] is the ground-truth pose of
    body b of structure s in image k of its sequence q (bodies in RTBStructure.bodies order).  A structure starts a
    sequence on image 0 at its ground truth (SetBodyAndJointPoses + StartModalities, :466-467); cycle i tracks image
    i + 1 and is judged against its ground truth (CalculatePoseResults).  The sequences may have different lengths: a
    structure whose sequence has ended is put on the first pose of its next one with Tracker.ResetStructures while the
    others keep tracking, so each structure's results are those of a tracker of its own.  The step's iteration number
    is the batch's cycle counter and a structure's first_iteration the cycle it started on: their difference -- all the
    modalities read -- is the sequence's own cycle index.  `load_images(s, q, k)` makes image k of sequence q current
    in the cameras of structure s.
    A library without reset_structures (the oracle) can only restart all structures of the context together: one
    structure, or sequences of equal length.
    judge_on_device (HIP library): ADD / ADD-S and their combination are formed on the device (Judge.set_structures);
    nothing is read before the last cycle.
    Returns results[s][q] = list of per-cycle dicts (frame_index, add_auc, adds_auc, add_curve, adds_curve)."""
    n = len(structures)
    device_reset = "reset_structures" in tracker.api._fn
    results = [[[] for _ in sequences] for sequences in gt_poses_per_structure]
    state = [[0, 0] for _ in range(n)]  # sequence, cycle inside it

    def start(which, iteration):
        for s in which:
            load_images(s, state[s][0], 0)
        if device_reset:
            for mode in sorted({structures[s].mode for s in which}):
                group = [s for s in which if structures[s].mode == mode]
                poses = [p for s in group for p in gt_poses_per_structure[s][state[s][0]][0]]
                if not tracker.ResetStructures([structures[s].optimizer for s in group], poses, mode, iteration):
                    raise RuntimeError("ResetStructures failed")
            return
        if len(which) != n:
            raise RuntimeError("this library restarts all structures of a context together (no reset_structures)")
        for s in which:
            set_body_and_joint_poses(structures[s], gt_poses_per_structure[s][state[s][0]][0])
        if not tracker.StartModalities(iteration):
            raise RuntimeError("StartModalities failed")

    active = [s for s in range(n) if len(gt_poses_per_structure[s]) > 0]
    start(active, 0)
    judge, pending, first_body = None, [], np.cumsum([0] + [len(st.bodies) for st in structures])
    if judge_on_device:
        total = sum(len(seq) - 1 for sequences in gt_poses_per_structure for seq in sequences)
        judge = tracker.CreateJudge([b for st in structures for b in st.bodies], max(1, total))
        for s, st in enumerate(structures):
            for b, evaluation in enumerate(st.evaluations):
                judge.set_vertices(int(first_body[s]) + b, evaluation.vertices)
        judge.set_structures([[[int(first_body[s]) + b for b in group] for group in st.groups]
                              for s, st in enumerate(structures)], [st.error_threshold for st in structures])
        last_gt = [list(gt_poses_per_structure[s][0][0]) if gt_poses_per_structure[s] else [np.eye(4, dtype=F)] * len(st.bodies)
                   for s, st in enumerate(structures)]
    cycle = 0
    while active:
        for s in active:
            load_images(s, state[s][0], state[s][1] + 1)
        if not tracker.ExecuteTrackingStep(cycle):
            raise RuntimeError("tracking step %d failed" % cycle)
        if judge_on_device:
            for s in active:
                last_gt[s] = list(gt_poses_per_structure[s][state[s][0]][state[s][1] + 1])
            row = judge.judge([p for gt in last_gt for p in gt], -1)
            pending += [(row, s, state[s][0], state[s][1]) for s in active]
        else:
            if not tracker.Sync():
                raise RuntimeError("tracking step %d failed" % cycle)
            for s in active:
                st, (q, i) = structures[s], state[s]
                gt = gt_poses_per_structure[s][q][i + 1]
                errors = [ev.errors(body.body2world_pose(), g) for ev, body, g in zip(st.evaluations, st.bodies, gt)]
                r = rtb_pose_result(errors, st.groups, st.error_threshold)
                r.update(frame_index=i)
                results[s][q].append(r)
        ended = []
        for s in list(active):
            state[s][1] += 1
            if state[s][1] + 1 < len(gt_poses_per_structure[s][state[s][0]]):
                continue
            state[s] = [state[s][0] + 1, 0]
            if state[s][0] < len(gt_poses_per_structure[s]):
                ended.append(s)
            else:
                active.remove(s)
        cycle += 1
        if ended:
            start(ended, cycle)
    if judge_on_device and pending:
        rows = judge.read_structures(0, pending[-1][0] + 1)
        for row, s, q, i in pending:
            r = rows[row, s]
            out = dict(frame_index=i)
            for key in ("add", "adds"):
                zeros = int(r[key + "_curve_zeros"])
                curve = np.ones(RTB_N_CURVE_VALUES, F)
                curve[:zeros] = 0.0
                out.update({key + "_auc": float(r[key + "_auc"]), key + "_curve": curve, key + "_curve_zeros": zeros})
            results[s][q].append(out)
    return results


# ---------------------------------------------------------------------------------------------------------
# RBOT dataset driver (examples/evaluate_rbot_dataset.cpp + rbot_evaluator.cpp)
# ---------------------------------------------------------------------------------------------------------
RBOT_INTRINSICS = (650.048, 647.183, 324.328 - 0.5, 257.323 - 0.5, 640, 512)  # rbot_evaluator.h:40-41
RBOT_BODY_NAMES = ("ape", "bakingsoda", "benchviseblue", "broccolisoup", "cam", "can", "cat", "clown", "cube", "driller",
                   "duck", "eggbox", "glue", "iron", "koalacandy", "lamp", "phone", "squirrel")
RBOT_SEQUENCE_NAMES = ("a_regular", "b_dynamiclight", "c_noisy", "d_occlusion")
RBOT_OCCLUSION_BODY = "squirrel_small"  # rbot_evaluator.h kOcclusionBodyName
RBOT_FOCUSED_IMAGE_SIZE = 200           # evaluate_rbot_dataset.cpp:47
RBOT_REGION_PARAMETERS = dict(  # evaluate_rbot_dataset.cpp:25-44, rbot_evaluator.cpp:267
    n_lines_max=200, use_adaptive_coverage=0, min_continuous_distance=3.0, function_length=8, distribution_length=12,
    function_amplitude=0.36, function_slope=0.0, learning_rate=1.3, scales=[5, 2, 2, 1],
    standard_deviations=[20.0, 7.0, 3.0, 1.5], n_histogram_bins=32, learning_rate_f=0.2, learning_rate_b=0.2,
    unconsidered_line_length=0.5, max_considered_line_length=20.0, n_unoccluded_iterations=0)
RBOT_MODEL_PARAMETERS = dict(sphere_radius=0.8, n_divides=4, n_points=200, max_radius_depth_offset=0.01,
                             stride_depth_offset=0.002, use_random_seed=False, image_size=2000)  # :548-551


def evaluate_rbot_dataset(open_context, dataset_directory, external_directory, body_names=RBOT_BODY_NAMES,
                          sequence_names=RBOT_SEQUENCE_NAMES, n_frames=1000, region_parameters=None,
                          model_parameters=None, tikhonov_parameter_rotation=1000.0,
                          tikhonov_parameter_translation=30000.0, n_corr_iterations=7, n_update_iterations=2,
                          report=None, shard=(0, 1), batch=1, judge_on_device=False, sequence_occlusions=None,
                          judge_occluder_on_own_pose=False, use_texture_modality=False, texture_parameters=None,
                          detector_parameters=None):
    """RBOTEvaluator::SetUp + Evaluate for the region modality: for every (sequence,
    body) a tracker on `dataset/<body>/frames/<sequence>NNNN.png`, started at `dataset/poses_first.txt`, reset on
    loss, scored with the 5 cm / 5 degree criterion.  Bodies are `dataset/<body>/<body>.obj` in millimetres
    (LoadSingleBody :527-535), their region models `external/models/<body>_model.bin` — generated on the device
    when missing or made with other parameters (GenerateSingleModel :546-556).  `open_context()` returns a fresh
    device context per run (one tracker per context).  Returns {(sequence, body): average result} and the overall
    average (CalculateAverageResult); `report`, if given, is called with each run's title and result.
    shard = (rank, world): this process takes every world-th run (the reference spreads the runs over OpenMP
    threads, rbot_evaluator.cpp:139-156; here one process per GPU takes its share and the caller merges the
    dictionaries).
    batch > 1 (HIP library): up to `batch` of this process's runs share one context -- each with its own body, model,
    loader camera and optimizer -- and go through evaluate_rbot_sequences, which resets the lost bodies alone; the
    results are those of batch = 1.
    judge_on_device (HIP library): the batched loop with the judgement and the reset on the device
    (evaluate_rbot_sequences; with batch = 1 a batch of one).
    sequence_occlusions: one bool per sequence name (None: all false -- the un-modelled sequences alone).  A sequence
    with True runs with modelled occlusions (SetUpTracker :213-332 without the texture modality): the evaluated body
    and RBOT_OCCLUSION_BODY, one RendererGeometry holding both, one FocusedBasicDepthRenderer on the run's camera that
    references both, two region modalities with ModelOcclusions, two rigid optimizers; the occluder follows
    `dataset/poses_second.txt`; the result's key is (sequence + "_modeled", body), the reference's title.  These runs
    go through evaluate_rbot_occlusion_sequences (HIP library, whatever `batch`): `batch` such runs -- 2 x batch
    bodies, batch renderers -- share a context.  judge_occluder_on_own_pose: see there.
    use_texture_modality (HIP library; use_texture_modality_ of SetUpTracker :244-249, :274-283): every run also gets a
    RendererGeometry with its body, a FocusedSilhouetteRenderer on its camera that references the body, and a
    TextureModality(body, camera, silhouette) with `texture_parameters` and the built-in detector
    (SetDetector(**detector_parameters)), behind the region modality in the optimizer's list.  A lost body is restarted
    with its texture modality -- StartModalities with batch = 1, Tracker.ResetBodies in a batch, the device judge with
    set_reset_renderers -- and the results are again those of batch = 1.  These runs are judged in the device judge's
    arithmetic wherever the judgement sits (judge_pose_result on the host), so that the host-judged and the
    device-judged loops report the same numbers float for float; runs without the argument keep rbot_pose_result.
    ValueError: with the oracle's context, which
    has no texture modality, and together with sequence_occlusions (the modelled-occlusion runs with texture are not
    built)."""
    import os

    from . import config as cfg
    from . import generator, host
    occlusions = list(sequence_occlusions) if sequence_occlusions is not None else [False] * len(sequence_names)
    if len(occlusions) != len(sequence_names):
        raise ValueError("sequence_occlusions needs one entry per sequence name")
    texture = None
    if use_texture_modality:
        if any(occlusions):
            raise ValueError("use_texture_modality together with sequence_occlusions is not supported: the runs with "
                             "modelled occlusions have no texture modality")
        texture = (dict(texture_parameters or {}), dict(detector_parameters or {}))
    if batch > 1 or judge_on_device or any(occlusions):
        return _evaluate_rbot_dataset_batched(open_context, dataset_directory, external_directory, body_names,
                                              sequence_names, n_frames, region_parameters, model_parameters,
                                              tikhonov_parameter_rotation, tikhonov_parameter_translation,
                                              n_corr_iterations, n_update_iterations, report, shard, max(1, batch),
                                              judge_on_device, occlusions, judge_occluder_on_own_pose, texture)
    poses_first = read_poses_rbot(os.path.join(dataset_directory, "poses_first.txt"), n_frames)
    region_parameters = dict(RBOT_REGION_PARAMETERS, **(region_parameters or {}))
    model_parameters = dict(RBOT_MODEL_PARAMETERS, **(model_parameters or {}))
    results = {}
    runs = [(sequence, name) for sequence in sequence_names for name in body_names]
    for sequence, name in runs[shard[0]::shard[1]]:
        api = open_context()
        body = generator.Body(api, name, os.path.join(dataset_directory, name, name + ".obj"), 0.001, True, False,
                              np.eye(4, dtype=F))
        model_path = os.path.join(external_directory, "models", name + "_model.bin")
        if cfg.model_bin_matches(model_path, True, model_parameters, body.body_data()):
            model = host.RegionModel(api, path=model_path)
        else:
            generation = {k: v for k, v in model_parameters.items() if k != "use_random_seed"}
            model = host.RegionModel.generate(api, body, **generation)
            cfg.write_model_bin(model_path, True, model_parameters, body.body_data(), *model.views())
        camera = generator.LoaderColorCamera(api, os.path.join(dataset_directory, name, "frames"), RBOT_INTRINSICS,
                                             sequence, 0, 4)
        modalities = [host.RegionModality(api, body, camera, model, **region_parameters)]
        if texture is not None:
            modalities.append(_rbot_texture_modality(api, body, camera, *texture))
        host.Optimizer(api, body=body, modalities=modalities,
                       tikhonov_parameter_rotation=tikhonov_parameter_rotation,
                       tikhonov_parameter_translation=tikhonov_parameter_translation)
        tracker = host.Tracker(api, n_corr_iterations, n_update_iterations)

        def load_image(k, camera=camera):
            camera.set_load_index(k)
            if not camera.UpdateImage():
                raise RuntimeError("Could not read image from %s" % camera.image_path())

        if texture is not None:
            _, average = evaluate_rbot_sequence(tracker, body, poses_first, load_image, n_frames,
                                                pose_result=judge_pose_result)
        else:
            _, average = evaluate_rbot_sequence(tracker, body, poses_first, load_image, n_frames)
        results[(sequence, name)] = average
        if report is not None:
            report(sequence + "_" + name, average)
    keys = ("translation_error", "rotation_error", "tracking_success", "complete_cycle")
    overall = {k: float(np.mean([r[k] for r in results.values()])) for k in keys}
    return results, overall


def _rbot_texture_modality(api, body, camera, texture_parameters, detector_parameters):
    """SetUpTracker's texture modality of the evaluated body (rbot_evaluator.cpp:244-249, :274-283) with the built-in
    detector: a silhouette renderer of the run's own that draws and references the body alone"""
    from . import host
    if not getattr(api, "is_hip", True):
        raise ValueError("use_texture_modality needs the HIP library: the oracle's context has no texture modality")
    geometry = host.RendererGeometry(api)
    geometry.AddBody(body)
    silhouette = host.FocusedSilhouetteRenderer(api, geometry, camera, image_size=RBOT_FOCUSED_IMAGE_SIZE)
    silhouette.AddReferencedBody(body)
    modality = host.TextureModality(api, body, camera, silhouette, **texture_parameters)
    modality.SetDetector(**detector_parameters)
    return modality


def _dataset_texture_modality(api, body, color, depth, texture_parameters, detector_parameters):
    """The texture modality of the YCB and OPT evaluators (ycb_evaluator.cpp:476-492, opt_evaluator.cpp:314-326): a
    RendererGeometry with the body, a FocusedSilhouetteRenderer on the colour camera with id type BODY that references
    it, TextureModality(body, colour camera, silhouette) -- with MeasureOcclusions(depth camera) where `depth` is given
    -- and the library's built-in detector in ORB's place.  The caller puts it on the optimizer behind the region and
    the depth modality (modality_ptrs()[2], ycb_evaluator.cpp:625), and has refused the oracle's context before."""
    from . import host
    geometry = host.RendererGeometry(api)
    geometry.AddBody(body)
    silhouette = host.FocusedSilhouetteRenderer(api, geometry, color, id_type=0,
                                                image_size=texture_parameters["focused_image_size"])
    silhouette.AddReferencedBody(body)
    if depth is not None:
        modality = host.TextureModality(api, body, color, silhouette, depth_camera=depth, measure_occlusions=1,
                                        **texture_parameters)
    else:
        modality = host.TextureModality(api, body, color, silhouette, **texture_parameters)
    modality.SetDetector(**detector_parameters)
    return modality


def _evaluate_rbot_dataset_batched(open_context, dataset_directory, external_directory, body_names, sequence_names,
                                   n_frames, region_parameters, model_parameters, tikhonov_parameter_rotation,
                                   tikhonov_parameter_translation, n_corr_iterations, n_update_iterations, report,
                                   shard, batch, judge_on_device=False, occlusions=None,
                                   judge_occluder_on_own_pose=False, texture=None):
    """evaluate_rbot_dataset with up to `batch` runs per context (same runs, same order, same results).  A context
    holds runs of one kind: un-modelled ones, or runs with modelled occlusions.  texture: (texture parameters, detector
    parameters) of use_texture_modality, or None."""
    import os

    from . import config as cfg
    from . import generator, host
    poses_first = read_poses_rbot(os.path.join(dataset_directory, "poses_first.txt"), n_frames)
    occlusions = list(occlusions) if occlusions is not None else [False] * len(sequence_names)
    poses_second = (read_poses_rbot(os.path.join(dataset_directory, "poses_second.txt"), n_frames)
                    if any(occlusions) else None)
    region_parameters = dict(RBOT_REGION_PARAMETERS, **(region_parameters or {}))
    model_parameters = dict(RBOT_MODEL_PARAMETERS, **(model_parameters or {}))
    results = {}
    runs = [(sequence, name, occluded) for sequence, occluded in zip(sequence_names, occlusions)
            for name in body_names][shard[0]::shard[1]]
    chunks = []  # consecutive runs of one kind, up to `batch` of them
    for run in runs:
        if chunks and len(chunks[-1]) < batch and chunks[-1][0][2] == run[2]:
            chunks[-1].append(run)
        else:
            chunks.append([run])

    def body_and_model(api, name, model=None):
        body = generator.Body(api, name, os.path.join(dataset_directory, name, name + ".obj"), 0.001, True, False,
                              np.eye(4, dtype=F))
        if model is not None:  # (the context has this body's model already)
            return body, model
        model_path = os.path.join(external_directory, "models", name + "_model.bin")
        if cfg.model_bin_matches(model_path, True, model_parameters, body.body_data()):
            model = host.RegionModel(api, path=model_path)
        else:
            generation = {k: v for k, v in model_parameters.items() if k != "use_random_seed"}
            model = host.RegionModel.generate(api, body, **generation)
            cfg.write_model_bin(model_path, True, model_parameters, body.body_data(), *model.views())
        return body, model

    for chunk in chunks:
        api = open_context()
        occluded = chunk[0][2]
        bodies, cameras, occluders = [], [], []
        occluder_model = None  # one per context: every run has its own occluding body, all of them share the model
        for sequence, name, _ in chunk:
            body, model = body_and_model(api, name)
            camera = generator.LoaderColorCamera(api, os.path.join(dataset_directory, name, "frames"), RBOT_INTRINSICS,
                                                 sequence, 0, 4)
            modality = host.RegionModality(api, body, camera, model, **region_parameters)
            if occluded:  # SetUpTracker :236-256, :268-269, :293-327
                occluder, occluder_model = body_and_model(api, RBOT_OCCLUSION_BODY, occluder_model)
                geometry = host.RendererGeometry(api)
                geometry.AddBody(body)
                geometry.AddBody(occluder)
                renderer = host.FocusedBasicDepthRenderer(api, geometry, camera, image_size=RBOT_FOCUSED_IMAGE_SIZE)
                renderer.AddReferencedBody(body)
                renderer.AddReferencedBody(occluder)
                modality.ModelOcclusions(renderer)
            modalities = [modality]
            if texture is not None:
                modalities.append(_rbot_texture_modality(api, body, camera, *texture))
            host.Optimizer(api, body=body, modalities=modalities,
                           tikhonov_parameter_rotation=tikhonov_parameter_rotation,
                           tikhonov_parameter_translation=tikhonov_parameter_translation)
            if occluded:
                occluder_modality = host.RegionModality(api, occluder, camera, occluder_model, **region_parameters)
                occluder_modality.ModelOcclusions(renderer)
                host.Optimizer(api, body=occluder, modalities=[occluder_modality],
                               tikhonov_parameter_rotation=tikhonov_parameter_rotation,
                               tikhonov_parameter_translation=tikhonov_parameter_translation)
                occluders.append(occluder)
            bodies.append(body)
            cameras.append(camera)
        tracker = host.Tracker(api, n_corr_iterations, n_update_iterations)

        def load_images(k, cameras=cameras):
            for camera in cameras:
                camera.set_load_index(k)
                if not camera.UpdateImage():
                    raise RuntimeError("Could not read image from %s" % camera.image_path())

        if occluded:
            _, averages = evaluate_rbot_occlusion_sequences(
                tracker, bodies, occluders, [poses_first] * len(chunk), [poses_second] * len(chunk), load_images,
                n_frames, judge_on_device=judge_on_device, judge_occluder_on_own_pose=judge_occluder_on_own_pose)
        elif texture is not None:
            _, averages = evaluate_rbot_sequences(tracker, bodies, [poses_first] * len(chunk), load_images, n_frames,
                                                  judge_on_device=judge_on_device, reset_renderers=True,
                                                  pose_result=judge_pose_result)
        else:
            _, averages = evaluate_rbot_sequences(tracker, bodies, [poses_first] * len(chunk), load_images, n_frames,
                                                  judge_on_device=judge_on_device)
        for (sequence, name, _), average in zip(chunk, averages):
            key = sequence + "_modeled" if occluded else sequence
            results[(key, name)] = average
            if report is not None:
                report(key + "_" + name, average)
    keys = ("translation_error", "rotation_error", "tracking_success", "complete_cycle")
    overall = {k: float(np.mean([r[k] for r in results.values()])) for k in keys}
    return results, overall


# ---------------------------------------------------------------------------------------------------------
# YCB-Video dataset driver (examples/evaluate_ycb_dataset.cpp + ycb_evaluator.cpp), without refinement, without
# modelled occlusions, single-region models
# ---------------------------------------------------------------------------------------------------------
YCB_INTRINSICS = (1066.778, 1067.487, 312.9869, 241.3109, 640, 480)  # ycb_evaluator.h:47-48
YCB_REGION_PARAMETERS = dict(  # evaluate_ycb_dataset.cpp:46-65
    n_lines_max=200, use_adaptive_coverage=0, min_continuous_distance=3.0, function_length=8, distribution_length=12,
    function_amplitude=0.43, function_slope=0.5, learning_rate=1.3, scales=[7, 4, 2],
    standard_deviations=[25.0, 15.0, 10.0], n_histogram_bins=16, learning_rate_f=0.2, learning_rate_b=0.2,
    unconsidered_line_length=0.5, max_considered_line_length=20.0, measured_depth_offset_radius=0.01,
    measured_occlusion_radius=0.01, measured_occlusion_threshold=0.03, n_unoccluded_iterations=0)
YCB_DEPTH_PARAMETERS = dict(  # evaluate_ycb_dataset.cpp:66-76
    n_points_max=200, use_adaptive_coverage=0, use_depth_scaling=0, stride_length=0.005,
    considered_distances=[0.07, 0.05, 0.04], standard_deviations=[0.05, 0.03, 0.02],
    measured_depth_offset_radius=0.01, measured_occlusion_radius=0.01, measured_occlusion_threshold=0.03,
    n_unoccluded_iterations=0)
# the fields of evaluate_ycb_dataset.cpp:77-107 that the modality has (its detector is the library's own, not ORB:
# orb_n_features = 300 becomes the built-in detector's n_features, the ORB pyramid has no counterpart)
YCB_TEXTURE_PARAMETERS = dict(
    focused_image_size=200, descriptor_distance_threshold=0.7, tukey_norm_constant=20.0,
    standard_deviations=[10.0, 10.0, 3.0],
    max_keyframe_rotation_difference=float(F(10.0) * F(np.pi) / F(180.0)), max_keyframe_age=1000, n_keyframes=1,
    measured_occlusion_radius=0.01, measured_occlusion_threshold=0.03)
YCB_DETECTOR_PARAMETERS = dict(n_features=300)  # set_orb_n_features(300), :86; the FAST threshold is the built-in's own
YCB_MODEL_PARAMETERS = dict(sphere_radius=0.8, n_divides=4, n_points=500, max_radius_depth_offset=0.05,
                            stride_depth_offset=0.002, use_random_seed=False, image_size=2000)  # :1131-1146


def ycb_sequence_name(sequence_id):
    return "%04d" % sequence_id  # SequenceIDToName :1312-1315


def ycb_keyframes(dataset_directory, sequence_name):
    """LoadKeyframes :1150-1183: image_sets/keyframe.txt holds lines '<sequence>/<frame>'"""
    import os
    frames = []
    with open(os.path.join(dataset_directory, "image_sets", "keyframe.txt")) as f:
        for line in f:
            sequence, _, frame = line.strip().partition("/")
            if sequence == sequence_name and frame:
                frames.append(int(frame))
    return frames


def ycb_sequence_bodies(dataset_directory, sequence_name):
    """SequenceBodyNames / BodyExistsInSequence :1262-1300: the first word of every line of 000001-box.txt"""
    import os
    with open(os.path.join(dataset_directory, "data", sequence_name, "000001-box.txt")) as f:
        return [line.split(" ")[0] for line in f if line.strip()]


def ycb_n_frames(dataset_directory, sequence_name):
    """NFramesInSequence :1302-1310"""
    import os
    i = 1
    while os.path.exists(os.path.join(dataset_directory, "data", sequence_name, "%06d-box.txt" % i)):
        i += 1
    return i - 1


def read_matlab_poses_ycb(path):
    """LoadMatlabGTPoses :903-944: one 'qw qx qy qz tx ty tz' line per keyframe"""
    with open(path) as f:
        return np.asarray([_quaternion_pose(*[float(x) for x in line.split(" ")[:7]]) for line in f if line.strip()], F)


def evaluate_ycb_dataset(open_context, dataset_directory, external_directory, sequence_ids, body_names,
                         use_matlab_gt_poses=True, n_vertices_evaluation=1000, region_parameters=None,
                         depth_parameters=None, model_parameters=None, tikhonov_parameter_rotation=1000.0,
                         tikhonov_parameter_translation=30000.0, n_corr_iterations=4, n_update_iterations=2,
                         report=None, shard=(0, 1), judge_on_device=False, use_texture_modality=False,
                         texture_parameters=None, detector_parameters=None, measure_occlusions_texture=True):
    """YCBEvaluator::SetUp + Evaluate with the region and the depth modality, measured occlusions, one run per
    (sequence, body present in it) (CreateRunConfigurations :1006-1022): bodies `dataset/models/<body>/textured.obj`
    in metres, frames `dataset/data/<sequence>/NNNNNN-{color,depth}.png` (depth scale 1e-4), keyframes from
    `dataset/image_sets/keyframe.txt`, ground truth from `external/poses/ground_truth/<sequence>_<body>.txt` (or the
    dataset's own `poses/<body>.txt`), models under `external/models/`.  Returns {(sequence, body): average} and
    the averages over all frames of all runs (CalculateAverageResult).  shard = (rank, world): every world-th run
    (see evaluate_rbot_dataset); the overall averages then cover this process's runs.
    judge_on_device (HIP library): ADD / ADD-S on the device (evaluate_ycb_sequence).
    use_texture_modality (HIP library; set_use_texture_modality(true), evaluate_ycb_dataset.cpp:125-133): every run also
    gets the texture modality of ycb_evaluator.cpp:476-492 (_dataset_texture_modality) with YCB_TEXTURE_PARAMETERS
    overridden by `texture_parameters`, measured occlusions on the depth camera unless measure_occlusions_texture is
    False, and the library's BUILT-IN DETECTOR (YCB_DETECTOR_PARAMETERS overridden by `detector_parameters`) -- not
    ORB: the reference's configuration with another detector, whose AUC is not claimed to equal the reference's.  The
    modality stands on the optimizer behind the region and the depth modality.  With the oracle's context: ValueError."""
    import os

    from . import config as cfg
    from . import generator, host
    texture_parameters = dict(YCB_TEXTURE_PARAMETERS, **(texture_parameters or {}))
    detector_parameters = dict(YCB_DETECTOR_PARAMETERS, **(detector_parameters or {}))
    region_parameters = dict(YCB_REGION_PARAMETERS, **(region_parameters or {}))
    depth_parameters = dict(YCB_DEPTH_PARAMETERS, **(depth_parameters or {}))
    model_parameters = dict(YCB_MODEL_PARAMETERS, **(model_parameters or {}))
    generation = {k: v for k, v in model_parameters.items() if k != "use_random_seed"}
    sequence_names = [ycb_sequence_name(i) for i in sequence_ids]
    n_frames = {ycb_sequence_name(i): ycb_n_frames(dataset_directory, ycb_sequence_name(i))
                for i in range(max(sequence_ids) + 1)
                if os.path.isdir(os.path.join(dataset_directory, "data", ycb_sequence_name(i)))}
    results, frame_results = {}, []
    runs = [(sequence, name) for sequence in sequence_names
            for name in body_names if name in ycb_sequence_bodies(dataset_directory, sequence)]
    for sequence, name in runs[shard[0]::shard[1]]:
        keyframes = ycb_keyframes(dataset_directory, sequence)
        api = open_context()
        if use_texture_modality and not getattr(api, "is_hip", True):  # (before a model is read or generated)
            raise ValueError("use_texture_modality needs the HIP library: the oracle's context has no texture modality")
        body = generator.Body(api, name, os.path.join(dataset_directory, "models", name, "textured.obj"), 1.0, True,
                              True, np.eye(4, dtype=F))
        models = []
        for region, klass, suffix in ((True, host.RegionModel, "_region_model.bin"),
                                      (False, host.DepthModel, "_depth_model.bin")):
            path = os.path.join(external_directory, "models", name + suffix)
            if cfg.model_bin_matches(path, region, model_parameters, body.body_data()):
                models.append(klass(api, path=path))
            else:
                models.append(klass.generate(api, body, **generation))
                cfg.write_model_bin(path, region, model_parameters, body.body_data(), *models[-1].views())
        directory = os.path.join(dataset_directory, "data", sequence)
        color = generator.LoaderColorCamera(api, directory, YCB_INTRINSICS, "", 1, 6, "-color")
        depth = generator.LoaderDepthCamera(api, directory, YCB_INTRINSICS, 0.0001, "", 1, 6, "-depth")
        region_modality = host.RegionModality(api, body, color, models[0], depth_camera=depth, measure_occlusions=1,
                                              **region_parameters)
        depth_modality = host.DepthModality(api, body, depth, models[1], measure_occlusions=1, **depth_parameters)
        modalities = [region_modality, depth_modality]
        if use_texture_modality:
            modalities.append(_dataset_texture_modality(api, body, color, depth if measure_occlusions_texture else None,
                                                        texture_parameters, detector_parameters))
        host.Optimizer(api, body=body, modalities=modalities,
                       tikhonov_parameter_rotation=tikhonov_parameter_rotation,
                       tikhonov_parameter_translation=tikhonov_parameter_translation)
        tracker = host.Tracker(api, n_corr_iterations, n_update_iterations)
        if use_matlab_gt_poses:
            gt = read_matlab_poses_ycb(os.path.join(external_directory, "poses", "ground_truth",
                                                    sequence + "_" + name + ".txt"))
        else:  # the dataset's pose file: the body's frames of all earlier sequences come first (LoadPoseBegin)
            begin = sum(n_frames[s] for s in sorted(n_frames) if s < sequence and
                        name in ycb_sequence_bodies(dataset_directory, s))
            gt = read_poses_ycb(os.path.join(dataset_directory, "poses", name + ".txt"), begin, n_frames[sequence],
                                keyframes)
        if len(gt) < len(keyframes):
            raise ValueError("ground truth of %s in sequence %s has %d poses for %d keyframes" %
                             (name, sequence, len(gt), len(keyframes)))

        def update_cameras(frame, color=color, depth=depth):
            for camera in (color, depth):
                camera.set_load_index(frame)
                if not camera.UpdateImage():
                    raise RuntimeError("Could not read image from %s" % camera.image_path())

        evaluation = YCBBodyEvaluation(body.vertices, n_vertices_evaluation)
        per_frame, average = evaluate_ycb_sequence(tracker, {name: body}, {name: evaluation}, {name: gt}, keyframes,
                                                   update_cameras, judge_on_device=judge_on_device)
        results[(sequence, name)] = average[name]
        frame_results += per_frame[name]
        if report is not None:
            report(sequence + ": " + name, average[name])
    overall = dict(add_auc=float(np.mean([r["add_auc"] for r in frame_results])),
                   adds_auc=float(np.mean([r["adds_auc"] for r in frame_results])),
                   complete_cycle=float(np.mean([r["complete_cycle"] for r in frame_results])))
    return results, overall


# ---------------------------------------------------------------------------------------------------------
# OPT (M3T/examples/opt_evaluator.cpp + evaluate_opt_dataset.cpp): Region + Depth, single bodies
# ---------------------------------------------------------------------------------------------------------
OPT_N_CURVE_VALUES = 100  # opt_evaluator.h:41
OPT_THRESHOLD_MAX = 0.2   # opt_evaluator.h:42
OPT_INTRINSICS = (1060.197, 1060.273, 964.809, 560.952, 1920, 1080)  # opt_evaluator.h:43-44
OPT_DEPTH2COLOR_POSE = np.asarray([[0.9999788893, -0.0052817802, 0.0037846718, -0.0525133559],  # opt_evaluator.h:45-49
                                   [0.0052971168, 0.9999777534, -0.0040537989, 0.0006022050],
                                   [-0.0037631764, 0.0040737612, 0.9999846214, -0.0003262078],
                                   [0.0, 0.0, 0.0, 1.0]], F)
OPT_GEOMETRY2BODY_TRANSLATIONS = dict(  # opt_evaluator.h:50-63 (kBody2Geometry2BodyPoseMap: pure translations)
    soda=(0.0006, -0.0004, -0.0549), chest=(-0.0002, -0.0009, -0.0377), ironman=(0.0023, 0.0005, -0.0506),
    house=(-0.0008, -0.0059, -0.0271), bike=(-0.0018, 0.0001, -0.0267), jet=(-0.0004, 0.0001, -0.0117))
OPT_BODY_NAMES = ("soda", "chest", "ironman", "house", "bike", "jet")  # evaluate_opt_dataset.cpp:13-14
OPT_BODY_ORIENTATIONS = ("b", "f", "l", "r")                           # :15
OPT_MOTION_PATTERNS = ("tr_1", "tr_2", "tr_3", "tr_4", "tr_5", "zo_1", "zo_2", "zo_3", "zo_4", "zo_5", "ir_1", "ir_2",
                       "ir_3", "ir_4", "ir_5", "or_1", "or_2", "or_3", "or_4", "or_5", "fl", "ml", "fm")  # :16-19
OPT_REGION_PARAMETERS = dict(  # evaluate_opt_dataset.cpp:24-40
    n_lines_max=200, use_adaptive_coverage=0, min_continuous_distance=3.0, function_length=8, distribution_length=12,
    function_amplitude=0.43, function_slope=0.5, learning_rate=1.3, scales=[6, 4, 1],
    standard_deviations=[15.0, 5.0, 1.5], n_histogram_bins=16, learning_rate_f=0.2, learning_rate_b=0.2,
    unconsidered_line_length=0.5, max_considered_line_length=20.0)
OPT_DEPTH_PARAMETERS = dict(  # evaluate_opt_dataset.cpp:41-48
    n_points_max=200, use_adaptive_coverage=0, use_depth_scaling=0, stride_length=0.005,
    considered_distances=[0.05, 0.02, 0.01], standard_deviations=[0.035, 0.035, 0.025])
# evaluate_opt_dataset.cpp:49-77: YCB's fields with other standard deviations; no measured occlusions (opt_evaluator.cpp:
# 314-326), so the two occlusion fields are not restated
OPT_TEXTURE_PARAMETERS = dict(
    focused_image_size=200, descriptor_distance_threshold=0.7, tukey_norm_constant=20.0,
    standard_deviations=[5.0, 1.0, 0.5],
    max_keyframe_rotation_difference=float(F(10.0) * F(np.pi) / F(180.0)), max_keyframe_age=1000, n_keyframes=1)
OPT_DETECTOR_PARAMETERS = dict(n_features=300)  # set_orb_n_features(300), :58
OPT_MODEL_PARAMETERS = dict(sphere_radius=0.8, n_divides=4, n_points=500, max_radius_depth_offset=0.05,
                            stride_depth_offset=0.002, use_random_seed=False, image_size=2000)  # opt_evaluator.cpp:531-543
OPT_TIKHONOV_PARAMETER_ROTATION = 1000.0      # evaluate_opt_dataset.cpp:78-79
OPT_TIKHONOV_PARAMETER_TRANSLATION = 30000.0  # :80
OPT_N_UPDATE_ITERATIONS = 2                   # :85
OPT_N_CORR_ITERATIONS = 4                     # :86
OPT_DEPTH_SCALE = 0.001                       # opt_evaluator.cpp:267


def opt_geometry2body_pose(body_name):
    """kBody2Geometry2BodyPoseMap.at(body_name) (opt_evaluator.h:50-63)"""
    pose = np.eye(4, dtype=F)
    pose[:3, 3] = OPT_GEOMETRY2BODY_TRANSLATIONS[body_name]
    return pose


def opt_sequence_name(body_name, body_orientation, motion_pattern):
    """CreateRunConfigurations (opt_evaluator.cpp:499-511)"""
    return body_name[:2] + "_" + motion_pattern + "_" + body_orientation


def opt_thresholds():
    """opt_evaluator.cpp:19-22"""
    step = F(OPT_THRESHOLD_MAX) / F(OPT_N_CURVE_VALUES)
    return np.asarray([step * (F(0.5) + F(i)) for i in range(OPT_N_CURVE_VALUES)], F)


def read_poses_opt(path, geometry2body):
    """OPTEvaluator::GetGTPosesOPTDataset (opt_evaluator.cpp:602-630): one pose per line, twelve numbers separated by
    blanks, filled as matrix(j, i) for i in 0..3 and j in 0..2 (column by column, the translation last), then
    pose * geometry2body^-1 in f32"""
    inverse = _inverse_pose_f32(np.asarray(geometry2body, F).reshape(4, 4))
    poses = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            t = line.split(" ")
            pose = np.eye(4, dtype=F)
            for i in range(4):
                for j in range(3):
                    pose[j, i] = F(t[3 * i + j])
            poses.append(_mul_pose_f32(pose, inverse))
    return np.asarray(poses, F).reshape(-1, 4, 4)


def opt_delta_pose(body2world_pose, gt_body2world_pose, geometry2body):
    """(body2world * geometry2body)^-1 * gt * geometry2body (opt_evaluator.cpp:466-468) as the device judge forms it
    (m3t_hip_judge_set_add_only): f64, left to right, the rigid inverse [R^T | -R^T t], every sum left to right,
    rounded to f32 once.  Returns the 3 x 4 matrix."""
    p = [[float(v) for v in row] for row in np.asarray(body2world_pose, F).reshape(4, 4)]
    t = [[float(v) for v in row] for row in np.asarray(gt_body2world_pose, F).reshape(4, 4)]
    g = [[float(v) for v in row] for row in np.asarray(geometry2body, F).reshape(4, 4)]
    a = [[(p[r][0] * g[0][c] + p[r][1] * g[1][c]) + p[r][2] * g[2][c] + (p[r][3] if c == 3 else 0.0)
          for c in range(4)] for r in range(3)]
    delta = np.zeros((3, 4), F)
    for r in range(3):
        i0, i1, i2 = a[0][r], a[1][r], a[2][r]
        i3 = -((i0 * a[0][3] + i1 * a[1][3]) + i2 * a[2][3])
        m = [((i0 * t[0][k] + i1 * t[1][k]) + i2 * t[2][k]) + i3 * t[3][k] for k in range(4)]
        for c in range(4):
            v = (m[0] * g[0][c] + m[1] * g[1][c]) + m[2] * g[2][c]
            delta[r, c] = F(v + m[3] if c == 3 else v)
    return delta


def vertices_diameter(api, vertices, chunk=512):
    """OPTEvaluator::CalculateDiameters (opt_evaluator.cpp:580-600): the largest distance between two vertices, by
    exhaustive search -- m3t_hip_vertices_diameter on the HIP library, elsewhere the same arithmetic in numpy, chunk
    rows at a time: per pair d2 = (dx*dx + dy*dy) + dz*dz in f32, the diameter the f32 root of the largest"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    if api is not None and "vertices_diameter" in api._fn:
        import ctypes as C
        out = C.c_float(0.0)
        api.call("vertices_diameter", v.ctypes.data_as(C.POINTER(C.c_float)), len(v), C.byref(out))
        return F(out.value)
    if len(v) < 1 or not np.isfinite(v).all():
        raise ValueError("vertices_diameter: needs at least one vertex and finite coordinates")
    best = F(0.0)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    for i in range(0, len(v), chunk):  # d2 is symmetric: the columns from the chunk's first row on
        dx = x[i:i + chunk, None] - x[None, i:]
        dy = y[i:i + chunk, None] - y[None, i:]
        dz = z[i:i + chunk, None] - z[None, i:]
        best = max(best, ((dx * dx + dy * dy) + dz * dz).max())
    return F(np.sqrt(F(best)))


class OPTBodyEvaluation:
    """the per-body data of OPTEvaluator::CalculatePoseResults (opt_evaluator.cpp:462-488): the reduced vertices of
    GenderateReducedVertices (:545-578; `vertices` as m3t::Body::vertices() holds them: the mesh's own, scaled,
    geometry2body not applied -- what generator.Body.vertices holds), the geometry-to-body pose and the diameter"""

    def __init__(self, vertices, geometry2body, diameter, n_vertices_evaluation=-1):
        self.vertices = np.ascontiguousarray(reduce_vertices(vertices, n_vertices_evaluation), F)
        self.geometry2body = np.asarray(geometry2body, F).reshape(4, 4)
        self.diameter = F(diameter)
        self.thresholds = opt_thresholds()

    def error(self, body2world_pose, gt_body2world_pose):
        """ADD in metres: the mean of |v - delta v|.  The reference forms delta and the sum in f32; this keeps the
        arithmetic of the device judge (f64 delta rounded once, f32 per vertex, f64 sum), as YCBBodyEvaluation does"""
        d = opt_delta_pose(body2world_pose, gt_body2world_pose, self.geometry2body)
        x, y, z = self.vertices[:, 0], self.vertices[:, 1], self.vertices[:, 2]
        ex = x - (((d[0, 0] * x + d[0, 1] * y) + d[0, 2] * z) + d[0, 3])
        ey = y - (((d[1, 0] * x + d[1, 1] * y) + d[1, 2] * z) + d[1, 3])
        ez = z - (((d[2, 0] * x + d[2, 1] * y) + d[2, 2] * z) + d[2, 3])
        norms = np.sqrt((ex * ex + ey * ey) + ez * ez)
        return float(F(norms.astype(np.float64).sum() / float(len(norms))))

    def result(self, body2world_pose, gt_body2world_pose):
        return self.result_of_error(self.error(body2world_pose, gt_body2world_pose))

    def result_of_error(self, add):
        """curve and area under curve from ADD in metres (judged here or on the device), :475-487 in f32"""
        error = F(add)
        curve = np.ones(OPT_N_CURVE_VALUES, F)
        for i in range(OPT_N_CURVE_VALUES):
            if error < F(self.diameter * self.thresholds[i]):
                break
            curve[i] = 0.0
        threshold = F(self.diameter * F(OPT_THRESHOLD_MAX))
        auc = F(F(OPT_THRESHOLD_MAX) * F(F(1.0) - min(F(error / threshold), F(1.0))))
        return dict(add_error=float(error), curve_values=curve, area_under_curve=float(auc))


def evaluate_opt_sequences(tracker, bodies, evaluations, gt_poses_per_body, load_images, judge_on_device=False):
    """The loop of OPTEvaluator::EvaluateRunConfiguration (opt_evaluator.cpp:204-251) for S independent bodies in ONE
    context, each with a list of sequences of its own: gt_poses_per_body[s][q][k] is the ground-truth pose of body s in
    image k of its sequence q.  A body starts a sequence on image 0 at its ground truth (:217-218); cycle i tracks image
    i + 1 and is judged against its ground truth (CalculatePoseResults).  The sequences may have different lengths: a
    body whose sequence has ended is put on the first pose of its next one with Tracker.ResetBodies while the others
    keep tracking, so each body's results are those of a tracker of its own.  The step's iteration number is the
    batch's cycle counter and a body's first_iteration the cycle it started on: their difference -- all the modalities
    read -- is the sequence's own cycle index.  `load_images(s, q, k)` makes image k of sequence q current in the
    cameras of body s.
    A library without reset_bodies (the oracle) can only restart all bodies of the context together: one body, or
    sequences of equal length.
    judge_on_device (HIP library): one judge, every body ADD-only with its geometry2body (Judge.set_add_only),
    judge(gt, -1) behind every step; no Sync() and no pose read per frame, the rows are read once at the end.
    Returns results[s][q] = list of per-cycle dicts (frame_index, add_error, area_under_curve, curve_values)."""
    n = len(bodies)
    device_reset = "reset_bodies" in tracker.api._fn
    results = [[[] for _ in sequences] for sequences in gt_poses_per_body]
    state = [[0, 0] for _ in range(n)]  # sequence, cycle inside it

    def start(which, iteration):
        for s in which:
            load_images(s, state[s][0], 0)
        poses = [gt_poses_per_body[s][state[s][0]][0] for s in which]
        if len(which) == n:  # all together: the reference's start (:217-218)
            for s, pose in zip(which, poses):
                bodies[s].set_body2world_pose(pose)
            if not tracker.StartModalities(iteration):
                raise RuntimeError("StartModalities failed")
        elif device_reset:
            if not tracker.ResetBodies([bodies[s] for s in which], poses, iteration):
                raise RuntimeError("ResetBodies failed")
        else:
            raise RuntimeError("this library restarts all bodies of a context together (no reset_bodies)")

    active = [s for s in range(n) if len(gt_poses_per_body[s]) > 0]
    if len(active) != n:
        raise ValueError("every body needs at least one sequence")
    start(active, 0)
    judge, pending = None, []
    if judge_on_device:
        total = max(sum(len(seq) - 1 for seq in sequences) for sequences in gt_poses_per_body)
        judge = tracker.CreateJudge(bodies, max(1, total))
        for s, evaluation in enumerate(evaluations):
            judge.set_vertices(s, evaluation.vertices)
            judge.set_add_only(s, evaluation.geometry2body)
        last_gt = [gt_poses_per_body[s][0][0] for s in range(n)]
    cycle = 0
    while active:
        for s in active:
            load_images(s, state[s][0], state[s][1] + 1)
        if not tracker.ExecuteTrackingStep(cycle):
            raise RuntimeError("tracking step %d failed" % cycle)
        if judge_on_device:
            for s in active:
                last_gt[s] = gt_poses_per_body[s][state[s][0]][state[s][1] + 1]
            row = judge.judge(last_gt, -1)
            pending += [(row, s, state[s][0], state[s][1]) for s in active]
        else:
            if not tracker.Sync():
                raise RuntimeError("tracking step %d failed" % cycle)
            for s in active:
                q, i = state[s]
                r = evaluations[s].result(bodies[s].body2world_pose(), gt_poses_per_body[s][q][i + 1])
                r.update(frame_index=i)
                results[s][q].append(r)
        ended = []
        for s in list(active):
            state[s][1] += 1
            if state[s][1] + 1 < len(gt_poses_per_body[s][state[s][0]]):
                continue
            state[s] = [state[s][0] + 1, 0]
            if state[s][0] < len(gt_poses_per_body[s]):
                ended.append(s)
            else:
                active.remove(s)
        cycle += 1
        if ended:
            start(ended, cycle)
    if judge_on_device and pending:
        rows = judge.read(0, pending[-1][0] + 1)
        for row, s, q, i in pending:
            r = evaluations[s].result_of_error(float(rows[row, s]["add_error"]))
            r.update(frame_index=i)
            results[s][q].append(r)
    return results


def opt_average_result(frame_results):
    """CalculateAverageResult / SumResults / DivideResult (opt_evaluator.cpp:402-460) over per-frame results, in f32"""
    auc, curve = F(0.0), np.zeros(OPT_N_CURVE_VALUES, F)
    for r in frame_results:
        auc = F(auc + F(r["area_under_curve"]))
        curve = (curve + r["curve_values"]).astype(F)
    n = F(max(1, len(frame_results)))
    return dict(area_under_curve=float(F(auc / n)), curve_values=(curve / n).astype(F))


def evaluate_opt_dataset(open_context, dataset_directory, external_directory, body_names=OPT_BODY_NAMES,
                         body_orientations=OPT_BODY_ORIENTATIONS, motion_patterns=OPT_MOTION_PATTERNS,
                         region_parameters=None, depth_parameters=None, model_parameters=None,
                         tikhonov_parameter_rotation=OPT_TIKHONOV_PARAMETER_ROTATION,
                         tikhonov_parameter_translation=OPT_TIKHONOV_PARAMETER_TRANSLATION,
                         n_corr_iterations=OPT_N_CORR_ITERATIONS, n_update_iterations=OPT_N_UPDATE_ITERATIONS,
                         report=None, shard=(0, 1), batch=1, n_vertices_evaluation=1000, calculate_diameters=True,
                         diameters=None, intrinsics=OPT_INTRINSICS, depth2color_pose=OPT_DEPTH2COLOR_POSE,
                         judge_on_device=False, use_texture_modality=False, texture_parameters=None,
                         detector_parameters=None):
    """OPTEvaluator::SetUp + Evaluate, by default in the Region + Depth configuration (the reference's example runs
    Region + Depth + Texture, evaluate_opt_dataset.cpp:93-95: that is use_texture_modality below): one run per
    (body, orientation, motion pattern) (CreateRunConfigurations :499-511) on `dataset/3D/<sequence>/color|depth/
    NNNN.png` from image 1 (loader cameras :261-271, depth scale 0.001, the depth camera's camera2world the
    depth-to-colour pose), ground truth `dataset/3D/poses/<sequence>.txt`, bodies `dataset/Model3D/<body>/<body>.obj`
    in metres with their geometry-to-body translations (LoadBodies :513-525), models under `external/models/`
    (GenerateModels :527-553), ADD over n_vertices_evaluation reduced vertices against the body's diameter.
    calculate_diameters: CalculateDiameters over all of a body's vertices (vertices_diameter: on the device with the
    HIP library); otherwise `diameters` gives them by body name (the reference's table is not restated).
    `intrinsics` and `depth2color_pose` default to the dataset's (a synthetic dataset brings its own).
    batch: up to `batch` bodies share one context, each with its own cameras and its own list of this process's
    sequences, through evaluate_opt_sequences (one body per context: batch = 1).  shard = (rank, world): every world-th
    run.  Returns {sequence name: average result}, and the averages per body and over "all" bodies of all their frames
    (CalculateAverageBodyResult :402-415).
    use_texture_modality (HIP library; set_use_texture_modality(true)): every body also gets the texture modality of
    opt_evaluator.cpp:314-326 (_dataset_texture_modality, no measured occlusions) with OPT_TEXTURE_PARAMETERS overridden
    by `texture_parameters` and the library's BUILT-IN DETECTOR (OPT_DETECTOR_PARAMETERS overridden by
    `detector_parameters`) -- not ORB: the reference's configuration with another detector, whose AUC is not claimed to
    equal the reference's.  The modality stands on the optimizer behind the region and the depth modality; in a batch,
    Tracker.ResetBodies restarts it with its body.  With the oracle's context: ValueError."""
    import os

    from . import config as cfg
    from . import generator, host
    texture_parameters = dict(OPT_TEXTURE_PARAMETERS, **(texture_parameters or {}))
    detector_parameters = dict(OPT_DETECTOR_PARAMETERS, **(detector_parameters or {}))
    region_parameters = dict(OPT_REGION_PARAMETERS, **(region_parameters or {}))
    depth_parameters = dict(OPT_DEPTH_PARAMETERS, **(depth_parameters or {}))
    model_parameters = dict(OPT_MODEL_PARAMETERS, **(model_parameters or {}))
    generation = {k: v for k, v in model_parameters.items() if k != "use_random_seed"}
    runs = [(name, opt_sequence_name(name, orientation, pattern)) for name in body_names
            for orientation in body_orientations for pattern in motion_patterns][shard[0]::shard[1]]
    per_body = {}
    for name, sequence in runs:
        per_body.setdefault(name, []).append(sequence)
    names = list(per_body)
    results, frames_of_body = {}, {name: [] for name in names}
    for first in range(0, len(names), max(1, batch)):
        chunk = names[first:first + max(1, batch)]
        api = open_context()
        if use_texture_modality and not getattr(api, "is_hip", True):  # (before a model is read or generated)
            raise ValueError("use_texture_modality needs the HIP library: the oracle's context has no texture modality")
        bodies, evaluations, cameras, gt = [], [], [], []
        for name in chunk:
            geometry2body = opt_geometry2body_pose(name) if name in OPT_GEOMETRY2BODY_TRANSLATIONS else np.eye(4, dtype=F)
            body = generator.Body(api, name, os.path.join(dataset_directory, "Model3D", name, name + ".obj"), 1.0, True,
                                  True, geometry2body)
            models = []
            for region, klass, suffix in ((True, host.RegionModel, "_region_model.bin"),
                                          (False, host.DepthModel, "_depth_model.bin")):
                path = os.path.join(external_directory, "models", name + suffix)
                if cfg.model_bin_matches(path, region, model_parameters, body.body_data()):
                    models.append(klass(api, path=path))
                else:
                    models.append(klass.generate(api, body, **generation))
                    cfg.write_model_bin(path, region, model_parameters, body.body_data(), *models[-1].views())
            directory = os.path.join(dataset_directory, "3D", per_body[name][0])
            color = generator.LoaderColorCamera(api, os.path.join(directory, "color"), intrinsics, "", 1, 4)
            depth = generator.LoaderDepthCamera(api, os.path.join(directory, "depth"), intrinsics, OPT_DEPTH_SCALE, "", 1,
                                                4, camera2world_pose=depth2color_pose)
            region_modality = host.RegionModality(api, body, color, models[0], **region_parameters)
            depth_modality = host.DepthModality(api, body, depth, models[1], **depth_parameters)
            modalities = [region_modality, depth_modality]
            if use_texture_modality:
                modalities.append(_dataset_texture_modality(api, body, color, None, texture_parameters,
                                                            detector_parameters))
            host.Optimizer(api, body=body, modalities=modalities,
                           tikhonov_parameter_rotation=tikhonov_parameter_rotation,
                           tikhonov_parameter_translation=tikhonov_parameter_translation)
            diameter = vertices_diameter(api, body.vertices) if calculate_diameters else diameters[name]
            bodies.append(body)
            evaluations.append(OPTBodyEvaluation(body.vertices, geometry2body, diameter, n_vertices_evaluation))
            cameras.append((color, depth))
            gt.append([read_poses_opt(os.path.join(dataset_directory, "3D", "poses", sequence + ".txt"), geometry2body)
                       for sequence in per_body[name]])
        tracker = host.Tracker(api, n_corr_iterations, n_update_iterations)

        def load_images(s, q, k, chunk=chunk, cameras=cameras):
            directory = os.path.join(dataset_directory, "3D", per_body[chunk[s]][q])
            for camera, kind in zip(cameras[s], ("color", "depth")):
                camera.load_directory = os.path.join(directory, kind)
                camera.set_load_index(1 + k)  # (drops what was prefetched from the last directory)
                if not camera.UpdateImage():
                    raise RuntimeError("Could not read image from %s" % camera.image_path())

        per_sequence = evaluate_opt_sequences(tracker, bodies, evaluations, gt, load_images,
                                              judge_on_device=judge_on_device)
        for s, name in enumerate(chunk):
            for q, sequence in enumerate(per_body[name]):
                results[sequence] = opt_average_result(per_sequence[s][q])
                frames_of_body[name] += per_sequence[s][q]
                if report is not None:
                    report(sequence, results[sequence])
    final = {name: opt_average_result(frames_of_body[name]) for name in names}
    final["all"] = opt_average_result([r for name in names for r in frames_of_body[name]])
    return results, final
