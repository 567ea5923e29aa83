"""The case table of the fused step kernels' parameter and geometry edges, and the helpers that run a case.

No test lives here.  tests/test_fused_edge_cases.py (CPU) runs every case through the oracle alone and checks that it
is *live* (finite poses, the objects that must move do, the line / point counts lie in the stated bracket);
tests/test_gpu_fused_edges.py runs every case through every fused launch shape on the device and compares it with the
oracle bit for bit.

A case says how to make its inputs, which parameters the modalities and the tracker get, what the oracle must show,
and -- `expect` -- which kernel the host has to launch in every launch shape.  The expected names are written down
from the host's rules in m3t_hip_api.hip (UploadTables: compact_possible, split_possible; ComputeLayout: layout.off_hist,
lds_compact_table) and m3t_step_plan.h (RigidSplitParts, PlanRigidStep), in `_expect` below:

  * compact shapes need function_length 8, distribution_length 12, n_lines_max <= 256 (M3T_COMPACT_THREADS) and every
    scale in 1..9; otherwise the one-workgroup kernel is launched (512 threads);
  * the LDS pair table of tracking_step_compact_table_kernel exists for 1024 <= bins^3 <= 32768 (16 and 32 bins) in
    Region-only batches; otherwise tracking_step_compact_kernel;
  * split shapes need >= 4 histogram bins and at most 256 lines and points (a part's elements must fit its share of
    the 256 exchange lanes, for every number of parts); otherwise the one-workgroup kernel;
  * a one-workgroup kernel is the _lds_ one where the pair table is staged in LDS (a RegionModality with bins^3 * 8
    bytes <= 32 KB: up to 16 bins), the _pair_ one where the batch has region AND depth modalities;
  * the per-object working set of the one-workgroup kernels (1024 + 31 * n_lines_max rounded up to 4, + 3 * n_lines_max
    * max(9, function_length + distribution_length - 1) floats) must fit the 160 KB LDS of a CU; a modality beyond that
    (more than 453 lines at the default lengths) is answered with M3T_ERR_UNSUPPORTED by every call that prepares a
    step, in every launch shape.
"""
import ctypes as C

import numpy as np

import scenes
import util
from util import syn

M3T_ERR_UNSUPPORTED = -3

# every developer override that selects a launch shape (cleared before a shape sets its own)
OVERRIDES = ("M3T_HIP_NO_SPLIT", "M3T_HIP_SPLIT_PARTS", "M3T_HIP_THREADS", "M3T_HIP_COMPACT", "M3T_HIP_COMPACT_TABLE",
             "M3T_HIP_COMPACT_TABLE_KB", "M3T_HIP_COMPACT_TABLE_CAP", "M3T_HIP_COMPACT_WIDE", "M3T_HIP_NO_PAIR",
             "M3T_HIP_NO_FUSED_HISTOGRAM")

_COMPACT = {"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT": "1"}
# launch shape -> (overrides, kind, parts or threads the override asks for)
SHAPES_REGION = {
    "split": ({}, "split", 8),
    "split16": ({"M3T_HIP_SPLIT_PARTS": "16"}, "split", 16),
    "split2": ({"M3T_HIP_SPLIT_PARTS": "2"}, "split", 2),
    "wg512": ({"M3T_HIP_NO_SPLIT": "1"}, "wg", 512),
    "wg256": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "256"}, "wg", 256),
    "wg128": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "128"}, "wg", 128),
    "compact": (dict(_COMPACT, M3T_HIP_COMPACT_TABLE="0", M3T_HIP_COMPACT_WIDE="0"), "compact", 256),
    "compact_table": (dict(_COMPACT), "table", 256),
    "compact_cap64": (dict(_COMPACT, M3T_HIP_COMPACT_TABLE_CAP="64"), "table", 256),
}
SHAPES_DEPTH = {
    "split": ({}, "split", 8),
    "split16": ({"M3T_HIP_SPLIT_PARTS": "16"}, "split", 16),
    "split2": ({"M3T_HIP_SPLIT_PARTS": "2"}, "split", 2),
    "split_nopair": ({"M3T_HIP_NO_PAIR": "1"}, "split_nopair", 8),
    "wg512": ({"M3T_HIP_NO_SPLIT": "1"}, "wg", 512),
    "wg256": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "256"}, "wg", 256),
    "wg128": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_THREADS": "128"}, "wg", 128),
    "compact": (dict(_COMPACT, M3T_HIP_COMPACT_TABLE="0", M3T_HIP_COMPACT_WIDE="0"), "compact", 256),
    "compact_wide": (dict(_COMPACT, M3T_HIP_COMPACT_WIDE="1"), "wide", 512),
}


class Case:
    def __init__(self, id, group, n_objects=3, inputs_args=None, region=None, depth=None, tracker=None,
                 with_depth=False, kinds=None, moves=None, lines=None, points=None, empty=(), edit=None,
                 small_histograms=False):
        self.id, self.group = id, group
        self.n_objects = n_objects
        self.with_depth = with_depth
        self.inputs_args = dict(inputs_args or {})
        self.edit = edit
        base_r = syn.YCB_REGION_PARAMS if with_depth else syn.RBOT_REGION_PARAMS
        self.region_params = dict(base_r, **(region or {}))
        self.depth_params = dict(syn.YCB_DEPTH_PARAMS, **(depth or {}))
        self.tracker_params = dict(syn.YCB_TRACKER if with_depth else syn.RBOT_TRACKER, **(tracker or {}))
        self.kinds = kinds
        # what the oracle must show: per object, does the pose change; (lo, hi) valid lines / points, inclusive
        self.moves = list(moves) if moves is not None else [True] * n_objects
        nl, npts = self.region_params["n_lines_max"], self.depth_params["n_points_max"]
        self.lines = list(lines) if lines is not None else [(1, nl)] * n_objects
        self.points = list(points) if points is not None else [(1, npts)] * n_objects
        self.empty = tuple(empty)  # objects without a single valid line: pose and histograms stay as started
        # too few samples for 96 mixed bins: even a 64-entry pair table never sends the host back to the plain kernel
        self.small_histograms = small_histograms
        self.first_scale = self.region_params["scales"][0]
        self.has_region = kinds is None or any("r" in k for k in kinds)
        self.unsupported = self.has_region and _lds_track_bytes(self.region_params) > 160 * 1024
        self.expect = _expect(self)

    def __repr__(self):
        return self.id

    @property
    def shapes(self):
        return SHAPES_DEPTH if self.with_depth else SHAPES_REGION

    def instance_kw(self):
        kw = dict(region_params=self.region_params, tracker_params=self.tracker_params)
        if self.with_depth:
            kw.update(depth_params=self.depth_params, use_depth=True)
            if self.kinds is not None:
                kw.update(kinds=self.kinds)
        return kw


def _lds_track_bytes(rp):
    """ComputeLayout, Region-only, histograms not staged (the smaller of the two layouts): misc | line state | chain,
    seg_f, seg_b"""
    nl = rp["n_lines_max"]
    ns = max(9, rp["function_length"] + rp["distribution_length"] - 1)
    return 4 * ((1024 + 31 * nl + 3) // 4 * 4 + 3 * nl * ns)


def _expect(case):
    """{shape: (kernel, workgroups per object, threads)} from the host's rules (module docstring)"""
    rp = case.region_params
    bins = rp["n_histogram_bins"]
    n_lines = rp["n_lines_max"] if case.has_region else 1
    elements = max(n_lines, case.depth_params["n_points_max"]) if case.with_depth else n_lines
    compact_ok = not case.has_region or (rp["function_length"] == 8 and rp["distribution_length"] == 12 and
                                         n_lines <= 256 and all(1 <= s <= 9 for s in rp["scales"]))
    split_ok = (not case.has_region or bins >= 4) and elements <= 256
    table_ok = compact_ok and not case.with_depth and 1024 <= bins ** 3 <= 32768
    staged = case.has_region and bins ** 3 * 8 <= 32 * 1024
    pair = case.with_depth and case.has_region

    def one_workgroup(nopair=False):
        return "tracking_step_%s%skernel" % ("lds_" if staged else "", "pair_" if pair and not nopair else "")

    out = {}
    for shape, (_, kind, arg) in case.shapes.items():
        if kind in ("split", "split_nopair"):
            nopair = kind == "split_nopair"
            if split_ok:
                out[shape] = ("tracking_step_split_pair_kernel" if pair and not nopair else "tracking_step_split_kernel",
                              arg, 512)
            else:
                out[shape] = (one_workgroup(nopair), 1, 512)
        elif kind == "wg":
            out[shape] = (one_workgroup(), 1, arg)
        elif not compact_ok:
            out[shape] = (one_workgroup(), 1, 512)
        elif kind == "table" and table_ok:
            out[shape] = ("tracking_step_compact_table_kernel", 1, 256)
        elif kind == "wide":
            out[shape] = ("tracking_step_compact_wide_kernel", 1, 512)
        else:
            out[shape] = ("tracking_step_compact_kernel", 1, 256)
    return out


# ---- edits of the generated inputs (each on the case's own copy) ------------------------------------------------------
def _ragged(inputs):
    """object 0 centred on the right image border, 1 far outside, 2 behind the camera, 3 as generated"""
    W, z = inputs.intr["width"], inputs.gt[0][0][2, 3]
    inputs.start[0] = inputs.gt[0][0].copy()
    inputs.start[0][0, 3] = (W - 1 - inputs.intr["ppu"]) * z / inputs.intr["fu"]
    inputs.start[1] = inputs.gt[1][0].copy()
    inputs.start[1][0, 3] += 3.0
    inputs.start[2] = inputs.gt[2][0].copy()
    inputs.start[2][2, 3] = -0.5


def _zero_depth_of_object_1(inputs):
    inputs.depth[1] = [np.zeros_like(f) for f in inputs.depth[1]]


def _scales(scales, deviations=None):
    return dict(region=dict(scales=scales, standard_deviations=deviations or [15.0] * len(scales)),
                tracker=dict(n_corr_iterations=len(scales)))  # every scale of the list is walked


_ODD_IMAGE = dict(syn.RBOT_INTRINSICS, width=333, height=251, ppu=166.5, ppv=125.5)

CASES = (
    # scale as a template argument: compact_walk<1..9>, chain_fill<1..7> + generic, region_segments<1..9>
    [Case("scales-" + "-".join(map(str, s)), "scale", **_scales(s, d)) for s, d in (
        ([1], None), ([2, 1], [7.0, 1.5]), ([3, 2], None), ([4, 3], None), ([5, 2, 2, 1], [20.0, 7.0, 3.0, 1.5]),
        ([6, 1], None), ([7, 4, 2], None), ([8, 5], None), ([9, 7, 5, 2], None))] +
    # scales the compact kernels must refuse
    [Case("scales-" + "-".join(map(str, s)), "refused-scale", **_scales(s)) for s in ([10, 3], [12])] +
    [Case("lengths-%d-%d" % (fl, dl), "lengths",
          region=dict(function_length=fl, distribution_length=dl, scales=[2, 1], standard_deviations=[7.0, 1.5]))
     for fl, dl in ((8, 12), (6, 10), (4, 16), (10, 8), (16, 16), (1, 2))] +
    [Case("bins-%d" % b, "bins", region=dict(n_histogram_bins=b)) for b in (2, 4, 8, 16, 32, 64)] +
    [Case("lines-5", "few-lines", region=dict(n_lines_max=5), small_histograms=True),
     Case("lines-10", "few-lines", region=dict(n_lines_max=10), small_histograms=True),
     Case("points120-lines200", "few-lines", inputs_args=dict(n_points=120), lines=[(1, 120)] * 3),
     Case("adaptive-100", "few-lines", inputs_args=dict(n_points=120),
          region=dict(n_lines_max=100, use_adaptive_coverage=1)),
     Case("adaptive-100-ref035", "few-lines", inputs_args=dict(n_points=120),
          region=dict(n_lines_max=100, use_adaptive_coverage=1, reference_contour_length=0.35)),
     # 300-point models: 256 lines are what a 256-thread compact workgroup holds, 257 are one too many
     Case("points300-lines256", "compact-limit", n_objects=2, inputs_args=dict(n_points=300),
          region=dict(n_lines_max=256), lines=[(256, 256)] * 2),
     Case("points300-lines257", "compact-limit", n_objects=2, inputs_args=dict(n_points=300),
          region=dict(n_lines_max=257), lines=[(257, 257)] * 2),
     # more lines than a workgroup has threads -- and more than the LDS of a CU holds
     Case("points600-lines513", "many-lines", n_objects=2, inputs_args=dict(n_points=600),
          region=dict(n_lines_max=513), lines=[(513, 513)] * 2),
     Case("points600-lines600", "many-lines", n_objects=2, inputs_args=dict(n_points=600),
          region=dict(n_lines_max=600), lines=[(600, 600)] * 2),
     Case("ragged", "ragged", n_objects=4, edit=_ragged, moves=[True, False, False, True],
          lines=[(1, 149), (0, 0), (0, 0), (1, 200)], empty=(1, 2)),
     Case("image-333x251", "image", inputs_args=dict(intr=_ODD_IMAGE))])

CASES_DEPTH = [
    Case("depth-points-200", "depth", with_depth=True),
    Case("depth-points-7", "depth", with_depth=True, depth=dict(n_points_max=7)),
    Case("depth-points-1", "depth", with_depth=True, depth=dict(n_points_max=1)),
    # object 1 never sees a valid depth sample: its lines still move it
    Case("depth-zero-frames", "depth", with_depth=True, edit=_zero_depth_of_object_1, points=[(1, 200), (0, 0), (1, 200)]),
    # the same with DepthModalities alone: that body keeps its pose
    Case("depth-only-zero-frames", "depth", with_depth=True, edit=_zero_depth_of_object_1, kinds=["d", "d", "d"],
         moves=[True, False, True], points=[(1, 200), (0, 0), (1, 200)]),
    Case("depth-lines5-points7", "depth", with_depth=True, region=dict(n_lines_max=5), depth=dict(n_points_max=7)),
]

ALL_CASES = CASES + CASES_DEPTH
BY_ID = {c.id: c for c in ALL_CASES}
PAIRS = [(c, s) for c in ALL_CASES for s in c.shapes]

_inputs = {}


def inputs_of(case):
    """the case's inputs, generated (and edited) once per process; runs do not change them"""
    if case.id not in _inputs:
        inputs = scenes.Inputs(case.n_objects, 3, n_divides=2, with_depth=case.with_depth, **case.inputs_args)
        if case.edit is not None:  # on a copy: objects with the same arguments may share arrays with a cached load
            inputs = scenes.subset(inputs, list(range(inputs.n_objects)))
            inputs.start = [p.copy() for p in inputs.start]
            inputs.depth = [list(frames) for frames in inputs.depth]
            case.edit(inputs)
        _inputs[case.id] = inputs
    return _inputs[case.id]


def shape_of(api):
    shape = (C.c_int * 4)()
    api.call("get_step_shape", shape)
    return list(shape)


def kernel_of(api):
    name = C.create_string_buffer(64)
    api.call("get_step_kernel", name, 64)
    return name.value.decode()


class Run:
    """what one context made of a case: poses[k] after frame k, the start poses, histograms after StartModalities and
    after the last frame; from the oracle the valid lines / points of every modality after the last frame, from the device
    the kernel and launch shape of every frame"""


def run(api, case, inputs, n_frames=None, device=False):
    inst = scenes.Instance(api, inputs, **case.instance_kw())
    out = Run()
    out.instance = inst
    out.start = np.stack(inst.poses())
    inst.upload_frame(0)
    out.started = inst.tracker.StartModalities(0)
    out.poses, out.kernels, out.shapes = [], [], []
    if not out.started:
        return out
    out.hist_start = [r.histograms() for r in inst.region]
    out.hist_frames = [out.hist_start]  # [k]: the histograms the walks of frame k read
    for k in range(n_frames or inputs.n_frames):
        inst.upload_frame(min(k, inputs.n_frames - 1))
        assert inst.tracker.ExecuteTrackingStep(k), (case.id, k)
        out.poses.append(np.stack(inst.poses()))  # (the read-back also waits for the step)
        out.hist_frames.append([r.histograms() for r in inst.region])
        if device:
            out.kernels.append(kernel_of(api))
            out.shapes.append(shape_of(api))
    out.hist = out.hist_frames[-1]
    if not device:  # (the fused kernels keep the line / point state in LDS: the device has no such read-back)
        out.n_lines = [len(r.data_lines()) for r in inst.region]
        out.n_points = [len(d.data_points()) for d in inst.depth]
    return out


def oracle_run(case, n_frames=None):
    return run(util.open_oracle(), case, inputs_of(case), n_frames)


TABLE_CAP = 64  # M3T_HIP_COMPACT_TABLE_CAP of the "compact_cap64" shape


def mixed_bins(hist_f, hist_b):
    """the bins that take a slot of the compacted pair table (m3t_compact.hip, compact_stage_table): every bin whose
    normalised pair is none of the three constant ones (0.5, 0.5) / (1, 0) / (0, 1)"""
    return int(np.count_nonzero((hist_f > 0) & (hist_b > 0) & (hist_f != hist_b)))


def table_kernels(ref, n_frames):
    """the kernel of every frame in the "compact_cap64" shape, from the oracle's histograms and the host's rule
    (m3t_step_plan.h, PlanRigidStep): every workgroup whose object has more mixed bins than the table holds walks with
    the global table and reports by how much; once a report exceeds half the table, the host launches the kernel without the table
    until StartModalities brings new histograms"""
    out, worst = [], 0
    for k in range(n_frames):
        out.append("tracking_step_compact_kernel" if worst > TABLE_CAP // 2 else "tracking_step_compact_table_kernel")
        worst = max([worst] + [mixed_bins(f, b) - TABLE_CAP for f, b in ref.hist_frames[k]])
    return out
