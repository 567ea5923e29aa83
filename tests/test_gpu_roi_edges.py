"""ROI ingest where tests/test_gpu_roi.py cannot see it fail.  In the synthetic scenes every frame starts
from the same background, so what a ring slot holds outside its rectangle (frame k - 2) IS the true frame k there: a
rectangle that is too small, a guard that passes a step it should have dropped, a pull that misses rows or columns --
all of them leave the poses "bit for bit those of whole frames".  Here every slot is POISONED before its rectangle
arrives: a whole batch of 255 - true (colour) or true // 2 + 1 (depth: in front of the scene) goes down the same copy
stream first, then the rectangle pull of the true block.  Whatever the step reads outside what was pulled is wrong in
every pixel.

  (a) poisoned sequences through each of the four guarded kernels and six motions: poses bit for bit those of the
      blocking whole-frame run, nobody unrecovered
  (b) the control: a block that is true only inside the bodies' projected boxes (no reach, no margin) does change the
      poses -- the poison is read, (a) has teeth
  (c) the device's rectangle table (m3t_hip_roi_get_rectangles) against tests/roi_reference.py: R_min within the
      device's rectangle within R_max, for every camera after every rectangle upload, from the poses the last enqueued
      step started from
  (d) the bytes roi_pull_kernel landed (m3t_hip_camera_download_slot) against the composite of poison and true block
      built from the DEVICE's rectangle (so (d) does not lean on (c)): 640 x 512 colour frames up to the full frame,
      u16 depth frames, and a 100 x 52 camera whose rows are 300 bytes with strips of 1 to 3 columns / rows at each edge
  (e) what roi_repair_kernel leaves: the runaway's whole frame and a whole-frame rectangle, the other slots untouched
  (f) the documented recovery from m3t_hip_roi_get_unrecovered
"""
import ctypes as C
import functools

import numpy as np
import pytest

import roi_reference as ref
import scenes
import util
from test_roi_bound import box_of
from util import syn

pytestmark = pytest.mark.gpu
capi = util.pkg._capi

# how test_gpu_roi.py selects the guarded kernels: (environment, the kernel the last step must report, region parameters)
KERNELS = {
    "split": ({}, "tracking_step_split_guard_kernel", None),
    "one workgroup": ({"M3T_HIP_NO_SPLIT": "1"}, "tracking_step_guard_kernel", None),
    "one workgroup, pair table in LDS": ({"M3T_HIP_NO_SPLIT": "1"}, "tracking_step_lds_guard_kernel",
                                         dict(syn.RBOT_REGION_PARAMS, n_histogram_bins=16)),
    "compact": ({"M3T_HIP_NO_SPLIT": "1", "M3T_HIP_COMPACT": "1"}, "tracking_step_compact_guard_kernel", None),
}
SMALL = dict(fu=120.0, fv=119.0, ppu=50.3, ppv=25.8, width=100, height=52)  # rows of 300 bytes, 6.5 bands of 8 rows


# ---- scenes: scenes.Inputs, edited as test_gpu_roi.runaway_inputs edits them -------------------------------------------
def shifted(pose, intr, du=0.0, dv=0.0):
    """the pose moved sideways by (du, dv) pixels at its depth"""
    out = np.array(pose, copy=True)
    out[0, 3] += du * out[2, 3] / intr["fu"]
    out[1, 3] += dv * out[2, 3] / intr["fv"]
    return out


def placed(pose, intr, u, v, z=None):
    """the pose with its origin at pixel (u, v), at depth z (default: its own)"""
    out = np.array(pose, copy=True)
    z = out[2, 3] if z is None else z
    out[:3, 3] = [(u - intr["ppu"]) * z / intr["fu"], (v - intr["ppv"]) * z / intr["fv"], z]
    return out


def rerender(inputs, i, frames=None):
    for k in (range(inputs.n_frames) if frames is None else frames):
        inputs.color[i][k] = inputs.scenes[i].render(inputs.gt[i][k])


def render_shared(inputs, objects, k):
    """one frame with all of `objects` in it, over the first one's background"""
    img = inputs.scenes[objects[0]].render(inputs.gt[objects[0]][k])
    for i in objects[1:]:
        sc = inputs.scenes[i]
        keep, sc.background = sc.background, img
        img = sc.render(inputs.gt[i][k])
        sc.background = keep
    return img


def motion_inputs(kind):
    """3 objects, 7 frames"""
    inputs = scenes.Inputs(3, 7, n_divides=2)
    intr, n = inputs.intr, inputs.n_frames
    if kind == "steady":
        pass
    elif kind == "runaway":  # object 1 runs away sideways by 2 cm (~24 pixels) per frame from frame 3 on
        for k in range(3, n):
            inputs.gt[1][k][0, 3] -= 0.02 * (k - 2)
        rerender(inputs, 1, range(3, n))
    elif kind == "approach":  # object 2 comes 2.5 cm closer per frame along its viewing ray
        for k in range(2, n):
            z = inputs.gt[2][k][2, 3]
            inputs.gt[2][k][:3, 3] *= (z - 0.025 * (k - 1)) / z
        rerender(inputs, 2, range(2, n))
    elif kind == "rotate":  # object 0 turns by 6 degrees per frame about its z axis: its longest extent (x) sweeps
        for k in range(2, n):
            inputs.gt[0][k][:3, :3] = inputs.gt[0][k][:3, :3] @ syn.rot_vec(np.array([0.0, 0.0, np.deg2rad(6.0) * (k - 1)]))
        rerender(inputs, 0, range(2, n))
    elif kind == "drift":  # object 0 starts 50 pixels from the left edge and drifts out by 8 pixels per frame: its
        z = inputs.gt[0][0][2, 3]  # outline crosses x = 0 from frame 3 on, two thirds of it stay visible in frame 6
        u0 = inputs.gt[0][0][0, 3] * intr["fu"] / z + intr["ppu"]
        inputs.start[0] = shifted(inputs.start[0], intr, du=50.0 - u0)
        for k in range(n):
            inputs.gt[0][k] = shifted(inputs.gt[0][k], intr, du=50.0 - u0 - 8.0 * k)
        rerender(inputs, 0)
    elif kind == "shared":  # objects 1 (the runaway) and 2 in one frame stream, apart from each other
        for i, (u, v) in ((1, (300.0, 150.0)), (2, (480.0, 380.0))):
            z = inputs.gt[i][0][2, 3]
            du = u - (inputs.gt[i][0][0, 3] * intr["fu"] / z + intr["ppu"])
            dv = v - (inputs.gt[i][0][1, 3] * intr["fv"] / z + intr["ppv"])
            inputs.start[i] = shifted(inputs.start[i], intr, du, dv)
            for k in range(n):
                inputs.gt[i][k] = shifted(inputs.gt[i][k], intr, du, dv)
        for k in range(3, n):
            inputs.gt[1][k][0, 3] -= 0.02 * (k - 2)
        inputs.camera_of = [0, 1, 1]
        for k in range(n):
            inputs.color[1][k] = inputs.color[2][k] = render_shared(inputs, [1, 2], k)
    else:
        raise ValueError(kind)
    return inputs


RECT_CAMERA_OF = [0, 1, 2, 3, 4, 5, 6, 6, 7, 7, 8, 9]


def rect_inputs():
    """12 static bodies in 10 cameras of 640 x 512: 0 mid-frame; 1-4 clipped at the left, right, top, bottom edge;
    5 wholly off the frame, alone; 6 on the frame + 7 off it on the right in one camera; 8 on the frame + 9 off it
    below in one camera; 10 behind the camera (every corner of its box at z <= 1e-3) and 11 across the camera plane
    (8 cm in front of the camera, a diagonal of its box along the view axis: the nearest corner lies 1.4 cm behind the
    plane, every model point at least 2 cm in front of it): the whole frame"""
    inputs = scenes.Inputs(12, 4, n_divides=2, n_models=3)
    intr = inputs.intr
    w, h = intr["width"], intr["height"]
    at = {0: (320.0, 256.0), 1: (20.0, 250.0), 2: (w - 25.0, 260.0), 3: (300.0, 15.0), 4: (330.0, h - 20.0),
          5: (w + 400.0, 200.0), 6: (200.0, 200.0), 7: (w + 400.0, 300.0), 8: (420.0, 180.0), 9: (250.0, h + 400.0),
          10: (320.0, 256.0), 11: (320.0, 256.0)}
    for i, (u, v) in at.items():
        pose = placed(inputs.gt[i][0], intr, u, v, z=-0.5 if i == 10 else None).astype(np.float32)
        if i == 11:
            lo, hi, _ = box_of(inputs.region_models[inputs.model_of[i]][0])
            d = np.array([-1.0, -1.0, 1.0]) * 0.5 * (hi - lo)
            d /= np.linalg.norm(d)
            axis = np.cross(d, [0.0, 0.0, -1.0])  # the rotation that turns the box's diagonal d towards the camera
            turn = syn.rot_vec(axis / np.linalg.norm(axis) * np.arctan2(np.linalg.norm(axis), -d[2]))
            pose = syn.make_pose(turn, np.array([0.0, 0.0, 0.08])).astype(np.float32)
            z = ref._corners(pose.astype(np.float64), lo, hi)[:, 2]
            assert z.min() < -0.01 and z.max() > 0.1  # (the case is what it says)
        inputs.start[i] = pose.copy()
        frame = inputs.scenes[i].background.copy() if i == 10 else inputs.scenes[i].render(pose)
        for k in range(inputs.n_frames):
            inputs.gt[i][k] = pose.copy()
            inputs.color[i][k] = frame
    inputs.camera_of = list(RECT_CAMERA_OF)
    for a, b in ((6, 7), (8, 9)):
        inputs.color[b] = inputs.color[a]
    return inputs


def strip_pose(box, pose, intr, reach_px, side):
    """CPU search over the reference: the body slid out of the frame on `side` until the rectangle of a reader of
    reach_px (no margin) is a strip of 2 columns / rows at that edge"""
    w, h = intr["width"], intr["height"]
    for d in np.arange(0.0, 400.0, 0.25):
        p = {"left": placed(pose, intr, -d, 0.5 * h), "right": placed(pose, intr, w + d, 0.5 * h),
             "top": placed(pose, intr, 0.5 * w, -d), "bottom": placed(pose, intr, 0.5 * w, h + d)}[side].astype(np.float32)
        r = ref.nominal(p, box, intr, reach_px, 0.0)
        n = {"left": r[2] + 1, "right": w - r[0], "top": r[3] + 1, "bottom": h - r[1]}[side]
        if n == 2:
            return p
    raise AssertionError("no pose found for a strip on the %s" % side)


def small_inputs():
    """6 static bodies, a camera of 100 x 52 each: strips at the left, right, top, bottom edge, an empty rectangle,
    the whole frame"""
    inputs = scenes.Inputs(6, 3, n_divides=2, n_models=3, intr=SMALL)
    intr = inputs.intr
    reach = ref.region_color_reach(capi.RegionModalityParams(**syn.RBOT_REGION_PARAMS), syn.RBOT_TRACKER["n_corr_iterations"])
    for i, side in enumerate(["left", "right", "top", "bottom", "far", "mid"]):
        box = box_of(inputs.region_models[inputs.model_of[i]][0])
        pose = inputs.gt[i][0].astype(np.float32)
        if side == "far":
            pose = placed(pose, intr, intr["width"] + 900.0, 20.0).astype(np.float32)
        elif side == "mid":
            pose = placed(pose, intr, 48.0, 27.0).astype(np.float32)
        else:
            pose = strip_pose(box, pose, intr, reach, side)
        inputs.start[i] = pose.copy()
        frame = inputs.scenes[i].render(pose)
        for k in range(inputs.n_frames):
            inputs.gt[i][k] = pose.copy()
            inputs.color[i][k] = frame
    return inputs


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def aligned_bytes(shape):
    """a zeroed uint8 array whose data starts on a 64-byte boundary (the pull reads 16 bytes at a time)"""
    n = int(np.prod(shape))
    raw = np.zeros(n + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n].reshape(shape)


class Group:
    """the cameras of one kind in a run: one batch ring, one host block per frame in the ring's layout (rows of
    `row_step` bytes, of which `row` are image and the rest padding filled with noise), and its poison twin"""

    def __init__(self, hip, inst, cams, frames, bytes_per_pixel, n_frames, rng):
        self.cams, self.first = [], []  # the distinct cameras, and the first object that looks through each
        for i, cam in enumerate(cams):
            if cam.id not in [c.id for c in self.cams]:
                self.cams.append(cam)
                self.first.append(i)
        self.n, self.bpp = len(self.cams), bytes_per_pixel
        self.h, self.w = frames[0][0].shape[:2]
        self.row = self.w * bytes_per_pixel
        self.row_step = (self.row + 63) // 64 * 64
        self.true, self.poison, self.mixed = [], [], []
        for k in range(n_frames):
            blocks = []
            for kind in ("true", "poison", "mixed"):
                b = aligned_bytes((self.n, self.h, self.row_step))
                b[:, :, self.row:] = rng.integers(0, 256, (self.n, self.h, self.row_step - self.row), dtype=np.uint8)
                inst.tracker.register_host_buffer(b)
                blocks.append(b)
            for j, i in enumerate(self.first):
                f = np.ascontiguousarray(frames[i][k])
                p = 255 - f if bytes_per_pixel == 3 else (f // 2 + 1).astype(f.dtype)
                assert np.all(p != f)
                blocks[0][j, :, :self.row] = f.view(np.uint8).reshape(self.h, self.row)
                blocks[1][j, :, :self.row] = p.view(np.uint8).reshape(self.h, self.row)
            blocks[2][...] = blocks[1]
            self.true.append(blocks[0])
            self.poison.append(blocks[1])
            self.mixed.append(blocks[2])
        self.ids = (C.c_int * self.n)(*[c.id for c in self.cams])
        hip.call("cameras_set_ring", self.ids, self.n, 2)

    def upload(self, hip, entry, slot, block):
        hip.call(entry, self.ids, self.n, slot, block.ctypes.data_as(C.c_void_p), block.strides[0], block.strides[1])

    def rectangles(self, hip, slot):
        out = np.zeros((self.n, 4), np.int32)
        hip.call("roi_get_rectangles", self.ids, self.n, slot, out.ctypes.data_as(C.POINTER(C.c_int)))
        return [tuple(int(x) for x in r) for r in out]

    def download(self, hip, slot):
        out = np.zeros((self.n, self.h, self.row), np.uint8)
        for j, cam in enumerate(self.cams):
            hip.call("camera_download_slot", cam.id, slot, out[j].ctypes.data_as(C.c_void_p), self.row)
        return out


class Run:
    pass


def read_list(hip, entry):
    bodies = (C.c_int * 64)()
    n = C.c_int(0)
    if entry == "roi_get_status":
        pulls = C.c_longlong(0)
        hip.call(entry, bodies, 64, C.byref(n), C.byref(pulls))
        return list(bodies[:min(n.value, 64)]), pulls.value
    hip.call(entry, bodies, 64, C.byref(n))
    return list(bodies[:min(n.value, 64)])


def blocking(inputs, with_depth=False, region_params=None, world2camera=None, n_frames=None):
    """the whole-frame hand-over: true frames only"""
    hip = util.open_hip()
    inst = scenes.Instance(hip, inputs, use_depth=with_depth, region_params=region_params)
    set_cameras(inst, world2camera)
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    out = []
    for k in range(1, n_frames or inputs.n_frames):
        inst.upload_frame(k)
        assert inst.tracker.ExecuteTrackingStep(k)
        out.append(np.stack(inst.poses()))
    return out


def set_cameras(inst, world2camera):
    if world2camera is not None:
        for i, (cam, dcam) in enumerate(zip(inst.color_cams, inst.depth_cams)):
            cam.set_world2camera_pose(world2camera[i])
            if dcam is not None:
                dcam.set_world2camera_pose(world2camera[i])


def roi(inputs, margin=24.0, with_depth=False, adaptive=False, expect_kernel=None, region_params=None, inspect=False,
        control=False, world2camera=None, n_frames=None, before_step=None, after_step=None, last_step_guarded=True):
    """the loop of test_gpu_roi.run with every slot poisoned before its rectangle arrives.  inspect: after every
    upload, the device's rectangles and the slots' bytes are read back (run.uploads).  control: the ROI upload's source
    is true only inside every body's projected box (reach 0, no margin) at the pose the step that reads it starts from"""
    n_frames = n_frames or inputs.n_frames
    run = Run()
    run.hip = hip = util.open_hip()
    run.inst = inst = scenes.Instance(hip, inputs, use_depth=with_depth, region_params=region_params)
    set_cameras(inst, world2camera)
    hip.call("set_roi_ingest", 2 if adaptive else 1, C.c_float(margin))
    rng = np.random.default_rng(17)
    run.groups = [Group(hip, inst, inst.color_cams, inputs.color, 3, n_frames, rng)]
    if with_depth:
        run.groups.append(Group(hip, inst, inst.depth_cams, inputs.depth, 2, n_frames, rng))
    # the readers of every camera, as BuildRoiTables forms them: (object, box, reach_px, reach_m)
    rp = dict(region_params or (syn.YCB_REGION_PARAMS if inputs.with_depth else syn.RBOT_REGION_PARAMS))
    if not inputs.with_depth:
        rp["measure_occlusions"] = 0
    rp, dp = capi.RegionModalityParams(**rp), capi.DepthModalityParams(**syn.YCB_DEPTH_PARAMS)
    n_corr = (syn.YCB_TRACKER if inputs.with_depth else syn.RBOT_TRACKER)["n_corr_iterations"]
    run.margin, run.intr = margin, inputs.intr
    run.w2c = [np.eye(4) if world2camera is None else np.asarray(world2camera[i], np.float64) for i in range(inputs.n_objects)]
    run.region_box = [box_of(inputs.region_models[inputs.model_of[i]][0]) for i in range(inputs.n_objects)]
    run.readers = []  # [group][camera of the group] -> [(object, box, reach_px, reach_m)]
    for g, group in enumerate(run.groups):
        cams = inst.color_cams if g == 0 else inst.depth_cams
        per_cam = []
        for cam in group.cams:
            readers = []
            for i in range(inputs.n_objects):
                if cams[i].id != cam.id:
                    continue
                if g == 0:
                    readers.append((i, run.region_box[i], ref.region_color_reach(rp, n_corr), 0.0))
                else:
                    if rp.measure_occlusions:
                        m, px = ref.region_depth_reach(rp)
                        readers.append((i, run.region_box[i], px, m))
                    m, px = ref.depth_reach(dp, inputs.intr["fu"])
                    readers.append((i, box_of(inputs.depth_models[inputs.model_of[i]][0]), px, m))
            per_cam.append(readers)
        run.readers.append(per_cam)
    run.poses, run.starts, run.uploads, run.misses, run.pulls = [], [], [], {}, 0

    def upload(slot, k, poses_at_read):
        for g, group in enumerate(run.groups):
            source = group.true[k]
            if control and k > 1:  # (the first upload goes as whole frames: true ones)
                source = group.mixed[k]
                for j, readers in enumerate(run.readers[g]):
                    for i, box, _, _ in readers:
                        r, _ = ref.body_bounds(run.w2c[i] @ poses_at_read[i].astype(np.float64), box, inputs.intr, 0.0, 0.0)
                        if r is not None:
                            b0, b1 = r[0] * group.bpp, (r[2] + 1) * group.bpp
                            source[j, r[1]:r[3] + 1, b0:b1] = group.true[k][j, r[1]:r[3] + 1, b0:b1]
            group.upload(hip, "cameras_upload_batch_async", slot, group.poison[k])
            group.upload(hip, "cameras_upload_batch_roi_async", slot, source)
            _, pulls = read_list(hip, "roi_get_status")  # (no step since the last read: the miss list is empty)
            # all uploads but the first (no step recorded yet) still went as rectangles, behind the poison
            assert pulls == run.pulls + (1 if k > 1 else 0), (k, g, pulls, run.pulls)
            run.pulls = pulls
        if inspect:
            run.uploads.append(dict(k=k, slot=slot, start=run.starts[-1] if run.starts else None,
                                    prev=run.starts[-2] if len(run.starts) > 1 else None,
                                    rects=[group.rectangles(hip, slot) for group in run.groups] if k > 1 else None,
                                    bytes=[group.download(hip, slot) for group in run.groups]))

    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0)
    upload(1, 1, inputs.start)  # (no step recorded yet: goes as whole frames)
    for k in range(1, n_frames):
        inst.tracker.select_slot(k % 2)
        run.starts.append(np.stack(inst.poses()))
        if before_step:
            before_step(run, k)
        assert inst.tracker.ExecuteTrackingStep(k)
        run.misses[k], _ = read_list(hip, "roi_get_status")
        if after_step:
            after_step(run, k)
        run.poses.append(np.stack(inst.poses()))
        if k + 1 < n_frames:
            upload((k + 1) % 2, k + 1, run.poses[-1])
    inst.tracker.ingest_sync()
    run.unrecovered = read_list(hip, "roi_get_unrecovered")
    kernel = C.create_string_buffer(128)
    hip.call("get_step_kernel", kernel, 128)
    run.kernel = kernel.value.decode()
    assert ("_guard_kernel" in run.kernel) == last_step_guarded, run.kernel  # the last step read rectangles
    assert expect_kernel is None or run.kernel == expect_kernel, run.kernel
    return run


def assert_bit_for_bit(got, expect):
    assert len(got) == len(expect)
    for k, (a, b) in enumerate(zip(got, expect)):
        assert np.array_equal(a, b), ("frame", k + 1, np.abs(a - b).max(axis=(1, 2)))


# ---- (c) and (d): what an inspected run recorded, against the reference --------------------------------------------------------
def margins_of(run, adaptive, moved_error=0.0):
    """[upload][group][camera][reader] -> margin in pixels"""
    rect_uploads = [u for u in run.uploads if u["rects"] is not None]
    out = [[[[run.margin] * len(readers) for readers in per_cam] for per_cam in run.readers] for _ in rect_uploads]
    if adaptive:
        for g, per_cam in enumerate(run.readers):
            for j, readers in enumerate(per_cam):
                for q, (i, box, px, m) in enumerate(readers):
                    poses = [(None if u["prev"] is None else run.w2c[i] @ u["prev"][i].astype(np.float64),
                              run.w2c[i] @ u["start"][i].astype(np.float64)) for u in rect_uploads]
                    for n, margin in enumerate(ref.adaptive_margins(poses, box, run.intr, px, m, run.margin, moved_error)):
                        out[n][g][j][q] = margin
    return out


def check_rectangles(run, adaptive=False):
    """(c): R_min within the device's rectangle within R_max for every camera after every rectangle upload; returns the
    device's rectangles [upload][group][camera] (None: empty).  Adaptive margins: R_min with the margins for a motion one
    pixel below the reference's, R_max for one pixel above (roi_reference.adaptive_margins)"""
    small, large = margins_of(run, adaptive, -1.0), margins_of(run, adaptive, 1.0)
    rect_uploads = [u for u in run.uploads if u["rects"] is not None]
    assert rect_uploads
    for n, u in enumerate(rect_uploads):
        for g, per_cam in enumerate(run.readers):
            for j, readers in enumerate(per_cam):
                lo, hi = [ref.camera_bounds([(run.w2c[i] @ u["start"][i].astype(np.float64), box, px + margins[n][g][j][q], m)
                                             for q, (i, box, px, m) in enumerate(readers)], run.intr)[side]
                          for side, margins in enumerate((small, large))]
                dev = ref.of_device(u["rects"][g][j])
                assert ref.contains(dev, lo), ("too small", u["k"], g, j, u["rects"][g][j], lo)
                assert ref.contains(hi, dev), ("too large", u["k"], g, j, u["rects"][g][j], hi)
    return [[[ref.of_device(r) for r in group] for group in u["rects"]] for u in rect_uploads]


def check_pulled_bytes(run):
    """(d): every slot, byte for byte, is the composite of the poison it held and the true block, by the device's own
    rectangle -- which also says that no padding byte of the host block shows up inside a row's width * bytes_per_pixel"""
    for u in run.uploads:
        for g, group in enumerate(run.groups):
            for j in range(group.n):
                rect = ref.full(run.intr) if u["rects"] is None else ref.of_device(u["rects"][g][j])
                expect = ref.pull_composite(group.poison[u["k"]][j][:, :group.row], group.true[u["k"]][j], rect, group.bpp)
                assert np.array_equal(u["bytes"][g][j], expect), (u["k"], g, j, rect, np.argwhere(u["bytes"][g][j] != expect)[:4])


# ---- (a) poisoned sequences ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _motion(kind):
    return motion_inputs(kind)


@pytest.mark.parametrize("kind", ["steady", "runaway", "approach", "rotate", "drift", "shared"])
@pytest.mark.parametrize("shape", list(KERNELS))
def test_poisoned_sequences_track_like_whole_frames(shape, kind, monkeypatch):
    """every slot poisoned outside what the pull lands: the poses of all bodies are those of the blocking whole-frame
    run bit for bit, nobody is left unrecovered; the sideways runaway -- alone in its camera or sharing it -- is named
    by roi_get_status, and only it (the body it shares the camera with stays committed while the camera is repaired).
    What poses cannot show: a reach that is a few pixels short in the rectangle AND the guard alike.  The guard takes
    the longest reach (49.5 pixels, the scale-5 lines of the first search) at every pose of the step, and the box /
    ellipsoid bound over-estimates the contour: on the oracle, with a body that jumps 23 pixels in one frame, poison
    only changes a pose once the rectangles are cut by 12 (downwards) to 16 (sideways) pixels.  The rectangle tests
    below pin the reach to the pixel instead"""
    env, kernel, params = KERNELS[shape]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    inputs = _motion(kind)
    expect = blocking(inputs, region_params=params)
    run = roi(inputs, margin=24.0, region_params=params, expect_kernel=kernel)
    missed = sorted({b for bodies in run.misses.values() for b in bodies})
    assert run.unrecovered == [], run.misses
    assert_bit_for_bit(run.poses, expect)
    if kind == "drift":  # the premise: part of the body is outside the frame in the last four frames, and it is tracked
        for k in range(3, inputs.n_frames):
            v = inputs.vertices[0] @ inputs.gt[0][k][:3, :3].T + inputs.gt[0][k][:3, 3]
            u = v[:, 0] * inputs.intr["fu"] / v[:, 2] + inputs.intr["ppu"]
            assert u.min() < 0.0 < u.max() and np.mean(u < 0.0) < 0.5, (k, u.min(), u.max())
        e = syn.pose_errors(run.poses[-1][0], inputs.gt[0][-1])
        assert e[1] < 0.03, e
    if kind == "steady":
        assert missed == []
    if kind in ("runaway", "shared"):
        assert missed == [1]  # body ids are creation order
        e = syn.pose_errors(run.poses[-1][1], inputs.gt[1][-1])
        assert e[1] < 0.02, e  # the runaway was tracked: the repeated steps saw its frames


def test_poisoned_region_and_depth():
    """Region + Depth with the YCB parameters (measured occlusions, the metre reach) on the split kernel: the slots of
    both cameras of every object are poisoned -- the depth poison lies in front of the scene"""
    inputs = scenes.Inputs(3, 6, n_divides=2, with_depth=True)
    expect = blocking(inputs, with_depth=True)
    run = roi(inputs, with_depth=True, expect_kernel="tracking_step_split_guard_kernel")
    assert run.unrecovered == [] and run.pulls >= 2 * (inputs.n_frames - 2)
    assert_bit_for_bit(run.poses, expect)


def test_poisoned_sequence_without_a_margin():
    """margin 0: the rectangle is the reach around the pose of two steps ago and nothing more, so whatever moves by a
    pixel fails the guard and is repeated on its whole frame -- the poses stay those of whole frames, repairs in most
    steps"""
    inputs = _motion("steady")
    run = roi(inputs, margin=0.0, expect_kernel="tracking_step_split_guard_kernel")
    assert run.unrecovered == [] and any(run.misses.values()), run.misses
    assert_bit_for_bit(run.poses, blocking(inputs))


@pytest.mark.parametrize("kind", ["steady", "runaway"])
def test_poisoned_adaptive_margins(kind):
    """set_roi_ingest(2, 48): per-body margins from the rectangles' motion, on the split kernel"""
    inputs = _motion(kind)
    expect = blocking(inputs)
    run = roi(inputs, margin=48.0, adaptive=True, expect_kernel="tracking_step_split_guard_kernel")
    assert run.unrecovered == []
    assert_bit_for_bit(run.poses, expect)


# ---- (b) the control -------------------------------------------------------------------------------------------------------------
def test_control_poison_outside_the_projected_boxes_changes_the_poses():
    """what (a) rests on: frames that are true only inside every body's projected box at the step's start pose (the
    reference at reach 0, no margin) and poison elsewhere -- the far ends of the correspondence and histogram lines lie
    in the poison -- do NOT give the whole-frame poses.  The guard still passes: the rectangle table is the device's"""
    inputs = _motion("steady")
    expect = blocking(inputs)
    run = roi(inputs, control=True)
    differs = [k + 1 for k, (a, b) in enumerate(zip(run.poses, expect)) if not np.array_equal(a, b)]
    assert differs, "the poison is not being read: the poisoned sequences prove nothing"
    assert 1 not in differs  # (the first step read whole true frames)


# ---- (c) rectangles, (d) pulled bytes ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rect_run():
    inputs = rect_inputs()
    return inputs, roi(inputs, inspect=True)


def test_rectangles_at_the_frame_edges(rect_run):
    """(c) mid-frame, clipped at each edge, off the frame alone and beside an on-frame reader, behind and across the
    camera plane"""
    inputs, run = rect_run
    full = ref.full(inputs.intr)
    for rects in check_rectangles(run):
        color = rects[0]  # cameras in RECT_CAMERA_OF's order
        assert color[0] is not None and color[0][0] > 0 and color[0][1] > 0 and color[0][2] < full[2] and color[0][3] < full[3]
        assert color[1][0] == 0 and color[1][2] < 320 and color[2][2] == full[2] and color[2][0] > 320
        assert color[3][1] == 0 and color[3][3] < 256 and color[4][3] == full[3] and color[4][1] > 256
        assert color[5] is None  # wholly off the frame, alone in its camera
        assert color[8] == full and color[9] == full  # the box lies behind / reaches across the camera plane
        # an off-frame reader leaves the on-frame reader's rectangle alone (m3t_roi_union skips an empty operand; it
        # used to stretch the camera's rectangle to the right / bottom edge -- R_max above fails on that)
        assert color[6][2] < full[2] and color[7][3] < full[3]


def test_rectangles_track_like_whole_frames_at_the_frame_edges(rect_run):
    inputs, run = rect_run
    assert run.unrecovered == [] and all(m == [] for m in run.misses.values()), run.misses
    assert_bit_for_bit(run.poses, blocking(inputs))
    for i in (5, 7, 9, 10):  # no pixel to work with: these bodies stay where they were
        assert all(np.array_equal(p[i], run.starts[0][i]) for p in run.poses), i


def test_pulled_bytes_of_colour_frames(rect_run):
    """(d) 640 x 512 x 3: rectangles of every kind in one launch, among them the whole frame as a rectangle (64 bands of
    8 rows x 120 chunks: two trips of the 512-stride loop) and an empty one, whose slot stays the poison byte for byte"""
    inputs, run = rect_run
    check_pulled_bytes(run)
    for u in run.uploads[1:]:
        for j in (8, 9):
            assert ref.of_device(u["rects"][0][j]) == ref.full(inputs.intr)
            assert np.array_equal(u["bytes"][0][j], run.groups[0].true[u["k"]][j][:, :run.groups[0].row])
        assert ref.of_device(u["rects"][0][5]) is None
        assert np.array_equal(u["bytes"][0][5], run.groups[0].poison[u["k"]][5][:, :run.groups[0].row])


@pytest.fixture(scope="module")
def depth_run():
    inputs = scenes.Inputs(3, 4, n_divides=2, with_depth=True)
    return inputs, roi(inputs, with_depth=True, inspect=True)


def test_rectangles_and_pulled_bytes_of_region_and_depth_readers(depth_run):
    """(c) two readers with different reaches on every depth camera (the RegionModality's measured occlusions: 1.1 cm;
    the DepthModality: 7.7 cm, both in metres at the box's nearest depth), (d) u16 frames"""
    inputs, run = depth_run
    assert [len(r) for r in run.readers[0]] == [1, 1, 1] and [len(r) for r in run.readers[1]] == [2, 2, 2]
    check_rectangles(run)
    check_pulled_bytes(run)
    assert run.unrecovered == []


def test_rectangles_under_a_world2camera_pose():
    """(c) cameras that are not at the world's origin: the rectangle is that of world2camera x body2world"""
    inputs = scenes.Inputs(3, 4, n_divides=2)
    w2c = [syn.make_pose(syn.rot_vec(np.array(r)), np.array(t)).astype(np.float32)
           for r, t in (((0.2, -0.1, 0.3), (0.1, -0.2, 0.05)), ((-0.4, 0.25, 0.0), (-0.3, 0.0, 0.2)), ((0.0, 0.0, 1.2), (0.0, 0.4, -0.1)))]
    for i in range(3):  # the same body2camera poses as before, up to f32 rounding
        inputs.start[i] = (np.linalg.inv(w2c[i].astype(np.float64)) @ inputs.start[i]).astype(np.float32)
    run = roi(inputs, inspect=True, world2camera=w2c)
    rects = check_rectangles(run)
    assert all(r is not None and ref.area(r) < ref.area(ref.full(inputs.intr)) for u in rects for r in u[0])
    check_pulled_bytes(run)
    assert_bit_for_bit(run.poses, blocking(inputs, world2camera=w2c))


def adaptive_inputs():
    """7 frames; object 0 lies just off the frame on the left and does not move (no line of it is valid): its rectangle
    is a strip at the left edge whose motion is 0 -- the margin's floor --; object 1 is the sideways runaway: the cap"""
    inputs = motion_inputs("runaway")
    intr = inputs.intr
    box = box_of(inputs.region_models[inputs.model_of[0]][0])
    pose = inputs.gt[0][0].astype(np.float32)
    for d in np.arange(0.0, 400.0, 1.0):  # slid out until the body's own outline ends 8 pixels left of the frame
        p = placed(pose, intr, -d, 250.0).astype(np.float32)
        if ref.nominal(p, box, intr, -1.0, 0.0)[2] < -8 + 1:
            break
    inputs.start[0] = p.copy()
    frame = inputs.scenes[0].render(p)
    for k in range(inputs.n_frames):
        inputs.gt[0][k] = p.copy()
        inputs.color[0][k] = frame
    return inputs


def test_adaptive_margin_sequence_floor_and_cap():
    """(c) the adaptive sequence: the margins of roi_rect_kernel restated from the recorded start poses -- whole margin
    while the motion is unknown, then max(2 m, 1.25 peak) + 3 in [4, 48] -- bracket the device's rectangles in every
    frame; the sequence holds a frame at the floor and one at the cap"""
    inputs = adaptive_inputs()
    run = roi(inputs, margin=48.0, adaptive=True, inspect=True)
    margins = margins_of(run, adaptive=True)
    assert len(margins) == 5
    assert [m[0][0][0] for m in margins][:2] == [48.0, 48.0] and 4.0 in [m[0][0][0] for m in margins][2:]  # the floor
    assert 48.0 in [m[0][1][0] for m in margins][2:] and min(m[0][1][0] for m in margins) < 48.0           # the cap
    rects = check_rectangles(run, adaptive=True)
    # the strip of object 0 shrinks with its margin: 44 pixels narrower at the floor than at the cap
    widths = [u[0][0][2] + 1 for u in rects]
    assert widths[0] - min(widths) == 44, widths
    check_pulled_bytes(run)
    assert run.unrecovered == []
    assert_bit_for_bit(run.poses, blocking(inputs))


def test_pulled_bytes_of_a_small_camera():
    """(d) 100 x 52 x 3: rows of 300 bytes (no multiple of 16) in a pitch of 320, 6 bands of 8 rows and one of 4.  Six
    cameras in one launch: strips of 2 columns at the left and the right edge (the 16-byte widening lands 16 / 12 bytes
    of each row), 2 rows at the top and the bottom edge, an empty rectangle, the whole frame.  The poses come from a CPU
    search over the reference; margin 0"""
    inputs = small_inputs()
    run = roi(inputs, margin=0.0, inspect=True)
    rects = check_rectangles(run)
    w, h = inputs.intr["width"], inputs.intr["height"]
    for color in (u[0] for u in rects):
        assert color[0][0] == 0 and 1 <= color[0][2] + 1 <= 3, color[0]
        assert color[1][2] == w - 1 and 1 <= w - color[1][0] <= 3, color[1]
        assert color[2][1] == 0 and 1 <= color[2][3] + 1 <= 3, color[2]
        assert color[3][3] == h - 1 and 1 <= h - color[3][1] <= 3, color[3]
        assert color[4] is None and color[5] == ref.full(inputs.intr), (color[4], color[5])
    check_pulled_bytes(run)
    assert run.unrecovered == []
    assert_bit_for_bit(run.poses, blocking(inputs))


# ---- (e) repair ------------------------------------------------------------------------------------------------------------------
def test_repair_fetches_the_runaways_whole_frame_and_nothing_else():
    """after the first step the runaway misses in: its slot is its whole true frame and its rectangle the frame; the
    other two slots still are their pull composites, poison outside.  A second step on the same slots finds the
    repaired camera's rectangle in order: no miss"""
    inputs = _motion("runaway")
    seen = {}

    def after_step(run, k):
        if run.misses[k] and not seen:
            slot, group = k % 2, run.groups[0]
            seen.update(k=k, misses=run.misses[k], rects=group.rectangles(run.hip, slot), bytes=group.download(run.hip, slot),
                        before=run.uploads[-1])
            assert run.inst.tracker.ExecuteTrackingStep(k)  # the same slots once more
            seen["again"], _ = read_list(run.hip, "roi_get_status")

    run = roi(inputs, inspect=True, after_step=after_step, n_frames=5)
    assert seen and seen["misses"] == [1], (seen.get("misses"), run.misses)
    k, group, before = seen["k"], run.groups[0], seen["before"]
    assert before["k"] == k and before["slot"] == k % 2
    full = ref.full(inputs.intr)
    assert ref.of_device(before["rects"][0][1]) != full  # it was a rectangle when the step began
    assert seen["rects"][1] == full
    assert np.array_equal(seen["bytes"][1], group.true[k][1][:, :group.row])
    for j in (0, 2):
        assert seen["rects"][j] == before["rects"][0][j] and ref.of_device(seen["rects"][j]) != full
        assert np.array_equal(seen["bytes"][j], before["bytes"][0][j])
        outside = np.ones((group.h, group.row), bool)
        b0, b1 = ref.pull_span(seen["rects"][j], group.bpp)
        outside[seen["rects"][j][1]:seen["rects"][j][3] + 1, b0:b1] = False
        assert np.array_equal(seen["bytes"][j][outside], group.poison[k][j][:, :group.row][outside])
    assert seen["again"] == []
    assert run.unrecovered == []


# ---- (f) unrecovered ----------------------------------------------------------------------------------------------------------
def test_unrecovered_bodies_are_named_and_recovered_by_a_whole_frame_upload():
    """The state of m3t_hip_roi_get_unrecovered IS reachable through public calls: m3t_hip_camera_set_world2camera_pose
    (here: with the pose the camera already has) marks the context's tables dirty (tables_dirty, m3t_hip_api.hip).  Called
    between the rectangle upload of frame k and step k, it makes the step rebuild the ROI tables: the rebuilt rectangle
    table cannot vouch for a slot that holds a rectangle (it says "empty"), and the host blocks of the uploads are
    forgotten.  Every body that reads such a slot fails the guard, no whole frame can be fetched, the repeat fails too:
    the runaway -- whose step is the one that outruns its rectangle in the undisturbed sequence -- is named, and so are
    the other bodies of rectangle slots; nobody's step is committed.  The documented way out -- the whole frames by
    camera_upload_slot, then the step again -- gives the poses of the blocking run for all bodies"""
    inputs = _motion("runaway")
    expect = blocking(inputs)
    undisturbed = roi(inputs)
    k_miss = min(k for k, bodies in undisturbed.misses.items() if bodies)
    seen = {}

    def before_step(run, k):
        if k == k_miss:
            run.inst.color_cams[1].set_world2camera_pose(np.eye(4))

    def after_step(run, k):
        if k == k_miss:
            seen["unrecovered"] = sorted(read_list(run.hip, "roi_get_unrecovered"))
            seen["poses"] = np.stack(run.inst.poses())
            for i, cam in enumerate(run.inst.color_cams):
                f = inputs.color[i][k]
                run.hip.call("camera_upload_slot", cam.id, k % 2, f.ctypes.data_as(C.c_void_p), f.strides[0])
            assert run.inst.tracker.ExecuteTrackingStep(k)
            seen["unrecovered after"] = read_list(run.hip, "roi_get_unrecovered")

    run = roi(inputs, before_step=before_step, after_step=after_step, n_frames=k_miss + 1, last_step_guarded=False)
    assert 1 in seen["unrecovered"] and seen["unrecovered"] == [0, 1, 2], seen["unrecovered"]
    assert np.array_equal(seen["poses"], run.starts[-1])  # the poses from before the step
    assert seen["unrecovered after"] == []
    assert_bit_for_bit(run.poses, expect[:k_miss])


def test_read_backs_refuse_what_they_cannot_answer():
    """roi_get_rectangles without ROI tables (ROI ingest off; on, but no step has built the tables), with a bad camera
    id or slot; camera_download_slot with a bad id, slot or row step"""
    inputs = _motion("steady")
    hip = util.open_hip()
    inst = scenes.Instance(hip, inputs)
    ids, out = (C.c_int * 1)(inst.color_cams[0].id), (C.c_int * 4)()
    assert hip.raw("roi_get_rectangles", ids, 1, 0, out) == capi.M3T_ERR_UNSUPPORTED
    hip.call("set_roi_ingest", 1, C.c_float(24.0))
    assert hip.raw("roi_get_rectangles", ids, 1, 0, out) == capi.M3T_ERR_UNSUPPORTED
    inst.upload_frame(0)
    assert inst.tracker.StartModalities(0) and inst.tracker.ExecuteTrackingStep(0)
    assert hip.raw("roi_get_rectangles", ids, 1, 0, out) == 0 and tuple(out) == ref.full(inputs.intr)
    assert hip.raw("roi_get_rectangles", ids, 1, 1, out) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("roi_get_rectangles", ids, 1, -1, out) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("roi_get_rectangles", (C.c_int * 1)(99), 1, 0, out) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("roi_get_rectangles", (C.c_int * 1)(-1), 1, 0, out) == capi.M3T_ERR_INVALID_ARGUMENT
    h, w = inputs.color[0][0].shape[:2]
    pixels = np.zeros((h, w * 3), np.uint8)
    p = pixels.ctypes.data_as(C.c_void_p)
    assert hip.raw("camera_download_slot", 99, 0, p, w * 3) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("camera_download_slot", ids[0], 1, p, w * 3) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("camera_download_slot", ids[0], 0, p, w * 3 - 1) == capi.M3T_ERR_INVALID_ARGUMENT
    assert hip.raw("camera_download_slot", ids[0], 0, p, w * 3) == 0
    assert np.array_equal(pixels, inputs.color[0][0].reshape(h, w * 3))
