"""Host-side mirror of the reference's object graph for the hot path.

Same class and method names as M3T (Body, ColorCamera, DepthCamera,
RegionModel, DepthModel, RegionModality, DepthModality, Link, Optimizer,
Constraint, Tracker with StartModalities / CalculateCorrespondences /
CalculateGradientAndHessian / CalculateOptimization / CalculateResults /
ExecuteTrackingStep; M3T/include/m3t/tracker.h:131-160), but every object is a
handle into ONE batched device context behind the C-ABI: a Tracker call runs
the step for all registered modalities in one launch sequence.

Error behaviour follows the reference: steps return bool (False + message on
stderr when something is not set up), constructors raise on invalid arguments.
"""
import ctypes as C
import sys

import numpy as np

from . import _capi
from ._capi import (DATA_LINE_DTYPE, DATA_POINT_DTYPE, M3T_MAX_TEXTURE_FEATURES, M3T_MAX_TEXTURE_KEYFRAMES,
                    TEXTURE_DATA_POINT_DTYPE, DepthModalityParams, DepthModelDesc, Intrinsics, M3TError,
                    RegionModalityParams, RegionModelDesc, TextureDetectorParams, TextureModalityParams, fptr, iptr, pose_arg, pose_ret)


class Tracker:
    """m3t::Tracker restricted to the tracking step (tracker.cpp:344-364, 430-517)."""

    def __init__(self, api, n_corr_iterations=5, n_update_iterations=2):
        self.api = api
        self.n_corr_iterations = n_corr_iterations
        self.n_update_iterations = n_update_iterations
        api.call("tracker_set_iterations", n_corr_iterations, n_update_iterations)

    def _step(self, name, *args):
        rc = self.api.raw(name, *args)
        if rc < 0:
            sys.stderr.write(self.api.last_error() + "\n")
            return False
        return True

    def StartModalities(self, iteration):
        return self._step("start_modalities", iteration)

    def CalculateCorrespondences(self, iteration, corr_iteration):
        return self._step("calculate_correspondences", iteration, corr_iteration)

    def CalculateGradientAndHessian(self, iteration, corr_iteration, update_iteration):
        return self._step("calculate_gradient_and_hessian", iteration, corr_iteration, update_iteration)

    def CalculateOptimization(self, iteration, corr_iteration, update_iteration):
        return self._step("calculate_optimization", iteration, corr_iteration, update_iteration)

    def CalculateResults(self, iteration):
        return self._step("calculate_results", iteration)

    def CalculateConsistentPoses(self):
        return self._step("calculate_consistent_poses")

    def CalculateOptimizationBegin(self):
        """first half of CalculateOptimization: the link sums of this process's modalities, 6 + 36 floats per link.
        Returns (pointer, count); device pointer for the HIP library, host pointer for the oracle."""
        ptr = _capi.c_float_p()
        n = C.c_size_t()
        self.api.call("calculate_optimization_begin", C.byref(ptr), C.byref(n))
        return ptr, n.value

    def CalculateOptimizationEnd(self):
        return self._step("calculate_optimization_end")

    def ExecuteTrackingStep(self, iteration):
        return self._step("execute_tracking_step", iteration)

    def ResetBodies(self, bodies, poses=None, iteration=0):
        """RBOTEvaluator::ResetBody (rbot_evaluator.cpp:334-352) for `bodies` alone, in one call (HIP library only):
        their poses (None: the poses stay), the start-modality renderers their modalities read, StartModality of their
        texture modalities that have the built-in detector (detection on the current frame at the new pose, then a
        keyframe; a texture modality fed through SetFeatures is refused) and StartModality(iteration) of their region
        modalities; every other body keeps its state bit for bit"""
        ids = np.asarray([b.id for b in bodies], np.int32)
        flat = None
        if poses is not None:
            assert len(poses) == len(ids)
            flat = np.ascontiguousarray(np.concatenate([pose_arg(p) for p in poses]) if len(ids) else
                                        np.zeros(0, np.float32), np.float32)
        if "reset_bodies" not in self.api._fn:
            raise M3TError(-3, "%sreset_bodies: this entry point exists in the HIP library only" % self.api.prefix)
        return self._step("reset_bodies", iptr(ids), fptr(flat) if flat is not None else None, len(ids), iteration)

    def ResetStructures(self, optimizers, poses, mode=0, iteration=0):
        """RTBEvaluator::SetBodyAndJointPoses (rtb_evaluator.cpp:809-858) + StartModalities(iteration) for the
        kinematic structures `optimizers` alone, in one call (HIP library only).  `poses`: one body2world pose per link
        that has a body, concatenated over the optimizers in each one's depth-first link order; mode 0: independent /
        projected, 1: constrained (body-less root, the poses start at its children).  Every other structure keeps its
        state bit for bit (m3t_hip_reset_structures)."""
        ids = np.asarray([o.id for o in optimizers], np.int32)
        flat = np.ascontiguousarray(np.concatenate([pose_arg(p) for p in poses]) if len(poses) else
                                    np.zeros(0, np.float32), np.float32)
        if "reset_structures" not in self.api._fn:
            raise M3TError(-3, "%sreset_structures: this entry point exists in the HIP library only" % self.api.prefix)
        return self._step("reset_structures", iptr(ids), len(ids), fptr(flat), int(mode), int(iteration))

    def CreateJudge(self, bodies, n_rows_max):
        """the evaluators' judgement of `bodies` on the device (HIP library only): see Judge"""
        return Judge(self.api, bodies, n_rows_max)

    def VerticesDiameter(self, vertices):
        """OPTEvaluator::CalculateDiameters (opt_evaluator.cpp:580-600) of one vertex set on the device (HIP library
        only): the largest distance between two vertices, as np.float32"""
        if "vertices_diameter" not in self.api._fn:
            raise M3TError(-3, "%svertices_diameter: this entry point exists in the HIP library only" % self.api.prefix)
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        out = C.c_float(0.0)
        self.api.call("vertices_diameter", fptr(v), len(v), C.byref(out))
        return np.float32(out.value)

    # asynchronous ingest (HIP library only)
    def register_host_buffer(self, array):
        """page-lock a caller-owned frame buffer so that asynchronous uploads overlap the tracking kernels"""
        self.api.call("host_register", array.ctypes.data_as(C.c_void_p), array.nbytes)

    def unregister_host_buffer(self, array):
        self.api.call("host_unregister", array.ctypes.data_as(C.c_void_p))

    def select_slot(self, slot):
        self.api.call("cameras_select_slot", slot)

    def ingest_sync(self):
        self.api.call("ingest_sync")

    def RefinePoses(self, n_corr_iterations=7, n_update_iterations=2):
        """m3t::Refiner::RefinePoses (refiner.cpp:76-117)"""
        return self._step("refine_poses", n_corr_iterations, n_update_iterations)

    def ExecuteTrackingCycle(self, iteration):  # ICG/RBGT/SRT3D name
        return self._step("execute_tracking_cycle", iteration)

    def Sync(self):
        return self._step("sync")


class Judge:
    """m3t_hip_judge_*: RBOTEvaluator::CalculatePoseResults / YCBEvaluator::CalculatePoseResults of a list of bodies on
    the device, with ResetBody of the bodies the device finds lost (reset_iteration >= 0: their poses, their region
    modalities and, after set_reset_renderers, their texture modalities with the built-in detector).  `judge` is
    enqueued behind the step like Tracker.ResetBodies and returns the index of the row it fills; nothing waits until
    `read`."""

    def __init__(self, api, bodies, n_rows_max):
        if "judge_create" not in api._fn:
            raise M3TError(-3, "%sjudge_create: this entry point exists in the HIP library only" % api.prefix)
        self.api = api
        self.bodies = list(bodies)
        self.n_rows_max = int(n_rows_max)
        ids = np.asarray([b.id for b in self.bodies], np.int32)
        out = C.c_int(-1)
        api.call("judge_create", iptr(ids), len(ids), self.n_rows_max, C.byref(out))
        self.id = out.value
        self._gt = np.zeros(16 * len(ids), np.float32)

    def set_thresholds(self, translation_error_threshold=0.05, rotation_error_threshold=5.0 * np.pi / 180.0):
        self.api.call("judge_set_thresholds", self.id, float(translation_error_threshold),
                      float(rotation_error_threshold))

    def set_vertices(self, body, vertices):
        """the (reduced) evaluation vertices of `body` (a listed Body or its index in the list): ADD / ADD-S"""
        index = body if isinstance(body, (int, np.integer)) else [b.id for b in self.bodies].index(body.id)
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        self.api.call("judge_set_vertices", self.id, int(index), fptr(v), len(v))

    def set_add_only(self, body, geometry2body=None):
        """judge `body` (a listed Body or its index in the list) as OPTEvaluator::CalculatePoseResults does
        (opt_evaluator.cpp:462-488): ADD over its evaluation vertices with `geometry2body` (4x4, None: identity) on both
        sides of the pose difference, no nearest-vertex search (adds_error = 0)"""
        index = body if isinstance(body, (int, np.integer)) else [b.id for b in self.bodies].index(body.id)
        g = None if geometry2body is None else fptr(pose_arg(geometry2body))
        self.api.call("judge_set_add_only", self.id, int(index), g)

    def set_reset_renderers(self, enable=True):
        """a resetting `judge` may run the start-modality renderers (ModelOcclusions / UseRegionChecking) that the
        region modalities of the bodies it resets read, and those of their texture modalities (the silhouette renderer,
        always) -- each once, decided on the device, nothing when no body is lost; off (the default): such bodies are
        refused"""
        self.api.call("judge_set_reset_renderers", self.id, int(bool(enable)))

    def set_reset_target(self, body, target=None):
        """entry `body` (a listed Body or its index in the list) is judged on its own pose as before, but when it is
        found lost `target` (a Body; None: the listed body again) takes the entry's ground-truth pose and the restart"""
        index = body if isinstance(body, (int, np.integer)) else [b.id for b in self.bodies].index(body.id)
        self.api.call("judge_set_reset_target", self.id, int(index), -1 if target is None else int(target.id))

    def raw_judge(self, gt_poses, reset_iteration=-1):
        """(status, row) without raising"""
        assert len(gt_poses) == len(self.bodies)
        g = self._gt.reshape(-1, 4, 4)
        for i, p in enumerate(gt_poses):  # column-major
            g[i] = np.asarray(p, np.float32).reshape(4, 4).T
        row = C.c_int(-1)
        rc = self.api.raw("judge_bodies", self.id, fptr(self._gt), int(reset_iteration), C.byref(row))
        return rc, row.value

    def judge(self, gt_poses, reset_iteration=-1):
        rc, row = self.raw_judge(gt_poses, reset_iteration)
        if rc < 0:
            raise M3TError(rc, self.api.last_error())
        return row

    def read(self, first_row, n_rows):
        """rows [first_row, first_row + n_rows) as a structured array [n_rows][n_bodies] (BODY_JUDGEMENT_DTYPE);
        waits for the last of them only"""
        out = np.zeros((n_rows, len(self.bodies)), _capi.BODY_JUDGEMENT_DTYPE)
        self.api.call("judge_read", self.id, int(first_row), int(n_rows), out.ctypes.data_as(C.c_void_p))
        return out

    def clear(self):
        self.api.call("judge_clear", self.id)

    def set_structures(self, structures, error_thresholds):
        """RTBEvaluator's ids_combined_bodies_ per structure: `structures` is a list (one entry per structure) of lists
        of groups, a group being a list of listed bodies (Body objects or indices into the judge's list);
        `error_thresholds`: one per structure.  Every later `judge` also writes a row of structure judgements."""
        ids = [b.id for b in self.bodies]
        first_group, first_index, listed = [0], [0], []
        for groups in structures:
            for group in groups:
                listed += [int(b) if isinstance(b, (int, np.integer)) else ids.index(b.id) for b in group]
                first_index.append(len(listed))
            first_group.append(len(first_index) - 1)
        thresholds = np.ascontiguousarray(error_thresholds, np.float32).reshape(-1)
        assert len(thresholds) == len(structures)
        self.n_structures = len(structures)
        self.api.call("judge_set_structures", self.id, self.n_structures, iptr(np.asarray(first_group, np.int32)),
                      iptr(np.asarray(first_index, np.int32)), iptr(np.asarray(listed + [0], np.int32)), fptr(thresholds))

    def read_structures(self, first_row, n_rows):
        """structure rows [first_row, first_row + n_rows) as a structured array [n_rows][n_structures]
        (STRUCTURE_JUDGEMENT_DTYPE); waits for the last of them only"""
        out = np.zeros((n_rows, self.n_structures), _capi.STRUCTURE_JUDGEMENT_DTYPE)
        self.api.call("judge_read_structures", self.id, int(first_row), int(n_rows), out.ctypes.data_as(C.c_void_p))
        return out


class Body:
    def __init__(self, api, body2world_pose=np.eye(4)):
        self.api = api
        self.id = api.call("body_create", fptr(pose_arg(body2world_pose)))

    def set_body2world_pose(self, pose):
        self.api.call("body_set_body2world_pose", self.id, fptr(pose_arg(pose)))

    def body2world_pose(self):
        buf = np.zeros(16, np.float32)
        self.api.call("body_get_body2world_pose", self.id, fptr(buf))
        return pose_ret(buf)

    def set_geometry(self, vertices, triangles, geometry2body_pose=np.eye(4), geometry_counterclockwise=True,
                     geometry_enable_culling=True, body_id=0, region_id=0):
        """the mesh of body.h (vertices in metres) for the renderer-fed branches"""
        v = np.ascontiguousarray(vertices, np.float32)
        t = np.ascontiguousarray(triangles, np.int32)
        g = _capi.BodyGeometry()
        g.vertices, g.n_vertices = fptr(v), len(v)
        g.triangles, g.n_triangles = iptr(t), len(t)
        g2b = pose_arg(geometry2body_pose)
        for i in range(16):
            g.geometry2body[i] = float(g2b[i])
        g.geometry_counterclockwise = int(geometry_counterclockwise)
        g.geometry_enable_culling = int(geometry_enable_culling)
        g.body_id, g.region_id = int(body_id), int(region_id)
        self.api.call("body_set_geometry", self.id, C.byref(g))


class ColorHistograms:
    """m3t::ColorHistograms shared by several RegionModalities (color_histograms.h:36-40)"""

    def __init__(self, api, n_bins=16, learning_rate_f=0.2, learning_rate_b=0.2):
        self.api = api
        self.n_bins = n_bins
        self.id = api.call("color_histograms_create", n_bins, learning_rate_f, learning_rate_b)


class RendererGeometry:
    """m3t::RendererGeometry: the bodies a renderer draws, in draw order"""

    def __init__(self, api):
        self.api = api
        self.id = api.call("renderer_geometry_create")

    def AddBody(self, body):
        self.api.call("renderer_geometry_add_body", self.id, body.id)


class _FocusedRenderer:
    def __init__(self, api, rid, image_size, silhouette):
        self.api, self.id, self.image_size, self.silhouette = api, rid, image_size, silhouette

    def AddReferencedBody(self, body):
        self.api.call("renderer_add_referenced_body", self.id, body.id)

    def StartRendering(self):
        self.api.call("renderer_start_rendering", self.id)
        return True

    def images(self):
        """(depth u16 [S,S], silhouette u8 [S,S] or None, corner_u, corner_v, scale, n_visible)"""
        s = self.image_size
        depth = np.zeros((s, s), np.uint16)
        sil = np.zeros((s, s), np.uint8) if self.silhouette else None
        info = np.zeros(3, np.float32)
        n = C.c_int()
        self.api.call("renderer_get_images", self.id, depth.ctypes.data_as(C.POINTER(C.c_uint16)),
                      sil.ctypes.data_as(C.POINTER(C.c_uint8)) if sil is not None else None, fptr(info), C.byref(n))
        return depth, sil, float(info[0]), float(info[1]), float(info[2]), n.value


class FocusedBasicDepthRenderer(_FocusedRenderer):
    """basic_depth_renderer.h:120-128"""

    def __init__(self, api, renderer_geometry, camera, image_size=200, z_min=0.02, z_max=10.0):
        rid = api.call("focused_depth_renderer_create", renderer_geometry.id, camera.id, image_size, z_min, z_max)
        super().__init__(api, rid, image_size, False)


class FocusedSilhouetteRenderer(_FocusedRenderer):
    """silhouette_renderer.h:150-155; id_type 0 = IDType::BODY, 1 = IDType::REGION"""

    def __init__(self, api, renderer_geometry, camera, id_type=0, image_size=200, z_min=0.02, z_max=10.0):
        rid = api.call("focused_silhouette_renderer_create", renderer_geometry.id, camera.id, id_type, image_size,
                       z_min, z_max)
        super().__init__(api, rid, image_size, True)


class _Camera:
    def __init__(self, api, cam_id, width, height, bytes_per_pixel):
        self.api = api
        self.id = cam_id
        self.width, self.height, self.bpp = width, height, bytes_per_pixel

    def UpdateImage(self, image):
        """image: (H, W, 3) uint8 BGR or (H, W) uint16; row stride taken from the array."""
        a = np.asarray(image)
        assert a.shape[0] == self.height and a.shape[1] == self.width, (a.shape, self.height, self.width)
        assert a.itemsize * (a.shape[2] if a.ndim == 3 else 1) == self.bpp
        if a.strides[1] != self.bpp or (a.ndim == 3 and a.strides[2] != 1):
            a = np.ascontiguousarray(a)
        self.api.call("camera_upload", self.id, a.ctypes.data_as(C.c_void_p), a.strides[0])
        return True

    # device-side frame ring + asynchronous ingest (HIP library only)
    def set_ring(self, n_slots):
        self.api.call("camera_set_ring", self.id, n_slots)

    def upload_slot(self, slot, image, asynchronous=False):
        """Stage `image` into ring slot `slot`.  With asynchronous=True the call returns at once and
        the array must stay alive and unchanged until slot_sync(slot) / Tracker.ingest_sync() (page-lock it once with
        Tracker.register_host_buffer for a true overlapped copy)."""
        a = np.asarray(image)
        assert a.shape[0] == self.height and a.shape[1] == self.width
        assert a.strides[1] == self.bpp, "asynchronous uploads borrow the buffer: it must be pixel-contiguous"
        self.api.call("camera_upload_slot_async" if asynchronous else "camera_upload_slot", self.id, slot,
                      a.ctypes.data_as(C.c_void_p), a.strides[0])

    def select_slot(self, slot):
        self.api.call("camera_select_slot", self.id, slot)

    def slot_sync(self, slot):
        """wait until this camera's last asynchronous upload into `slot` has left its host buffer (and for no other
        copy: Tracker.ingest_sync waits for all cameras)"""
        self.api.call("camera_slot_sync", self.id, slot)

    def set_world2camera_pose(self, pose):
        self.api.call("camera_set_world2camera_pose", self.id, fptr(pose_arg(pose)))


def _intr(fu, fv, ppu, ppv, width, height):
    return Intrinsics(fu, fv, ppu, ppv, width, height)


class ColorCamera(_Camera):
    def __init__(self, api, fu, fv, ppu, ppv, width, height, world2camera_pose=np.eye(4)):
        i = _intr(fu, fv, ppu, ppv, width, height)
        cid = api.call("color_camera_create", C.byref(i), fptr(pose_arg(world2camera_pose)))
        super().__init__(api, cid, width, height, 3)


class DepthCamera(_Camera):
    def __init__(self, api, fu, fv, ppu, ppv, width, height, depth_scale, world2camera_pose=np.eye(4)):
        i = _intr(fu, fv, ppu, ppv, width, height)
        cid = api.call("depth_camera_create", C.byref(i), fptr(pose_arg(world2camera_pose)), depth_scale)
        super().__init__(api, cid, width, height, 2)
        self.depth_scale = depth_scale


class RegionModel:
    """Sparse viewpoint model for regions (runtime part of region_model.cpp)."""

    def __init__(self, api, path=None, data_points=None, orientations=None, contour_lengths=None,
                 stride_depth_offset=0.002, max_radius_depth_offset=0.05):
        self.api = api
        if path is not None:
            self.id = api.call("region_model_load", str(path).encode())
        else:
            dp = np.ascontiguousarray(data_points, np.float32)
            ori = np.ascontiguousarray(orientations, np.float32)
            cl = np.ascontiguousarray(contour_lengths, np.float32)
            assert dp.ndim == 3 and dp.shape[2] == _capi.M3T_REGION_POINT_FLOATS
            d = RegionModelDesc(dp.shape[0], dp.shape[1], fptr(dp), fptr(ori), fptr(cl), stride_depth_offset,
                                max_radius_depth_offset)
            self.id = api.call("region_model_create", C.byref(d))
        nv, npts, me = C.c_int(), C.c_int(), C.c_float()
        api.call("region_model_info", self.id, C.byref(nv), C.byref(npts), C.byref(me))
        self.n_views, self.n_points, self.max_contour_length = nv.value, npts.value, me.value

    def GetClosestView(self, body2camera_pose):
        v = C.c_int()
        self.api.call("region_model_closest_view", self.id, fptr(pose_arg(body2camera_pose)), C.byref(v))
        return v.value

    @classmethod
    def generate(cls, api, body, **params):
        """RegionModel::GenerateModel without OpenGL (HIP library only); body needs set_geometry()"""
        self = cls.__new__(cls)
        self.api = api
        # associated: (body, movable, same_region) triples of RegionModel::AddAssociatedBody
        associated = params.pop("associated", ())
        gp = C.byref(_capi.ModelGenerationParams(**params))
        if associated:
            ids = np.asarray([b.id for b, _, _ in associated], np.int32)
            mov = np.asarray([int(m) for _, m, _ in associated], np.int32)
            same = np.asarray([int(s) for _, _, s in associated], np.int32)
            self.id = api.call("region_model_generate_associated", body.id, gp, len(ids), iptr(ids), iptr(mov), iptr(same))
        else:
            self.id = api.call("region_model_generate", body.id, gp)
        nv, npts, me = C.c_int(), C.c_int(), C.c_float()
        api.call("region_model_info", self.id, C.byref(nv), C.byref(npts), C.byref(me))
        self.n_views, self.n_points, self.max_contour_length = nv.value, npts.value, me.value
        return self

    def views(self):
        pts = np.zeros((self.n_views, self.n_points, _capi.M3T_REGION_POINT_FLOATS), np.float32)
        ori = np.zeros((self.n_views, 3), np.float32)
        ext = np.zeros(self.n_views, np.float32)
        self.api.call("region_model_get_views", self.id, fptr(pts), fptr(ori), fptr(ext))
        return pts, ori, ext


class DepthModel:
    def __init__(self, api, path=None, data_points=None, orientations=None, surface_areas=None,
                 stride_depth_offset=0.002, max_radius_depth_offset=0.05):
        self.api = api
        if path is not None:
            self.id = api.call("depth_model_load", str(path).encode())
        else:
            dp = np.ascontiguousarray(data_points, np.float32)
            ori = np.ascontiguousarray(orientations, np.float32)
            sa = np.ascontiguousarray(surface_areas, np.float32)
            assert dp.ndim == 3 and dp.shape[2] == _capi.M3T_DEPTH_POINT_FLOATS
            d = DepthModelDesc(dp.shape[0], dp.shape[1], fptr(dp), fptr(ori), fptr(sa), stride_depth_offset,
                               max_radius_depth_offset)
            self.id = api.call("depth_model_create", C.byref(d))
        nv, npts, me = C.c_int(), C.c_int(), C.c_float()
        api.call("depth_model_info", self.id, C.byref(nv), C.byref(npts), C.byref(me))
        self.n_views, self.n_points, self.max_surface_area = nv.value, npts.value, me.value

    def GetClosestView(self, body2camera_pose):
        v = C.c_int()
        self.api.call("depth_model_closest_view", self.id, fptr(pose_arg(body2camera_pose)), C.byref(v))
        return v.value

    @classmethod
    def generate(cls, api, body, **params):
        """DepthModel::GenerateModel without OpenGL (HIP library only); body needs set_geometry()"""
        self = cls.__new__(cls)
        self.api = api
        occlusion_bodies = params.pop("occlusion_bodies", ())  # DepthModel::AddOcclusionBody
        gp = C.byref(_capi.ModelGenerationParams(**params))
        if occlusion_bodies:
            ids = np.asarray([b.id for b in occlusion_bodies], np.int32)
            self.id = api.call("depth_model_generate_occluded", body.id, gp, len(ids), iptr(ids))
        else:
            self.id = api.call("depth_model_generate", body.id, gp)
        nv, npts, me = C.c_int(), C.c_int(), C.c_float()
        api.call("depth_model_info", self.id, C.byref(nv), C.byref(npts), C.byref(me))
        self.n_views, self.n_points, self.max_surface_area = nv.value, npts.value, me.value
        return self

    def views(self):
        pts = np.zeros((self.n_views, self.n_points, _capi.M3T_DEPTH_POINT_FLOATS), np.float32)
        ori = np.zeros((self.n_views, 3), np.float32)
        ext = np.zeros(self.n_views, np.float32)
        self.api.call("depth_model_get_views", self.id, fptr(pts), fptr(ori), fptr(ext))
        return pts, ori, ext


class _Modality:
    def gradient_hessian(self):
        g = np.zeros(6, np.float32)
        h = np.zeros(36, np.float32)
        self.api.call("modality_get_gradient_hessian", self.id, fptr(g), fptr(h))
        return g, h.reshape(6, 6).T.copy()

    def gradient(self):
        return self.gradient_hessian()[0]

    def hessian(self):
        return self.gradient_hessian()[1]

    def set_gradient_hessian(self, g, h):
        g = np.ascontiguousarray(g, np.float32).reshape(6)
        h = np.ascontiguousarray(np.asarray(h, np.float32).reshape(6, 6).T).reshape(36)
        self.api.call("modality_set_gradient_hessian", self.id, fptr(g), fptr(h))


class RegionModality(_Modality):
    def __init__(self, api, body, color_camera, region_model, depth_camera=None, params=None, **kw):
        self.api = api
        self.params = params if params is not None else RegionModalityParams(**kw)
        self.id = api.call("region_modality_create", C.byref(self.params), body.id, color_camera.id,
                           region_model.id, depth_camera.id if depth_camera is not None else -1)
        self.n_bins = self.params.n_histogram_bins

    def UseSharedColorHistograms(self, color_histograms):
        self.api.call("region_modality_use_shared_color_histograms", self.id, color_histograms.id)
        self.n_bins = color_histograms.n_bins

    def ModelOcclusions(self, depth_renderer):
        self.api.call("region_modality_model_occlusions", self.id, depth_renderer.id)

    def UseRegionChecking(self, silhouette_renderer):
        self.api.call("region_modality_use_region_checking", self.id, silhouette_renderer.id)

    def data_lines(self):
        n = C.c_int()
        cap = self.params.n_lines_max
        out = np.zeros(cap, DATA_LINE_DTYPE)
        self.api.call("region_modality_get_lines", self.id, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        return out[:min(n.value, cap)]

    def histograms(self):
        n = self.n_bins ** 3
        f = np.zeros(n, np.float32)
        b = np.zeros(n, np.float32)
        self.api.call("region_modality_get_histograms", self.id, fptr(f), fptr(b))
        return f, b

    def set_histograms(self, f, b):
        f = np.ascontiguousarray(f, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        assert f.size == self.n_bins ** 3 and b.size == f.size
        self.api.call("region_modality_set_histograms", self.id, fptr(f), fptr(b))


class DepthModality(_Modality):
    def __init__(self, api, body, depth_camera, depth_model, params=None, **kw):
        self.api = api
        self.params = params if params is not None else DepthModalityParams(**kw)
        self.id = api.call("depth_modality_create", C.byref(self.params), body.id, depth_camera.id, depth_model.id)

    def ModelOcclusions(self, depth_renderer):
        self.api.call("depth_modality_model_occlusions", self.id, depth_renderer.id)

    def UseSilhouetteChecking(self, silhouette_renderer):
        self.api.call("depth_modality_use_silhouette_checking", self.id, silhouette_renderer.id)

    def data_points(self):
        n = C.c_int()
        cap = self.params.n_points_max
        out = np.zeros(cap, DATA_POINT_DTYPE)
        self.api.call("depth_modality_get_points", self.id, out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
        return out[:min(n.value, cap)]


class TextureModality(_Modality):
    """TextureModality behind its feature detector (texture_modality.cpp): the caller detects and describes features in
    the focused image of RegionOfInterest() and hands them over with SetFocusedFeatures (or SetFeatures, in full-image
    coordinates); keyframes, matching, g/H and keyframe renewal run on the device.
    descriptor_norm="hamming": rows of descriptor_bytes (32 or 64) uint8, matched with the Hamming norm (ORB, BRISK,
    FREAK).  descriptor_norm="l2": rows of descriptor_bytes / 4 float32, matched with the L2 norm as include/m3t_hip.h
    pins it (SIFT: descriptor_bytes=512; DAISY: 4 * its number of floats); the built-in detector is refused there."""

    def __init__(self, api, body, color_camera, silhouette_renderer, depth_camera=None, params=None,
                 descriptor_norm="hamming", **kw):
        if descriptor_norm not in ("hamming", "l2"):
            raise ValueError("descriptor_norm=%r: \"hamming\" or \"l2\"" % (descriptor_norm,))
        self.api = api
        self.params = params if params is not None else TextureModalityParams(**kw)
        self.descriptor_norm = descriptor_norm
        self.detector = None  # TextureDetectorParams while the built-in detector is set
        self.id = api.call("texture_modality_create_l2" if descriptor_norm == "l2" else "texture_modality_create",
                           C.byref(self.params), body.id, color_camera.id, silhouette_renderer.id,
                           depth_camera.id if depth_camera is not None else -1)
        # a row of descriptors as the caller hands it over and gets it back
        self.descriptor_dtype = np.float32 if descriptor_norm == "l2" else np.uint8
        self.descriptor_width = self.params.descriptor_bytes // 4 if descriptor_norm == "l2" else self.params.descriptor_bytes

    def ModelOcclusions(self, depth_renderer):
        self.api.call("texture_modality_model_occlusions", self.id, depth_renderer.id)

    def RegionOfInterest(self):
        """CalculateScaleAndRegionOfInterest at the body's current pose: ((x, y, width, height), scale), or None where
        the reference returns false (then SetFeatures with no features)"""
        roi = np.zeros(4, np.int32)
        scale = np.zeros(1, np.float32)
        valid = C.c_int()
        self.api.call("texture_modality_get_region_of_interest", self.id, iptr(roi), fptr(scale), C.byref(valid))
        return ((int(roi[0]), int(roi[1]), int(roi[2]), int(roi[3])), np.float32(scale[0])) if valid.value else None

    def SetFeatures(self, keypoints, descriptors):
        """keypoints: n x 2 in full-image coordinates; descriptors: n rows of descriptor_bytes (uint8), for an L2
        modality an n x descriptor_bytes / 4 float32 array (another dtype or width: ValueError)"""
        keypoints = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
        if self.descriptor_norm == "l2":
            descriptors = self._l2_rows(descriptors, len(keypoints))
        else:
            descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(len(keypoints), self.params.descriptor_bytes) \
                if len(keypoints) == 0 else np.ascontiguousarray(descriptors, np.uint8).reshape(len(keypoints), -1)
            if len(keypoints) and descriptors.shape[1] != self.params.descriptor_bytes:
                raise ValueError("descriptors must have %d bytes per row" % self.params.descriptor_bytes)
        self.api.call("texture_modality_set_features", self.id, fptr(keypoints),
                      descriptors.ctypes.data_as(C.POINTER(C.c_uint8)), len(keypoints))

    def _l2_rows(self, descriptors, n):
        descriptors = np.asarray(descriptors)
        if n == 0 and descriptors.size == 0:
            return np.zeros((0, self.descriptor_width), np.float32)
        if descriptors.dtype != np.float32:
            raise ValueError("descriptors of an L2 modality must be float32, not %s" % descriptors.dtype)
        if descriptors.ndim != 2 or descriptors.shape != (n, self.descriptor_width):
            raise ValueError("descriptors must be %d x %d float32, not %s" % (n, self.descriptor_width, descriptors.shape))
        return np.ascontiguousarray(descriptors)

    def SetDetector(self, params=None, builtin=True, **kw):
        """the built-in detector (TextureDetectorParams or its fields as keywords): detection is then enqueued with
        StartModalities and with every correspondence search, and SetFeatures is refused; SetDetector(builtin=False)
        hands the features back to the caller"""
        if not builtin:
            self.detector = None
            self.api.call("texture_modality_set_detector", self.id, None)
            return
        detector = params if params is not None else TextureDetectorParams(**kw)
        self.api.call("texture_modality_set_detector", self.id, C.byref(detector))  # (refused for an L2 modality)
        self.detector = detector

    def features(self):
        """(keypoints n x 2 in full-image coordinates, descriptors n x descriptor_bytes uint8 -- for an L2 modality
        n x descriptor_bytes / 4 float32) the modality holds; waits for the stream"""
        n = C.c_int()
        self.api.call("texture_modality_get_features", self.id, None, None, 0, C.byref(n))
        keypoints = np.zeros((max(n.value, 1), 2), np.float32)
        descriptors = np.zeros((max(n.value, 1), self.params.descriptor_bytes), np.uint8)
        self.api.call("texture_modality_get_features", self.id, fptr(keypoints),
                      descriptors.ctypes.data_as(C.POINTER(C.c_uint8)), n.value, C.byref(n))
        return keypoints[:n.value], descriptors[:n.value].view(self.descriptor_dtype)

    def focused_image(self):
        """the grey focused image (height x width, uint8) of the last built-in detection, or None when it had no valid
        region of interest; waits for the stream"""
        width, height = C.c_int(), C.c_int()
        self.api.call("texture_modality_get_focused_image", self.id, None, 0, C.byref(width), C.byref(height))
        if width.value == 0 or height.value == 0:
            return None
        pixels = np.zeros((height.value, width.value), np.uint8)
        self.api.call("texture_modality_get_focused_image", self.id, pixels.ctypes.data_as(C.POINTER(C.c_uint8)),
                      pixels.size, C.byref(width), C.byref(height))
        return pixels

    def SetFocusedFeatures(self, roi, scale, focused_keypoints, descriptors):
        """keypoints of the focused image: pt = roi.x + pt.x / scale in f32 (texture_modality.cpp:884-887)"""
        pts = np.asarray(focused_keypoints, np.float32).reshape(-1, 2)
        scale = np.float32(scale)
        full = np.empty_like(pts)
        full[:, 0] = np.float32(roi[0]) + pts[:, 0] / scale
        full[:, 1] = np.float32(roi[1]) + pts[:, 1] / scale
        self.SetFeatures(full, descriptors)

    def points(self):
        """data_points_ of the last CalculateCorrespondences / CalculateGradientAndHessian"""
        cap = self.params.n_keyframes * M3T_MAX_TEXTURE_FEATURES
        n = C.c_int()
        self.api.call("texture_modality_get_points", self.id, None, 0, C.byref(n))
        out = np.zeros(min(n.value, cap), TEXTURE_DATA_POINT_DTYPE)
        if len(out):
            self.api.call("texture_modality_get_points", self.id, out.ctypes.data_as(C.c_void_p), len(out), C.byref(n))
        return out[:min(n.value, len(out))]

    def keyframes(self):
        """(keyframe_age, [points of the oldest keyframe (k x 3), ..., of the newest])"""
        nk, age = C.c_int(), C.c_int()
        counts = np.zeros(M3T_MAX_TEXTURE_KEYFRAMES, np.int32)
        self.api.call("texture_modality_get_keyframes", self.id, C.byref(nk), C.byref(age), iptr(counts), None, 0)
        total = int(counts.sum())
        xyz = np.zeros((max(total, 1), 3), np.float32)
        self.api.call("texture_modality_get_keyframes", self.id, C.byref(nk), C.byref(age), iptr(counts), fptr(xyz),
                      len(xyz))
        edges = np.concatenate([[0], np.cumsum(counts[:nk.value])])
        return age.value, [xyz[edges[k]:edges[k + 1]].copy() for k in range(nk.value)]


class Link:
    def __init__(self, api, body=None, parent=None, body2joint_pose=np.eye(4), joint2parent_pose=np.eye(4),
                 free_directions=(1, 1, 1, 1, 1, 1), fixed_body2joint_pose=True):
        self.api = api
        fd = np.asarray(free_directions, np.int32)
        self.id = api.call("link_create", body.id if body is not None else -1,
                           parent.id if parent is not None else -1, fptr(pose_arg(body2joint_pose)),
                           fptr(pose_arg(joint2parent_pose)), iptr(fd), int(fixed_body2joint_pose))
        self._default_body2joint_pose = np.array(body2joint_pose, np.float32)
        self._default_joint2parent_pose = np.array(joint2parent_pose, np.float32)

    def AddModality(self, modality):
        self.api.call("link_add_modality", self.id, modality.id)

    def link2world_pose(self):
        buf = np.zeros(16, np.float32)
        self.api.call("link_get_link2world_pose", self.id, fptr(buf))
        return pose_ret(buf)

    def set_link2world_pose(self, pose):
        """Link::set_link2world_pose (link.cpp:138-140); for a link with a body this is the body's pose"""
        self.api.call("link_set_link2world_pose", self.id, fptr(pose_arg(pose)))

    def ResetJointPoses(self):
        """Link::ResetJointPoses (link.cpp:243-246): back to the poses the link was created with"""
        self.api.call("link_set_joint_poses", self.id, fptr(pose_arg(self._default_body2joint_pose)),
                      fptr(pose_arg(self._default_joint2parent_pose)))

    def set_body2joint_pose(self, pose):
        self.api.call("link_set_joint_poses", self.id, fptr(pose_arg(pose)), None)

    def set_joint2parent_pose(self, pose):
        self.api.call("link_set_joint_poses", self.id, None, fptr(pose_arg(pose)))

    def body2joint_pose(self):
        buf = np.zeros(16, np.float32)
        self.api.call("link_get_joint_poses", self.id, fptr(buf), None)
        return pose_ret(buf)

    def joint2parent_pose(self):
        buf = np.zeros(16, np.float32)
        self.api.call("link_get_joint_poses", self.id, None, fptr(buf))
        return pose_ret(buf)


class Optimizer:
    def __init__(self, api, root_link=None, body=None, modalities=(), tikhonov_parameter_rotation=1000.0,
                 tikhonov_parameter_translation=30000.0):
        self.api = api
        if root_link is not None:
            self.id = api.call("optimizer_create", root_link.id, tikhonov_parameter_rotation,
                               tikhonov_parameter_translation)
        else:
            ids = np.asarray([m.id for m in modalities], np.int32)
            self.id = api.call("optimizer_create_rigid", body.id, len(ids), iptr(ids),
                               tikhonov_parameter_rotation, tikhonov_parameter_translation)


class Constraint:
    def __init__(self, api, optimizer, link1, link2, body12joint1_pose=np.eye(4), body22joint2_pose=np.eye(4),
                 constraint_directions=(0, 0, 0, 0, 0, 0)):
        cd = np.asarray(constraint_directions, np.int32)
        self.id = api.call("constraint_create", optimizer.id, link1.id, link2.id, fptr(pose_arg(body12joint1_pose)),
                           fptr(pose_arg(body22joint2_pose)), iptr(cd))


class SoftConstraint:
    """include/m3t/soft_constraint.h:52-62 (same defaults)"""

    def __init__(self, api, optimizer, link1, link2, body12joint1_pose=np.eye(4), body22joint2_pose=np.eye(4),
                 constraint_directions=(0, 0, 0, 0, 0, 0), max_distance_rotation=0.0, max_distance_translation=0.0,
                 standard_deviation_rotation=0.01, standard_deviation_translation=0.001):
        cd = np.asarray(constraint_directions, np.int32)
        self.id = api.call("soft_constraint_create", optimizer.id, link1.id, link2.id,
                           fptr(pose_arg(body12joint1_pose)), fptr(pose_arg(body22joint2_pose)), iptr(cd),
                           max_distance_rotation, max_distance_translation, standard_deviation_rotation,
                           standard_deviation_translation)


__all__ = ["Tracker", "Body", "ColorCamera", "DepthCamera", "RegionModel", "DepthModel", "RegionModality",
           "DepthModality", "Link", "Optimizer", "Constraint", "SoftConstraint", "RendererGeometry", "ColorHistograms",
           "FocusedBasicDepthRenderer", "FocusedSilhouetteRenderer", "M3TError", "RegionModalityParams",
           "DepthModalityParams"]
