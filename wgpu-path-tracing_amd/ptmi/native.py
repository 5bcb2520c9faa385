"""ctypes binding of libptmi.so (include/ptmi.h) — the HIP wavefront path tracer.

No fallback: if the library or a gfx950 device is missing, `Context()` raises.
"""
import ctypes
import functools
import os
import types

import numpy as np

from . import layout

_LIB_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib")
LIB_PATH = os.environ.get("PTMI_LIB") or os.path.join(_LIB_DIR, "libptmi.so")   # PTMI_LIB: A/B another build of the same ABI

TRAVERSAL_AUTO, TRAVERSAL_GLOBAL, TRAVERSAL_LDS, TRAVERSAL_GLOBAL_EXACT = 0, 1, 2, 3
ATLAS_RGBA16F, ATLAS_RGBA32F = 1, 2

# every symbol include/ptmi.h declares
EXPORTS = [
    "ptmi_abi_version", "ptmi_create", "ptmi_destroy", "ptmi_last_error", "ptmi_upload_scene",
    "ptmi_upload_atlas", "ptmi_resize", "ptmi_set_options", "ptmi_get_options", "ptmi_dispatch",
    "ptmi_synchronize", "ptmi_read_output", "ptmi_write_output", "ptmi_output_device_ptr",
    "ptmi_bind_output_device", "ptmi_set_stream", "ptmi_blit", "ptmi_get_stats", "ptmi_reset_stats",
    "ptmi_debug_raygen", "ptmi_debug_intersect", "ptmi_debug_occluded", "ptmi_debug_math", "ptmi_debug_exact_math", "ptmi_get_size",
    "ptmi_debug_image_stats", "ptmi_debug_build_image", "ptmi_debug_read_image", "ptmi_throttle", "ptmi_multi_throttle",
    "ptmi_multi_create", "ptmi_multi_destroy", "ptmi_multi_last_error", "ptmi_multi_count", "ptmi_multi_context",
    "ptmi_multi_upload_scene", "ptmi_multi_upload_atlas", "ptmi_multi_resize", "ptmi_multi_set_options", "ptmi_multi_get_options",
    "ptmi_multi_dispatch", "ptmi_multi_gather", "ptmi_multi_synchronize", "ptmi_multi_read_output", "ptmi_multi_write_output",
    "ptmi_multi_blit", "ptmi_multi_get_stats", "ptmi_multi_reset_stats", "ptmi_multi_gather_ms",
    "ptmi_set_aovs", "ptmi_get_aovs", "ptmi_read_aov", "ptmi_aov_device_ptr",
    "ptmi_set_moments", "ptmi_get_moments", "ptmi_read_moments", "ptmi_moments_device_ptr",
    "ptmi_denoise", "ptmi_denoised_device_ptr", "ptmi_blit_denoised",
    "ptmi_dispatch_adaptive", "ptmi_adaptive_status",
    "ptmi_reproject", "ptmi_reproject_status", "ptmi_debug_center_rays",
    "ptmi_set_motion", "ptmi_get_motion", "ptmi_motion_commit", "ptmi_motion_status", "ptmi_read_motion", "ptmi_motion_device_ptr",
    "ptmi_debug_motion_prev",
    "ptmi_upload_environment", "ptmi_set_environment", "ptmi_environment_status", "ptmi_multi_upload_environment",
    "ptmi_multi_set_environment", "ptmi_debug_env_lookup", "ptmi_debug_env_sample", "ptmi_debug_env_table",
    "ptmi_multi_set_aovs", "ptmi_multi_get_aovs", "ptmi_multi_set_moments", "ptmi_multi_get_moments", "ptmi_multi_gather_planes",
    "ptmi_multi_read_aov", "ptmi_multi_read_moments", "ptmi_multi_dispatch_adaptive", "ptmi_multi_adaptive_status",
    "ptmi_multi_denoise", "ptmi_multi_blit_denoised",
    "ptmi_set_medium", "ptmi_get_medium", "ptmi_multi_set_medium", "ptmi_debug_medium_step", "ptmi_debug_medium_tr",
    "ptmi_upload_medium_density", "ptmi_medium_grid_status", "ptmi_multi_upload_medium_density", "ptmi_debug_medium_density",
    "ptmi_debug_medium_track", "ptmi_debug_medium_grid_check",
    "ptmi_update_triangles", "ptmi_update_materials", "ptmi_update_lights", "ptmi_scene_update_status",
    "ptmi_multi_update_triangles", "ptmi_multi_update_materials", "ptmi_multi_update_lights", "ptmi_multi_scene_update_status",
    "ptmi_rebuild_tree", "ptmi_rebuild_status", "ptmi_multi_rebuild_tree", "ptmi_multi_rebuild_status",
    "ptmi_set_alpha_cutoff", "ptmi_alpha_status", "ptmi_multi_set_alpha_cutoff", "ptmi_multi_alpha_status",
    "ptmi_debug_alpha_intersect", "ptmi_debug_alpha_occluded",
    "ptmi_set_alpha_blend", "ptmi_alpha_blend_status", "ptmi_multi_set_alpha_blend", "ptmi_multi_alpha_blend_status",
    "ptmi_set_triangle_groups", "ptmi_transform_groups", "ptmi_transform_status", "ptmi_normal_matrix", "ptmi_debug_read_triangles",
    "ptmi_multi_set_triangle_groups", "ptmi_multi_transform_groups", "ptmi_multi_transform_status",
    "ptmi_set_skin", "ptmi_pose_skin", "ptmi_skin_status", "ptmi_multi_set_skin", "ptmi_multi_pose_skin", "ptmi_multi_skin_status",
    "ptmi_set_morph", "ptmi_pose_morph", "ptmi_morph_status", "ptmi_multi_set_morph", "ptmi_multi_pose_morph", "ptmi_multi_morph_status",
    "ptmi_set_projections", "ptmi_get_projections", "ptmi_multi_set_projections", "ptmi_multi_get_projections",
    "ptmi_upload_bake_surface", "ptmi_dispatch_bake", "ptmi_bake_status", "ptmi_bake_dilate", "ptmi_debug_bake_rays",
    "ptmi_upload_probes", "ptmi_dispatch_probes", "ptmi_probe_status", "ptmi_probe_sh", "ptmi_probe_irradiance",
    "ptmi_debug_probe_rays", "ptmi_debug_probe_tables",
    "ptmi_set_probe_depth", "ptmi_get_probe_depth", "ptmi_read_probe_depth", "ptmi_write_probe_depth", "ptmi_probe_depth_device_ptr",
    "ptmi_probe_visibility",
    "ptmi_scissor_status",
    "ptmi_bake_denoise", "ptmi_bake_denoised_device_ptr", "ptmi_write_moments",
]
# ptmi_scissor_status.reason (include/ptmi.h PTMI_SCISSOR_*)
(SCISSOR_APPLIED, SCISSOR_OFF, SCISSOR_NOT_PLAIN, SCISSOR_ENVIRONMENT, SCISSOR_MEDIUM, SCISSOR_AOV, SCISSOR_MOMENTS, SCISSOR_ALPHA,
 SCISSOR_PROJECTION, SCISSOR_NO_PROMISE, SCISSOR_NOTHING) = range(11)
MULTI_LOOPBACK = 1
MULTI_PLANE_MOMENTS, MULTI_PLANE_OUTPUT = 0x100, 0x200      # gather_planes: with the AOV_* bits
# first-hit planes (include/ptmi.h ptmi_set_aovs): name -> (bit, numpy dtype, channels)
AOV_ALBEDO, AOV_NORMAL, AOV_ID = 1, 2, 4
AOVS = {"albedo": (AOV_ALBEDO, np.float32, 4), "normal": (AOV_NORMAL, np.float32, 4), "id": (AOV_ID, np.uint32, 2)}
ABI_VERSION = 4


class PtmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptmi error {code}: {msg}")
        self.code = code


class Options(ctypes.Structure):
    _fields_ = [("max_bounces", ctypes.c_uint32), ("do_mis", ctypes.c_uint32),
                ("tile_y0", ctypes.c_uint32), ("tile_y1", ctypes.c_uint32),
                ("frames_per_batch", ctypes.c_uint32), ("traversal", ctypes.c_uint32),
                ("cull", ctypes.c_uint32), ("timing", ctypes.c_uint32), ("keep_reference_tree", ctypes.c_uint32),
                ("tile_parts", ctypes.c_uint32), ("tile_part", ctypes.c_uint32), ("tile_strip", ctypes.c_uint32),
                ("perf_mode", ctypes.c_uint32), ("reserved_a", ctypes.c_uint32), ("overlap", ctypes.c_uint32),
                ("reserved_b", ctypes.c_uint32 * 4), ("tree_builder", ctypes.c_uint32),
                ("leaves", ctypes.c_uint32), ("leaf_tris", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 1)]


class DenoiseParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_uint32), ("demodulate", ctypes.c_uint32), ("phi_color", ctypes.c_float),
                ("phi_normal", ctypes.c_float), ("phi_depth", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


class AdaptiveParams(ctypes.Structure):
    """ptmi_adaptive_params; 0 picks a field's default (include/ptmi.h), threshold has none"""
    _fields_ = [("threshold", ctypes.c_float), ("floor", ctypes.c_float), ("min_frames", ctypes.c_uint32),
                ("max_frames", ctypes.c_uint32), ("step", ctypes.c_uint32), ("neighbourhood", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


class AdaptiveStatus(ctypes.Structure):
    _fields_ = [("active", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("min_count", ctypes.c_uint32),
                ("max_count", ctypes.c_uint32), ("rounds", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class ReprojectParams(ctypes.Structure):
    """ptmi_reproject_params; 0 picks a field's default (include/ptmi.h)"""
    _fields_ = [("max_history", ctypes.c_uint32), ("depth_tolerance", ctypes.c_float), ("match_ids", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 5)]


class ReprojectStatus(ctypes.Structure):
    _fields_ = [("carried", ctypes.c_uint64), ("disoccluded", ctypes.c_uint64), ("missed", ctypes.c_uint64),
                ("samples", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class MotionStatus(ctypes.Structure):
    """ptmi_motion_status (include/ptmi.h ptmi_set_motion)"""
    _fields_ = [("on", ctypes.c_uint32), ("epochs", ctypes.c_uint32), ("dirty_first", ctypes.c_uint32), ("dirty_count", ctypes.c_uint32),
                ("moved", ctypes.c_uint64), ("moved_carried", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Environment(ctypes.Structure):
    """ptmi_environment; intensity 0 picks 1 (include/ptmi.h)"""
    _fields_ = [("intensity", ctypes.c_float), ("rotation", ctypes.c_float), ("sample", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 5)]


class EnvironmentStatus(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("sampled", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("weight_sum", ctypes.c_double)]

    def as_dict(self):
        return {"width": int(self.width), "height": int(self.height), "sampled": int(self.sampled), "weight_sum": float(self.weight_sum)}


class Medium(ctypes.Structure):
    """ptmi_medium: one homogeneous medium inside an axis-aligned box (include/ptmi.h)"""
    _fields_ = [("sigma_t", ctypes.c_float), ("albedo", ctypes.c_float * 3), ("g", ctypes.c_float),
                ("box_min", ctypes.c_float * 3), ("box_max", ctypes.c_float * 3), ("reserved", ctypes.c_uint32 * 5)]

    def as_dict(self):
        return {"sigma_t": float(self.sigma_t), "albedo": tuple(self.albedo), "g": float(self.g),
                "box": (tuple(self.box_min), tuple(self.box_max))}


class MediumGrid(ctypes.Structure):
    """ptmi_medium_grid: how the medium's density grid is looked up (include/ptmi.h)"""
    _fields_ = [("filter", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


class MediumGridStatus(ctypes.Structure):
    _fields_ = [("nx", ctypes.c_uint32), ("ny", ctypes.c_uint32), ("nz", ctypes.c_uint32), ("filter", ctypes.c_uint32),
                ("rho_min", ctypes.c_float), ("rho_max", ctypes.c_float), ("rho_mean", ctypes.c_double)]

    def as_dict(self):
        return {"dims": (int(self.nx), int(self.ny), int(self.nz)), "filter": int(self.filter), "rho_min": float(self.rho_min),
                "rho_max": float(self.rho_max), "rho_mean": float(self.rho_mean)}


FILTER_NEAREST, FILTER_LINEAR = 0, 1


class SceneUpdateStatus(ctypes.Structure):
    """struct ptmi_scene_update_status: the triangle updates since the last upload (include/ptmi.h)"""
    _fields_ = [("updates", ctypes.c_uint32), ("quantised_kept", ctypes.c_uint32), ("plan_ms", ctypes.c_double),
                ("refit_ms", ctypes.c_double), ("cost_built", ctypes.c_double), ("cost_now", ctypes.c_double),
                ("root_min", ctypes.c_float * 3), ("root_max", ctypes.c_float * 3), ("reserved", ctypes.c_uint32 * 4)]

    def as_dict(self):
        return {"updates": int(self.updates), "quantised_kept": int(self.quantised_kept), "plan_ms": float(self.plan_ms),
                "refit_ms": float(self.refit_ms), "cost_built": float(self.cost_built), "cost_now": float(self.cost_now),
                "root_box": (tuple(self.root_min), tuple(self.root_max))}


class RebuildParams(ctypes.Structure):
    """ptmi_rebuild_params; builder 0 picks the device builder where it applies (include/ptmi.h)"""
    _fields_ = [("builder", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


class RebuildStatus(ctypes.Structure):
    """struct ptmi_rebuild_status: the rebuilds of the walked tree since the last upload (include/ptmi.h)"""
    _fields_ = [("rebuilds", ctypes.c_uint32), ("builder_used", ctypes.c_uint32), ("build_ms", ctypes.c_double),
                ("cost_before", ctypes.c_double), ("cost_after", ctypes.c_double)]

    def as_dict(self):
        return {"rebuilds": int(self.rebuilds), "builder_used": int(self.builder_used), "build_ms": float(self.build_ms),
                "cost_before": float(self.cost_before), "cost_after": float(self.cost_after)}


class GroupTransform(ctypes.Structure):
    """ptmi_group_transform: the matrix of one triangle group (include/ptmi.h ptmi_transform_groups)"""
    _fields_ = [("group", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("m", ctypes.c_float * 12), ("nm", ctypes.c_float * 9),
                ("reserved1", ctypes.c_uint32)]


GROUP_TRANSFORM = np.dtype([("group", "<u4"), ("reserved0", "<u4"), ("m", "<f4", (12,)), ("nm", "<f4", (9,)), ("reserved1", "<u4")])


class TransformStatus(ctypes.Structure):
    """struct ptmi_transform_status: the group table in place and the transforms since it was set (include/ptmi.h)"""
    _fields_ = [("present", ctypes.c_uint32), ("n_groups", ctypes.c_uint32), ("transforms", ctypes.c_uint32),
                ("last_moved", ctypes.c_uint32), ("first_bad", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("transform_ms", ctypes.c_double)]

    def as_dict(self):
        return {"present": int(self.present), "n_groups": int(self.n_groups), "transforms": int(self.transforms),
                "last_moved": int(self.last_moved), "first_bad": int(self.first_bad), "transform_ms": float(self.transform_ms)}


class SkinCorner(ctypes.Structure):
    """ptmi_skin_corner: the joints and weights of one corner of a skinned triangle (include/ptmi.h ptmi_set_skin)"""
    _fields_ = [("joint", ctypes.c_uint32 * 4), ("weight", ctypes.c_float * 4)]


JointTransform, JOINT_TRANSFORM = GroupTransform, GROUP_TRANSFORM      # ptmi_joint_transform: the same record, `group` is the joint


class SkinStatus(ctypes.Structure):
    """struct ptmi_skin_status: the skin in place and the poses since it was set (include/ptmi.h)"""
    _fields_ = [("present", ctypes.c_uint32), ("n_joints", ctypes.c_uint32), ("n_skinned", ctypes.c_uint32), ("poses", ctypes.c_uint32),
                ("first_bad", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("pose_ms", ctypes.c_double)]

    def as_dict(self):
        return {"present": int(self.present), "n_joints": int(self.n_joints), "n_skinned": int(self.n_skinned), "poses": int(self.poses),
                "first_bad": int(self.first_bad), "pose_ms": float(self.pose_ms)}


class MorphStatus(ctypes.Structure):
    """struct ptmi_morph_status: the morph in place and the poses since it was set (include/ptmi.h)"""
    _fields_ = [("present", ctypes.c_uint32), ("n_targets", ctypes.c_uint32), ("n_morphed", ctypes.c_uint32), ("n_records", ctypes.c_uint32),
                ("n_in_skin", ctypes.c_uint32), ("poses", ctypes.c_uint32), ("active_targets", ctypes.c_uint32),
                ("first_bad", ctypes.c_uint32), ("skin_stale", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("pose_ms", ctypes.c_double)]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n not in ("reserved", "pose_ms")}
        d["pose_ms"] = float(self.pose_ms)
        return d


class AlphaParams(ctypes.Structure):
    """ptmi_alpha_params; max_layers 0 picks the default (include/ptmi.h)"""
    _fields_ = [("max_layers", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class AlphaStatus(ctypes.Structure):
    """struct ptmi_alpha_status: the cutoff table in place and what its loops counted since reset_stats (include/ptmi.h)"""
    _fields_ = [("present", ctypes.c_uint32), ("n_materials", ctypes.c_uint32), ("n_cutout", ctypes.c_uint32),
                ("max_layers", ctypes.c_uint32), ("path_passes", ctypes.c_uint64), ("path_exhausted", ctypes.c_uint64),
                ("shadow_passes", ctypes.c_uint64), ("shadow_exhausted", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class AlphaBlendParams(ctypes.Structure):
    """ptmi_alpha_blend_params; max_layers 0 picks the default (include/ptmi.h)"""
    _fields_ = [("max_layers", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class AlphaBlendStatus(ctypes.Structure):
    """struct ptmi_alpha_blend_status: the blend table in place and what the loops counted for it since reset_stats (include/ptmi.h)"""
    _fields_ = [("present", ctypes.c_uint32), ("n_materials", ctypes.c_uint32), ("n_blend", ctypes.c_uint32),
                ("max_layers", ctypes.c_uint32), ("seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("path_tests", ctypes.c_uint64), ("path_passes", ctypes.c_uint64),
                ("shadow_tests", ctypes.c_uint64), ("shadow_passes", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class BakeParams(ctypes.Structure):
    """ptmi_bake_params (include/ptmi.h ptmi_dispatch_bake)"""
    _fields_ = [("first_frame", ctypes.c_uint32), ("bias", ctypes.c_float), ("reserved", ctypes.c_uint32 * 2)]


class BakeStatus(ctypes.Structure):
    _fields_ = [("present", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("covered", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class BakeDenoiseParams(ctypes.Structure):
    """ptmi_bake_denoise_params (include/ptmi.h ptmi_bake_denoise); 0 picks a field's default"""
    _fields_ = [("iterations", ctypes.c_uint32), ("dilate", ctypes.c_uint32), ("phi_color", ctypes.c_float),
                ("phi_normal", ctypes.c_float), ("phi_position", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


class ProbeParams(ctypes.Structure):
    """ptmi_probe_params (include/ptmi.h ptmi_dispatch_probes)"""
    _fields_ = [("first_frame", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class ProbeStatus(ctypes.Structure):
    _fields_ = [("present", ctypes.c_uint32), ("tile", ctypes.c_uint32), ("count", ctypes.c_uint32), ("enabled", ctypes.c_uint32),
                ("texels", ctypes.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ProbeDepthParams(ctypes.Structure):
    """ptmi_probe_depth_params (include/ptmi.h ptmi_set_probe_depth)"""
    _fields_ = [("max_distance", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


class ProbeVisibilityParams(ctypes.Structure):
    """ptmi_probe_visibility_params (include/ptmi.h ptmi_probe_visibility)"""
    _fields_ = [("m", ctypes.c_uint32), ("sharpness_log2", ctypes.c_uint32), ("border", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ScissorStatus(ctypes.Structure):
    """struct ptmi_scissor_status: the frame scissor of the last dispatch, and the paths not traced since reset_stats (include/ptmi.h)"""
    _fields_ = [("x0", ctypes.c_uint32), ("x1", ctypes.c_uint32), ("y0", ctypes.c_uint32), ("y1", ctypes.c_uint32),
                ("applied", ctypes.c_uint32), ("reason", ctypes.c_uint32), ("skipped", ctypes.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Stats(ctypes.Structure):
    _fields_ = [("paths", ctypes.c_uint64), ("segments", ctypes.c_uint64), ("shadow_rays", ctypes.c_uint64),
                ("dispatches", ctypes.c_uint64), ("frames", ctypes.c_uint64),
                ("segments_by_bounce", ctypes.c_uint64 * 64),
                ("gpu_ms", ctypes.c_double), ("extend_ms", ctypes.c_double), ("extend_launches", ctypes.c_uint64),
                ("shade_ms", ctypes.c_double), ("shadow_ms", ctypes.c_double),
                ("bvh_depth", ctypes.c_uint32), ("traversal_used", ctypes.c_uint32),
                ("frames_per_batch_used", ctypes.c_uint32), ("radiance_stride_bytes", ctypes.c_uint32),
                ("shadow_traced", ctypes.c_uint64), ("shade_launches", ctypes.c_uint64), ("shadow_launches", ctypes.c_uint64),
                ("raygen_ms", ctypes.c_double), ("compact_ms", ctypes.c_double), ("accumulate_ms", ctypes.c_double),
                ("upload_ms", ctypes.c_double), ("upload_tree_ms", ctypes.c_double), ("upload_copy_ms", ctypes.c_double),
                ("leaves_used", ctypes.c_uint32), ("leaf_tris_used", ctypes.c_uint32),
                ("extend_variant", ctypes.c_uint32), ("shadow_variant", ctypes.c_uint32), ("verify_failed", ctypes.c_uint64),
                ("tree_builder_used", ctypes.c_uint32), ("shade_tables", ctypes.c_uint32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "segments_by_bounce"}
        d["segments_by_bounce"] = [int(v) for v in self.segments_by_bounce if v]
        return d


# the calls both handle types have, with the same arguments after the handle: ptmi_X(ctx, ...) and ptmi_multi_X(m, ...)
_SHARED = {
    "destroy": [], "last_error": [], "synchronize": [], "reset_stats": [], "resize": [ctypes.c_uint32, ctypes.c_uint32],
    "upload_scene": [ctypes.c_void_p, ctypes.c_uint32] * 4,
    "upload_atlas": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int],
    "set_options": [ctypes.c_void_p], "get_options": [ctypes.c_void_p], "dispatch": [ctypes.c_void_p, ctypes.c_uint32],
    "throttle": [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)], "read_output": [ctypes.c_void_p, ctypes.c_size_t],
    "write_output": [ctypes.c_void_p, ctypes.c_size_t], "blit": [ctypes.c_void_p, ctypes.c_size_t] * 2,
    "get_stats": [ctypes.c_void_p],
    "upload_environment": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p],
    "set_environment": [ctypes.c_void_p],
    "set_medium": [ctypes.c_void_p],
    "upload_medium_density": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p],
    "set_aovs": [ctypes.c_uint32], "get_aovs": [ctypes.POINTER(ctypes.c_uint32)], "read_aov": [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t],
    "set_moments": [ctypes.c_uint32], "get_moments": [ctypes.POINTER(ctypes.c_uint32)], "read_moments": [ctypes.c_void_p, ctypes.c_size_t],
    "denoise": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t], "blit_denoised": [ctypes.c_void_p, ctypes.c_size_t] * 2,
    "dispatch_adaptive": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32], "adaptive_status": [ctypes.c_void_p],
    "update_triangles": [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p],
    "update_materials": [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p],
    "update_lights": [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p],
    "scene_update_status": [ctypes.c_void_p],
    "rebuild_tree": [ctypes.c_void_p], "rebuild_status": [ctypes.c_void_p],
    "set_alpha_cutoff": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p], "alpha_status": [ctypes.c_void_p],
    "set_alpha_blend": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p], "alpha_blend_status": [ctypes.c_void_p],
    "set_triangle_groups": [ctypes.c_void_p, ctypes.c_uint32], "transform_groups": [ctypes.c_void_p, ctypes.c_uint32],
    "transform_status": [ctypes.c_void_p],
    "set_skin": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32], "pose_skin": [ctypes.c_void_p, ctypes.c_uint32],
    "skin_status": [ctypes.c_void_p],
    "set_morph": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32],
    "pose_morph": [ctypes.c_void_p, ctypes.c_uint32], "morph_status": [ctypes.c_void_p],
    "set_projections": [ctypes.c_uint32], "get_projections": [ctypes.POINTER(ctypes.c_uint32)],
}
# lightmap baking (include/ptmi.h ptmi_upload_bake_surface ...): a single context's calls, arguments after the handle
_BAKE = {
    "ptmi_upload_bake_surface": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32],
    "ptmi_dispatch_bake": [ctypes.c_void_p, ctypes.c_uint32],
    "ptmi_bake_status": [ctypes.c_void_p],
    "ptmi_bake_dilate": [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_debug_bake_rays": [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6,
    "ptmi_bake_denoise": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_bake_denoised_device_ptr": [],
    "ptmi_write_moments": [ctypes.c_void_p, ctypes.c_size_t],
}
# light probes (include/ptmi.h ptmi_upload_probes ...): likewise
_PROBES = {
    "ptmi_upload_probes": [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32],
    "ptmi_dispatch_probes": [ctypes.c_void_p, ctypes.c_uint32],
    "ptmi_probe_status": [ctypes.c_void_p],
    "ptmi_probe_sh": [ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_probe_irradiance": [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_debug_probe_rays": [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 6,
    "ptmi_set_probe_depth": [ctypes.c_void_p],
    "ptmi_get_probe_depth": [ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p],
    "ptmi_read_probe_depth": [ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_write_probe_depth": [ctypes.c_void_p, ctypes.c_size_t],
    "ptmi_probe_depth_device_ptr": [],
    "ptmi_probe_visibility": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t],
}
_lib = None


def load():
    """Loads libptmi.so; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PtmiError(-2, f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build`")
        L = ctypes.CDLL(LIB_PATH)
        for name in EXPORTS:
            getattr(L, name)
        if L.ptmi_abi_version() != ABI_VERSION:
            raise PtmiError(-1, f"{LIB_PATH} has ABI {L.ptmi_abi_version()}, this binding expects {ABI_VERSION}: rebuild it")
        vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
        for prefix in ("ptmi_", "ptmi_multi_"):
            for name, args in _SHARED.items():
                getattr(L, prefix + name).argtypes = [vp] + args
        L.ptmi_last_error.restype = L.ptmi_multi_last_error.restype = ctypes.c_char_p
        L.ptmi_create.argtypes = [ctypes.c_int, vp]
        L.ptmi_output_device_ptr.restype = vp
        L.ptmi_output_device_ptr.argtypes = [vp]
        L.ptmi_bind_output_device.argtypes = [vp, vp, sz]
        L.ptmi_set_stream.argtypes = [vp, vp]
        L.ptmi_get_size.argtypes = [vp, vp, vp]
        L.ptmi_debug_image_stats.argtypes = [vp, u32, vp, u32, vp]
        L.ptmi_debug_build_image.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_read_image.argtypes = [vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_raygen.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_intersect.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_occluded.argtypes = [vp, u32, vp, vp, vp, vp]
        L.ptmi_debug_math.argtypes = [vp, ctypes.c_int, u32, vp, vp, vp, vp]
        L.ptmi_debug_exact_math.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        L.ptmi_multi_create.argtypes = [ctypes.c_int, vp, u32, vp]
        L.ptmi_multi_count.argtypes = [vp]
        L.ptmi_multi_context.restype = vp
        L.ptmi_multi_context.argtypes = [vp, ctypes.c_int]
        L.ptmi_multi_gather.argtypes = [vp]
        L.ptmi_multi_gather_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.ptmi_multi_gather_planes.argtypes = [vp, u32]
        L.ptmi_aov_device_ptr.restype = vp
        L.ptmi_aov_device_ptr.argtypes = [vp, u32]
        L.ptmi_moments_device_ptr.restype = vp
        L.ptmi_moments_device_ptr.argtypes = [vp]
        L.ptmi_denoised_device_ptr.restype = vp
        L.ptmi_denoised_device_ptr.argtypes = [vp]
        L.ptmi_reproject.argtypes = [vp, vp, vp, vp]
        L.ptmi_reproject_status.argtypes = [vp, vp]
        L.ptmi_debug_center_rays.argtypes = [vp, vp, vp, vp, sz]
        L.ptmi_set_motion.argtypes = [vp, u32]
        L.ptmi_get_motion.argtypes = [vp, vp]
        L.ptmi_motion_commit.argtypes = [vp]
        L.ptmi_motion_status.argtypes = [vp, vp]
        L.ptmi_read_motion.argtypes = [vp, vp, sz]
        L.ptmi_motion_device_ptr.restype = vp
        L.ptmi_motion_device_ptr.argtypes = [vp]
        L.ptmi_debug_motion_prev.argtypes = [vp, u32, u32, vp]
        L.ptmi_environment_status.argtypes = [vp, vp]
        L.ptmi_debug_env_lookup.argtypes = [vp, u32, vp, vp]
        L.ptmi_debug_env_sample.argtypes = [vp, u32, vp, vp, vp, vp]
        L.ptmi_debug_env_table.argtypes = [vp, u32, u32, ctypes.c_int, vp, vp, vp, ctypes.POINTER(ctypes.c_double)]
        L.ptmi_get_medium.argtypes = [vp, vp, ctypes.POINTER(u32)]
        L.ptmi_debug_medium_step.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ptmi_debug_medium_tr.argtypes = [vp, u32, vp, vp, vp, vp]
        L.ptmi_medium_grid_status.argtypes = [vp, vp]
        L.ptmi_debug_medium_density.argtypes = [vp, u32, vp, vp]
        L.ptmi_debug_medium_grid_check.argtypes = [vp, vp, u32, u32, u32, vp, vp]
        L.ptmi_debug_medium_track.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.ptmi_debug_alpha_intersect.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.ptmi_debug_alpha_occluded.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.ptmi_normal_matrix.restype = None
        L.ptmi_normal_matrix.argtypes = [vp, vp]
        L.ptmi_debug_read_triangles.argtypes = [vp, u32, u32, vp]
        for name, args in list(_BAKE.items()) + list(_PROBES.items()):      # (a tool that loads an older build of the ABI takes them off EXPORTS)
            if name in EXPORTS:
                getattr(L, name).argtypes = [vp] + args
        if "ptmi_debug_probe_tables" in EXPORTS:
            L.ptmi_debug_probe_tables.argtypes = [u32, vp, vp]
        if "ptmi_probe_depth_device_ptr" in EXPORTS:
            L.ptmi_probe_depth_device_ptr.restype = vp
        if "ptmi_bake_denoised_device_ptr" in EXPORTS:
            L.ptmi_bake_denoised_device_ptr.restype = vp
        if "ptmi_scissor_status" in EXPORTS:
            L.ptmi_scissor_status.argtypes = [vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def image_stats(scene):
    """Host-only report on the traversal image ptmi_upload_scene would build (include/ptmi.h: ptmi_debug_image_stats)."""
    L = load()
    out = (ctypes.c_double * 8)()
    rc = L.ptmi_debug_image_stats(_p(scene.tris), len(scene.tris), _p(scene.nodes), len(scene.nodes), out)
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    keys = ("wide_nodes", "leaves", "depth", "quantised_nodes", "stream_dwords", "containment_violations",
            "mean_area_growth", "stream_mismatches")
    return dict(zip(keys, list(out)))


def probe_tables(tile):
    """Host-only: the two tables of a probe tile (include/ptmi.h ptmi_debug_probe_tables): (tile * tile, 4) float32 (d_t, dw_t) and
    (tile * tile, 9) float32 basis"""
    L = load()
    dir_dw, basis = np.zeros((tile * tile, 4), np.float32), np.zeros((tile * tile, 9), np.float32)
    rc = L.ptmi_debug_probe_tables(tile, _p(dir_dw), _p(basis))
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    return dir_dw, basis


def normal_matrix(m):
    """Host-only: the 3 x 3 that goes with the 3 x 4 affine m for the normals (include/ptmi.h ptmi_normal_matrix): the cofactors of
    its upper 3 x 3, as 9 float32, row-major."""
    m = np.ascontiguousarray(m, np.float32).reshape(12)
    nm = np.zeros(9, np.float32)
    load().ptmi_normal_matrix(_p(m), _p(nm))
    return nm


def group_ops(ops):
    """GROUP_TRANSFORM records from an array of them, or from (group, m[, nm]) tuples; nm None / absent derives it (normal_matrix)"""
    if isinstance(ops, np.ndarray) and ops.dtype == GROUP_TRANSFORM:
        return np.ascontiguousarray(ops)
    out = np.zeros(len(ops), GROUP_TRANSFORM)
    for i, op in enumerate(ops):
        g, m, nm = (tuple(op) + (None,))[:3]
        m = np.asarray(m, np.float32).reshape(12)
        out[i]["group"], out[i]["m"] = g, m
        out[i]["nm"] = normal_matrix(m) if nm is None else np.asarray(nm, np.float32).reshape(9)
    return out


def joint_ops(joints):
    """JOINT_TRANSFORM records of a complete pose from an array of them, or from one (m, nm) pair per joint in joint order; nm None
    derives it (normal_matrix). Record i names joint i."""
    if isinstance(joints, np.ndarray) and joints.dtype == JOINT_TRANSFORM:
        return np.ascontiguousarray(joints)
    return group_ops([(i,) + tuple(j) for i, j in enumerate(joints)])


def _env_texels(texels):
    """(texels as a contiguous (H, W, 4) float16 / float32 array, its PTMI_ATLAS_* format)"""
    a = np.ascontiguousarray(texels)
    if a.dtype not in (np.float16, np.float32):
        a = a.astype(np.float32)
    assert a.ndim == 3 and a.shape[2] == 4, "an environment is (H, W, 4) RGBA texels"
    return a, ATLAS_RGBA16F if a.dtype == np.float16 else ATLAS_RGBA32F


def env_table(texels, fmt=None, width=None, height=None):
    """Host-only: the tables upload_environment would build (include/ptmi.h: ptmi_debug_env_table):
    (c [H, W] f32, prob [H * W] f32, alias [H * W] u32, weight_sum). fmt / width / height override what the array says (for tests)."""
    L = load()
    a, f = _env_texels(texels)
    h, w = a.shape[:2]
    w, h, f = (w if width is None else width), (h if height is None else height), (f if fmt is None else fmt)
    n = a.shape[0] * a.shape[1]
    c, prob, alias = np.zeros(a.shape[:2], np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    ws = ctypes.c_double(0.0)
    rc = L.ptmi_debug_env_table(_p(a), w, h, f, _p(c), _p(prob), _p(alias), ctypes.byref(ws))
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    return c, prob, alias, ws.value


def medium_grid_check(rho, filter=FILTER_NEAREST, dims=None, reserved=(0, 0, 0, 0, 0, 0, 0), medium=None):
    """Host-only: the checks upload_medium_density would run (include/ptmi.h: ptmi_debug_medium_grid_check) for the grid rho, shape
    (nz, ny, nx), on the medium given as set_medium's keywords (None: without the optical-depth limit); the MediumGridStatus the
    upload would leave, or PtmiError. dims = (nx, ny, nz) overrides what the array's shape says."""
    L = load()
    a = np.ascontiguousarray(rho, np.float32)
    if dims is None:
        dims = a.shape[::-1]
    prm = MediumGrid(filter, (ctypes.c_uint32 * 7)(*reserved))
    m = None
    if medium is not None:
        f3 = ctypes.c_float * 3
        alb = np.broadcast_to(np.asarray(medium.get("albedo", 1.0), np.float32), (3,))
        m = ctypes.byref(Medium(medium["sigma_t"], f3(*alb), medium.get("g", 0.0), f3(*medium["box"][0]), f3(*medium["box"][1]),
                                (ctypes.c_uint32 * 5)()))
    st = MediumGridStatus()
    rc = L.ptmi_debug_medium_grid_check(m, _p(a), dims[0], dims[1], dims[2], ctypes.byref(prm), ctypes.byref(st))
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    return st


class ImageInfo(ctypes.Structure):
    _fields_ = [("leaves_used", ctypes.c_uint32), ("n_wnodes", ctypes.c_uint32), ("n_tris", ctypes.c_uint32),
                ("root_ref", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("n_leaves", ctypes.c_uint32),
                ("max_leaf_tris", ctypes.c_uint32), ("quantised", ctypes.c_uint32),
                ("root_min", ctypes.c_float * 3), ("root_max", ctypes.c_float * 3),
                ("pad", ctypes.c_float), ("safe_origin", ctypes.c_float),
                ("q_origin", ctypes.c_float * 3), ("q_scale", ctypes.c_float * 3), ("ref_depth", ctypes.c_uint32)]


def build_image(scene, leaves=0, leaf_tris=0, keep_reference_tree=0):
    """Host-only: the traversal image ptmi_upload_scene would build (include/ptmi.h: ptmi_debug_build_image), as numpy arrays:
    (info, wnodes [n, 16] f32, qnodes [n, 8] u32 or None, tripos [m, 12] f32, leafbox [n_triangles, 8] f32 or None)."""
    L = load()
    o = Options()
    o.leaves, o.leaf_tris, o.keep_reference_tree = leaves, leaf_tris, keep_reference_tree
    info = ImageInfo()
    args = (_p(scene.tris), len(scene.tris), _p(scene.nodes), len(scene.nodes), ctypes.byref(o), ctypes.byref(info))
    rc = L.ptmi_debug_build_image(*args, None, None, None, None)
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    wn = np.zeros((info.n_wnodes, 16), np.float32)
    qn = np.zeros((info.n_wnodes, 8), np.uint32) if info.quantised else None
    tp = np.zeros((info.n_tris, 12), np.float32)
    lb = np.zeros((len(scene.tris), 8), np.float32) if info.leaves_used == 2 else None
    rc = L.ptmi_debug_build_image(*args, _p(wn), _p(qn), _p(tp), _p(lb))
    if rc != 0:
        raise PtmiError(rc, L.ptmi_last_error(None).decode())
    return info, wn, qn, tp, lb


def _read_image(L, h, n_triangles, ck):
    """ptmi_debug_read_image on context handle h, whose last upload had n_triangles triangles (the rows of leafbox8)"""
    info = ImageInfo()
    ck(L.ptmi_debug_read_image(h, ctypes.byref(info), None, None, None, None))
    wn = np.zeros((info.n_wnodes, 16), np.float32)
    qn = np.zeros((info.n_wnodes, 8), np.uint32) if info.quantised else None
    tp = np.zeros((info.n_tris, 12), np.float32)
    lb = np.zeros((n_triangles, 8), np.float32) if info.leaves_used == 2 else None
    ck(L.ptmi_debug_read_image(h, ctypes.byref(info), _p(wn), _p(qn), _p(tp), _p(lb)))
    return info, wn, qn, tp, lb


def _aov(name):
    if name not in AOVS:
        raise ValueError(f"unknown AOV plane {name!r}: one of {sorted(AOVS)}")
    return AOVS[name]


class _Handle:
    """What Context and MultiContext share. self._c holds the calls both C handle types have (_SHARED), bound once by the
    class's prefix: self._c.resize is ptmi_resize for a Context and ptmi_multi_resize for a MultiContext."""

    _prefix = None

    def __init__(self, *create_args):
        self.L = load()
        c = self._c
        h = ctypes.c_void_p()
        rc = getattr(self.L, self._prefix + "create")(*create_args, ctypes.byref(h))
        if rc != 0:
            raise PtmiError(rc, c.last_error(None).decode())
        self.h = h
        self.width = self.height = 0
        self._uploaded_tris = 0

    @functools.cached_property
    def _c(self):
        return types.SimpleNamespace(**{name: getattr(self.L, self._prefix + name) for name in _SHARED})

    def _ck(self, rc):
        if rc != 0:
            raise PtmiError(rc, self._c.last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._c.destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- resources -----------------------------------------------------------
    def upload_scene(self, scene):
        for a, dt in ((scene.tris, layout.TRIANGLE), (scene.mats, layout.MATERIAL),
                      (scene.nodes, layout.BVH_NODE), (scene.lights, layout.LIGHT)):
            assert a.dtype == dt and a.flags.c_contiguous
        self._ck(self._c.upload_scene(self.h, _p(scene.tris), len(scene.tris), _p(scene.mats), len(scene.mats),
                                      _p(scene.nodes), len(scene.nodes), _p(scene.lights), len(scene.lights)))
        self._uploaded_tris = len(scene.tris)
        a = scene.atlas
        if a is None:
            self._ck(self._c.upload_atlas(self.h, None, 0, 0, 0))
        else:
            assert a.ndim == 3 and a.shape[2] == 4 and a.flags.c_contiguous
            fmt = ATLAS_RGBA16F if a.dtype == np.float16 else ATLAS_RGBA32F
            self._ck(self._c.upload_atlas(self.h, _p(a), a.shape[1], a.shape[0], fmt))

    # -- edits of the loaded scene in place (include/ptmi.h ptmi_update_triangles) ------------------------------------
    def _update(self, call, first, records, dtype):
        records = np.ascontiguousarray(records)
        assert records.dtype == dtype
        self._ck(call(self.h, first, len(records), _p(records) if len(records) else None))

    def update_triangles(self, first, tris):
        """writes the TRIANGLE records tris over the loaded scene's from index `first` on and refits the trees on the device; the
        caller restarts accumulation"""
        self._update(self._c.update_triangles, first, tris, layout.TRIANGLE)

    def update_materials(self, first, mats):
        self._update(self._c.update_materials, first, mats, layout.MATERIAL)

    def update_lights(self, first, lights):
        self._update(self._c.update_lights, first, lights, layout.LIGHT)

    def scene_update_status(self):
        st = SceneUpdateStatus()
        self._ck(self._c.scene_update_status(self.h, ctypes.byref(st)))
        return st

    # -- the walked tree rebuilt in place (include/ptmi.h ptmi_rebuild_tree) --------------------------------------------
    def rebuild_tree(self, builder=0, reserved=(0, 0, 0, 0, 0, 0, 0)):
        """builds the walked own-leaf tree anew from the triangles as they stand on the device and swaps it in: the image a fresh
        upload of the edited scene would build. builder 1: the host's, 2 (and 0): the device's where it applies. Returns the
        RebuildStatus."""
        prm = RebuildParams(builder, (ctypes.c_uint32 * 7)(*reserved))
        self._ck(self._c.rebuild_tree(self.h, ctypes.byref(prm)))
        return self.rebuild_status()

    def rebuild_status(self):
        st = RebuildStatus()
        self._ck(self._c.rebuild_status(self.h, ctypes.byref(st)))
        return st

    # -- triangle groups moved by matrix on the device (include/ptmi.h ptmi_set_triangle_groups) ------------------------
    def set_triangle_groups(self, groups, n_triangles=None):
        """tags every uploaded triangle with a group id (uint32 per triangle, uploaded order) and snapshots the rest pose; None
        removes the table. n_triangles overrides the array's length (for tests)."""
        if groups is None:
            self._ck(self._c.set_triangle_groups(self.h, None, 0))
            return
        g = np.ascontiguousarray(groups, np.uint32).reshape(-1)
        self._ck(self._c.set_triangle_groups(self.h, _p(g), len(g) if n_triangles is None else n_triangles))

    def transform_groups(self, ops, n_ops=None):
        """sets the matrices of the groups named: every member triangle becomes T(rest pose), and the trees are refitted on the
        device. ops: GROUP_TRANSFORM records, or (group, m[, nm]) tuples with m a 3 x 4 row-major affine (see group_ops). n_ops
        overrides the count passed (for tests; ops None then passes NULL)."""
        if ops is None:
            self._ck(self._c.transform_groups(self.h, None, n_ops or 0))
            return
        rec = group_ops(ops)
        self._ck(self._c.transform_groups(self.h, _p(rec) if len(rec) else None, len(rec) if n_ops is None else n_ops))

    def transform_status(self):
        st = TransformStatus()
        self._ck(self._c.transform_status(self.h, ctypes.byref(st)))
        return st

    # -- skinned triangles posed on the device (include/ptmi.h ptmi_set_skin) --------------------------------------------
    def set_skin(self, triangles, corners=None, n_joints=0, n_skinned=None):
        """lists the skinned triangles (ascending uint32 indices, uploaded order) with three layout.SKIN_CORNER records each, for a
        skeleton of n_joints, and snapshots their rest pose; triangles None removes the skin. corners None passes NULL and n_skinned
        overrides the count passed (for tests)."""
        if triangles is None:
            self._ck(self._c.set_skin(self.h, None, None, 0, n_joints))
            return
        t = np.ascontiguousarray(triangles, np.uint32).reshape(-1)
        q = None if corners is None else np.ascontiguousarray(corners, layout.SKIN_CORNER).reshape(-1)
        if q is not None and len(q) != 3 * len(t):
            raise ValueError(f"{len(q)} corner records for {len(t)} triangles: three each")
        self._ck(self._c.set_skin(self.h, _p(t) if len(t) else None, None if q is None or not len(q) else _p(q),
                                  len(t) if n_skinned is None else n_skinned, n_joints))

    def pose_skin(self, joints, n_joints=None):
        """poses the skin: every listed triangle becomes the blend of its joints' matrices applied to its rest pose, and the trees are
        refitted on the device. joints: a complete pose, JOINT_TRANSFORM records or one (m, nm_or_None) pair per joint (see joint_ops).
        n_joints overrides the count passed (for tests; joints None then passes NULL)."""
        if joints is None:
            self._ck(self._c.pose_skin(self.h, None, n_joints or 0))
            return
        rec = joint_ops(joints)
        self._ck(self._c.pose_skin(self.h, _p(rec) if len(rec) else None, len(rec) if n_joints is None else n_joints))

    def skin_status(self):
        st = SkinStatus()
        self._ck(self._c.skin_status(self.h, ctypes.byref(st)))
        return st

    # -- morphed triangles posed on the device (include/ptmi.h ptmi_set_morph) ------------------------------------------
    def set_morph(self, triangles, row_start=None, deltas=None, n_targets=0, n_morphed=None):
        """lists the morphed triangles (ascending uint32 indices, uploaded order) with their layout.MORPH_DELTA records in
        compressed-row form (row e: deltas[row_start[e]:row_start[e + 1]], ascending by target) for n_targets targets, and snapshots
        their rest pose; triangles None removes the morph. row_start / deltas None pass NULL and n_morphed overrides the count passed
        (for tests)."""
        if triangles is None:
            self._ck(self._c.set_morph(self.h, None, None, None, 0, n_targets))
            return
        t = np.ascontiguousarray(triangles, np.uint32).reshape(-1)
        r = None if row_start is None else np.ascontiguousarray(row_start, np.uint32).reshape(-1)
        d = None if deltas is None else np.ascontiguousarray(deltas, layout.MORPH_DELTA).reshape(-1)
        if r is not None and len(r) != len(t) + 1:
            raise ValueError(f"{len(r)} row bounds for {len(t)} triangles: one more than triangles")
        if r is not None and d is not None and len(r) and int(r.max()) > len(d):
            raise ValueError(f"row_start reaches {int(r.max())} of {len(d)} records")
        self._ck(self._c.set_morph(self.h, _p(t) if len(t) else None, _p(r), None if d is None or not len(d) else _p(d),
                                   len(t) if n_morphed is None else n_morphed, n_targets))

    def pose_morph(self, weights, n_targets=None):
        """poses the morph: every listed triangle becomes its rest record plus the weighted deltas of its row (targets of weight zero
        are skipped), and the trees are refitted on the device; triangles the skin in place lists too go to the skin's rest pose
        instead and wait for pose_skin. weights: one float per target. n_targets overrides the count passed (for tests; weights None
        then passes NULL)."""
        if weights is None:
            self._ck(self._c.pose_morph(self.h, None, n_targets or 0))
            return
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        self._ck(self._c.pose_morph(self.h, _p(w) if len(w) else None, len(w) if n_targets is None else n_targets))

    def morph_status(self):
        st = MorphStatus()
        self._ck(self._c.morph_status(self.h, ctypes.byref(st)))
        return st

    # -- alpha cutouts (include/ptmi.h ptmi_set_alpha_cutoff) ---------------------------------------------------------
    def set_alpha_cutoff(self, cutoff, max_layers=0, reserved=(0, 0, 0), n_materials=None):
        """The per-material cutoff table of the loaded scene: one float per uploaded material, 0 = opaque, > 0 = a hit is absent
        where the albedo map's alpha is below it. cutoff None removes the table. max_layers 0 picks the default; n_materials
        overrides the array's length (for tests)."""
        prm = AlphaParams(max_layers, (ctypes.c_uint32 * 3)(*reserved))
        if cutoff is None:
            self._ck(self._c.set_alpha_cutoff(self.h, None, 0, ctypes.byref(prm)))
            return
        a = np.ascontiguousarray(cutoff, np.float32).reshape(-1)
        self._ck(self._c.set_alpha_cutoff(self.h, _p(a), len(a) if n_materials is None else n_materials, ctypes.byref(prm)))

    def alpha_status(self):
        st = AlphaStatus()
        self._ck(self._c.alpha_status(self.h, ctypes.byref(st)))
        return st

    # -- alpha blending (include/ptmi.h ptmi_set_alpha_blend) ----------------------------------------------------------
    def set_alpha_blend(self, factor, max_layers=0, seed=0, reserved=(0, 0), n_materials=None):
        """The per-material blend table of the loaded scene: one float per uploaded material, < 0 = not blended, f in [0, 1] = a
        hit is absent where f * the albedo map's alpha <= the ray's own hash. factor None removes the table. max_layers 0 picks the
        default; n_materials overrides the array's length (for tests)."""
        prm = AlphaBlendParams(max_layers, seed, (ctypes.c_uint32 * 2)(*reserved))
        if factor is None:
            self._ck(self._c.set_alpha_blend(self.h, None, 0, ctypes.byref(prm)))
            return
        a = np.ascontiguousarray(factor, np.float32).reshape(-1)
        self._ck(self._c.set_alpha_blend(self.h, _p(a), len(a) if n_materials is None else n_materials, ctypes.byref(prm)))

    def alpha_blend_status(self):
        st = AlphaBlendStatus()
        self._ck(self._c.alpha_blend_status(self.h, ctypes.byref(st)))
        return st

    def upload_environment(self, texels, intensity=0.0, rotation=0.0, sample=0, reserved=(0, 0, 0, 0, 0)):
        """The environment map behind every miss (include/ptmi.h ptmi_upload_environment): (H, W, 4) float16 / float32 texels,
        equirectangular, row 0 at the +Y pole. texels None removes it."""
        if texels is None:
            self._ck(self._c.upload_environment(self.h, None, 0, 0, 0, None))
            return
        a, fmt = _env_texels(texels)
        prm = Environment(intensity, rotation, sample, (ctypes.c_uint32 * 5)(*reserved))
        self._ck(self._c.upload_environment(self.h, _p(a), a.shape[1], a.shape[0], fmt, ctypes.byref(prm)))

    def set_environment(self, intensity=0.0, rotation=0.0, sample=0, reserved=(0, 0, 0, 0, 0)):
        """intensity / rotation / sample of the map in place, without a re-upload"""
        prm = Environment(intensity, rotation, sample, (ctypes.c_uint32 * 5)(*reserved))
        self._ck(self._c.set_environment(self.h, ctypes.byref(prm)))

    def set_medium(self, sigma_t=None, albedo=(1.0, 1.0, 1.0), g=0.0, box=None, reserved=(0, 0, 0, 0, 0)):
        """One homogeneous scattering medium inside the axis-aligned box (min, max) (include/ptmi.h ptmi_set_medium): extinction
        sigma_t per unit length, single-scattering albedo per channel (a scalar: all three), Henyey-Greenstein asymmetry g.
        sigma_t None removes it."""
        if sigma_t is None:
            self._ck(self._c.set_medium(self.h, None))
            return
        alb = np.broadcast_to(np.asarray(albedo, np.float32), (3,))
        f3 = ctypes.c_float * 3
        m = Medium(sigma_t, f3(*alb), g, f3(*box[0]), f3(*box[1]), (ctypes.c_uint32 * 5)(*reserved))
        self._ck(self._c.set_medium(self.h, ctypes.byref(m)))

    def upload_medium_density(self, rho, filter=FILTER_NEAREST, dims=None, reserved=(0, 0, 0, 0, 0, 0, 0)):
        """A density grid for the medium in place (include/ptmi.h ptmi_upload_medium_density): float32 multipliers in [0, 1] of its
        sigma_t as an array of shape (nz, ny, nx), x fastest, stretched over its box; filter 0 nearest, 1 trilinear. rho None removes
        the grid. dims = (nx, ny, nz) overrides what the array's shape says."""
        if rho is None:
            self._ck(self._c.upload_medium_density(self.h, None, 0, 0, 0, None))
            return
        a = np.ascontiguousarray(rho, np.float32)
        if dims is None:
            assert a.ndim == 3, "a density grid is an array of shape (nz, ny, nx)"
            dims = a.shape[::-1]
        prm = MediumGrid(filter, (ctypes.c_uint32 * 7)(*reserved))
        self._ck(self._c.upload_medium_density(self.h, _p(a), dims[0], dims[1], dims[2], ctypes.byref(prm)))

    def resize(self, width, height):
        self._ck(self._c.resize(self.h, width, height))
        self.width, self.height = width, height

    def _before_set_options(self, o, kw):
        """set_options starts from the current options o, adjusted here before the keywords kw are applied"""

    def set_options(self, **kw):
        o = self.options()
        self._before_set_options(o, kw)
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k}")
            setattr(o, k, int(v))
        self._ck(self._c.set_options(self.h, ctypes.byref(o)))

    def options(self):
        o = Options()
        self._ck(self._c.get_options(self.h, ctypes.byref(o)))
        return o

    # -- the compute pass ------------------------------------------------------
    def dispatch(self, camera, n_frames=1):
        assert camera.dtype == layout.CAMERA
        self._ck(self._c.dispatch(self.h, _p(camera), n_frames))

    def synchronize(self):
        self._ck(self._c.synchronize(self.h))

    def throttle(self, max_in_flight=0xFFFFFFFF):
        """Blocks until at most max_in_flight dispatches are unfinished (default: only polls); returns how many are."""
        n = ctypes.c_uint32(0)
        self._ck(self._c.throttle(self.h, max_in_flight, ctypes.byref(n)))
        return int(n.value)

    def read_output(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(self._c.read_output(self.h, _p(out), out.size))
        return out

    def write_output(self, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        self._ck(self._c.write_output(self.h, _p(arr), arr.size))

    def stats(self):
        s = Stats()
        self._ck(self._c.get_stats(self.h, ctypes.byref(s)))
        return s

    def reset_stats(self):
        self._ck(self._c.reset_stats(self.h))

    # -- first-hit planes (include/ptmi.h ptmi_set_aovs) ----------------------------
    def set_aovs(self, *planes):
        """set_aovs('albedo', 'normal', 'id') or set_aovs(mask); set_aovs() turns every plane off"""
        mask = 0
        for p in planes:
            mask |= int(p) if not isinstance(p, str) else _aov(p)[0]
        self._ck(self._c.set_aovs(self.h, mask))

    def aovs(self):
        """the names of the planes that are on"""
        m = ctypes.c_uint32(0)
        self._ck(self._c.get_aovs(self.h, ctypes.byref(m)))
        return tuple(n for n, (bit, _, _) in AOVS.items() if m.value & bit)

    def read_aov(self, name):
        """(H, W, 4) float32 for 'albedo' / 'normal', (H, W, 2) uint32 (triangle, material) for 'id'"""
        bit, dt, ch = _aov(name)
        out = np.empty((self.height, self.width, ch), dt)
        self._ck(self._c.read_aov(self.h, bit, _p(out), out.nbytes))
        return out

    # -- sample moments and the denoiser (include/ptmi.h ptmi_set_moments, ptmi_denoise) ----------------------
    def set_moments(self, on=True):
        self._ck(self._c.set_moments(self.h, int(on)))

    def moments(self):
        """whether the sample-moments plane is on"""
        m = ctypes.c_uint32(0)
        self._ck(self._c.get_moments(self.h, ctypes.byref(m)))
        return bool(m.value)

    # -- camera projections (include/ptmi.h ptmi_set_projections) ------------------------------------------------
    def set_projections(self, on=True):
        """while on, the projection words of every camera this handle is given are honoured (layout.make_camera(projection=, ymag=))"""
        self._ck(self._c.set_projections(self.h, int(on)))

    def projections(self):
        m = ctypes.c_uint32(0)
        self._ck(self._c.get_projections(self.h, ctypes.byref(m)))
        return bool(m.value)

    def read_moments(self):
        """(H, W, 4) float32: mean luminance, mean squared luminance, frames folded, 0"""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(self._c.read_moments(self.h, _p(out), out.size))
        return out

    def denoise(self, iterations=0, demodulate=0, phi_color=0.0, phi_normal=0.0, phi_depth=0.0, reserved=(0, 0, 0), dst=True):
        """the denoised output buffer, (H, W, 4) float32 with w = 0; 0 picks a parameter's default (include/ptmi.h).
        dst=False: only queue it on the context's stream (denoised_device_ptr, blit_denoised) and return None."""
        prm = DenoiseParams(iterations, demodulate, phi_color, phi_normal, phi_depth, (ctypes.c_uint32 * 3)(*reserved))
        out = np.empty((self.height, self.width, 4), np.float32) if dst else None
        self._ck(self._c.denoise(self.h, ctypes.byref(prm), _p(out), 0 if out is None else out.size))
        return out

    def blit_denoised(self, want_f32=True, want_rgba8=True):
        """blit() of the denoised plane: (canvas float RGBA or None, canvas uint8 RGBA or None), row 0 = top"""
        f = np.empty((self.height, self.width, 4), np.float32) if want_f32 else None
        b = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        self._ck(self._c.blit_denoised(self.h, _p(f), 0 if f is None else f.size, _p(b), 0 if b is None else b.size))
        return f, b

    # -- adaptive sampling (include/ptmi.h ptmi_dispatch_adaptive) ---------------------------------------------

    def _dispatch_adaptive(self, camera, rounds, threshold, floor, min_frames, max_frames, step, neighbourhood, reserved):
        assert camera.dtype == layout.CAMERA
        prm = AdaptiveParams(threshold, floor, min_frames, max_frames, step, neighbourhood, (ctypes.c_uint32 * 2)(*reserved))
        self._ck(self._c.dispatch_adaptive(self.h, _p(camera), ctypes.byref(prm), rounds))

    def adaptive_status(self):
        st = AdaptiveStatus()
        self._ck(self._c.adaptive_status(self.h, ctypes.byref(st)))
        return st


class Context(_Handle):
    """One device context = the reference Renderer's GPU resources (bind group 0)."""

    _prefix = "ptmi_"

    def __init__(self, device=0):
        super().__init__(device)

    def output_device_ptr(self):
        return self.L.ptmi_output_device_ptr(self.h)

    def bind_output_device(self, ptr, nbytes):
        self._ck(self.L.ptmi_bind_output_device(self.h, ctypes.c_void_p(ptr), nbytes))

    def set_stream(self, stream_handle):
        self._ck(self.L.ptmi_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def blit(self, want_f32=True, want_rgba8=True):
        """The reference's blit pass (blit.wgsl): (canvas float RGBA or None, canvas uint8 RGBA or None), row 0 = top."""
        f = np.empty((self.height, self.width, 4), np.float32) if want_f32 else None
        b = np.empty((self.height, self.width, 4), np.uint8) if want_rgba8 else None
        self._ck(self.L.ptmi_blit(self.h, _p(f), 0 if f is None else f.size, _p(b), 0 if b is None else b.size))
        return f, b

    # -- device addresses of the planes, and adaptive rounds on this context ---------------------------------
    def aov_device_ptr(self, name):
        return self.L.ptmi_aov_device_ptr(self.h, _aov(name)[0])

    def moments_device_ptr(self):
        return self.L.ptmi_moments_device_ptr(self.h)

    def denoised_device_ptr(self):
        return self.L.ptmi_denoised_device_ptr(self.h)

    def dispatch_adaptive(self, camera, rounds=1, threshold=0.0, floor=0.0, min_frames=0, max_frames=0, step=0, neighbourhood=0,
                          reserved=(0, 0)):
        """`rounds` rounds of `step` further frames for the pixels the rule of include/ptmi.h selects; needs set_moments().
        camera frame_index 0 restarts, any other value continues from the per-pixel counts."""
        self._dispatch_adaptive(camera, rounds, threshold, floor, min_frames, max_frames, step, neighbourhood, reserved)

    # -- reprojection (include/ptmi.h ptmi_reproject) -----------------------------------------------------------
    def reproject(self, from_cam, to_cam, max_history=0, depth_tolerance=0.0, match_ids=0, reserved=(0, 0, 0, 0, 0)):
        """rewrites the output buffer, the moments plane and the first-hit planes for to_cam from what they hold for from_cam; needs
        the 'normal' plane and set_moments(). 0 picks a parameter's default. Asynchronous."""
        assert from_cam.dtype == layout.CAMERA and to_cam.dtype == layout.CAMERA
        prm = ReprojectParams(max_history, depth_tolerance, match_ids, (ctypes.c_uint32 * 5)(*reserved))
        self._ck(self.L.ptmi_reproject(self.h, _p(from_cam), _p(to_cam), ctypes.byref(prm)))

    def scissor_status(self):
        """The frame scissor of the last dispatch (include/ptmi.h ptmi_scissor_status): its rectangle, whether it was applied, the
        reason when not, and the paths it has spared since reset_stats."""
        st = ScissorStatus()
        self._ck(self.L.ptmi_scissor_status(self.h, ctypes.byref(st)))
        return st

    def reproject_status(self):
        st = ReprojectStatus()
        self._ck(self.L.ptmi_reproject_status(self.h, ctypes.byref(st)))
        return st

    def debug_center_rays(self, camera):
        """the centre rays reproject() traces for `camera`: origins and directions, (H * W, 3) float32 each, index y * W + x"""
        n = self.width * self.height
        o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self._ck(self.L.ptmi_debug_center_rays(self.h, _p(camera), _p(o), _p(d), o.size))
        return o, d

    # -- lightmap baking (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake) ---------------------------
    @staticmethod
    def _bake_params(first_frame, bias, reserved):
        """None where every argument is its default: the call then passes NULL"""
        if first_frame == 0 and bias is None and tuple(reserved) == (0, 0):
            return None
        return ctypes.byref(BakeParams(first_frame, 1e-6 if bias is None else bias, (ctypes.c_uint32 * 2)(*reserved)))

    def upload_bake_surface(self, texels, width=None, height=None):
        """texels: (H, W) layout.BAKE_TEXEL records (ptmi.bake.rasterise makes them), the context's size; None removes the surface.
        width / height override what the array's shape says (for tests)."""
        if texels is None:
            self._ck(self.L.ptmi_upload_bake_surface(self.h, None, 0, 0))
            return
        t = np.ascontiguousarray(texels, layout.BAKE_TEXEL)
        assert t.ndim == 2, "a bake surface is an (H, W) array of BAKE_TEXEL records"
        h, w = t.shape
        self._ck(self.L.ptmi_upload_bake_surface(self.h, _p(t), w if width is None else width, h if height is None else height))

    def dispatch_bake(self, n_frames=1, first_frame=0, bias=None, reserved=(0, 0)):
        """n_frames frames of every covered texel from first_frame on, folded into the output buffer read as a lightmap. bias None:
        the default, 1e-6. Asynchronous."""
        self._ck(self.L.ptmi_dispatch_bake(self.h, self._bake_params(first_frame, bias, reserved), n_frames))

    def bake_status(self):
        st = BakeStatus()
        self._ck(self.L.ptmi_bake_status(self.h, ctypes.byref(st)))
        return st

    def bake_dilate(self, passes=1, n_floats=None):
        """the gutter-filled copy of the output buffer, (H, W, 4) float32: rgb, and w = 1 covered / 2 filled / 0 empty. n_floats
        overrides the count passed (for tests)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(self.L.ptmi_bake_dilate(self.h, passes, _p(out), out.size if n_floats is None else n_floats))
        return out

    def bake_denoise(self, iterations=0, dilate=0, phi_color=0.0, phi_normal=0.0, phi_position=0.0, reserved=(0, 0, 0), dst=True,
                     n_floats=None):
        """the filtered lightmap (include/ptmi.h ptmi_bake_denoise), (H, W, 4) float32: rgb, and w = 1 covered / 2 filled by one of
        the `dilate` gutter passes / 0 empty. Needs a surface and set_moments() during the bake; 0 picks a parameter's default.
        dst=False: only queue it on the context's stream (bake_denoised_device_ptr) and return None. n_floats overrides the count
        passed (for tests)."""
        prm = BakeDenoiseParams(iterations, dilate, phi_color, phi_normal, phi_position, (ctypes.c_uint32 * 3)(*reserved))
        out = np.zeros((self.height, self.width, 4), np.float32) if dst else None
        n = (0 if out is None else out.size) if n_floats is None else n_floats
        self._ck(self.L.ptmi_bake_denoise(self.h, ctypes.byref(prm), _p(out), n))
        return out

    def bake_denoised_device_ptr(self):
        return self.L.ptmi_bake_denoised_device_ptr(self.h)

    def write_moments(self, plane, n_floats=None):
        """replaces the moments plane: W * H * 4 float32 (read_moments' layout). n_floats overrides the count passed (for tests)."""
        a = np.ascontiguousarray(plane, np.float32)
        self._ck(self.L.ptmi_write_moments(self.h, _p(a), a.size if n_floats is None else n_floats))

    def debug_bake_rays(self, xs, ys, frames, first_frame=0, bias=None, reserved=(0, 0)):
        """the first ray of texel (xs[i], ys[i]) at frames[i]: origins, directions (n, 3) float32 and RNG states (n,) uint32"""
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, frames))
        n = len(xs)
        o, d, rng = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        self._ck(self.L.ptmi_debug_bake_rays(self.h, self._bake_params(first_frame, bias, reserved), n, _p(xs), _p(ys), _p(frames),
                                             _p(o), _p(d), _p(rng)))
        return o, d, rng

    # -- light probes (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes) -----------------------------------
    @staticmethod
    def _probe_params(first_frame, reserved):
        """None where every argument is its default: the call then passes NULL"""
        if first_frame == 0 and tuple(reserved) == (0, 0, 0):
            return None
        return ctypes.byref(ProbeParams(first_frame, (ctypes.c_uint32 * 3)(*reserved)))

    def upload_probes(self, probes, tile=8, count=None):
        """probes: layout.PROBE records (ptmi.probes.records makes them) for an atlas of tile x tile tiles, the context's size; None
        removes the probes. count overrides the array's length (for tests)."""
        if probes is None:
            self._ck(self.L.ptmi_upload_probes(self.h, None, 0, 0))
            return
        p = np.ascontiguousarray(probes, layout.PROBE).ravel()
        self._ck(self.L.ptmi_upload_probes(self.h, _p(p), len(p) if count is None else count, tile))

    def dispatch_probes(self, n_frames=1, first_frame=0, reserved=(0, 0, 0)):
        """n_frames frames of every texel of the enabled probes' tiles from first_frame on, folded into the output buffer read as the
        probe atlas. Asynchronous."""
        self._ck(self.L.ptmi_dispatch_probes(self.h, self._probe_params(first_frame, reserved), n_frames))

    def probe_status(self):
        st = ProbeStatus()
        self._ck(self.L.ptmi_probe_status(self.h, ctypes.byref(st)))
        return st

    def probe_sh(self, n_floats=None):
        """SH9 of every probe's tile of the output buffer: (count, 9, 3) float32. n_floats overrides the count passed (for tests)."""
        out = np.zeros((self.probe_status().count, 9, 3), np.float32)
        self._ck(self.L.ptmi_probe_sh(self.h, _p(out), out.size if n_floats is None else n_floats))
        return out

    def probe_irradiance(self, m, n_floats=None):
        """the m x m irradiance tile (E / pi) of every probe: (count, m, m, 4) float32, w = 1 for an enabled probe"""
        n = self.probe_status().count
        out = np.zeros((n, m, m, 4) if 0 < m <= 64 else (n, 1, 1, 4), np.float32)
        self._ck(self.L.ptmi_probe_irradiance(self.h, m, _p(out), out.size if n_floats is None else n_floats))
        return out

    def debug_probe_rays(self, xs, ys, frames, first_frame=0, reserved=(0, 0, 0)):
        """the first ray of texel (xs[i], ys[i]) at frames[i]: origins, directions (n, 3) float32 and RNG states (n,) uint32"""
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, frames))
        n = len(xs)
        o, d, rng = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        self._ck(self.L.ptmi_debug_probe_rays(self.h, self._probe_params(first_frame, reserved), n, _p(xs), _p(ys), _p(frames),
                                              _p(o), _p(d), _p(rng)))
        return o, d, rng

    # -- probe visibility (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility) --------------------------
    def set_probe_depth(self, max_distance=None, reserved=(0, 0, 0)):
        """turns the probe depth plane on with this clamp (ptmi.probes.max_distance gives a lattice's default); None turns it off"""
        if max_distance is None:
            self._ck(self.L.ptmi_set_probe_depth(self.h, None))
            return
        self._ck(self.L.ptmi_set_probe_depth(self.h, ctypes.byref(ProbeDepthParams(max_distance, (ctypes.c_uint32 * 3)(*reserved)))))

    def get_probe_depth(self):
        """the clamp (a float) while the plane is on, else None"""
        on, p = ctypes.c_uint32(0), ProbeDepthParams()
        self._ck(self.L.ptmi_get_probe_depth(self.h, ctypes.byref(on), ctypes.byref(p)))
        return float(p.max_distance) if on.value else None

    def read_probe_depth(self, n_floats=None):
        """(H, W, 4) float32: (mean d, mean d^2, hit fraction, 0) per probe texel. n_floats overrides the count passed (for tests)."""
        out = np.zeros((max(self.height, 1), max(self.width, 1), 4), np.float32)
        self._ck(self.L.ptmi_read_probe_depth(self.h, _p(out), out.size if n_floats is None else n_floats))
        return out

    def write_probe_depth(self, plane, n_floats=None):
        """restores a cached plane: W * H * 4 float32"""
        a = np.ascontiguousarray(plane, np.float32)
        self._ck(self.L.ptmi_write_probe_depth(self.h, _p(a), a.size if n_floats is None else n_floats))

    def probe_depth_device_ptr(self):
        return self.L.ptmi_probe_depth_device_ptr(self.h)

    def probe_visibility(self, m, sharpness_log2=6, border=False, reserved=0, n_floats=None):
        """the visibility tile of every probe, the depth plane filtered by cos^(2^sharpness_log2): (count, side, side, 4) float32 with
        side = m + 2 * border, (mean d, mean d^2, hit fraction, 1); zeros for a disabled probe"""
        n, b = self.probe_status().count, int(border)
        side = m + 2 * b if 0 < m <= 64 and 0 <= b <= 1 else 1
        out = np.zeros((n, side, side, 4), np.float32)
        q = ProbeVisibilityParams(m, sharpness_log2, b, reserved)
        self._ck(self.L.ptmi_probe_visibility(self.h, ctypes.byref(q), _p(out), out.size if n_floats is None else n_floats))
        return out

    # -- motion: reprojection across a geometry edit (include/ptmi.h ptmi_set_motion) ---------------------------
    def set_motion(self, on=True):
        self._ck(self.L.ptmi_set_motion(self.h, int(on)))

    def motion(self):
        """whether motion is on"""
        m = ctypes.c_uint32(0)
        self._ck(self.L.ptmi_get_motion(self.h, ctypes.byref(m)))
        return bool(m.value)

    def motion_commit(self):
        """previous positions := current, over the dirty range. Asynchronous."""
        self._ck(self.L.ptmi_motion_commit(self.h))

    def motion_status(self):
        st = MotionStatus()
        self._ck(self.L.ptmi_motion_status(self.h, ctypes.byref(st)))
        return st

    def read_motion(self, n_floats=None):
        """(H, W, 4) float32: where the pixel's surface was under reproject()'s from_cam, in pixels relative to the pixel (x, y), its
        distance there (z), and 0 / 1 / 2 for carried / disoccluded / missed. n_floats overrides the count passed (for tests)."""
        out = np.empty((self.height, self.width, 4), np.float32)
        self._ck(self.L.ptmi_read_motion(self.h, _p(out), out.size if n_floats is None else n_floats))
        return out

    def motion_device_ptr(self):
        return self.L.ptmi_motion_device_ptr(self.h)

    def debug_motion_prev(self, first, count):
        """the previous positions of triangles [first, first + count): (count, 3, 3) float32, v0, v1, v2"""
        out = np.zeros((count, 3, 3), np.float32)
        self._ck(self.L.ptmi_debug_motion_prev(self.h, first, count, _p(out) if count else None))
        return out

    # -- environment lighting (include/ptmi.h ptmi_upload_environment) ------------------------------------------
    def environment_status(self):
        st = EnvironmentStatus()
        self._ck(self.L.ptmi_environment_status(self.h, ctypes.byref(st)))
        return st

    def debug_env_lookup(self, d):
        """(Le.rgb, pdf) of each unit direction, (n, 4) float32"""
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        out = np.zeros((len(d), 4), np.float32)
        self._ck(self.L.ptmi_debug_env_lookup(self.h, len(d), _p(d), _p(out)))
        return out

    def debug_env_sample(self, r):
        """the kernels' environment sampling on the uniforms r (n, 4): (directions (n, 3), (Le.rgb, density) (n, 4), texels (n,))"""
        r = np.ascontiguousarray(r, np.float32).reshape(-1, 4)
        d, out, tex = np.zeros((len(r), 3), np.float32), np.zeros((len(r), 4), np.float32), np.zeros(len(r), np.uint32)
        self._ck(self.L.ptmi_debug_env_sample(self.h, len(r), _p(r), _p(d), _p(out), _p(tex)))
        return d, out, tex

    # -- the participating medium (include/ptmi.h ptmi_set_medium) ----------------------------------------------------
    def get_medium(self):
        """the medium in place as a Medium, or None"""
        m, present = Medium(), ctypes.c_uint32(0)
        self._ck(self.L.ptmi_get_medium(self.h, ctypes.byref(m), ctypes.byref(present)))
        return m if present.value else None

    def debug_medium_step(self, o, d, t_hit, r):
        """one path segment of the medium in place on the uniforms r (n, 3) = (r, xi1, xi2) for the rays (o, d) and hit distances t_hit
        (inf: a miss): (scattered (n,) bool, x (n, 3), direction (n, 3), (a, b, s, phase density) (n, 4))"""
        o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        t_hit, r = np.ascontiguousarray(t_hit, np.float32).reshape(-1), np.ascontiguousarray(r, np.float32).reshape(-1, 3)
        n = len(o)
        assert len(d) == n and len(t_hit) == n and len(r) == n
        sc, x, dr, out = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
        self._ck(self.L.ptmi_debug_medium_step(self.h, n, _p(o), _p(d), _p(t_hit), _p(r), _p(sc), _p(x), _p(dr), _p(out)))
        return sc != 0, x, dr, out

    def debug_medium_tr(self, o, wi, dist):
        """the transmittance a next-event sample from o towards wi, dist away (< 0: directional), takes: (n,) float32"""
        o, wi = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(wi, np.float32).reshape(-1, 3)
        dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
        assert len(wi) == len(o) and len(dist) == len(o)
        tr = np.zeros(len(o), np.float32)
        self._ck(self.L.ptmi_debug_medium_tr(self.h, len(o), _p(o), _p(wi), _p(dist), _p(tr)))
        return tr

    # -- the medium's density grid (include/ptmi.h ptmi_upload_medium_density) ---------------------------------------------
    def medium_grid_status(self):
        st = MediumGridStatus()
        self._ck(self.L.ptmi_medium_grid_status(self.h, ctypes.byref(st)))
        return st

    def debug_medium_density(self, p):
        """the grid lookup at the points p (n, 3): (n,) float32"""
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        rho = np.zeros(len(p), np.float32)
        self._ck(self.L.ptmi_debug_medium_density(self.h, len(p), _p(p), _p(rho)))
        return rho

    def debug_medium_track(self, o, d, t_end, rng, mode):
        """mode 0: delta tracking of the rays (o, d) up to t_end (inf: a miss); mode 1: ratio tracking towards dist = t_end (< 0:
        directional); each ray draws from its kernel RNG state rng[i]. (scattered (n,) bool, t (n,), value (n,), tentative collisions (n,)
        uint32, RNG states afterwards (n,) uint32): t, value = scatter distance and rho there (mode 0), the segment's end and T (mode 1)"""
        o, d = np.ascontiguousarray(o, np.float32).reshape(-1, 3), np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        t_end, rng = np.ascontiguousarray(t_end, np.float32).reshape(-1), np.ascontiguousarray(rng, np.uint32).reshape(-1)
        n = len(o)
        assert len(d) == n and len(t_end) == n and len(rng) == n
        sc, steps, after = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        t, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._ck(self.L.ptmi_debug_medium_track(self.h, n, _p(o), _p(d), _p(t_end), _p(rng), mode, _p(sc), _p(t), _p(v), _p(steps), _p(after)))
        return sc != 0, t, v, steps, after

    def read_triangles(self, first=0, count=None):
        """the live TRIANGLE records [first, first + count) as they stand on the device (count None: to the end of the upload)"""
        if count is None:
            count = self._uploaded_tris - first
        out = np.zeros(max(count, 0), layout.TRIANGLE)
        self._ck(self.L.ptmi_debug_read_triangles(self.h, first, count, _p(out) if len(out) else None))
        return out

    def read_image(self):
        """The traversal image the last upload_scene put on the device (include/ptmi.h: ptmi_debug_read_image), as build_image()
        returns it: (info, wnodes, qnodes or None, tripos, leafbox or None)."""
        return _read_image(self.L, self.h, self._uploaded_tris, self._ck)

    # -- per-stage entry points ------------------------------------------------
    def debug_raygen(self, camera, xs, ys, frames):
        xs, ys, frames = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, frames))
        n = len(xs)
        o, d, rng = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        self._ck(self.L.ptmi_debug_raygen(self.h, _p(camera), n, _p(xs), _p(ys), _p(frames), _p(o), _p(d), _p(rng)))
        return o, d, rng

    def debug_intersect(self, o, d):
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = len(o)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        tri = np.zeros(n, np.uint32)
        self._ck(self.L.ptmi_debug_intersect(self.h, n, _p(o), _p(d), _p(t), _p(tri), _p(u), _p(v)))
        return t, tri, u, v

    def debug_occluded(self, o, d, dist):
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        dist = np.ascontiguousarray(dist, np.float32)
        occ = np.zeros(len(o), np.uint8)
        self._ck(self.L.ptmi_debug_occluded(self.h, len(o), _p(o), _p(d), _p(dist), _p(occ)))
        return occ

    def debug_alpha_intersect(self, o, d):
        """debug_intersect through the path loop of the active cutoff or blend table: (t along the given ray, triangle, holes passed)"""
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        n = len(o)
        t, tri, layers = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._ck(self.L.ptmi_debug_alpha_intersect(self.h, n, _p(o), _p(d), _p(t), _p(tri), _p(layers)))
        return t, tri, layers

    def debug_alpha_occluded(self, o, d, dist):
        """debug_occluded through the shadow loop of the active cutoff table: (occluded, holes passed)"""
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
        dist = np.ascontiguousarray(dist, np.float32)
        occ, layers = np.zeros(len(o), np.uint8), np.zeros(len(o), np.uint32)
        self._ck(self.L.ptmi_debug_alpha_occluded(self.h, len(o), _p(o), _p(d), _p(dist), _p(occ), _p(layers)))
        return occ, layers

    def debug_math(self, op, a, b=None, c=None):
        a = np.ascontiguousarray(a, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        c = None if c is None else np.ascontiguousarray(c, np.float32)
        out = np.zeros_like(a)
        self._ck(self.L.ptmi_debug_math(self.h, op, a.size, _p(a), _p(b), _p(c), _p(out)))
        return out

    def debug_exact_math(self, which):
        """(inputs among all 2^32 float patterns whose short-form result differs from the IEEE expansion, smallest such pattern);
        which = 0: 1/x, 1: sqrt(x), 2: the triangle test's 1/x (|x| >= 1e-6). include/ptmi.h."""
        n, first = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._ck(self.L.ptmi_debug_exact_math(self.h, which, ctypes.byref(n), ctypes.byref(first)))
        return int(n.value), int(first.value)


class MultiContext(_Handle):
    """Several devices of one node behind one handle (include/ptmi.h ptmi_multi_*): the frame's rows are dealt out as
    interleaved strips, every device accumulates its own, gather() assembles the frame on the first device through RCCL.
    loopback=True replaces the collective with device-to-device copies, so that one device can stand in for several."""

    _prefix = "ptmi_multi_"

    def __init__(self, devices, loopback=False):
        super().__init__(len(devices), (ctypes.c_int * len(devices))(*devices), MULTI_LOOPBACK if loopback else 0)
        self.n = len(devices)

    def _before_set_options(self, o, kw):
        """the library deals out the rows: no tile of the caller's, and the automatic strip height unless kw names one"""
        o.tile_parts = o.tile_part = 0
        if "tile_strip" not in kw:
            o.tile_strip = 0

    def read_triangles(self, i, first=0, count=None):
        """Context.read_triangles of device i's context (ptmi_multi_context)"""
        h = self.L.ptmi_multi_context(self.h, i)
        count = self._uploaded_tris - first if count is None else count
        out = np.zeros(max(count, 0), layout.TRIANGLE)
        rc = self.L.ptmi_debug_read_triangles(h, first, count, _p(out) if len(out) else None)
        if rc != 0:
            raise PtmiError(rc, self.L.ptmi_last_error(h).decode())
        return out

    def read_image(self, i):
        """Context.read_image of device i's context (ptmi_multi_context)"""
        h = self.L.ptmi_multi_context(self.h, i)

        def ck(rc):
            if rc != 0:
                raise PtmiError(rc, self.L.ptmi_last_error(h).decode())
        return _read_image(self.L, h, self._uploaded_tris, ck)

    def gather(self):
        self._ck(self.L.ptmi_multi_gather(self.h))

    def gather_planes(self, *planes):
        """assembles the named planes on the first device in one pass: 'albedo', 'normal', 'id', 'moments', 'output', or bit masks"""
        mask = 0
        for p in planes:
            mask |= int(p) if not isinstance(p, str) else {"moments": MULTI_PLANE_MOMENTS, "output": MULTI_PLANE_OUTPUT}.get(p) or _aov(p)[0]
        self._ck(self.L.ptmi_multi_gather_planes(self.h, mask))

    def dispatch_adaptive_rounds(self, camera, rounds=1, threshold=0.0, floor=0.0, min_frames=0, max_frames=0, step=0, neighbourhood=0,
                                 reserved=(0, 0)):
        """Context.dispatch_adaptive over every device's strips (ptmi_multi_dispatch_adaptive): the same arguments, the same planes
        afterwards. With neighbourhood=1 the devices exchange their pixels' flags every round."""
        self._dispatch_adaptive(camera, rounds, threshold, floor, min_frames, max_frames, step, neighbourhood, reserved)

    def blit(self):
        b = np.empty((self.height, self.width, 4), np.uint8)
        self._ck(self.L.ptmi_multi_blit(self.h, None, 0, _p(b), b.size))
        return b

    def gather_ms(self):
        ms = ctypes.c_double(-1.0)
        self._ck(self.L.ptmi_multi_gather_ms(self.h, ctypes.byref(ms)))
        return ms.value
