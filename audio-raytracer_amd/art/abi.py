"""ctypes mirror of include/art.h, include/art_device.h and include/art_synth.h.

Struct layouts are byte-identical to the C# structs of the reference (2-byte packing):
  ColliderAABBStruct   DataTypes/Collider Structs/ColliderAABBStruct.cs:10-14   (20 B)
  ColliderOBBStruct    DataTypes/Collider Structs/ColliderOBBStruct.cs:10-24    (26 B)
  ColliderSphereStruct DataTypes/Collider Structs/ColliderSphereStruct.cs:10-14 (16 B)
  AudioTargetRTSettings DataTypes/AudioTargetRTSettings.cs:11-16               (24 B)
The numpy dtypes below are the same layouts, so collider arrays can be handed to the C ABI as
raw pointers (NativeArray.GetUnsafePtr() in the Unity host).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# ----------------------------------------------------------------------------- numpy dtypes
HALF3 = np.dtype([("x", "<u2"), ("y", "<u2"), ("z", "<u2")])
MATERIAL = np.dtype([("absorption", "<u2"), ("density", "<u2"), ("echo", "<u2")])
AABB = np.dtype([("center", "<u2", 3), ("size", "<u2", 3), ("material", "<u2", 3), ("audio_target_id", "<i2")])
OBB = np.dtype([("center", "<u2", 3), ("size", "<u2", 3), ("rot", "<u2", 3), ("material", "<u2", 3),
                ("audio_target_id", "<i2")])
SPHERE = np.dtype([("center", "<u2", 3), ("radius", "<u2"), ("material", "<u2", 3), ("audio_target_id", "<i2")])
SETTINGS = np.dtype([("muffle_strength", "<f4"), ("reverb_strength", "<f4"), ("reverb_volume", "<f4"),
                     ("perceived_position", "<f4", 3)])
DSP_PARAMS = np.dtype([("dry_level", "<f4"), ("dry_boost", "<f4"), ("muffle_cutoff", "<f4"), ("muffle_alpha", "<f4"),
                       ("muffle_active", "<i4"), ("reserved", "<i4")])
assert AABB.itemsize == 20 and OBB.itemsize == 26 and SPHERE.itemsize == 16
assert SETTINGS.itemsize == 24 and DSP_PARAMS.itemsize == 24

# ----------------------------------------------------------------------------- constants
ART_STAGE_RAYTRACE = 0x1
ART_STAGE_PERMEATE = 0x2
ART_STAGE_REDUCE = 0x4
ART_STAGE_DSP_PARAMS = 0x8
ART_STAGE_ALL = 0xF

ART_OK = 0
ART_E_INVALID = -1
ART_E_DEVICE = -2
ART_E_UNSUPPORTED = -3
ART_E_NOMEM = -4
ART_E_STATE = -5
ERROR_NAMES = {ART_E_INVALID: "ART_E_INVALID", ART_E_DEVICE: "ART_E_DEVICE", ART_E_UNSUPPORTED: "ART_E_UNSUPPORTED",
               ART_E_NOMEM: "ART_E_NOMEM", ART_E_STATE: "ART_E_STATE"}

ART_CTX_COUNT_TESTS = 0x1
ART_CTX_TIME_KERNELS = 0x2
ART_CTX_FORCE_REFERENCE_ORDER = 0x4
ART_CTX_COUNT_EXECUTED = 0x10
ART_CTX_RESIDENT_COLLIDERS = 0x20  # art_colliders.h
ART_CTX_TIME_EACH_KERNEL = 0x200
ART_CTX_EVENT_EACH_LAUNCH = 0x400  # art_launch_device records its completion event (the caller may drop its stream)
ART_CTX_RESIDENT_TARGETS = 0x800  # art_colliders.h: positions and T come from the last art_targets_sync
ART_CTX_TARGET_OWNERS_FOLLOW = 0x1000  # art_colliders.h: a swapped target's colliders take its new index
# art_debug_last_plan: the launch plan of the throughput raytrace stage (art_device.h)
ART_PLAN_FUSED, ART_PLAN_HM, ART_PLAN_SPLIT, ART_PLAN_FOLD, ART_PLAN_PER_BOUNCE = 0x1, 0x2, 0x4, 0x8, 0x10
ART_PLAN_TAB, ART_PLAN_OBB, ART_PLAN_EX, ART_PLAN_CHUNKED = 0x20, 0x40, 0x80, 0x100
PLAN_NAMES = {ART_PLAN_FUSED: "FUSED", ART_PLAN_HM: "HM", ART_PLAN_SPLIT: "SPLIT", ART_PLAN_FOLD: "FOLD",
              ART_PLAN_PER_BOUNCE: "PER_BOUNCE", ART_PLAN_TAB: "TAB", ART_PLAN_OBB: "OBB", ART_PLAN_EX: "EX",
              ART_PLAN_CHUNKED: "CHUNKED"}


def plan_names(bits: int) -> str:
    return "|".join(n for b, n in PLAN_NAMES.items() if bits & b) or "0"


ART_KIND_SPHERE, ART_KIND_AABB, ART_KIND_OBB = 0, 1, 2
# art_debug_bvh_records (include/art_device.h): which array, and the 32-byte record as it lies in memory
ART_DEBUG_BVH_BOUNDS, ART_DEBUG_BVH_NODES = 0, 1
CULL_REC = np.dtype([("lo", "<f4", 3), ("fscale", "<f4"), ("hi", "<f4", 3), ("factor", "<f4")])
# art_debug_cells_lists (include/art_device.h): which array of the muffle direction-cell lists
ART_DEBUG_CELLS_STARTS, ART_DEBUG_CELLS_ENTRIES, ART_DEBUG_CELLS_OK, ART_DEBUG_CELLS_FAR, ART_DEBUG_CELLS_INFO = 0, 1, 2, 3, 4
# art_debug_last_dsp_kernel (include/art_dsp.h): the kernel the last per-sample DSP call launched
ART_DSP_KERNEL_NONE, ART_DSP_KERNEL_TILED, ART_DSP_KERNEL_LANE, ART_DSP_KERNEL_MIX = 0, 1, 2, 3
ART_OUT_HIT_RESULTS = 0x1
# art_fan.ray_hit_ids: ColliderType (Enums/ColliderType.cs) << 30 | index in that type's array
ART_COLLIDER_AABB, ART_COLLIDER_OBB, ART_COLLIDER_SPHERE = 1, 2, 3
ART_HIT_NONE = 0xFFFFFFFF


def hit_id(ctype: int, index: int) -> int:
    return (ctype << 30) | index

ART_OWN_SPHERE, ART_OWN_AABB, ART_OWN_OBB = 0, 1, 2


# ----------------------------------------------------------------------------- ctypes structs
class art_curve(C.Structure):
    _fields_ = [("baked", C.POINTER(C.c_float)), ("sample_count", C.c_int32), ("length", C.c_float)]


class art_dsp_desc(C.Structure):
    _fields_ = [("reverb_dry_level_min", C.c_float), ("reverb_dry_level_max", C.c_float),
                ("reverb_dry_boost_min", C.c_float), ("reverb_dry_boost_max", C.c_float),
                ("muffle_cutoff_min", C.c_float), ("muffle_cutoff_max", C.c_float),
                ("reverb_volume_curve", art_curve), ("muffle_curve", art_curve), ("sample_rate", C.c_int32)]


class art_frame_desc(C.Structure):
    _fields_ = [("ray_directions", C.c_void_p), ("ray_count", C.c_int32),
                ("aabb_colliders", C.c_void_p), ("aabb_count", C.c_int32),
                ("obb_colliders", C.c_void_p), ("obb_count", C.c_int32),
                ("sphere_colliders", C.c_void_p), ("sphere_count", C.c_int32),
                ("audio_target_positions", C.c_void_p), ("audio_target_count", C.c_int32),
                ("max_ray_life", C.c_float), ("max_hits_per_ray", C.c_int32),
                ("max_muffle_hit_distance", C.c_float), ("muffle_effectiveness", C.c_float),
                ("permeation_strength_per_ray", C.c_float), ("permeation_effectiveness", C.c_float),
                ("max_reverb_distance", C.c_float), ("batch_size", C.c_int32), ("batch_slots", C.c_int32),
                ("stages", C.c_uint32), ("dsp", C.POINTER(art_dsp_desc))]


class art_fan(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("echo_ray_distances", C.c_void_p), ("muffle_ray_hits", C.c_void_p),
                ("permeation_power_remains", C.c_void_p), ("settings", C.c_void_p), ("dsp_params", C.c_void_p),
                ("ray_hit_points", C.c_void_p), ("ray_hit_counts", C.c_void_p), ("ray_hit_ids", C.c_void_p)]


class art_test_counts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rt_sphere", "rt_aabb", "rt_obb", "perm_hit_sphere", "perm_hit_aabb",
                                           "perm_hit_obb", "perm_loss_sphere", "perm_loss_aabb", "perm_loss_obb")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class art_fan_layout(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("stride", "settings_off", "dsp_off", "muffle_off", "perm_off", "echo_off",
                                           "hit_points_off", "hit_counts_off", "hit_ids_off")]


class art_kernel_times(C.Structure):
    _fields_ = [("raytrace_ms", C.c_double), ("permeate_ms", C.c_double), ("reduce_ms", C.c_double),
                ("launches", C.c_int32), ("kernel_marks_dropped", C.c_int32), ("kernel_ms", C.c_double * 4),
                ("kernel_launches", C.c_int32 * 4)]


# art_kernel_times.kernel_ms order (ART_KERNEL_*)
KERNEL_FAMILIES = ("nearest_first_kernel", "echo_muffle_kernel", "vis_kernel", "muffle_kernel")


class art_collider_sync_stats(C.Structure):
    _fields_ = [("dirty_records", C.c_int32), ("full_prep", C.c_int32), ("reallocated", C.c_int32),
                ("cells_rebuilt", C.c_int32), ("bytes_uploaded", C.c_uint64)]


class art_target_sync_stats(C.Structure):
    _fields_ = [("dirty_targets", C.c_int32), ("count_changed", C.c_int32), ("lists_rebuilt", C.c_int32),
                ("lists_full_rebuild", C.c_int32), ("bytes_uploaded", C.c_uint64)]


class art_target_resize_stats(C.Structure):  # ABI 3.7
    _fields_ = [("kept_bound", C.c_int32), ("added", C.c_int32), ("removed", C.c_int32), ("lists_moved", C.c_int32),
                ("lists_rebuilt", C.c_int32), ("lists_full_rebuild", C.c_int32), ("bytes_uploaded", C.c_uint64)]


class art_collider_resize_stats(C.Structure):  # ABI 3.10
    _fields_ = [("kept_bound", C.c_int32), ("added", C.c_int32), ("removed", C.c_int32), ("relabelled", C.c_int32),
                ("bvh_rebuilt", C.c_int32), ("levels_changed", C.c_int32), ("cells_rebuilt", C.c_int32),
                ("bytes_uploaded", C.c_uint64)]


class art_exec_kernel(C.Structure):
    _fields_ = [("sphere", C.c_uint64), ("aabb", C.c_uint64), ("obb", C.c_uint64), ("cull_box", C.c_uint64),
                ("cell_entries", C.c_uint64)]


EXEC_KERNELS = ("nearest", "echo", "muffle")  # art_exec_counts.by_kernel order


class art_exec_counts(C.Structure):
    _fields_ = [("sphere", C.c_uint64), ("aabb", C.c_uint64), ("obb", C.c_uint64), ("cull_box", C.c_uint64),
                ("cell_entries", C.c_uint64), ("launches", C.c_uint64), ("muffle_fallback", C.c_uint64),
                ("echo_pairs", C.c_uint64), ("bounce_rays", C.c_uint64 * 16), ("by_kernel", art_exec_kernel * 3)]


# include/art_dsp.h
class art_stereo(C.Structure):
    _fields_ = [("left", C.c_float), ("right", C.c_float)]


class art_dsp_state(C.Structure):
    _fields_ = [("previous_muffle", art_stereo), ("previous_lp", art_stereo), ("previous_hp", art_stereo),
                ("previous_input", art_stereo)]


class art_spatializer_settings(C.Structure):
    _fields_ = [("pan_strength", C.c_float), ("rear_attenuation_strength", C.c_float),
                ("distance_based_panning", C.c_int32), ("max_pan_distance", C.c_float),
                ("distance_based_rear_attenuation", C.c_int32), ("max_rear_attenuation_distance", C.c_float),
                ("max_elevation_effect_distance", C.c_float),
                ("low_pass_cutoff_min", C.c_float), ("low_pass_cutoff_max", C.c_float), ("low_pass_volume", C.c_float),
                ("high_pass_cutoff_min", C.c_float), ("high_pass_cutoff_max", C.c_float), ("high_pass_volume", C.c_float),
                ("muffle_curve", art_curve), ("muffle_cutoff_min", C.c_float), ("muffle_cutoff_max", C.c_float),
                ("reverb_volume_curve", art_curve), ("reverb_dry_boost_min", C.c_float),
                ("reverb_dry_boost_max", C.c_float)]


class art_audio_source(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("frames", C.c_int32), ("channels", C.c_int32),
                ("muffle_strength", C.c_float), ("reverb_volume", C.c_float), ("local_dir", C.c_float * 3),
                ("listener_distance", C.c_float), ("volume_multiplier", C.c_float),
                ("state", C.POINTER(art_dsp_state))]


class art_dsp_source_params(C.Structure):
    _fields_ = [("muffle_alpha", C.c_float), ("dry_boost", C.c_float), ("gain_left", C.c_float),
                ("gain_right", C.c_float), ("filter_alpha", C.c_float), ("volume", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class art_listener(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("rotation", C.c_float * 4)]


LISTENER = np.dtype([("position", np.float32, 3), ("rotation", np.float32, 4)])
DSP_STATE = np.dtype([("previous_muffle", np.float32, 2), ("previous_lp", np.float32, 2),
                      ("previous_hp", np.float32, 2), ("previous_input", np.float32, 2)])
DSP_SOURCE_PARAMS = np.dtype([("muffle_alpha", np.float32), ("dry_boost", np.float32), ("gain_left", np.float32),
                       ("gain_right", np.float32), ("filter_alpha", np.float32), ("volume", np.float32),
                       ("flags", np.int32), ("reserved", np.int32)])


class art_synth_config(C.Structure):
    _fields_ = [("sphere_count", C.c_int32), ("aabb_count", C.c_int32), ("obb_count", C.c_int32),
                ("target_count", C.c_int32), ("fan_count", C.c_int32), ("ray_count", C.c_int32),
                ("owned_type", C.c_int32), ("seed", C.c_uint64)]


# Every symbol include/*.h declares, with its ctypes signature.
VP, I32, U32, U64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64
SIGNATURES = {
    # art.h
    "art_create": (I32, [U32, C.POINTER(VP)]),
    "art_destroy": (None, [VP]),
    "art_last_error": (C.c_char_p, [VP]),
    "art_schedule": (I32, [VP, C.POINTER(art_frame_desc), C.POINTER(art_fan), I32, C.POINTER(U64)]),
    "art_is_completed": (I32, [VP, U64]),
    "art_complete": (I32, [VP, U64]),
    "art_set_flags": (I32, [VP, U32]),
    "art_last_test_counts": (I32, [VP, C.POINTER(art_test_counts)]),
    "art_version": (U32, []),
    # art_device.h
    "art_fan_layout_get": (I32, [C.POINTER(art_frame_desc), U32, C.POINTER(art_fan_layout)]),
    "art_scene_bind": (I32, [VP, C.POINTER(art_frame_desc)]),
    "art_launch_device": (I32, [VP, VP, I32, VP, U32, VP]),
    "art_count_device": (I32, [VP, VP, I32, VP, U32, VP, C.POINTER(art_test_counts)]),
    "art_kernel_timing": (I32, [VP, C.POINTER(art_kernel_times)]),
    "art_executed_counts": (I32, [VP, C.POINTER(art_exec_counts)]),
    "art_debug_leaf_order": (I32, [VP, C.POINTER(U32), I32]),
    "art_debug_bvh_records": (I32, [VP, I32, C.POINTER(C.c_float), I32]),
    "art_debug_last_plan": (I32, [VP, C.POINTER(U32)]),
    "art_debug_echo_decided": (I32, [VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "art_debug_sphere_slack": (I32, [VP, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "art_debug_node_margin_cap": (I32, [VP, C.c_float, C.c_float, C.c_float, I32, C.c_float, C.POINTER(C.c_float),
                                        C.POINTER(C.c_float)]),
    "art_debug_cells_lists": (I32, [VP, I32, C.POINTER(U32), I32]),
    # art_dsp.h
    "art_dsp_process": (I32, [VP, C.POINTER(art_spatializer_settings), C.POINTER(art_audio_source), I32, I32]),
    "art_dsp_source_params_get": (I32, [C.POINTER(art_spatializer_settings), C.POINTER(art_audio_source), I32,
                                        C.POINTER(art_dsp_source_params)]),
    "art_dsp_process_device": (I32, [VP, VP, VP, VP, I32, I32, VP]),
    "art_debug_last_dsp_kernel": (I32, [VP]),
    "art_fibonacci_directions_device": (I32, [VP, I32, VP, VP]),
    "art_dsp_tick_params_host": (I32, [C.POINTER(art_spatializer_settings), I32, VP, C.POINTER(art_fan), I32, VP, I32, VP,
                                       VP]),
    "art_dsp_settings_bind": (I32, [VP, C.POINTER(art_spatializer_settings), I32]),
    "art_dsp_tick_params_classes_host": (I32, [VP, I32, I32, VP, C.POINTER(art_fan), I32, VP, I32, VP, VP, VP]),
    "art_dsp_settings_bind_classes": (I32, [VP, VP, I32, I32]),
    "art_dsp_target_classes_set": (I32, [VP, VP, I32]),
    "art_dsp_target_classes_get": (I32, [VP, VP, I32]),
    "art_dsp_target_classes_follow": (I32, [VP, VP, I32, I32, C.c_uint8]),
    "art_dsp_tick_params_device": (I32, [VP, VP, U32, I32, VP, VP, VP, VP]),
    "art_dsp_tick_device": (I32, [VP, VP, U32, I32, VP, VP, VP, VP, I32, VP, VP]),
    "art_dsp_mix_device": (I32, [VP, VP, VP, VP, I32, I32, I32, VP, VP]),
    "art_dsp_tick_mix_device": (I32, [VP, VP, U32, I32, VP, VP, VP, VP, I32, VP, VP, VP]),
    "art_dsp_mix_host": (I32, [VP, VP, VP, I32, I32, I32, VP]),
    "art_dsp_sources_follow_host": (I32, [VP, I32, I32, VP, I32, I32, VP, VP, VP, VP, C.c_float]),
    "art_dsp_sources_follow_device": (I32, [VP, VP, I32, I32, VP, I32, I32, VP, VP, VP, VP, C.c_float, VP]),
    # art_colliders.h
    "art_collider_add": (I32, [VP, I32, VP, C.POINTER(I32)]),
    "art_collider_set": (I32, [VP, I32, I32, VP]),
    "art_collider_set_many": (I32, [VP, I32, VP, VP, I32]),
    "art_collider_remove_swapback": (I32, [VP, I32, I32]),
    "art_collider_get": (I32, [VP, I32, I32, VP]),
    "art_collider_count": (I32, [VP, I32]),
    "art_colliders_clear": (I32, [VP]),
    "art_colliders_sync": (I32, [VP]),
    "art_colliders_last_sync": (I32, [VP, C.POINTER(art_collider_sync_stats)]),
    "art_colliders_reserve": (I32, [VP, I32, I32, I32]),
    "art_collider_capacity": (I32, [VP, I32]),
    "art_colliders_last_resize": (I32, [VP, C.POINTER(art_collider_resize_stats)]),
    "art_target_add": (I32, [VP, VP, C.POINTER(I32)]),
    "art_target_set": (I32, [VP, I32, VP]),
    "art_target_set_many": (I32, [VP, VP, VP, I32]),
    "art_target_remove_swapback": (I32, [VP, I32]),
    "art_target_get": (I32, [VP, I32, VP]),
    "art_target_count": (I32, [VP]),
    "art_target_synced_count": (I32, [VP]),
    "art_targets_clear": (I32, [VP]),
    "art_targets_sync": (I32, [VP]),
    "art_targets_last_sync": (I32, [VP, C.POINTER(art_target_sync_stats)]),
    "art_debug_cells_arena": (I32, [VP, C.POINTER(U64), C.POINTER(U64), C.POINTER(U32)]),
    "art_targets_reserve": (I32, [VP, I32]),
    "art_target_capacity": (I32, [VP]),
    "art_targets_last_resize": (I32, [VP, C.POINTER(art_target_resize_stats)]),
    "art_debug_target_sync_map": (I32, [VP, VP, I32]),
    "art_target_follow_map": (I32, [VP, VP, I32, C.POINTER(I32)]),
    "art_target_follow_mark": (I32, [VP]),
    "art_target_last_remove_owners": (I32, [VP, VP]),
    "art_device_count": (I32, []),
    "art_create_on": (I32, [C.POINTER(I32), I32, C.POINTER(VP)]),
    # art_synth.h
    "art_synth_scene": (I32, [C.POINTER(art_synth_config), VP, VP, VP, VP, VP, VP]),
    "art_fibonacci_directions": (None, [I32, VP]),
    "art_f32tof16": (C.c_uint16, [C.c_float]),
    "art_f16tof32": (C.c_float, [C.c_uint16]),
    "art_f32tof16_range": (None, [U32, U32, VP]),
    "art_f32tof16_device": (I32, [VP, U32, U32, VP, VP]),
    "art_recip_exact_device": (I32, [VP, U32, U32, VP, VP]),
}

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libart.so")

_lib = None


def _preload_torch_hip_runtime():
    """One HIP runtime per process. torch ships its own libamdhip64.so (SONAME libamdhip64.so.7,
    the same SONAME as /opt/rocm's). If libart.so loaded /opt/rocm's copy first, a later
    `import torch` would map a second runtime and torch would see no GPU. Loading torch's copy
    by path first makes libart.so bind to it (SONAME match) and lets torch reuse it (same file).
    ART_HIP_RUNTIME=system keeps /opt/rocm's runtime."""
    if os.environ.get("ART_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library(path: str | None = None) -> C.CDLL:
    """Load libart.so (the HIP extension). Fails loudly when it has not been built: there is no
    CPU fallback for the product path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    _preload_torch_hip_runtime()
    p = path or os.environ.get("ART_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"libart.so not found at {p}: build it with `make -C audio-raytracer_amd` "
                          "(or __graft_entry__.build()); the GPU path has no CPU fallback")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib
