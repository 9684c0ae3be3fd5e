"""Loader for libpbrhip.so (the HIP/C++ core).  There is no fallback: if the library is missing or
cannot be loaded this module raises, and every compute entry point of the library itself fails
with PBRHIP_ENODEVICE when no MI355X is visible."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBRHIP_LIB") or os.path.join(HERE, "libpbrhip.so")  # PBRHIP_LIB: A/B builds
CSRC = os.path.join(HERE, "csrc")

ABI_VERSION = 6  # PBRHIP_ABI_VERSION of include/pbrhip.h (struct layouts of this binding)

# every symbol include/pbrhip.h declares
EXPORTS = [
    "pbrhip_abi_version", "pbrhip_math_mode", "pbrhip_sizeof_render_stats", "pbrhip_last_error", "pbrhip_device_count", "pbrhip_set_device", "pbrhip_scene_create", "pbrhip_scene_destroy",
    "pbrhip_scene_add_triangle_mesh", "pbrhip_scene_add_curve_mesh", "pbrhip_scene_add_principled_material",
    "pbrhip_scene_add_hair_material", "pbrhip_scene_add_texture", "pbrhip_scene_add_area_light", "pbrhip_scene_create_local_scene",
    "pbrhip_scene_add_mesh_to_local_scene", "pbrhip_scene_create_instance", "pbrhip_scene_attach_light_ids",
    "pbrhip_scene_attach_material_ids", "pbrhip_scene_commit", "pbrhip_scene_set_bvh_builder", "pbrhip_scene_aabb",
    "pbrhip_scene_update_principled_material", "pbrhip_scene_update_hair_material", "pbrhip_scene_info", "pbrhip_scene_set_environment",
    "pbrhip_scene_set_camera", "pbrhip_camera_rays",
    "pbrhip_render", "pbrhip_render_device", "pbrhip_trace_closest", "pbrhip_trace_any", "pbrhip_leaf_eval", "pbrhip_texture_fetch", "pbrhip_create_tiles",
    "pbrhip_render_multi", "pbrhip_scene_replicate", "pbrhip_comm_unique_id", "pbrhip_comm_create", "pbrhip_comm_destroy",
    "pbrhip_comm_reduce_layer", "pbrhip_comm_gather_layer",
    "pbrhip_render_features", "pbrhip_render_features_device", "pbrhip_denoise", "pbrhip_denoise_device",
    "pbrhip_lbvh_build", "pbrhip_scene_wide_info", "pbrhip_qtree_collapse",
    "pbrhip_scene_update_triangle_mesh", "pbrhip_scene_update_curve_mesh", "pbrhip_scene_update_instance_transform", "pbrhip_scene_refit",
    "pbrhip_tree_refit",
    "pbrhip_scene_update_triangle_mesh_device", "pbrhip_scene_update_curve_mesh_device", "pbrhip_scene_read_slots",
    "pbrhip_render_adaptive", "pbrhip_render_adaptive_device", "pbrhip_adaptive_step",
    "pbrhip_render_rays", "pbrhip_render_rays_device", "pbrhip_render_features_rays_device", "pbrhip_projection_rays_device",
    "pbrhip_scene_snapshot_pose", "pbrhip_render_motion", "pbrhip_render_motion_device", "pbrhip_temporal_accumulate", "pbrhip_temporal_accumulate_device",
    "pbrhip_scene_object_ids", "pbrhip_scene_object_ids_device", "pbrhip_svgf_accumulate", "pbrhip_svgf_accumulate_device", "pbrhip_svgf_filter",
    "pbrhip_svgf_filter_device",
    "pbrhip_render_features_emission", "pbrhip_render_features_emission_device", "pbrhip_emission_split", "pbrhip_emission_split_device",
    "pbrhip_emission_merge", "pbrhip_emission_merge_device",
    "pbrhip_trace_closest_device", "pbrhip_trace_any_device", "pbrhip_nearest_point", "pbrhip_nearest_point_device",
    "pbrhip_scene_signed_distance_info", "pbrhip_signed_distance", "pbrhip_signed_distance_device", "pbrhip_signed_distance_grid_device",
    "pbrhip_scene_read_pseudonormals",
    "pbrhip_trace_all", "pbrhip_trace_all_device",
    "pbrhip_k_nearest", "pbrhip_k_nearest_device",
    "pbrhip_scene_shadow_grid_info", "pbrhip_scene_read_shadow_grid",
]


def build(force=False):
    """Compile libpbrhip.so for gfx950 with hipcc (works without a GPU)."""
    args = ["make", "-s", "-C", CSRC, "-j4"]
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (hipcc, gfx950). pbrlab_amd has no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _lib.pbrhip_last_error.restype = C.c_char_p
        _lib.pbrhip_abi_version.restype = C.c_uint32
        _lib.pbrhip_math_mode.restype = C.c_uint32
        _lib.pbrhip_sizeof_render_stats.restype = C.c_size_t
        vp, u32, f32 = C.c_void_p, C.c_uint32, C.c_float
        _lib.pbrhip_render_features.argtypes = _lib.pbrhip_render_features_device.argtypes = [vp, vp, vp, vp, vp]
        _lib.pbrhip_denoise.argtypes = _lib.pbrhip_denoise_device.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, vp, u32, f32, f32, u32, u32, vp]
        _lib.pbrhip_lbvh_build.argtypes = [C.c_int, vp, vp, vp, u32, vp, vp, vp]
        _lib.pbrhip_qtree_collapse.argtypes = [C.c_int, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
        _lib.pbrhip_scene_wide_info.argtypes = [vp, vp, vp, vp]
        _lib.pbrhip_scene_update_triangle_mesh.argtypes = [vp, u32, vp, u32, vp, u32]
        _lib.pbrhip_scene_update_curve_mesh.argtypes = [vp, u32, vp, u32]
        _lib.pbrhip_scene_update_instance_transform.argtypes = [vp, u32, vp]
        _lib.pbrhip_scene_refit.argtypes = [vp]
        _lib.pbrhip_scene_update_triangle_mesh_device.argtypes = [vp, u32, vp, u32, vp, u32, vp]
        _lib.pbrhip_scene_update_curve_mesh_device.argtypes = [vp, u32, vp, u32, vp]
        _lib.pbrhip_scene_read_slots.argtypes = [vp, vp, vp, vp]
        _lib.pbrhip_tree_refit.argtypes = [C.c_int, u32, vp, vp, vp, u32, vp, u32, C.c_int, vp, vp, u32]
        _lib.pbrhip_render_adaptive.argtypes = _lib.pbrhip_render_adaptive_device.argtypes = [vp, vp, f32, u32, vp, vp, vp, vp, vp, vp, vp]
        _lib.pbrhip_adaptive_step.argtypes = [C.c_int, u32, u32, vp, vp, u32, u32, f32, vp, u32, vp, vp, vp, vp, vp]
        _lib.pbrhip_render_rays.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]
        _lib.pbrhip_render_rays_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]
        _lib.pbrhip_render_features_rays_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        _lib.pbrhip_projection_rays_device.argtypes = [vp, u32, f32, u32, u32, u32, u32, C.c_uint64, vp, vp]
        _lib.pbrhip_scene_snapshot_pose.argtypes = [vp]
        _lib.pbrhip_render_motion.argtypes = _lib.pbrhip_render_motion_device.argtypes = [vp, vp, vp, vp, vp]
        _lib.pbrhip_temporal_accumulate.argtypes = _lib.pbrhip_temporal_accumulate_device.argtypes = [C.c_int, u32, u32, vp, vp, vp, vp, vp, vp, f32, f32, f32, u32, vp]
        _lib.pbrhip_scene_object_ids.argtypes = [vp, vp, C.c_size_t, u32, vp]
        _lib.pbrhip_scene_object_ids_device.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
        _lib.pbrhip_svgf_accumulate.argtypes = _lib.pbrhip_svgf_accumulate_device.argtypes = [C.c_int, u32, u32] + [vp] * 11 + [f32, f32, f32, u32, vp, vp]
        _lib.pbrhip_svgf_filter.argtypes = _lib.pbrhip_svgf_filter_device.argtypes = [C.c_int, u32, u32] + [vp] * 6 + [u32, f32, f32, u32, vp, vp]
        _lib.pbrhip_render_features_emission.argtypes = _lib.pbrhip_render_features_emission_device.argtypes = [vp] * 6
        _lib.pbrhip_emission_split.argtypes = _lib.pbrhip_emission_split_device.argtypes = [C.c_int, u32, u32] + [vp] * 7
        _lib.pbrhip_emission_merge.argtypes = _lib.pbrhip_emission_merge_device.argtypes = [C.c_int, u32, u32] + [vp] * 4
        _lib.pbrhip_trace_closest_device.argtypes = _lib.pbrhip_nearest_point_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        _lib.pbrhip_trace_any_device.argtypes = _lib.pbrhip_nearest_point.argtypes = [vp, vp, C.c_size_t, vp, vp]
        _lib.pbrhip_scene_signed_distance_info.argtypes = [vp, vp]
        _lib.pbrhip_signed_distance.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
        _lib.pbrhip_signed_distance_device.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp]
        _lib.pbrhip_signed_distance_grid_device.argtypes = [vp, vp, vp, vp, f32, vp, vp]
        _lib.pbrhip_scene_read_pseudonormals.argtypes = [vp, vp, vp]
        _lib.pbrhip_trace_all.argtypes = [vp, vp, C.c_size_t, u32, vp, vp]
        _lib.pbrhip_trace_all_device.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, vp]
        _lib.pbrhip_k_nearest.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, vp]
        _lib.pbrhip_k_nearest_device.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, vp, vp]
        if hasattr(_lib, "pbrhip_scene_shadow_grid_info"):  # (an earlier commit's library loaded through PBRHIP_LIB for an A/B has no grid)
            _lib.pbrhip_scene_shadow_grid_info.argtypes = [vp, vp]
            _lib.pbrhip_scene_read_shadow_grid.argtypes = [vp, vp, C.c_size_t]
        if _lib.pbrhip_abi_version() != ABI_VERSION:
            v = _lib.pbrhip_abi_version()
            _lib = None
            raise RuntimeError(f"{LIB_PATH} has struct layout version {v}, this binding was written for {ABI_VERSION}: rebuild")
    return _lib
