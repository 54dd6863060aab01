"""ctypes mirror of include/wurblpt_hip.h (the C ABI of the device library).

Field order and types must match the header exactly; tests/test_abi.py checks the sizes
against values compiled from the header.
"""
import ctypes as C

WPT_ABI_VERSION = 5
WPT_OK = 0

NODE_INNER, NODE_TRIANGLE, NODE_SPHERE, NODE_EMPTY = 0, 1, 2, 3
MATF_TOF_LIGHT = 16
TOF_MAX_PHASES = 8
LIGHT_GROUPS_MAX, LIGHT_GROUP_NONE = 255, 0xff
VIEWS_MAX_PIXELS = 0x7fffffff  # WPT_VIEWS_MAX_PIXELS: the pixels of a batch of views, and of a split render's streams
SPLIT_PIXELS_PER_LANE = 4      # wpt_split_plan: the pixels per lane a frame is split for
MAT_NONE, MAT_LAMBERTIAN, MAT_LIGHT_DIFFUSE, MAT_MIRROR, MAT_GGX, MAT_GLASS, MAT_MODPHONG, MAT_TWOSIDED, MAT_RGL, MAT_LIGHT_SPOT = range(10)


class BvhNode(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("link", C.c_uint32), ("kind", C.c_uint32)]


class TriGeom(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("instance", C.c_uint32), ("v1", C.c_float * 3), ("material", C.c_uint32),
                ("v2", C.c_float * 3), ("flags", C.c_uint32)]


class TriAttr(C.Structure):
    _fields_ = [("n0", C.c_float * 3), ("n1", C.c_float * 3), ("n2", C.c_float * 3),
                ("tc0", C.c_float * 2), ("tc1", C.c_float * 2), ("tc2", C.c_float * 2),
                ("t0", C.c_float * 3), ("t1", C.c_float * 3), ("t2", C.c_float * 3)]


class Instance(C.Structure):
    _fields_ = [("N", C.c_float * 9), ("material", C.c_uint32), ("flags", C.c_uint32), ("animation", C.c_int32)]


class Keyframe(C.Structure):
    _fields_ = [("t", C.c_float), ("translation", C.c_float * 3), ("rotation", C.c_float * 4), ("scaling", C.c_float * 3)]


class Animation(C.Structure):
    _fields_ = [("first_keyframe", C.c_uint32), ("keyframe_count", C.c_uint32)]


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("rotation", C.c_float * 4),
                ("material", C.c_uint32), ("animation", C.c_int32), ("reserved", C.c_uint32 * 2)]


class Hotspot(C.Structure):
    _fields_ = [("prim", C.c_uint32), ("transform", C.c_uint32), ("kind", C.c_uint32), ("animation", C.c_int32),
                ("p0", C.c_float * 3), ("p1", C.c_float * 3), ("p2", C.c_float * 3), ("M", C.c_float * 16)]


class Material(C.Structure):
    _fields_ = [("type", C.c_uint32), ("flags", C.c_uint32), ("normal_tex", C.c_int32), ("tex", C.c_int32 * 5),
                ("v", (C.c_float * 4) * 5), ("f", C.c_float * 4)]


class Texture(C.Structure):
    _fields_ = [("type", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("comps", C.c_uint32),
                ("texel_type", C.c_uint32), ("linearize_srgb", C.c_uint32), ("child", C.c_int32),
                ("reserved", C.c_uint32), ("texel_offset", C.c_uint64), ("coord_factor", C.c_float * 2),
                ("coord_offset", C.c_float * 2), ("a", C.c_float * 4), ("b", C.c_float * 4)]


class RglWarp(C.Structure):
    _fields_ = [("size_x", C.c_uint32), ("size_y", C.c_uint32), ("dims", C.c_uint32), ("param_size", C.c_uint32 * 3),
                ("param_stride", C.c_uint32 * 3), ("param_values", C.c_uint32 * 3), ("data", C.c_uint32),
                ("marginal_cdf", C.c_uint32), ("conditional_cdf", C.c_uint32), ("patch_size", C.c_float * 2),
                ("inv_patch_size", C.c_float * 2)]


class RglBrdf(C.Structure):
    _fields_ = [("ndf", RglWarp), ("sigma", RglWarp), ("vndf", RglWarp), ("luminance", RglWarp), ("rgb", RglWarp),
                ("isotropic", C.c_uint32), ("jacobian", C.c_uint32)]


class Envmap(C.Structure):
    _fields_ = [("type", C.c_uint32), ("compat", C.c_uint32), ("tex", C.c_int32), ("N", C.c_int32),
                ("M", C.c_void_p), ("Ms", C.c_void_p), ("Mcs", C.c_void_p), ("cube_tex", C.c_int32 * 6)]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("node_count", C.c_uint32), ("tri_count", C.c_uint32),
                ("instance_count", C.c_uint32), ("material_count", C.c_uint32), ("texture_count", C.c_uint32),
                ("hotspot_count", C.c_uint32), ("sphere_count", C.c_uint32), ("texel_bytes", C.c_uint64),
                ("nodes", C.POINTER(BvhNode)), ("tri_geom", C.POINTER(TriGeom)), ("tri_attr", C.POINTER(TriAttr)),
                ("instances", C.POINTER(Instance)), ("materials", C.POINTER(Material)),
                ("textures", C.POINTER(Texture)), ("texels", C.c_void_p), ("hotspots", C.POINTER(Hotspot)),
                ("envmap", Envmap), ("spheres", C.POINTER(Sphere)), ("rgl_count", C.c_uint32), ("reserved", C.c_uint32),
                ("rgl_data_count", C.c_uint64), ("rgl_brdfs", C.POINTER(RglBrdf)), ("rgl_data", C.POINTER(C.c_float)),
                ("animation_count", C.c_uint32), ("keyframe_count", C.c_uint32), ("animations", C.POINTER(Animation)),
                ("keyframes", C.POINTER(Keyframe))]


class Camera(C.Structure):
    _fields_ = [("l", C.c_float), ("r", C.c_float), ("b", C.c_float), ("t", C.c_float),
                ("translation", C.c_float * 3), ("rotation", C.c_float * 4), ("scaling", C.c_float * 3),
                ("lens_radius", C.c_float), ("focus_dist", C.c_float),
                ("distortion_type", C.c_uint32), ("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("p1", C.c_float),
                ("p2", C.c_float), ("b1", C.c_float), ("b2", C.c_float), ("b3", C.c_float), ("b4", C.c_float),
                ("dist_center", C.c_float * 2), ("dist_focal_length", C.c_float * 2), ("dist_inverse_focal_length", C.c_float * 2),
                ("surround_mode", C.c_uint32), ("stereoscopic_distance", C.c_float), ("animation", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("max_path_components", C.c_uint32), ("rr_threshold", C.c_float),
                ("randomize_ray_over_pixel", C.c_uint32), ("min_hit_distance", C.c_float),
                ("min_dist_to_light", C.c_float), ("max_dist_to_light", C.c_float),
                ("min_path_len", C.c_float), ("max_path_len", C.c_float), ("t0", C.c_float), ("t1", C.c_float)]


class Shutter(C.Structure):
    """wpt_shutter: the rolling shutter of the wpt_render_shutter_* calls"""
    _fields_ = [("row_time", C.c_float), ("from_top", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TofSensor(C.Structure):
    """wpt_tof_sensor: the time-of-flight sensor's constants and the phase offsets of the phase images of one launch"""
    _fields_ = [("pixel_area", C.c_float), ("exposure_time", C.c_float), ("contrast", C.c_float), ("frac_modfreq_c", C.c_float),
                ("phase_count", C.c_uint32), ("tau", C.c_float * TOF_MAX_PHASES)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "rays", "node_visits", "leaf_tests", "pdf_tests", "scatters")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class ProgressInfo(C.Structure):
    """wpt_progress_info: the header of a saved progressive session"""
    _fields_ = [(n, C.c_uint32) for n in ("version", "width", "height", "samples_sqrt", "block_start", "block_size", "rows_done", "reserved")] \
        + [("tag", C.c_uint64), ("state_bytes", C.c_uint64)]


class DenoiseParams(C.Structure):
    """wpt_denoise_params; the defaults are the header's"""
    _fields_ = [("sigma_l", C.c_float), ("sigma_z", C.c_float), ("normal_log2", C.c_uint32), ("iterations", C.c_uint32)]

    def __init__(self, sigma_l=1.0, sigma_z=0.1, normal_log2=7, iterations=5):
        super().__init__(sigma_l, sigma_z, normal_log2, iterations)


DENOISE_MAX_ITERATIONS, DENOISE_MAX_NORMAL_LOG2 = 8, 16
DENOISE_ALBEDO_FLOOR = 1.0 / 64  # what an albedo_floor <= 0 of wpt_postproc_denoise_demodulated* stands for


class TemporalParams(C.Structure):
    """wpt_temporal_params; the defaults are the header's"""
    _fields_ = [("max_history", C.c_float), ("normal_cos_min", C.c_float), ("position_tolerance", C.c_float), ("reserved", C.c_uint32)]

    def __init__(self, max_history=32.0, normal_cos_min=0.9, position_tolerance=0.02, reserved=0):
        super().__init__(max_history, normal_cos_min, position_tolerance, reserved)


TEMPORAL_HISTORY_BYTES_PER_PIXEL = 48  # WPT_TEMPORAL_HISTORY_BYTES_PER_PIXEL: three records of four floats


# the saved state of a progressive session (include/wurblpt_hip.h has the layout)
PROGRESS_MAGIC, PROGRESS_STATE_VERSION, PROGRESS_HEADER_BYTES, PROGRESS_CARRY_BYTES = 0x50545057, 1, 224, 32


STRUCT_SIZES = {
    "wpt_bvh_node": (BvhNode, 32), "wpt_tri_geom": (TriGeom, 48), "wpt_tri_attr": (TriAttr, 96),
    "wpt_instance": (Instance, 48), "wpt_sphere": (Sphere, 48), "wpt_hotspot": (Hotspot, 116), "wpt_material": (Material, 128),
    "wpt_texture": (Texture, 88), "wpt_rgl_warp": (RglWarp, 76), "wpt_rgl_brdf": (RglBrdf, 388), "wpt_camera": (Camera, 140), "wpt_params": (Params, 40), "wpt_shutter": (Shutter, 16),
    "wpt_keyframe": (Keyframe, 44), "wpt_animation": (Animation, 8),
    "wpt_counters": (Counters, 48), "wpt_tof_sensor": (TofSensor, 52),
    "wpt_progress_info": (ProgressInfo, 48), "wpt_denoise_params": (DenoiseParams, 16),
    "wpt_temporal_params": (TemporalParams, 16),
}


# ---- the functions: name -> (restype, argtypes), applied by device.lib() when it loads the library ----
# One entry per function the header declares; tests/test_abi.py holds every entry to the header's prototype (parameter count,
# pointer or scalar, width, signedness, return type).  restype: _I for wpt_status and int, None for void.  A pointer the Python
# callers hand over as a record (byref) is POINTER(record); one they hand over as an address is c_void_p.
_I, _U, _Q, _F, _P, _S = C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p, C.c_char_p
_pU, _pQ, _pP, _pS = C.POINTER(_U), C.POINTER(_Q), C.POINTER(_P), C.POINTER(_S)
_CAM, _PAR, _TOF, _DEN = C.POINTER(Camera), C.POINTER(Params), C.POINTER(TofSensor), C.POINTER(DenoiseParams)
_TMP = C.POINTER(TemporalParams)
_SHU = C.POINTER(Shutter)
_SCP = [_P, _CAM, _PAR]  # wpt_scene* scene, const wpt_camera* camera, const wpt_params* params
_WARP = [_P, _U, _U, _U, _CAM, _I, _P]  # wpt_postproc_lens_warp_host, wpt_postproc_distance_to_coords_host

FUNCTIONS = {
    "wpt_device_count": (_I, []),
    "wpt_select_device": (_I, [_I]),
    "wpt_current_device": (_I, [C.POINTER(_I)]),
    "wpt_device_name": (_S, [_I]),
    "wpt_device_lanes": (_I, [_I, _pU]),
    "wpt_build_info": (_S, []),
    "wpt_last_error": (_S, []),
    "wpt_scene_upload": (_I, [C.POINTER(SceneDesc), _pP]),
    "wpt_scene_free": (None, [_P]),
    "wpt_scene_check": (_I, [_P]),
    "wpt_scene_folded_links": (_I, [_P, _pU]),
    "wpt_scene_bypassed_nodes": (_I, [_P, _pU]),
    "wpt_render_block_device": (_I, _SCP + [_U] * 5 + [_P] * 3),
    "wpt_render_block": (_I, _SCP + [_U] * 5 + [_P]),
    "wpt_render_bands_device": (_I, [_P] * 3 + [_U] * 6 + [_P] * 3),
    "wpt_render_bands": (_I, [_P] * 3 + [_U] * 6 + [_P]),
    "wpt_shutter_row_interval": (_I, [_SHU, _F, _F, _U, _U, _P, _P]),
    "wpt_shutter_span": (_I, [_SHU, _F, _F, _U, _P, _P]),
    "wpt_render_shutter_block_device": (_I, _SCP + [_SHU] + [_U] * 5 + [_P] * 3),
    "wpt_render_shutter_bands_device": (_I, _SCP + [_SHU] + [_U] * 6 + [_P] * 3),
    "wpt_render_shutter_bands": (_I, _SCP + [_SHU] + [_U] * 6 + [_P]),
    "wpt_render_shutter_block": (_I, _SCP + [_SHU] + [_U] * 5 + [_P]),
    "wpt_render_transient_block_device": (_I, _SCP + [_P] + [_U] * 6 + [_P] * 3),
    "wpt_render_transient_block": (_I, _SCP + [_P] + [_U] * 6 + [_P] * 2),
    "wpt_render_light_groups_block_device": (_I, _SCP + [_P] + [_U] * 8 + [_P] * 3),
    "wpt_render_light_groups_block": (_I, _SCP + [_P] + [_U] * 8 + [_P] * 2),
    "wpt_render_tof_block_device": (_I, _SCP + [_TOF] + [_U] * 5 + [_P] * 2),
    "wpt_render_tof_block": (_I, _SCP + [_TOF] + [_U] * 5 + [_P]),
    "wpt_tof_accumulate_host": (_I, [_TOF, _U, _F, _F, _I, _P]),
    "wpt_render_views_device": (_I, [_P, _CAM, _U, _PAR, _U, _U, _U] + [_P] * 3),
    "wpt_render_views": (_I, [_P, _CAM, _U, _PAR, _U, _U, _U, _P]),
    "wpt_render_view_streams_device": (_I, [_P, _CAM, _P, _U, _PAR, _U, _U, _U] + [_P] * 3),
    "wpt_render_view_streams": (_I, [_P, _CAM, _P, _U, _PAR, _U, _U, _U, _P]),
    "wpt_render_split_device": (_I, _SCP + [_U] * 5 + [_P] * 4),
    "wpt_render_split": (_I, _SCP + [_U] * 5 + [_P] * 2),
    "wpt_split_plan": (_I, [_Q, _U, _U, _pU, _pU]),
    "wpt_render_adaptive_block_device": (_I, _SCP + [_U, _U, _P, _U, _U] + [_P] * 3),
    "wpt_render_adaptive_block": (_I, _SCP + [_U, _U, _P, _U, _U] + [_P] * 2),
    "wpt_ground_truth_device": (_I, [_P] * 6 + [_U, _U, _P, _P]),
    "wpt_ground_truth": (_I, [_P] * 6 + [_U, _U, _P]),
    "wpt_first_hit_colours_device": (_I, [_P] * 3 + [_U, _U] + [_P] * 4),
    "wpt_first_hit_colours": (_I, [_P] * 3 + [_U, _U] + [_P] * 3),
    "wpt_progress_covers": (_I, [_U, _U, _U]),
    "wpt_progress_begin": (_I, _SCP + [_U] * 5 + [_Q, _pP]),
    "wpt_progress_advance_device": (_I, [_P, _U, _P, _P]),
    "wpt_progress_advance": (_I, [_P, _U, _P]),
    "wpt_progress_rows_done": (_U, [_P]),
    "wpt_progress_rows_total": (_U, [_P]),
    "wpt_progress_preview_device": (_I, [_P, _P, _P]),
    "wpt_progress_preview": (_I, [_P, _P]),
    "wpt_progress_end": (None, [_P]),
    "wpt_progress_state_bytes": (_I, [_P, _pQ]),
    "wpt_progress_save": (_I, [_P, _P, _Q]),
    "wpt_progress_restore": (_I, [_P, _P, _Q, _CAM, _PAR, _Q, _pP]),
    "wpt_progress_state_info": (_I, [_P, _Q, C.POINTER(ProgressInfo)]),
    "wpt_postproc_to_srgb": (_I, [_P, _P, _Q, _P]),
    "wpt_postproc_max_luminance": (_I, [_P, _Q, _P, _P]),
    "wpt_postproc_uniform_rational_quantization": (_I, [_P, _P, _Q, _F, _F, _P]),
    "wpt_postproc_scale_luminance": (_I, [_P, _P, _Q, _F, _F, _P]),
    "wpt_postproc_host": (_I, [_I, _P, _P, _Q, _F, _F]),
    "wpt_postproc_mix_planes": (_I, [_P, _U, _Q, _Q, _P, _P, _P]),
    "wpt_postproc_mix_planes_host": (_I, [_P, _U, _Q, _Q, _P, _P]),
    "wpt_postproc_mean_planes": (_I, [_P, _U, _Q, _Q, _P, _P, _P]),
    "wpt_postproc_mean_planes_host": (_I, [_P, _U, _Q, _Q, _P, _P]),
    "wpt_postproc_merge_means": (_I, [_P, _U, _P, _U, _Q, _P, _P]),
    "wpt_postproc_merge_means_host": (_I, [_P, _U, _P, _U, _Q, _P]),
    "wpt_postproc_denoise": (_I, [_P] * 6 + [_U, _U, _DEN] + [_P] * 3),
    "wpt_postproc_denoise_host": (_I, [_P] * 6 + [_U, _U, _DEN] + [_P] * 2),
    "wpt_postproc_denoise_form": (_S, [_U]),
    "wpt_postproc_denoise_demodulated": (_I, [_P] * 8 + [_U, _U, _DEN, _F] + [_P] * 3),
    "wpt_postproc_denoise_demodulated_host": (_I, [_P] * 8 + [_U, _U, _DEN, _F] + [_P] * 2),
    "wpt_postproc_temporal_accumulate": (_I, [_P] * 9 + [_U, _U, _TMP] + [_P] * 3),
    "wpt_postproc_temporal_accumulate_host": (_I, [_P] * 9 + [_U, _U, _TMP] + [_P] * 2),
    "wpt_postproc_denoise_history": (_I, [_P, _U, _U, _DEN] + [_P] * 3),
    "wpt_postproc_denoise_history_host": (_I, [_P, _U, _U, _DEN] + [_P] * 2),
    "wpt_postproc_resample": (_I, [_P] + [_U] * 5 + [_P, _P]),
    "wpt_postproc_resample_host": (_I, [_P] + [_U] * 5 + [_P]),
    "wpt_postproc_lens_warp": (_I, _WARP + [_P]),
    "wpt_postproc_lens_warp_host": (_I, _WARP),
    "wpt_postproc_distance_to_coords": (_I, _WARP + [_P]),
    "wpt_postproc_distance_to_coords_host": (_I, _WARP),
    "wpt_postproc_despeckle": (_I, [_P, _U, _U, _U, _F, _P, _P]),
    "wpt_postproc_despeckle_host": (_I, [_P, _U, _U, _U, _F, _P]),
    "wpt_postproc_despeckle_form": (_S, []),
    "wpt_postproc_image_ops_tile": (None, [_pU, _pU]),
    "wpt_set_despeckle_form": (_I, [_I]),
    "wpt_set_launch_config": (_I, [_U, _U]),
    "wpt_set_wavefront": (_I, [_U] * 4),
    "wpt_set_walk": (_I, [_U]),
    "wpt_set_top_nodes": (_I, [_U]),
    "wpt_set_slices": (_I, [_U]),
    "wpt_set_bypass": (_I, [_U]),
    "wpt_set_scheduler_stats": (_I, [_P]),
    "wpt_slices_plan": (_I, [_U, _U, _U, _pU, _pU]),
    "wpt_last_slice_stats": (_I, [_pQ, _pQ]),
    "wpt_fold_plan": (_I, [_P, _pU, _P]),
    "wpt_bypass_plan": (_I, [_P, _pU, _P]),
    "wpt_kernel_name": (_S, []),
    "wpt_kernel_form": (_S, []),
    "wpt_kernel_workgroup": (_U, [_pU]),
    "wpt_kernel_hit_data": (_U, []),
    "wpt_kernel_materials_in_lds": (_U, []),
    "wpt_kernel_launch_record": (_U, []),
    "wpt_material_places": (_I, [_U] * 6 + [_pU, _pU]),
    "wpt_kernel_choice": (_I, [_U] * 9 + [_pS, _pS, _pU, _pQ, _pU]),
    "wpt_kernel_table_entry": (_I, [_U, _pU, _pS]),
    "wpt_launch_plan": (_I, [_U] * 10 + [_pU]),
    "wpt_last_render_passes": (_U, []),
}

# exported but not declared in the header: the test hooks (wpt_capi_selftest.hip, wpt_capi_scene.hip)
TEST_HOOK_FUNCTIONS = {
    "wpt_selftest_math": (_I, [_I, _I, _P, _P, _P]),
    "wpt_selftest_aabb": (_I, [_I, _P, _P, _P]),
    "wpt_selftest_triangle": (_I, [_I, _I, _P, _P]),
    "wpt_selftest_rayaux": (_I, [_I, _P, _P]),
    "wpt_selftest_sphere": (_I, [_I, _P, _P, _P]),
    "wpt_selftest_hits": (_I, [_P, _I, _P, _P]),
    "wpt_selftest_hits_host": (_I, [_P, _I, _P, _P]),
    "wpt_scene_get_envmap_tables": (_I, [_P] * 4),
}
