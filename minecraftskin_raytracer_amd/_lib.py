"""Loader for the product library libmcrt.so (HIP kernels + C ABI).  No fallback of any kind: if the
library is missing, loading fails loudly."""
from __future__ import annotations

import ctypes as C
import os

from . import abi

PKG = os.path.dirname(os.path.abspath(__file__))
# MCRT_LIB selects another build of the SAME library (kernel tuning experiments); there is still no fallback
LIB_PATH = os.environ.get("MCRT_LIB") or os.path.join(PKG, "libmcrt.so")

_lib = None

# every symbol include/mcrt.h declares
EXPORTED_SYMBOLS = [
    "mcrt_config_init", "mcrt_generate_tiles", "mcrt_abi_version", "mcrt_device_count", "mcrt_last_error",
    "mcrt_render", "mcrt_render_tile", "mcrt_scene_create", "mcrt_scene_destroy", "mcrt_render_device", "mcrt_owned_pixel_rows",
    "mcrt_unpack_rows_device", "mcrt_quantize_rgba8_device", "mcrt_quantize_rgba8", "mcrt_last_timings",
    "mcrt_time_render_device", "mcrt_build_skin_scene", "mcrt_build_default_scene", "mcrt_builtin_pose",
    "mcrt_scene_desc_free", "mcrt_scene_flatten", "mcrt_probe_intersect", "mcrt_probe_trace",
    "mcrt_probe_mt_uniform", "mcrt_probe_detmath", "mcrt_probe_detmath_range", "mcrt_probe_div_const",
    "mcrt_render_device_ex", "mcrt_write_png_rgba8", "mcrt_encode_png_rgba8", "mcrt_write_png_f32", "mcrt_render_png",
    "mcrt_assemble_frame_device", "mcrt_scene_set_lanes", "mcrt_trim", "mcrt_scene_check", "mcrt_render_multi",
    "mcrt_render_rgba8", "mcrt_render_rect", "mcrt_render_batch_device", "mcrt_render_batch", "mcrt_last_batch_info",
    "mcrt_scene_set_background", "mcrt_render_ex", "mcrt_render_batch_ex", "mcrt_render_png_ex",
    "mcrt_bg_plate_info", "mcrt_draw_plate_info",
    "mcrt_render_layers_device", "mcrt_render_layers_batch_device", "mcrt_render_layers", "mcrt_render_layers_batch",
    "mcrt_scene_pick", "mcrt_skin_texel",
    "mcrt_render_ground_device", "mcrt_render_ground_batch_device", "mcrt_render_ground", "mcrt_scene_floor",
    "mcrt_render_reflection_device", "mcrt_render_reflection_batch_device", "mcrt_render_reflection",
    "mcrt_render_light_device", "mcrt_render_light_batch_device", "mcrt_render_light",
    "mcrt_scene_create_skin", "mcrt_scene_set_skin_device", "mcrt_scene_set_skins_batch_device", "mcrt_scene_set_skin",
    "mcrt_skin_pool_map", "mcrt_probe_scene_blob", "mcrt_probe_units",
    "mcrt_bake_light_device", "mcrt_bake_light_batch_device", "mcrt_bake_light", "mcrt_bake_texel_table", "mcrt_scene_texels",
    "mcrt_scene_set_view", "mcrt_scene_set_view_device", "mcrt_scene_set_views_batch_device", "mcrt_skin_view_table",
    "mcrt_shot_init", "mcrt_shot_scratch_bytes", "mcrt_composite_shot_batch_device", "mcrt_render_shot_batch_device",
    "mcrt_render_shot_device", "mcrt_render_shot", "mcrt_render_shot_batch", "mcrt_render_shot_png",
    "mcrt_render_ground_occlusion_device", "mcrt_render_ground_occlusion_batch_device", "mcrt_render_ground_occlusion",
    "mcrt_shot_scratch_bytes_occ", "mcrt_render_shot_batch_device_occ", "mcrt_composite_shot_batch_device_occ",
    "mcrt_render_shot_batch_occ", "mcrt_render_shot_png_occ",
    "mcrt_shot_ex_init", "mcrt_shot_scratch_bytes_ex", "mcrt_composite_shot_batch_device_ex", "mcrt_render_shot_batch_device_ex",
    "mcrt_render_shot_batch_ex", "mcrt_render_shot_png_ex",
    "mcrt_build_skin_scene_model", "mcrt_scene_create_skin_model", "mcrt_skin_texel_model", "mcrt_skin_pool_map_model",
    "mcrt_skin_view_table_model", "mcrt_skin_model_of",
    "mcrt_scene_set_extra_lights", "mcrt_scene_extra_lights", "mcrt_render_lights", "mcrt_render_png_lights",
    "mcrt_probe_sample_rows", "mcrt_sample_table_info",
    "mcrt_device_tables_info", "mcrt_scene_tables", "mcrt_probe_seed_words",
    "mcrt_build_skin_scene_cape", "mcrt_cape_texel", "mcrt_cape_pool_map", "mcrt_scene_create_skin_cape",
    "mcrt_scene_set_cape", "mcrt_scene_set_cape_device", "mcrt_scene_set_capes_batch_device",
    "mcrt_skin_view_table_cape", "mcrt_scene_set_view_cape", "mcrt_scene_set_view_cape_device", "mcrt_scene_set_views_cape_batch_device",
    "mcrt_render_light_multi_device", "mcrt_render_light_multi_batch_device", "mcrt_render_light_multi",
    "mcrt_bake_light_multi_device", "mcrt_bake_light_multi_batch_device", "mcrt_bake_light_multi",
]


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m minecraftskin_raytracer_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    desc_p = C.POINTER(abi.McrtSceneDesc)
    cfg_p = C.POINTER(abi.McrtConfig)
    u8_p = C.POINTER(C.c_uint8)
    f_p = abi.c_float_p
    vp = C.c_void_p
    layers_p = C.POINTER(abi.McrtLayers)
    ground_p = C.POINTER(abi.McrtGround)
    ground_occlusion_p = C.POINTER(abi.McrtGroundOcclusion)
    reflection_p = C.POINTER(abi.McrtReflection)
    light_p = C.POINTER(abi.McrtLightPlanes)
    bake_p = C.POINTER(abi.McrtBakePlanes)
    light_multi_p = C.POINTER(abi.McrtLightPlanesMulti)
    bake_multi_p = C.POINTER(abi.McrtBakePlanesMulti)
    shot_p = C.POINTER(abi.McrtShot)
    shot_ex_p = C.POINTER(abi.McrtShotEx)
    lights_p = C.POINTER(abi.McrtLightSource)
    sig = {
        "mcrt_config_init": (None, [cfg_p]),
        "mcrt_generate_tiles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(abi.McrtTile), C.c_int]),
        "mcrt_abi_version": (C.c_int, []),
        "mcrt_device_count": (C.c_int, []),
        "mcrt_last_error": (C.c_char_p, []),
        "mcrt_render": (C.c_int, [desc_p, cfg_p, f_p, abi.PROGRESS_FN, vp, C.c_int]),
        "mcrt_render_tile": (C.c_int, [desc_p, cfg_p, C.c_int, f_p, C.c_int]),
        "mcrt_render_rect": (C.c_int, [desc_p, cfg_p, C.POINTER(abi.McrtTile), f_p, C.c_int]),
        "mcrt_render_rgba8": (C.c_int, [desc_p, cfg_p, u8_p, abi.PROGRESS_FN, vp, C.POINTER(C.c_int), C.c_int, C.c_int]),
        "mcrt_scene_create": (C.c_int, [desc_p, C.c_int, C.POINTER(vp)]),
        "mcrt_scene_destroy": (None, [vp]),
        "mcrt_render_device": (C.c_int, [vp, cfg_p, C.c_int, C.c_int, C.c_int, vp, vp]),
        "mcrt_owned_pixel_rows": (C.c_int, [cfg_p, C.c_int, C.c_int]),
        "mcrt_render_device_ex": (C.c_int, [vp, cfg_p, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "mcrt_render_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, vp, vp, C.c_size_t, vp]),
        "mcrt_render_batch": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, f_p, u8_p, C.c_int]),
        "mcrt_last_batch_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mcrt_scene_set_background": (C.c_int, [vp, C.c_int]),
        "mcrt_render_ex": (C.c_int, [desc_p, cfg_p, C.c_int, f_p, u8_p, abi.PROGRESS_FN, vp, C.POINTER(C.c_int), C.c_int, C.c_int]),
        "mcrt_render_batch_ex": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, C.c_int, f_p, u8_p, C.c_int]),
        "mcrt_render_png_ex": (C.c_int, [desc_p, cfg_p, C.c_int, C.c_char_p, C.c_int]),
        "mcrt_scene_set_extra_lights": (C.c_int, [vp, lights_p, C.c_int]),
        "mcrt_scene_extra_lights": (C.c_int, [vp, lights_p, C.c_int]),
        "mcrt_render_lights": (C.c_int, [desc_p, cfg_p, lights_p, C.c_int, C.c_int, f_p, u8_p, abi.PROGRESS_FN, vp, C.POINTER(C.c_int), C.c_int, C.c_int]),
        "mcrt_render_png_lights": (C.c_int, [desc_p, cfg_p, lights_p, C.c_int, C.c_int, C.c_char_p, C.c_int]),
        "mcrt_render_layers_device": (C.c_int, [vp, cfg_p, layers_p, vp]),
        "mcrt_render_layers_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, layers_p, C.c_size_t, vp]),
        "mcrt_render_layers": (C.c_int, [desc_p, cfg_p, layers_p, C.c_int]),
        "mcrt_render_layers_batch": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, layers_p, C.c_int]),
        "mcrt_render_ground_device": (C.c_int, [vp, cfg_p, C.c_float, ground_p, vp]),
        "mcrt_render_ground_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, f_p, ground_p, C.c_size_t, vp]),
        "mcrt_render_ground": (C.c_int, [desc_p, cfg_p, C.c_float, ground_p, C.c_int]),
        "mcrt_scene_floor": (C.c_int, [desc_p, f_p]),
        "mcrt_render_ground_occlusion_device": (C.c_int, [vp, cfg_p, C.c_float, ground_occlusion_p, vp]),
        "mcrt_render_ground_occlusion_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, f_p, ground_occlusion_p, C.c_size_t, vp]),
        "mcrt_render_ground_occlusion": (C.c_int, [desc_p, cfg_p, C.c_float, ground_occlusion_p, C.c_int]),
        "mcrt_render_reflection_device": (C.c_int, [vp, cfg_p, C.c_float, reflection_p, vp]),
        "mcrt_render_reflection_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, f_p, reflection_p, C.c_size_t, vp]),
        "mcrt_render_reflection": (C.c_int, [desc_p, cfg_p, C.c_float, reflection_p, C.c_int]),
        "mcrt_render_light_device": (C.c_int, [vp, cfg_p, light_p, vp]),
        "mcrt_render_light_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, light_p, C.c_size_t, vp]),
        "mcrt_render_light": (C.c_int, [desc_p, cfg_p, light_p, C.c_int]),
        "mcrt_bake_light_device": (C.c_int, [vp, cfg_p, C.c_int, bake_p, vp]),
        "mcrt_bake_light_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, C.c_int, bake_p, C.c_size_t, vp]),
        "mcrt_bake_light": (C.c_int, [desc_p, cfg_p, C.c_int, bake_p, C.c_int]),
        "mcrt_render_light_multi_device": (C.c_int, [vp, cfg_p, light_multi_p, vp]),
        "mcrt_render_light_multi_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, light_multi_p, C.c_size_t, vp]),
        "mcrt_render_light_multi": (C.c_int, [desc_p, cfg_p, lights_p, C.c_int, light_multi_p, C.c_int]),
        "mcrt_bake_light_multi_device": (C.c_int, [vp, cfg_p, C.c_int, bake_multi_p, vp]),
        "mcrt_bake_light_multi_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, C.c_int, bake_multi_p, C.c_size_t, vp]),
        "mcrt_bake_light_multi": (C.c_int, [desc_p, cfg_p, lights_p, C.c_int, C.c_int, bake_multi_p, C.c_int]),
        "mcrt_bake_texel_table": (C.c_int, [desc_p, abi.c_int32_p, C.c_int]),
        "mcrt_scene_texels": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "mcrt_scene_pick": (C.c_int, [vp, cfg_p, abi.c_int32_p, C.c_int, vp]),
        "mcrt_skin_texel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mcrt_scene_create_skin": (C.c_int, [C.c_int, f_p, desc_p, C.c_int, C.POINTER(vp)]),
        "mcrt_scene_create_skin_model": (C.c_int, [C.c_int, C.c_int, f_p, desc_p, C.c_int, C.POINTER(vp)]),
        "mcrt_skin_texel_model": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mcrt_skin_pool_map_model": (C.c_int, [C.c_int, C.c_int, abi.c_int32_p, C.c_int]),
        "mcrt_skin_view_table_model": (C.c_int, [C.c_int, C.c_int, f_p, desc_p, vp, C.c_size_t]),
        "mcrt_skin_model_of": (C.c_int, [u8_p, C.c_int, C.c_int]),
        "mcrt_build_skin_scene_model": (C.c_int, [u8_p, C.c_int, C.c_int, C.c_int, f_p, C.POINTER(desc_p)]),
        "mcrt_scene_set_skin_device": (C.c_int, [vp, vp, vp]),
        "mcrt_scene_set_skins_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.c_size_t, vp]),
        "mcrt_scene_set_skin": (C.c_int, [vp, u8_p]),
        "mcrt_skin_pool_map": (C.c_int, [C.c_int, abi.c_int32_p, C.c_int]),
        "mcrt_scene_set_view": (C.c_int, [vp, f_p, desc_p]),
        "mcrt_scene_set_view_device": (C.c_int, [vp, f_p, desc_p, vp]),
        "mcrt_scene_set_views_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.POINTER(desc_p), vp]),
        "mcrt_skin_view_table": (C.c_int, [C.c_int, f_p, desc_p, vp, C.c_size_t]),
        "mcrt_build_skin_scene_cape": (C.c_int, [u8_p, C.c_int, C.c_int, C.c_int, f_p, u8_p, C.c_float, C.POINTER(desc_p)]),
        "mcrt_cape_texel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "mcrt_cape_pool_map": (C.c_int, [abi.c_int32_p, C.c_int]),
        "mcrt_scene_create_skin_cape": (C.c_int, [C.c_int, C.c_int, f_p, desc_p, C.c_float, C.c_int, C.POINTER(vp)]),
        "mcrt_scene_set_cape": (C.c_int, [vp, u8_p]),
        "mcrt_scene_set_cape_device": (C.c_int, [vp, vp, vp]),
        "mcrt_scene_set_capes_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.c_size_t, vp]),
        "mcrt_skin_view_table_cape": (C.c_int, [C.c_int, C.c_int, f_p, desc_p, C.c_float, vp, C.c_size_t]),
        "mcrt_scene_set_view_cape": (C.c_int, [vp, f_p, desc_p, f_p]),
        "mcrt_scene_set_view_cape_device": (C.c_int, [vp, f_p, desc_p, f_p, vp]),
        "mcrt_scene_set_views_cape_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, vp, C.POINTER(desc_p), vp, vp]),
        "mcrt_shot_init": (None, [shot_p]),
        "mcrt_shot_scratch_bytes": (C.c_size_t, [cfg_p, shot_p, C.c_int]),
        "mcrt_composite_shot_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_p, C.POINTER(abi.McrtShotInputs), C.c_size_t, vp, vp, C.c_size_t, vp]),
        "mcrt_render_shot_batch_device": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_p, f_p, vp, C.c_size_t, vp, vp, C.c_size_t, vp]),
        "mcrt_render_shot_device": (C.c_int, [vp, cfg_p, shot_p, C.c_float, vp, C.c_size_t, vp, vp, vp]),
        "mcrt_render_shot": (C.c_int, [desc_p, cfg_p, shot_p, C.c_float, f_p, u8_p, C.c_int]),
        "mcrt_render_shot_batch": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, shot_p, f_p, f_p, u8_p, C.c_int]),
        "mcrt_render_shot_png": (C.c_int, [desc_p, cfg_p, shot_p, C.c_float, C.c_char_p, C.c_int]),
        "mcrt_shot_scratch_bytes_occ": (C.c_size_t, [cfg_p, shot_p, C.c_float, C.c_int]),
        "mcrt_render_shot_batch_device_occ": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_p, C.c_float, f_p, vp, C.c_size_t, vp, vp, C.c_size_t, vp]),
        "mcrt_composite_shot_batch_device_occ": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_p, C.POINTER(abi.McrtShotInputs), vp, C.c_float, C.c_size_t, vp,
                                                           vp, C.c_size_t, vp]),
        "mcrt_render_shot_batch_occ": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, shot_p, C.c_float, f_p, f_p, u8_p, C.c_int]),
        "mcrt_render_shot_png_occ": (C.c_int, [desc_p, cfg_p, shot_p, C.c_float, C.c_float, C.c_char_p, C.c_int]),
        "mcrt_shot_ex_init": (None, [shot_ex_p]),
        "mcrt_shot_scratch_bytes_ex": (C.c_size_t, [cfg_p, shot_ex_p, C.c_int]),
        "mcrt_composite_shot_batch_device_ex": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_ex_p, C.POINTER(abi.McrtShotInputs), vp, C.c_size_t, vp, vp,
                                                          C.c_size_t, vp, vp]),
        "mcrt_render_shot_batch_device_ex": (C.c_int, [C.POINTER(vp), C.c_int, cfg_p, shot_ex_p, f_p, vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp]),
        "mcrt_render_shot_batch_ex": (C.c_int, [C.POINTER(desc_p), C.c_int, cfg_p, shot_ex_p, f_p, f_p, u8_p, vp, C.c_int]),
        "mcrt_render_shot_png_ex": (C.c_int, [desc_p, cfg_p, shot_ex_p, C.c_float, C.c_char_p, C.c_int, vp, C.c_int]),
        "mcrt_probe_scene_blob": (C.c_int, [vp, vp, C.c_size_t]),
        "mcrt_write_png_rgba8": (C.c_int, [C.c_char_p, u8_p, C.c_int, C.c_int]),
        "mcrt_encode_png_rgba8": (C.c_size_t, [u8_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
        "mcrt_write_png_f32": (C.c_int, [C.c_char_p, f_p, C.c_int, C.c_int]),
        "mcrt_render_png": (C.c_int, [desc_p, cfg_p, C.c_char_p, C.c_int]),
        "mcrt_assemble_frame_device": (C.c_int, [cfg_p, C.c_int, vp, C.c_size_t, vp, vp]),
        "mcrt_scene_set_lanes": (C.c_int, [vp, C.c_int]),
        "mcrt_trim": (None, []),
        "mcrt_scene_check": (C.c_int, [vp]),
        "mcrt_unpack_rows_device": (C.c_int, [cfg_p, C.c_int, C.c_int, vp, vp, vp]),
        "mcrt_quantize_rgba8_device": (C.c_int, [vp, vp, C.c_size_t, vp]),
        "mcrt_quantize_rgba8": (None, [f_p, u8_p, C.c_size_t]),
        "mcrt_last_timings": (C.c_int, [C.POINTER(abi.McrtTimings)]),
        "mcrt_time_render_device": (C.c_int, [vp, cfg_p, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, f_p]),
        "mcrt_render_multi": (C.c_int, [desc_p, cfg_p, f_p, abi.PROGRESS_FN, vp, C.POINTER(C.c_int), C.c_int, C.c_int]),
        "mcrt_build_skin_scene": (C.c_int, [u8_p, C.c_int, C.c_int, f_p, C.POINTER(desc_p)]),
        "mcrt_build_default_scene": (C.c_int, [f_p, C.POINTER(desc_p)]),
        "mcrt_builtin_pose": (C.c_int, [C.c_int, f_p]),
        "mcrt_scene_desc_free": (None, [desc_p]),
        "mcrt_scene_flatten": (C.c_size_t, [desc_p, vp, C.c_size_t]),
        "mcrt_probe_intersect": (C.c_int, [vp, f_p, C.c_int, vp]),
        "mcrt_probe_trace": (C.c_int, [vp, cfg_p, f_p, C.c_int, C.c_int, f_p]),
        "mcrt_probe_mt_uniform": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, f_p]),
        "mcrt_probe_detmath": (C.c_int, [C.c_int, C.c_int, f_p, f_p, C.c_size_t, f_p]),
        "mcrt_probe_detmath_range": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_uint64)]),
        "mcrt_probe_div_const": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class McrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mcrt error {code}: {msg}")
        self.code = code


def check(rc: int) -> None:
    if rc != 0:
        raise McrtError(rc, load().mcrt_last_error().decode("utf-8", "replace"))
