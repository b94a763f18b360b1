"""MI355X-native tile-render hot path of MinecraftSkin_Raytracer (HIP kernels behind a C ABI)."""
from .abi import Config, Mesh, Scene, Texture  # noqa: F401
from .skins import synthetic_skin  # noqa: F401
from .api import (  # noqa: F401
    DeviceScene,
    SkinBatch,
    assemble_frame_device,
    bg_plate_info,
    draw_plate_info,
    ImageWriter,
    MeshBuilder,
    SceneDesc,
    TileRenderer,
    device_count,
    flatten,
    getBuiltinPoses,
    last_batch_info,
    probe_detmath,
    probe_detmath_range,
    probe_mt_uniform,
    quantize_rgba8,
    quantize_rgba8_device,
    render_batch_device,
    render_layers_batch_device,
    render_ground_batch_device,
    render_reflection_batch_device,
    render_light_batch_device,
    scene_floor,
    set_skins_batch_device,
    skin_pool_map,
    skin_texel,
    render_png,
    trim,
    unpack_rows_device,
)

__all__ = [
    "Config", "Mesh", "Scene", "Texture", "synthetic_skin", "DeviceScene", "MeshBuilder", "SceneDesc",
    "TileRenderer", "device_count", "flatten", "getBuiltinPoses", "probe_detmath", "probe_detmath_range",
    "probe_mt_uniform", "quantize_rgba8", "quantize_rgba8_device", "unpack_rows_device", "ImageWriter", "render_png", "assemble_frame_device", "trim",
    "render_batch_device", "last_batch_info", "bg_plate_info", "draw_plate_info", "render_layers_batch_device", "skin_texel",
    "render_ground_batch_device", "render_reflection_batch_device", "render_light_batch_device", "scene_floor", "SkinBatch", "set_skins_batch_device", "skin_pool_map",
]
