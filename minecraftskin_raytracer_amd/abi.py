"""ctypes mirror of include/mcrt.h (struct layouts + helpers to build scene descriptions).

Pure declarations: this module loads no library.  The product loader is ``_lib.py``; the test-only
oracle / compiled-reference loaders live under ``tests/``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import InitVar, dataclass, field, fields
from typing import List, Optional, Sequence

import numpy as np

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)

MCRT_OK = 0
MCRT_ERR_INVALID = 1
MCRT_ERR_NO_DEVICE = 2
MCRT_ERR_HIP = 3
MCRT_ERR_NOMEM = 4
SKIN_CLASSIC = 0  # MCRT_SKIN_*: the player model of a skin scene
SKIN_SLIM = 1
LAYOUT_FRAME = 0
LAYOUT_PACKED = 1
BACKGROUND_REFERENCE = 0  # MCRT_BACKGROUND_*: every pixel as the reference renders it (the default)
BACKGROUND_TRANSPARENT = 1  # the figure alone: misses add nothing, straight alpha (include/mcrt.h)
BACKGROUNDS = {"reference": BACKGROUND_REFERENCE, "transparent": BACKGROUND_TRANSPARENT}


def background_mode(name) -> int:
    """``"reference"`` / ``"transparent"`` → MCRT_BACKGROUND_*; anything else raises ``ValueError``."""
    if not isinstance(name, str) or name not in BACKGROUNDS:
        raise ValueError(f"background must be 'reference' or 'transparent', not {name!r}")
    return BACKGROUNDS[name]


class McrtConfig(C.Structure):
    """RayTracer::Config — /root/reference/src/raytracer/raytracer.h:10-38."""

    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("max_bounces", C.c_int32),
        ("samples_per_pixel", C.c_int32),
        ("tile_size", C.c_int32),
        ("thread_count", C.c_int32),
        ("soft_shadows", C.c_int32),
        ("shadow_samples", C.c_int32),
        ("ao_enabled", C.c_int32),
        ("ao_samples", C.c_int32),
        ("ao_radius", C.c_float),
        ("ao_intensity", C.c_float),
        ("dof_enabled", C.c_int32),
        ("aperture", C.c_float),
        ("focus_distance", C.c_float),
        ("gradient_bg", C.c_int32),
        ("gradient_scale", C.c_float),
        ("bg_center", C.c_float * 4),
        ("bg_edge", C.c_float * 4),
    ]


class McrtTexture(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("n_pixels", C.c_int64),
        ("rgba", c_float_p),
    ]


class McrtMesh(C.Structure):
    _fields_ = [
        ("n_triangles", C.c_int32),
        ("tri_vertices", c_float_p),
        ("tri_texture", c_int32_p),
        ("n_local_triangles", C.c_int32),
        ("local_tri_vertices", c_float_p),
        ("is_outer_layer", C.c_int32),
        ("has_rotation", C.c_int32),
        ("pivot", C.c_float * 3),
        ("rot_x", C.c_float),
        ("rot_z", C.c_float),
    ]


class McrtSceneDesc(C.Structure):
    _fields_ = [
        ("n_meshes", C.c_int32),
        ("meshes", C.POINTER(McrtMesh)),
        ("n_textures", C.c_int32),
        ("textures", C.POINTER(McrtTexture)),
        ("light_position", C.c_float * 3),
        ("light_color", C.c_float * 4),
        ("light_intensity", C.c_float),
        ("light_radius", C.c_float),
        ("camera_position", C.c_float * 3),
        ("camera_target", C.c_float * 3),
        ("camera_up", C.c_float * 3),
        ("camera_fov", C.c_float),
        ("background_color", C.c_float * 4),
    ]


class McrtTile(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class McrtHit(C.Structure):
    _fields_ = [
        ("hit", C.c_int32),
        ("t", C.c_float),
        ("point", C.c_float * 3),
        ("normal", C.c_float * 3),
        ("texture_color", C.c_float * 4),
        ("is_outer_layer", C.c_int32),
    ]


class McrtTimings(C.Structure):
    _fields_ = [
        ("flatten_ms", C.c_float),
        ("h2d_ms", C.c_float),
        ("kernel_ms", C.c_float),
        ("d2h_ms", C.c_float),
        ("total_ms", C.c_float),
    ]


class McrtLayers(C.Structure):
    """mcrt_layers: one pointer per plane (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("depth", C.c_void_p), ("normal", C.c_void_p), ("albedo", C.c_void_p), ("id", C.c_void_p)]


class McrtSurface(C.Structure):
    """mcrt_surface: what is under one pixel (mcrt_scene_pick)."""

    _fields_ = [
        ("mesh", C.c_int32),
        ("face", C.c_int32),
        ("tx", C.c_int32),
        ("ty", C.c_int32),
        ("t", C.c_float),
        ("point", C.c_float * 3),
        ("normal", C.c_float * 4),
        ("albedo", C.c_float * 4),
    ]


ID_BACK = 8  # MCRT_ID_BACK: the outer layer's exit face
ID_OUTER = 16  # MCRT_ID_OUTER: HitResult::isOuterLayer
GROUND_MAX_SAMPLES = 113  # shadowSamples of a ground pass with softShadows on
GROUND_OCCLUSION_MAX_SAMPLES = 113  # aoSamples of a ground-occlusion pass: 1 .. 113
REFLECTION_MAX_BOUNCES = 8  # maxBounces of a reflection pass
LIGHT_MAX_SAMPLES = 113  # shadowSamples (with softShadows on) and aoSamples (with the occlusion plane) of a light pass
BAKE_MAX_GRID = 4  # sub-samples per texel and axis of a light bake: grid 1..4


class McrtGround(C.Structure):
    """mcrt_ground: one pointer per plane of a ground-shadow pass (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("visibility", C.c_void_p), ("distance", C.c_void_p), ("matte", C.c_void_p)]


class McrtGroundOcclusion(C.Structure):
    """mcrt_ground_occlusion: one pointer per plane of a ground-occlusion pass (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("occlusion", C.c_void_p), ("matte", C.c_void_p)]


class McrtReflection(C.Structure):
    """mcrt_reflection: one pointer per plane of a ground-reflection pass (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("rgba", C.c_void_p), ("rgba8", C.c_void_p), ("distance", C.c_void_p)]


class McrtLightPlanes(C.Structure):
    """mcrt_light_planes: one pointer per plane of a light pass (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("visibility", C.c_void_p), ("occlusion", C.c_void_p), ("direct", C.c_void_p)]


class McrtBakePlanes(C.Structure):
    """mcrt_bake_planes: one pointer per plane of a light bake (device or host memory, by entry point); NULL = not wanted."""

    _fields_ = [("position", C.c_void_p), ("normal", C.c_void_p), ("visibility", C.c_void_p), ("occlusion", C.c_void_p), ("direct", C.c_void_p)]


@dataclass(frozen=True)
class PlaneFamily:
    """The output planes of one pass.  ``struct``: the ctypes structure, one pointer per plane in the order of ``formats``;
    ``entry``: the C name of the pass's one-shot host form, which ``_device`` and ``_batch_device`` follow for the forms on
    resident scenes; ``formats``: per plane, in canonical order, ``(dtype, components)`` of one pixel (of one pool texel for a
    bake); ``miss``: what a plane holds where nothing is hit, 0 for a plane not listed; ``noun``: what the selection's messages
    call a plane."""

    struct: type
    entry: str
    formats: dict
    miss: dict
    noun: str = "plane"

    @property
    def names(self) -> tuple:
        return tuple(self.formats)

    def select(self, planes) -> tuple:
        """The wanted planes in canonical order; an empty selection or an unknown name raises ``ValueError``."""
        if isinstance(planes, str):
            planes = (planes,)
        names = tuple(planes)
        for n in names:
            if not isinstance(n, str) or n not in self.formats:
                raise ValueError(f"{self.noun}s must be taken from {self.names}, not {n!r}")
        if not names:
            raise ValueError(f"no {self.noun} selected")
        return tuple(n for n in self.formats if n in names)

    def empty(self, name: str, n: int, *shape: int) -> np.ndarray:
        """One plane for n frames of ``shape`` (height, width; none for a bake's n texels), holding the miss value: what a frame
        of zero size keeps."""
        dtype, comps = self.formats[name]
        a = np.zeros((n,) + shape + ((comps,) if comps > 1 else ()), dtype)
        if name in self.miss:
            a[...] = self.miss[name]
        return a


_F1, _F4, _FLT_MAX = (np.float32, 1), (np.float32, 4), np.finfo(np.float32).max
# One row per family: a new pass, or a new plane of a pass, is added here (and to its structure above).
LAYERS = PlaneFamily(McrtLayers, "mcrt_render_layers", {"depth": _F1, "normal": _F4, "albedo": _F4, "id": (np.int32, 4)},
                     {"depth": _FLT_MAX, "id": (-1, 0, -1, -1)}, noun="layer")
GROUND = PlaneFamily(McrtGround, "mcrt_render_ground", {"visibility": _F1, "distance": _F1, "matte": (np.uint8, 1)},
                     {"visibility": 1, "distance": _FLT_MAX})
GROUND_OCCLUSION = PlaneFamily(McrtGroundOcclusion, "mcrt_render_ground_occlusion", {"occlusion": _F1, "matte": (np.uint8, 1)}, {"occlusion": 1})
REFLECTION = PlaneFamily(McrtReflection, "mcrt_render_reflection", {"rgba": _F4, "rgba8": (np.uint8, 4), "distance": _F1}, {"distance": _FLT_MAX})
LIGHT = PlaneFamily(McrtLightPlanes, "mcrt_render_light", {"visibility": _F1, "occlusion": _F1, "direct": _F4}, {"visibility": 1, "occlusion": 1})
BAKE = PlaneFamily(McrtBakePlanes, "mcrt_bake_light", {"position": _F4, "normal": _F4, "visibility": _F1, "occlusion": _F1, "direct": _F4},
                   {"visibility": 1, "occlusion": 1})
FAMILIES = {"layers": LAYERS, "ground": GROUND, "ground_occlusion": GROUND_OCCLUSION, "reflection": REFLECTION, "light": LIGHT, "bake": BAKE}

# the names these had before the table
LAYER_NAMES, LAYER_FORMATS, layer_names = LAYERS.names, LAYERS.formats, LAYERS.select
GROUND_NAMES, GROUND_FORMATS, ground_names = GROUND.names, {k: d for k, (d, _) in GROUND.formats.items()}, GROUND.select  # (a bare dtype per plane)
GROUND_OCCLUSION_NAMES, GROUND_OCCLUSION_FORMATS, ground_occlusion_names = (
    GROUND_OCCLUSION.names, {k: d for k, (d, _) in GROUND_OCCLUSION.formats.items()}, GROUND_OCCLUSION.select)  # (a bare dtype per plane)
REFLECTION_NAMES, REFLECTION_FORMATS, reflection_names = REFLECTION.names, REFLECTION.formats, REFLECTION.select
LIGHT_NAMES, LIGHT_FORMATS, light_names = LIGHT.names, LIGHT.formats, LIGHT.select
BAKE_NAMES, BAKE_FORMATS, bake_names = BAKE.names, BAKE.formats, BAKE.select


PAGE_COLOR = 0  # MCRT_PAGE_*: the page of a studio shot is Shot.pageColor
PAGE_REFERENCE = 1  # the reference's background (the config's gradient, or the scene's colour) at the pixel centre
PAGE_TRANSPARENT = 2  # no page: the shot as a straight-alpha cut-out (the ``_ex`` entries only)
PAGES = {"color": PAGE_COLOR, "reference": PAGE_REFERENCE}
PAGES_EX = {**PAGES, "transparent": PAGE_TRANSPARENT}


class McrtShot(C.Structure):
    """mcrt_shot: the settings of a studio shot's blend (include/mcrt.h)."""

    _fields_ = [("page", C.c_int32), ("page_color", C.c_float * 3), ("shadow_strength", C.c_float), ("reflectivity", C.c_float),
                ("reflection_fade", C.c_float)]


class McrtShotEx(C.Structure):
    """mcrt_shot_ex: mcrt_shot (whose page may be PAGE_TRANSPARENT), the floor-occlusion strength and the shadow's colour."""

    _fields_ = [("shot", McrtShot), ("floor_occlusion", C.c_float), ("shadow_color", C.c_float * 3)]


class McrtShotInputs(C.Structure):
    """mcrt_shot_inputs: the device planes mcrt_composite_shot_batch_device blends; all but the figure may be NULL."""

    _fields_ = [("figure", C.c_void_p), ("visibility", C.c_void_p), ("reflection", C.c_void_p), ("reflection_distance", C.c_void_p)]


@dataclass
class Shot:
    """mcrt_shot with mcrt_shot_init's defaults: the figure over the reference's background, a ground shadow of strength 0.6
    and a floor reflection of reflectivity 0.35 that does not fade.  ``page``: ``"reference"`` or ``"color"`` (then
    ``pageColor``); ``reflectionFade``: the reflection distance at which the mirror image has vanished, 0 = no fade;
    ``floorOcclusion``: the strength of the floor's contact occlusion (the ground-occlusion pass at the config's ``aoSamples`` /
    ``aoRadius``), 0 = none.  It is no field of mcrt_shot: the entries that take it (``*_occ``) take it as an argument.
    ``page="transparent"``: no page — the shot as a straight-alpha cut-out; ``shadowColor``: the colour of the shadow and of the
    floor occlusion, (0, 0, 0) = black.  Both travel in mcrt_shot_ex (``to_c_ex``), and ``shadowColor`` is carried like
    ``floorOcclusion``."""

    page: str = "reference"
    pageColor: Sequence[float] = (1.0, 1.0, 1.0)
    shadowStrength: float = 0.6
    reflectivity: float = 0.35
    reflectionFade: float = 0.0
    # the last parameter of the constructor and an attribute like the others, but no dataclass field: ``dataclasses.asdict`` and
    # ``fields`` — what describes mcrt_shot — stay as they were
    floorOcclusion: InitVar[float] = 0.0
    # ``shadowColor``: a keyword of the constructor (``_shot_init`` below) and an attribute, and nothing the dataclass knows of

    def __post_init__(self, floorOcclusion):
        self.floorOcclusion = float(floorOcclusion)
        self.shadowColor = (0.0, 0.0, 0.0)

    def __eq__(self, other):
        if other.__class__ is not self.__class__:
            return NotImplemented
        return (all(getattr(self, f.name) == getattr(other, f.name) for f in fields(self)) and self.floorOcclusion == other.floorOcclusion
                and self.shadowColor == other.shadowColor)

    def __repr__(self):
        body = ", ".join(f"{f.name}={getattr(self, f.name)!r}" for f in fields(self))
        if self.floorOcclusion != 0.0:
            body += f", floorOcclusion={self.floorOcclusion!r}"
        if self.shadowColor != (0.0, 0.0, 0.0):
            body += f", shadowColor={self.shadowColor!r}"
        return f"Shot({body})"

    def to_c(self) -> McrtShot:
        if self.page == "transparent":
            raise ValueError("page 'transparent' has no mcrt_shot: it travels in mcrt_shot_ex, see Shot.to_c_ex()")
        return self._base(PAGES)

    def to_c_ex(self) -> "McrtShotEx":
        """mcrt_shot_ex: every page, with ``floorOcclusion`` and ``shadowColor``."""
        s = McrtShotEx()
        s.shot = self._base(PAGES_EX)
        s.floor_occlusion = float(self.floorOcclusion)
        for i in range(3):
            s.shadow_color[i] = self.shadowColor[i]
        return s

    def needs_ex(self) -> bool:
        """Whether the shot needs the ``_ex`` entries by itself: a transparent page or a shadow colour other than 0."""
        return self.page == "transparent" or any(c != 0.0 for c in self.shadowColor)

    def _base(self, pages) -> McrtShot:
        if not isinstance(self.page, str) or self.page not in pages:
            raise ValueError(f"page must be {', '.join(repr(p) for p in pages)}, not {self.page!r}")
        s = McrtShot()
        s.page = pages[self.page]
        for i in range(3):
            s.page_color[i] = float(self.pageColor[i])
        s.shadow_strength = float(self.shadowStrength)
        s.reflectivity = float(self.reflectivity)
        s.reflection_fade = float(self.reflectionFade)
        return s


def _shot_init(self, *args, shadowColor=(0.0, 0.0, 0.0), **kw):
    _shot_fields_init(self, *args, **kw)
    self.shadowColor = tuple(float(c) for c in shadowColor)
    if len(self.shadowColor) != 3:
        raise ValueError(f"shadowColor must hold three channels, not {len(self.shadowColor)}")


_shot_fields_init = Shot.__init__
_shot_init.__doc__ = _shot_fields_init.__doc__
Shot.__init__ = _shot_init


MAX_EXTRA_LIGHTS = 3  # MCRT_MAX_EXTRA_LIGHTS: the lights a handle carries beside the scene's own


class McrtLightSource(C.Structure):
    """mcrt_light_source: one extra light (include/mcrt.h, "extra lights")."""

    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float), ("color", C.c_float * 4)]


assert C.sizeof(McrtLightSource) == 32


@dataclass
class Light:
    """An extra light — a fill or rim light beside the scene's own: the reference's Light{position, color, radius}.  A radius
    below 1e-4 is a point light.  Of ``color`` the first three channels count."""

    position: Sequence[float]
    color: Sequence[float] = (1.0, 1.0, 1.0, 1.0)
    radius: float = 3.0

    def to_c(self) -> McrtLightSource:
        if len(self.position) != 3 or len(self.color) not in (3, 4):
            raise ValueError("a Light takes a position of three coordinates and a colour of three or four channels")
        l = McrtLightSource()
        for i in range(3):
            l.position[i] = float(self.position[i])
        for i in range(4):
            l.color[i] = float(self.color[i]) if i < len(self.color) else 1.0
        l.radius = float(self.radius)
        return l


def light_array(lights):
    """(ctypes array or None, count) of a sequence of ``Light`` (None or empty: no extra lights) for the entries that take them."""
    lights = list(lights) if lights is not None else []
    if len(lights) > MAX_EXTRA_LIGHTS:
        raise ValueError(f"at most {MAX_EXTRA_LIGHTS} extra lights, not {len(lights)}")
    for l in lights:
        if not isinstance(l, Light):
            raise TypeError(f"extra lights are abi.Light values, not {type(l).__name__}")
    if not lights:
        return None, 0
    return (McrtLightSource * len(lights))(*[l.to_c() for l in lights]), len(lights)


MAX_LIGHTS = 1 + MAX_EXTRA_LIGHTS  # MCRT_MAX_LIGHTS: light 0 is the scene's own


class McrtLightPlanesMulti(C.Structure):
    """mcrt_light_planes_multi: a visibility and a direct plane per light, occlusion and the clamped sum; NULL = not wanted."""

    _fields_ = [("visibility", C.c_void_p * MAX_LIGHTS), ("direct", C.c_void_p * MAX_LIGHTS), ("occlusion", C.c_void_p), ("combined", C.c_void_p)]


class McrtBakePlanesMulti(C.Structure):
    """mcrt_bake_planes_multi: mcrt_bake_planes with a visibility and a direct plane per light, and the mean of the clamped sums."""

    _fields_ = [("position", C.c_void_p), ("normal", C.c_void_p), ("visibility", C.c_void_p * MAX_LIGHTS), ("occlusion", C.c_void_p),
                ("direct", C.c_void_p * MAX_LIGHTS), ("combined", C.c_void_p)]


assert C.sizeof(McrtLightPlanesMulti) == 8 * (2 * MAX_LIGHTS + 2) and C.sizeof(McrtBakePlanesMulti) == 8 * (2 * MAX_LIGHTS + 4)

# The planes of the passes under extra lights (include/mcrt.h, "light layers and bake under extra lights").  A structure member
# that holds a pointer per light is ONE name here: ``visibility`` is (M, ...) and ``direct`` (M, ..., 4) in the wrappers' results.
# They are rows beside FAMILIES, not in it: a PlaneFamily describes a structure of one pointer per name.
LIGHT_MULTI_FORMATS = {"visibility": (np.float32, 1), "direct": (np.float32, 4), "occlusion": (np.float32, 1), "combined": (np.float32, 4)}
BAKE_MULTI_FORMATS = {"position": (np.float32, 4), "normal": (np.float32, 4), "visibility": (np.float32, 1), "occlusion": (np.float32, 1),
                      "direct": (np.float32, 4), "combined": (np.float32, 4)}
LIGHT_MULTI_NAMES, BAKE_MULTI_NAMES = tuple(LIGHT_MULTI_FORMATS), tuple(BAKE_MULTI_FORMATS)
PER_LIGHT_NAMES = ("visibility", "direct")  # the members with a plane per light
MULTI_MISS = {"visibility": 1, "occlusion": 1}  # what a plane holds at a miss, for a dead texel and for a light the handle lacks; else 0


def multi_names(names: tuple, planes) -> tuple:
    """The wanted planes of LIGHT_MULTI_NAMES / BAKE_MULTI_NAMES in canonical order, as ``PlaneFamily.select`` words it."""
    if isinstance(planes, str):
        planes = (planes,)
    chosen = tuple(planes)
    for n in chosen:
        if not isinstance(n, str) or n not in names:
            raise ValueError(f"planes must be taken from {names}, not {n!r}")
    if not chosen:
        raise ValueError("no plane selected")
    return tuple(n for n in names if n in chosen)


def light_indices(lights_k) -> tuple:
    """The light indices k a per-light plane is asked for: None = all MAX_LIGHTS, else a sequence of 0 .. MAX_LIGHTS - 1, ascending."""
    if lights_k is None:
        return tuple(range(MAX_LIGHTS))
    ks = tuple(sorted({int(k) for k in lights_k}))
    if not ks or ks[0] < 0 or ks[-1] >= MAX_LIGHTS:
        raise ValueError(f"light indices must be taken from 0 .. {MAX_LIGHTS - 1}")
    return ks


PROGRESS_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)

SURFACE_DTYPE = np.dtype(
    [
        ("mesh", np.int32),
        ("face", np.int32),
        ("tx", np.int32),
        ("ty", np.int32),
        ("t", np.float32),
        ("point", np.float32, 3),
        ("normal", np.float32, 4),
        ("albedo", np.float32, 4),
    ]
)
assert SURFACE_DTYPE.itemsize == C.sizeof(McrtSurface) == 64

HIT_DTYPE = np.dtype(
    [
        ("hit", np.int32),
        ("t", np.float32),
        ("point", np.float32, 3),
        ("normal", np.float32, 3),
        ("texture_color", np.float32, 4),
        ("is_outer_layer", np.int32),
    ]
)
assert HIT_DTYPE.itemsize == C.sizeof(McrtHit)


# ------------------------------------------------------------------------------------------------
# Python-side value types mirroring the reference's data model (Scene/Mesh/Light/Camera/Config)
# ------------------------------------------------------------------------------------------------
@dataclass
class Config:
    """RayTracer::Config with the reference's in-class defaults (raytracer.h:10-38)."""

    width: int = 256
    height: int = 256
    maxBounces: int = 3
    samplesPerPixel: int = 1
    tileSize: int = 32
    threadCount: int = 0
    softShadows: bool = True
    shadowSamples: int = 8
    aoEnabled: bool = False
    aoSamples: int = 8
    aoRadius: float = 3.0
    aoIntensity: float = 0.5
    dofEnabled: bool = False
    aperture: float = 0.5
    focusDistance: float = 0.0
    gradientBg: bool = True
    gradientScale: float = 1.0
    bgCenter: Sequence[float] = (0.91, 0.89, 0.86, 1.0)
    bgEdge: Sequence[float] = (0.56, 0.63, 0.71, 1.0)

    def to_c(self) -> McrtConfig:
        c = McrtConfig()
        c.width, c.height = int(self.width), int(self.height)
        c.max_bounces = int(self.maxBounces)
        c.samples_per_pixel = int(self.samplesPerPixel)
        c.tile_size = int(self.tileSize)
        c.thread_count = int(self.threadCount)
        c.soft_shadows = int(bool(self.softShadows))
        c.shadow_samples = int(self.shadowSamples)
        c.ao_enabled = int(bool(self.aoEnabled))
        c.ao_samples = int(self.aoSamples)
        c.ao_radius = float(self.aoRadius)
        c.ao_intensity = float(self.aoIntensity)
        c.dof_enabled = int(bool(self.dofEnabled))
        c.aperture = float(self.aperture)
        c.focus_distance = float(self.focusDistance)
        c.gradient_bg = int(bool(self.gradientBg))
        c.gradient_scale = float(self.gradientScale)
        for i in range(4):
            c.bg_center[i] = float(self.bgCenter[i])
            c.bg_edge[i] = float(self.bgEdge[i])
        return c


@dataclass
class Texture:
    """TextureRegion (skin/texture_region.h:8-27). pixels: (n, 4) float32, row-major."""

    width: int
    height: int
    pixels: np.ndarray

    @staticmethod
    def solid(color: Sequence[float], w: int, h: int) -> "Texture":
        px = np.tile(np.asarray(color, dtype=np.float32).reshape(1, 4), (w * h, 1))
        return Texture(w, h, px)


@dataclass
class Mesh:
    """Mesh (scene/mesh.h:12-27) reduced to what the ray tracer reads."""

    triangles: np.ndarray  # (n, 9) float32  v0 v1 v2
    tri_texture: List[Optional[Texture]]  # per triangle; None = nullptr
    isOuterLayer: bool = False
    hasRotation: bool = False
    pivot: Sequence[float] = (0.0, 0.0, 0.0)
    rotX: float = 0.0
    rotZ: float = 0.0
    localTriangles: Optional[np.ndarray] = None  # (n, 9) float32


@dataclass
class Scene:
    """Scene/Light/Camera (scene/scene.h:10-34)."""

    meshes: List[Mesh] = field(default_factory=list)
    light_position: Sequence[float] = (0.0, 0.0, 0.0)
    light_color: Sequence[float] = (0.0, 0.0, 0.0, 1.0)  # Color() default
    light_intensity: float = 1.0
    light_radius: float = 3.0
    camera_position: Sequence[float] = (0.0, 0.0, 0.0)
    camera_target: Sequence[float] = (0.0, 0.0, 0.0)
    camera_up: Sequence[float] = (0.0, 0.0, 0.0)
    camera_fov: float = 60.0
    backgroundColor: Sequence[float] = (0.0, 0.0, 0.0, 1.0)


class SceneDescHolder:
    """Owns the numpy buffers behind a McrtSceneDesc built from a Python ``Scene``."""

    def __init__(self, scene: Scene):
        self._keep = []
        tex_index = {}
        textures: List[Texture] = []
        meshes_c = (McrtMesh * max(1, len(scene.meshes)))()
        for i, m in enumerate(scene.meshes):
            tri = np.ascontiguousarray(m.triangles, dtype=np.float32).reshape(-1, 9)
            loc = (
                np.ascontiguousarray(m.localTriangles, dtype=np.float32).reshape(-1, 9)
                if m.localTriangles is not None
                else np.zeros((0, 9), np.float32)
            )
            tix = np.full(len(tri), -1, dtype=np.int32)
            for t, tex in enumerate(m.tri_texture):
                if tex is None:
                    continue
                key = id(tex)
                if key not in tex_index:
                    tex_index[key] = len(textures)
                    textures.append(tex)
                tix[t] = tex_index[key]
            self._keep += [tri, loc, tix]
            mc = meshes_c[i]
            mc.n_triangles = len(tri)
            mc.tri_vertices = tri.ctypes.data_as(c_float_p)
            mc.tri_texture = tix.ctypes.data_as(c_int32_p)
            mc.n_local_triangles = len(loc)
            mc.local_tri_vertices = loc.ctypes.data_as(c_float_p)
            mc.is_outer_layer = int(bool(m.isOuterLayer))
            mc.has_rotation = int(bool(m.hasRotation))
            for k in range(3):
                mc.pivot[k] = float(m.pivot[k])
            mc.rot_x = float(m.rotX)
            mc.rot_z = float(m.rotZ)
        tex_c = (McrtTexture * max(1, len(textures)))()
        for i, t in enumerate(textures):
            px = np.ascontiguousarray(t.pixels, dtype=np.float32).reshape(-1, 4)
            self._keep.append(px)
            tex_c[i].width = int(t.width)
            tex_c[i].height = int(t.height)
            tex_c[i].n_pixels = len(px)
            tex_c[i].rgba = px.ctypes.data_as(c_float_p)
        d = McrtSceneDesc()
        d.n_meshes = len(scene.meshes)
        d.meshes = meshes_c
        d.n_textures = len(textures)
        d.textures = tex_c
        for k in range(3):
            d.light_position[k] = float(scene.light_position[k])
            d.camera_position[k] = float(scene.camera_position[k])
            d.camera_target[k] = float(scene.camera_target[k])
            d.camera_up[k] = float(scene.camera_up[k])
        for k in range(4):
            d.light_color[k] = float(scene.light_color[k])
            d.background_color[k] = float(scene.backgroundColor[k])
        d.light_intensity = float(scene.light_intensity)
        d.light_radius = float(scene.light_radius)
        d.camera_fov = float(scene.camera_fov)
        self._keep += [meshes_c, tex_c]
        self.desc = d

    @property
    def ptr(self):
        return C.byref(self.desc)


def desc_to_numpy(desc: McrtSceneDesc) -> dict:
    """Deep-copies a scene description into plain numpy/python data (for comparisons/fixtures)."""
    out = {"meshes": [], "textures": []}
    for i in range(desc.n_textures):
        t = desc.textures[i]
        n = int(t.n_pixels)
        px = np.ctypeslib.as_array(t.rgba, shape=(n * 4,)).copy().reshape(n, 4) if n > 0 else np.zeros((0, 4), np.float32)
        out["textures"].append({"width": int(t.width), "height": int(t.height), "pixels": px})
    for i in range(desc.n_meshes):
        m = desc.meshes[i]
        nt, nl = int(m.n_triangles), int(m.n_local_triangles)
        tri = np.ctypeslib.as_array(m.tri_vertices, shape=(nt * 9,)).copy().reshape(nt, 9) if nt else np.zeros((0, 9), np.float32)
        tix = np.ctypeslib.as_array(m.tri_texture, shape=(nt,)).copy() if nt else np.zeros((0,), np.int32)
        loc = np.ctypeslib.as_array(m.local_tri_vertices, shape=(nl * 9,)).copy().reshape(nl, 9) if nl else np.zeros((0, 9), np.float32)
        out["meshes"].append(
            {
                "triangles": tri,
                "tri_texture": tix,
                "localTriangles": loc,
                "isOuterLayer": int(m.is_outer_layer),
                "hasRotation": int(m.has_rotation),
                "pivot": np.array(list(m.pivot), np.float32),
                "rotX": np.float32(m.rot_x),
                "rotZ": np.float32(m.rot_z),
            }
        )
    for k in ("light_position", "light_color", "camera_position", "camera_target", "camera_up", "background_color"):
        out[k] = np.array(list(getattr(desc, k)), np.float32)
    for k in ("light_intensity", "light_radius", "camera_fov"):
        out[k] = np.float32(getattr(desc, k))
    return out


def scene_from_numpy(d: dict) -> Scene:
    """Inverse of desc_to_numpy → Python ``Scene`` (textures shared by index)."""
    texs = [Texture(int(t["width"]), int(t["height"]), np.asarray(t["pixels"], np.float32)) for t in d["textures"]]
    meshes = []
    for m in d["meshes"]:
        meshes.append(
            Mesh(
                triangles=np.asarray(m["triangles"], np.float32),
                tri_texture=[texs[i] if i >= 0 else None for i in np.asarray(m["tri_texture"]).tolist()],
                isOuterLayer=bool(m["isOuterLayer"]),
                hasRotation=bool(m["hasRotation"]),
                pivot=tuple(float(x) for x in m["pivot"]),
                rotX=float(m["rotX"]),
                rotZ=float(m["rotZ"]),
                localTriangles=np.asarray(m["localTriangles"], np.float32),
            )
        )
    return Scene(
        meshes=meshes,
        light_position=tuple(float(x) for x in d["light_position"]),
        light_color=tuple(float(x) for x in d["light_color"]),
        light_intensity=float(d["light_intensity"]),
        light_radius=float(d["light_radius"]),
        camera_position=tuple(float(x) for x in d["camera_position"]),
        camera_target=tuple(float(x) for x in d["camera_target"]),
        camera_up=tuple(float(x) for x in d["camera_up"]),
        camera_fov=float(d["camera_fov"]),
        backgroundColor=tuple(float(x) for x in d["background_color"]),
    )


def declare_common(lib, prefix: str) -> None:
    """Declares argtypes/restypes of the render/probe entry points that the product, the oracle and
    the compiled reference export under different prefixes."""
    desc_p = C.POINTER(McrtSceneDesc)
    cfg_p = C.POINTER(McrtConfig)

    def opt(name, restype, argtypes):
        fn = getattr(lib, prefix + name, None)
        if fn is not None:
            fn.restype = restype
            fn.argtypes = argtypes
        return fn

    opt("generate_tiles", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(McrtTile), C.c_int])
    opt("render_tile", C.c_int, [desc_p, cfg_p, C.POINTER(McrtTile), c_float_p])
    opt("intersect", C.c_int, [desc_p, c_float_p, C.c_int, C.c_void_p])
    opt("intersect_mesh", C.c_int, [desc_p, C.c_int, c_float_p, C.c_int, C.c_void_p])
    opt("trace", C.c_int, [desc_p, cfg_p, c_float_p, C.c_int, C.c_int, C.c_int, c_float_p])
    opt("shade", C.c_int, [desc_p, C.POINTER(McrtHit), c_float_p, c_float_p, C.c_float, c_float_p])
    opt("in_shadow", C.c_int, [desc_p, c_float_p, c_float_p, c_float_p])
    opt("soft_shadow", C.c_float, [desc_p, c_float_p, c_float_p, C.c_int, C.c_uint32])
    opt("ao", C.c_float, [desc_p, c_float_p, c_float_p, C.c_int, C.c_float, C.c_uint32])
    opt("background", None, [desc_p, cfg_p, C.c_float, C.c_float, c_float_p])
    opt("camera_ray", None, [desc_p, C.c_float, C.c_float, C.c_float, c_float_p])
    opt("mt_uniform", None, [C.c_uint32, C.c_int, c_float_p])
    opt("mt_uniform_std", None, [C.c_uint32, C.c_int, c_float_p])
    opt("seed_cast", C.c_uint32, [C.c_float])
    opt("quantize", None, [c_float_p, C.POINTER(C.c_uint8), C.c_size_t])
    opt("build_skin_scene", C.c_int, [C.POINTER(C.c_uint8), C.c_int, C.c_int, c_float_p, C.POINTER(desc_p)])
    opt("build_default_scene", C.c_int, [c_float_p, C.POINTER(desc_p)])
    opt("builtin_pose", C.c_int, [C.c_int, c_float_p])
    opt("scene_desc_free", None, [desc_p])


def fptr(a: np.ndarray):
    return a.ctypes.data_as(c_float_p)
