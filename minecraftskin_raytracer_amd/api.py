"""Host-side mirror of the reference's interface for the render hot path.

Names follow the reference (``TileRenderer.render/generateTiles/lastErrors``, ``Config`` =
``RayTracer::Config``, ``MeshBuilder.buildScene/buildDefaultScene``), argument meaning and error
behaviour too; every render goes through the C ABI of ``libmcrt.so`` into the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from ._lib import McrtError, check, load
from .abi import Config, Mesh, Scene, SceneDescHolder, Texture

Image = np.ndarray  # (H, W, 4) float32 — skin/image.h:9-15


def trim() -> None:
    """Free the device workspace kept for reuse by destroyed scenes (mcrt_trim)."""
    load().mcrt_trim()


def device_count() -> int:
    return int(load().mcrt_device_count())


class _OwnedDescPtr(C.POINTER(abi.McrtSceneDesc)):
    """A ``POINTER(McrtSceneDesc)`` that keeps the object owning the pointed-to arrays alive: a ``.ptr`` taken
    from a temporary (``skin_scene(...).ptr``) stays valid for as long as the pointer itself is referenced."""

    _type_ = abi.McrtSceneDesc


class SceneDesc:
    """A scene description the library can consume: either built from a Python ``Scene`` or owned by
    the native scene builder.  ``.ptr`` is a ``POINTER(McrtSceneDesc)``-compatible object that holds a
    reference to this description."""

    def __init__(self, scene: Optional[Scene] = None, _native=None):
        self._holder = SceneDescHolder(scene) if scene is not None else None
        self._native = _native

    @property
    def ptr(self):
        raw = self._native if self._native is not None else C.pointer(self._holder.desc)
        p = C.cast(raw, _OwnedDescPtr)
        p._owner = self  # the description (and through it the arrays) lives as long as the pointer
        return p

    @property
    def desc(self) -> abi.McrtSceneDesc:
        return self._native.contents if self._native is not None else self._holder.desc

    def to_numpy(self) -> dict:
        return abi.desc_to_numpy(self.desc)

    def __del__(self):
        if getattr(self, "_native", None) is not None:
            try:
                load().mcrt_scene_desc_free(self._native)
            except Exception:
                pass
            self._native = None


def _as_desc(scene) -> SceneDesc:
    if isinstance(scene, SceneDesc):
        return scene
    if isinstance(scene, Scene):
        return SceneDesc(scene)
    raise TypeError("scene must be a Scene or SceneDesc")


class MeshBuilder:
    """scene/mesh_builder.h:7-34 (scene construction from skin data; native implementation)."""

    @staticmethod
    def buildScene(skin_rgba8: np.ndarray, pose: Optional[Sequence[float]] = None, model: str = "classic", cape: Optional[np.ndarray] = None,
                   cape_angle: float = 10.0) -> SceneDesc:
        """SkinParser::parse (64x64 / 64x32 RGBA8) + MeshBuilder::buildScene.  ``model``: ``"classic"`` (the reference's figure),
        ``"slim"`` (arms 3 texels wide, 64x64 skins only) or ``"auto"`` (``skin_model`` of the image).  ``cape``: a cape image,
        (32, 64, 4) uint8, hung on the figure's back as its last mesh at ``cape_angle`` degrees (0 .. 90) from the body
        (mcrt_build_skin_scene_cape); ``None``: no cape, the call as it always was."""
        skin = np.ascontiguousarray(skin_rgba8, np.uint8)
        if skin.ndim != 3 or skin.shape[2] != 4:
            raise ValueError("skin must be (H, W, 4) uint8")
        h, w = skin.shape[:2]
        if model == "auto" and w == 64 and h in (64, 32):
            model = skin_model(skin)
        if model not in ("classic", "slim", "auto"):
            raise ValueError("model must be 'classic', 'slim' or 'auto'")
        if model == "slim" and h != 64:
            raise ValueError("the slim model exists for 64x64 skins only")
        p = np.asarray(pose if pose is not None else [0.0] * 12, np.float32)
        out = C.POINTER(abi.McrtSceneDesc)()
        if cape is not None:
            c = _cape_image(cape)
            if w != 64 or h not in (64, 32):
                raise ValueError(f"Invalid skin dimensions: {w}x{h} (expected 64x64 or 64x32)")
            check(load().mcrt_build_skin_scene_cape(skin.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, abi.SKIN_SLIM if model == "slim" else abi.SKIN_CLASSIC,
                                                    abi.fptr(p), c.ctypes.data_as(C.POINTER(C.c_uint8)), float(cape_angle), C.byref(out)))
            return SceneDesc(_native=out)
        if model == "slim":
            rc = load().mcrt_build_skin_scene_model(skin.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, abi.SKIN_SLIM, abi.fptr(p), C.byref(out))
        else:
            rc = load().mcrt_build_skin_scene(skin.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, abi.fptr(p), C.byref(out))
        if rc != 0:
            # skin_parser.cpp:122-131: only 64x64 and 64x32 are valid
            raise ValueError(f"Invalid skin dimensions: {w}x{h} (expected 64x64 or 64x32)")
        return SceneDesc(_native=out)

    @staticmethod
    def buildDefaultScene(pose: Optional[Sequence[float]] = None) -> SceneDesc:
        p = np.asarray(pose if pose is not None else [0.0] * 12, np.float32)
        out = C.POINTER(abi.McrtSceneDesc)()
        check(load().mcrt_build_default_scene(abi.fptr(p), C.byref(out)))
        return SceneDesc(_native=out)


CAPE_SHAPE = (32, 64, 4)
CAPE_TEXELS = 372


def _cape_image(cape) -> np.ndarray:
    a = np.ascontiguousarray(cape, np.uint8)
    if a.shape != CAPE_SHAPE:
        raise ValueError("a cape image is (32, 64, 4) uint8: 64x32 RGBA8")
    return a


def getBuiltinPoses() -> List[np.ndarray]:
    """scene/pose.h:25-92 → 7 poses x 12 floats ({head, body, rArm, lArm, rLeg, lLeg} x {rotX, rotZ})."""
    out = []
    for i in range(7):
        p = np.zeros(12, np.float32)
        check(load().mcrt_builtin_pose(i, abi.fptr(p)))
        out.append(p)
    return out


def _devices(device):
    """``device`` argument of the render entry points → (one index, None) or (None, list of indices; [] = every visible
    device).  Accepts any integer type (numpy, torch device indices), ``"all"`` / ``-1``, or a sequence of indices."""
    import operator

    if isinstance(device, str):
        if device != "all":
            raise ValueError("device must be an index, 'all' or a sequence of indices")
        return None, []
    try:
        d = operator.index(device)
    except TypeError:
        devs = [operator.index(x) for x in device]
        if any(x < 0 for x in devs):
            raise ValueError("device indices must be >= 0")
        return None, devs
    if d == -1:
        return None, []
    if d < 0:
        raise ValueError("device must be >= 0, or -1 / 'all' for every visible device")
    return d, None


def _frame(config: Config) -> Tuple[int, int, bool]:
    """(width, height) with negatives as 0, and whether the frame holds no tile: then a call writes nothing."""
    w, h = max(config.width, 0), max(config.height, 0)
    return w, h, w == 0 or h == 0 or config.tileSize <= 0


def _default_frames(n: int, h: int, w: int, rgba8: bool) -> np.ndarray:
    """n frames of Image(w, h)'s default Color() = (0, 0, 0, 1): (n, h, w, 4) float32, or uint8 (0, 0, 0, 255) with ``rgba8``."""
    out = np.zeros((n, h, w, 4), np.uint8 if rgba8 else np.float32)
    out[..., 3] = 255 if rgba8 else 1.0
    return out


def _desc_array(descs):
    return (C.POINTER(abi.McrtSceneDesc) * max(len(descs), 1))(*[d.ptr for d in descs])


class TileRenderer:
    """raytracer/tile_renderer.h:16-47."""

    _errors: List[Tuple[int, str]] = []

    @staticmethod
    def generateTiles(imageWidth: int, imageHeight: int, tileSize: int) -> List[Tuple[int, int, int, int]]:
        lib = load()
        n = lib.mcrt_generate_tiles(imageWidth, imageHeight, tileSize, None, 0)
        arr = (abi.McrtTile * max(n, 1))()
        lib.mcrt_generate_tiles(imageWidth, imageHeight, tileSize, arr, n)
        return [(arr[i].x, arr[i].y, arr[i].width, arr[i].height) for i in range(n)]

    @staticmethod
    def render(scene, config: Config, progressCallback: Optional[Callable[[int, int], None]] = None,
               device=0, gather: bool = False, out: Optional[np.ndarray] = None, background: str = "reference", lights=None) -> Image:
        """TileRenderer::render.  Per-frame failures never raise (tile_renderer.cpp:158-166): they are
        recorded as one ``(-1, message)`` entry in ``lastErrors()`` and the image keeps Color() =
        (0,0,0,1) pixels.

        ``device``: an index, ``"all"`` / ``-1`` (every visible device) or a sequence of indices — one rank per
        entry, cyclic tile rows (mcrt_render_multi; ``gather`` selects the peer-copy assembly on the first
        device instead of per-device downloads).  ``out``: a (H, W, 4) float32 C-contiguous array to render
        into (the reference returns a fresh Image per call; a caller that renders repeatedly can keep one).
        ``background``: ``"reference"`` (the default) or ``"transparent"`` — the figure alone, straight alpha, pixels
        without a hit (0,0,0,0) (MCRT_BACKGROUND_TRANSPARENT, include/mcrt.h).  ``lights``: up to three ``abi.Light`` — fill
        and rim lights beside the scene's own (include/mcrt.h, "extra lights")."""
        mode = abi.background_mode(background)
        extra, n_extra = abi.light_array(lights)
        lib = load()
        d = _as_desc(scene)
        c = config.to_c()
        w, h, no_frame = _frame(config)
        if out is None:
            out = _default_frames(1, h, w, False)[0]
        elif out.shape != (h, w, 4) or out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a C-contiguous (height, width, 4) float32 array")
        TileRenderer._errors = []
        if no_frame:
            return out
        cb = abi.PROGRESS_FN((lambda done, total, _u: progressCallback(done, total))) if progressCallback else C.cast(None, abi.PROGRESS_FN)
        one, devs = _devices(device)
        if n_extra:
            if one is not None:
                devs = [one]
            arr = (C.c_int * max(len(devs), 1))(*devs)
            rc = lib.mcrt_render_lights(d.ptr, C.byref(c), extra, n_extra, mode, abi.fptr(out), None, cb, None, arr if devs else None, len(devs),
                                        1 if gather else 0)
        elif mode != abi.BACKGROUND_REFERENCE:
            if one is not None:
                devs = [one]
            arr = (C.c_int * max(len(devs), 1))(*devs)
            rc = lib.mcrt_render_ex(d.ptr, C.byref(c), mode, abi.fptr(out), None, cb, None, arr if devs else None, len(devs), 1 if gather else 0)
        elif one is not None:
            rc = lib.mcrt_render(d.ptr, C.byref(c), abi.fptr(out), cb, None, one)
        else:
            arr = (C.c_int * max(len(devs), 1))(*devs)
            rc = lib.mcrt_render_multi(d.ptr, C.byref(c), abi.fptr(out), cb, None, arr if devs else None, len(devs), 1 if gather else 0)
        if rc != 0:
            TileRenderer._errors = [(-1, lib.mcrt_last_error().decode("utf-8", "replace"))]
            out[...] = 0.0
            out[..., 3] = 1.0
        return out

    @staticmethod
    def renderTile(tile: Tuple[int, int, int, int], scene, config: Config, output: np.ndarray, device: int = 0) -> None:
        """TileRenderer::renderTile (tile_renderer.cpp:71-127): one Tile ``(x, y, width, height)`` — any rectangle of the
        frame, its own mt19937(y * width + x) — into ``output`` ((H, W, 4) float32), every other pixel untouched.
        Failures are recorded in ``lastErrors()``."""
        if output.shape != (config.height, config.width, 4) or output.dtype != np.float32 or not output.flags["C_CONTIGUOUS"]:
            raise ValueError("output must be a C-contiguous (height, width, 4) float32 array")
        c = config.to_c()
        t = abi.McrtTile(*[int(v) for v in tile])
        lib = load()
        if lib.mcrt_render_rect(_as_desc(scene).ptr, C.byref(c), C.byref(t), abi.fptr(output), int(device)) != 0:
            TileRenderer._errors.append((-1, lib.mcrt_last_error().decode("utf-8", "replace")))

    @staticmethod
    def renderRGBA8(scene, config: Config, device=0, gather: bool = False, background: str = "reference", lights=None) -> np.ndarray:
        """The frame as the RGBA8 plane ImageWriter::writePNG would encode ((H, W, 4) uint8), quantised in the kernels'
        epilogue: 4 B per pixel over PCIe / xGMI instead of 16 (mcrt_render_rgba8).  ``device``, ``background`` and ``lights``
        as for ``render``."""
        mode = abi.background_mode(background)
        extra, n_extra = abi.light_array(lights)
        lib = load()
        c = config.to_c()
        w, h, no_frame = _frame(config)
        out = _default_frames(1, h, w, True)[0]
        TileRenderer._errors = []
        if no_frame:
            return out
        one, devs = _devices(device)
        if one is not None:
            devs = [one]
        arr = (C.c_int * max(len(devs), 1))(*devs)
        if n_extra:
            rc = lib.mcrt_render_lights(_as_desc(scene).ptr, C.byref(c), extra, n_extra, mode, None, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        C.cast(None, abi.PROGRESS_FN), None, arr if devs else None, len(devs), 1 if gather else 0)
        elif mode != abi.BACKGROUND_REFERENCE:
            rc = lib.mcrt_render_ex(_as_desc(scene).ptr, C.byref(c), mode, None, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    C.cast(None, abi.PROGRESS_FN), None, arr if devs else None, len(devs), 1 if gather else 0)
        else:
            rc = lib.mcrt_render_rgba8(_as_desc(scene).ptr, C.byref(c), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(None, abi.PROGRESS_FN), None,
                                       arr if devs else None, len(devs), 1 if gather else 0)
        if rc != 0:
            TileRenderer._errors = [(-1, lib.mcrt_last_error().decode("utf-8", "replace"))]
            out[...] = 0
            out[..., 3] = 255
        return out

    @staticmethod
    def renderBatch(scenes, config: Config, device: int = 0, rgba8: bool = False, background: str = "reference") -> np.ndarray:
        """N frames of one config in one call (mcrt_render_batch): frame i equals ``render(scenes[i], config)`` bit for bit
        (or ``renderRGBA8`` with ``rgba8``).  Returns (N, H, W, 4) float32, or uint8 with ``rgba8``.  Small frames go
        through batched kernels, one launch sequence for the whole batch; ``lastBatchInfo()`` tells how it ran.
        ``background`` as for ``render``, for every frame.  Unlike ``render``, failures raise ``McrtError``."""
        mode = abi.background_mode(background)
        descs = [_as_desc(s) for s in scenes]
        n = len(descs)
        w, h, _ = _frame(config)
        out = _default_frames(n, h, w, rgba8)
        c = config.to_c()
        arr = _desc_array(descs)
        f = None if rgba8 else abi.fptr(out)
        b = out.ctypes.data_as(C.POINTER(C.c_uint8)) if rgba8 else None
        if mode != abi.BACKGROUND_REFERENCE:
            check(load().mcrt_render_batch_ex(arr, n, C.byref(c), mode, f, b, int(device)))
        else:
            check(load().mcrt_render_batch(arr, n, C.byref(c), f, b, int(device)))
        return out

    @staticmethod
    def renderLayers(scene, config: Config, layers=abi.LAYER_NAMES, device: int = 0) -> dict:
        """What is under each pixel (mcrt_render_layers): a dict of the wanted planes — ``depth`` (H, W) float32 (FLT_MAX at a
        miss), ``normal`` and ``albedo`` (H, W, 4) float32, ``id`` (H, W, 4) int32 ``{mesh, face, tx, ty}`` (``{-1, 0, -1, -1}``
        at a miss; ``face & 7`` the face slot, ``abi.ID_BACK`` / ``abi.ID_OUTER`` flags).  One pixel-centre ray per pixel, no
        shading: of ``config`` only width, height and tileSize matter.  Failures raise ``McrtError``."""
        out = TileRenderer.renderLayersBatch([scene], config, layers, device)
        return {k: v[0] for k, v in out.items()}

    @staticmethod
    def renderLayersBatch(scenes, config: Config, layers=abi.LAYER_NAMES, device: int = 0) -> dict:
        """``renderLayers`` for N scenes of one config in one launch (mcrt_render_layers_batch): the same planes with a leading
        N."""
        names = abi.LAYERS.select(layers)
        descs = [_as_desc(s) for s in scenes]
        n = len(descs)
        w, h, no_frame = _frame(config)
        out = {k: abi.LAYERS.empty(k, n, h, w) for k in names}
        if n == 0 or no_frame:
            return out
        c = config.to_c()
        planes = abi.McrtLayers(**{k: v.ctypes.data for k, v in out.items()})
        check(load().mcrt_render_layers_batch(_desc_array(descs), n, C.byref(c), C.byref(planes), int(device)))
        return out

    @staticmethod
    def renderGround(scene, config: Config, ground: Optional[float] = None, planes=abi.GROUND_NAMES, device: int = 0) -> dict:
        """The figure's soft shadow on the floor plane y = ``ground`` (mcrt_render_ground; ``None``: the scene's floor,
        ``scene_floor`` — the lowest vertex, which for a 64x64 skin is the outer leg layer, 0.5 below the soles): a dict of the wanted planes, (H, W) each — ``visibility`` float32, the share of the light's samples
        that reach the plane's point under the pixel (1 where the pixel's ray misses the plane), ``distance`` float32, the ray
        parameter of that point (FLT_MAX at a miss), ``matte`` uint8, the quantised ``1 - visibility``: the alpha of a black
        shadow image to put under the transparent figure.  Of ``config`` only width, height, tileSize, softShadows and
        shadowSamples (at most 113 with softShadows) matter.  Failures raise ``McrtError``."""
        out = TileRenderer.renderGroundBatch([scene], config, ground, planes, device)
        return {k: v[0] for k, v in out.items()}

    @staticmethod
    def renderGroundBatch(scenes, config: Config, ground=None, planes=abi.GROUND_NAMES, device: int = 0) -> dict:
        """``renderGround`` for N scenes of one config: the same planes with a leading N.  ``ground``: ``None`` (every scene's
        own floor), one height for all, or a sequence of N heights.  This host form is a LOOP of ``mcrt_render_ground`` calls —
        each uploads its scene, launches, downloads and synchronises — and gains nothing from the batched kernel; the batched
        path is ``render_ground_batch_device`` on resident ``DeviceScene`` handles (one launch per 4096 frames)."""
        return _render_pass_loop(abi.GROUND, scenes, config, planes, device, ground)

    @staticmethod
    def renderGroundOcclusion(scene, config: Config, ground: Optional[float] = None, planes=abi.GROUND_OCCLUSION_NAMES, device: int = 0) -> dict:
        """The figure's contact occlusion on the floor plane y = ``ground`` (mcrt_render_ground_occlusion; ``None``: the scene's
        floor, ``scene_floor``): a dict of the wanted planes, (H, W) each — ``occlusion`` float32, the reference's ambient
        occlusion at the plane's point under the pixel (1 where nothing is near, and where the pixel's ray misses the plane),
        ``matte`` uint8, the quantised ``1 - occlusion``: the alpha of a black contact-shadow image to put under the transparent
        figure.  Of ``config`` only width, height, tileSize, aoSamples (1 to 113) and aoRadius matter — not aoEnabled.  Failures
        raise ``McrtError``."""
        out = TileRenderer.renderGroundOcclusionBatch([scene], config, ground, planes, device)
        return {k: v[0] for k, v in out.items()}

    @staticmethod
    def renderGroundOcclusionBatch(scenes, config: Config, ground=None, planes=abi.GROUND_OCCLUSION_NAMES, device: int = 0) -> dict:
        """``renderGroundOcclusion`` for N scenes of one config: the same planes with a leading N.  ``ground``: ``None`` (every
        scene's own floor), one height for all, or a sequence of N heights.  This host form is a LOOP of
        ``mcrt_render_ground_occlusion`` calls, like ``renderGroundBatch``; the batched path is
        ``render_ground_occlusion_batch_device`` on resident ``DeviceScene`` handles (one launch per 4096 frames)."""
        return _render_pass_loop(abi.GROUND_OCCLUSION, scenes, config, planes, device, ground)

    @staticmethod
    def renderReflection(scene, config: Config, ground: Optional[float] = None, planes=abi.REFLECTION_NAMES, device: int = 0) -> dict:
        """The figure mirrored in the floor plane y = ``ground`` (mcrt_render_reflection; ``None``: the scene's floor,
        ``scene_floor``): a dict of the wanted planes — ``rgba`` (H, W, 4) float32, the colour the reference's recursion returns
        for the floor's reflection ray, straight alpha, zero where nothing is mirrored; ``rgba8`` (H, W, 4) uint8, the same
        quantised; ``distance`` (H, W) float32, the reflection ray's hit distance (FLT_MAX without a hit).  Of ``config`` only
        width, height, tileSize, maxBounces (at most 8), softShadows and shadowSamples (at most 113 with softShadows) matter.
        Failures raise ``McrtError``."""
        out = TileRenderer.renderReflectionBatch([scene], config, ground, planes, device)
        return {k: v[0] for k, v in out.items()}

    @staticmethod
    def renderReflectionBatch(scenes, config: Config, ground=None, planes=abi.REFLECTION_NAMES, device: int = 0) -> dict:
        """``renderReflection`` for N scenes of one config: the same planes with a leading N.  ``ground``: ``None`` (every
        scene's own floor), one height for all, or a sequence of N heights.  This host form is a LOOP of
        ``mcrt_render_reflection`` calls; the batched path is ``render_reflection_batch_device`` on resident ``DeviceScene``
        handles (one launch per 4096 frames)."""
        return _render_pass_loop(abi.REFLECTION, scenes, config, planes, device, ground)

    @staticmethod
    def renderShot(scene, config: Config, shot: Optional[abi.Shot] = None, ground: Optional[float] = None, rgba8: bool = True,
                   device: int = 0, bounds: bool = False):
        """The studio shot (mcrt_render_shot): the figure on a page, with its ground shadow and its floor reflection at
        y = ``ground`` (``None``: the scene's floor, ``scene_floor``), blended on the device — (H, W, 4) uint8, or float32 with
        ``rgba8=False``; alpha is 255 / 1.0 everywhere.  ``shot``: ``abi.Shot`` (``None``: its defaults).  The figure is the
        ``background="transparent"`` render of ``config``; the definition of the blend is in include/mcrt.h.  With
        ``shot.floorOcclusion`` > 0 the floor's contact occlusion (``renderGroundOcclusion`` at the config's aoSamples /
        aoRadius) darkens the page too.  ``Shot(page="transparent")``: the shot as a straight-alpha cut-out, and with
        ``bounds=True`` the pair (image, (4,) int32 {x0, y0, x1, y1}): the box of the pixels with alpha > 0.  Failures raise
        ``McrtError``."""
        got = TileRenderer.renderShotBatch([scene], config, shot, ground, rgba8, device, bounds)
        return (got[0][0], got[1][0]) if bounds else got[0]

    @staticmethod
    def renderShotBatch(scenes, config: Config, shot: Optional[abi.Shot] = None, ground=None, rgba8: bool = True, device: int = 0,
                        bounds: bool = False):
        """``renderShot`` for N scenes of one config in one call (mcrt_render_shot_batch): one batched render, one ground and
        one reflection launch, one blend, one download.  ``ground``: ``None`` (every scene's own floor), one height for all, or
        N heights.  Returns (N, H, W, 4) uint8, or float32 with ``rgba8=False``; with ``bounds=True`` (transparent page only)
        the pair (images, (N, 4) int32 boxes) through mcrt_render_shot_batch_ex."""
        variant, shot_args = _shot_variant(shot, bounds)
        descs = [_as_desc(d) for d in scenes]
        n = len(descs)
        heights = _ground_heights(descs, ground)
        w, h, _ = _frame(config)
        out = _default_frames(n, h, w, rgba8)
        c = config.to_c()
        buf = out if out.size else np.zeros(4, out.dtype)  # (no frame: the call checks its arguments and writes nothing)
        f = None if rgba8 else abi.fptr(buf)
        b = buf.ctypes.data_as(C.POINTER(C.c_uint8)) if rgba8 else None
        boxes = _empty_bounds(max(n, 1), w, h)
        ex_args = (C.c_void_p(boxes.ctypes.data if bounds else None),) if variant == "_ex" else ()
        check(getattr(load(), "mcrt_render_shot_batch" + variant)(_desc_array(descs), n, C.byref(c), *shot_args, _height_array(heights), f, b, *ex_args,
                                                                  int(device)))
        return (out, boxes[:n]) if bounds else out

    @staticmethod
    def renderLight(scene, config: Config, planes=abi.LIGHT_NAMES, device: int = 0) -> dict:
        """What the light does on the figure itself (mcrt_render_light), at the primary hit of each pixel-centre ray: a dict of
        the wanted planes — ``visibility`` (H, W) float32, the share of the disk light that reaches the surface (1 at a miss);
        ``occlusion`` (H, W) float32, ``1 - occluded / aoSamples`` whatever ``aoEnabled`` says (1 at a miss); ``direct``
        (H, W, 4) float32, ``shade()`` with that visibility before ambient occlusion and bounces, alpha the texel's (zero at a
        miss).  The beauty frame at 1 spp, 0 bounces is ``direct`` without AO and ``clip(direct.rgb * (1 - aoIntensity *
        (1 - occlusion)), 0, 1)`` with it, bit for bit.  Of ``config`` only width, height, tileSize, softShadows, shadowSamples
        (at most 113 with softShadows), aoSamples (1 to 113) and aoRadius matter.  Failures raise ``McrtError``."""
        out = TileRenderer.renderLightBatch([scene], config, planes, device)
        return {k: v[0] for k, v in out.items()}

    @staticmethod
    def renderLightBatch(scenes, config: Config, planes=abi.LIGHT_NAMES, device: int = 0) -> dict:
        """``renderLight`` for N scenes of one config: the same planes with a leading N.  This host form is a LOOP of
        ``mcrt_render_light`` calls; the batched path is ``render_light_batch_device`` on resident ``DeviceScene`` handles (one
        launch per kernel and 4096 frames)."""
        return _render_pass_loop(abi.LIGHT, scenes, config, planes, device)

    @staticmethod
    def bakeLight(scene, config: Config, grid: int = 1, planes=abi.BAKE_NAMES, device: int = 0) -> dict:
        """The light terms in TEXTURE space (mcrt_bake_light): one value per texel of the scene's texel pool, in pool order —
        ``texel_table(scene)`` names each texel's owner face.  A dict of the wanted planes, n = the pool's size: ``position``
        (n, 4) float32, the texel centre on its face with w = 1 (w = 0 for a dead texel: one without an owner or with alpha 0);
        ``normal`` (n, 4), the face's outward normal; ``visibility`` (n,) and ``occlusion`` (n,), the means of computeSoftShadow
        (or shade()'s own shadow test) and computeAO over ``grid`` x ``grid`` sub-samples of the texel (1 for a dead texel);
        ``direct`` (n, 4), the mean of ``shade()`` with the view vector along the normal, alpha the texel's (zero for a dead
        texel).  Of ``config`` only softShadows, shadowSamples (at most 113 with softShadows), aoSamples (1 to 113) and aoRadius
        matter.  Failures raise ``McrtError``."""
        names = abi.BAKE.select(planes)
        grid = _bake_grid(grid)
        d = _as_desc(scene)
        n = len(texel_table(d))
        out = {k: abi.BAKE.empty(k, n) for k in names}
        if n == 0:
            return out
        c = config.to_c()
        frame = abi.McrtBakePlanes(**{k: v.ctypes.data for k, v in out.items()})
        check(load().mcrt_bake_light(d.ptr, C.byref(c), grid, C.byref(frame), int(device)))
        return out

    @staticmethod
    def renderLightMulti(scene, config: Config, lights=(), planes=abi.LIGHT_MULTI_NAMES, light_indices=None, device: int = 0) -> dict:
        """``renderLight`` with planes PER LIGHT, under 0 to 3 extra ``lights`` (``abi.Light``) beside the scene's own
        (mcrt_render_light_multi): what a compositor needs to dim, recolour or switch off one light.  A dict of the wanted planes:
        ``visibility`` (M, H, W) and ``direct`` (M, H, W, 4), row k for light k — 0 the scene's own, 1.. the extra lights in
        order; a light that is not there is a black light: 1 / zeros — restricted to ``light_indices`` where given (then M is
        their number, ascending); ``occlusion`` (H, W); ``combined`` (H, W, 4) = ``clip(direct[0] + direct[1] + ..., 0, 1)`` with
        ``direct[0]``'s alpha, which is the beauty frame under the same lights at 1 spp, 0 bounces on every hit pixel (with AO:
        ``clip(combined.rgb * (1 - aoIntensity * (1 - occlusion)), 0, 1)``), bit for bit."""
        names = abi.multi_names(abi.LIGHT_MULTI_NAMES, planes)
        ks = abi.light_indices(light_indices)
        extra, n_extra = abi.light_array(lights)
        h, w = max(int(config.height), 0), max(int(config.width), 0)
        out = _multi_empty(abi.LIGHT_MULTI_FORMATS, names, len(ks), (h, w))
        if h == 0 or w == 0 or config.tileSize <= 0:
            return out
        frame = _multi_host_planes(abi.McrtLightPlanesMulti, out, ks)
        c = config.to_c()
        check(load().mcrt_render_light_multi(_as_desc(scene).ptr, C.byref(c), extra, n_extra, C.byref(frame), int(device)))
        return out

    @staticmethod
    def bakeLightMulti(scene, config: Config, grid: int = 1, lights=(), planes=abi.BAKE_MULTI_NAMES, light_indices=None, device: int = 0) -> dict:
        """``bakeLight`` with planes PER LIGHT, under 0 to 3 extra ``lights`` (mcrt_bake_light_multi): ``visibility`` (M, n) and
        ``direct`` (M, n, 4) as ``renderLightMulti`` lays them out, ``position``, ``normal`` and ``occlusion`` as ``bakeLight``
        gives them, and ``combined`` (n, 4): the mean over the sub-samples of the clamped sum of the lights' terms (not the clamp
        of the means)."""
        names = abi.multi_names(abi.BAKE_MULTI_NAMES, planes)
        ks = abi.light_indices(light_indices)
        extra, n_extra = abi.light_array(lights)
        grid = _bake_grid(grid)
        d = _as_desc(scene)
        n = len(texel_table(d))
        out = _multi_empty(abi.BAKE_MULTI_FORMATS, names, len(ks), (n,))
        if n == 0:
            return out
        frame = _multi_host_planes(abi.McrtBakePlanesMulti, out, ks)
        c = config.to_c()
        check(load().mcrt_bake_light_multi(d.ptr, C.byref(c), extra, n_extra, grid, C.byref(frame), int(device)))
        return out

    @staticmethod
    def lastBatchInfo() -> dict:
        """How the last batch call on this thread ran (mcrt_last_batch_info): ``batched_frames`` taken by the batched
        kernels and ``launch_sequences`` enqueued (1 when the whole batch went through them at once)."""
        return last_batch_info()

    @staticmethod
    def lastErrors() -> List[Tuple[int, str]]:
        return list(TileRenderer._errors)

    @staticmethod
    def lastTimings() -> dict:
        t = abi.McrtTimings()
        load().mcrt_last_timings(C.byref(t))
        return {k: getattr(t, k) for k, _ in abi.McrtTimings._fields_}


def _render_pass_loop(family: abi.PlaneFamily, scenes, config: Config, planes, device, *ground) -> dict:
    """The host form of a pass for N scenes: a loop of calls of the family's one-shot entry, frame i into row i of the wanted
    planes.  ``ground``: the heights argument of a pass that has a floor plane, nothing for one that has none."""
    names = family.select(planes)
    descs = [_as_desc(s) for s in scenes]
    n = len(descs)
    heights = [_ground_heights(descs, g) for g in ground]
    w, h, no_frame = _frame(config)
    out = {k: family.empty(k, n, h, w) for k in names}
    if n == 0 or no_frame:
        return out
    c = config.to_c()
    entry = getattr(load(), family.entry)
    for i, d in enumerate(descs):
        frame = family.struct(**{k: v[i].ctypes.data for k, v in out.items()})
        check(entry(d.ptr, C.byref(c), *[hs[i] for hs in heights], C.byref(frame), int(device)))
    return out


def _shot_variant(shot, asked: bool = False) -> Tuple[str, tuple]:
    """Which of the three forms of a shot entry a call takes, as the suffix of its C name, and the arguments that stand for the
    shot in it (``None``: the defaults).  ``"_ex"`` with (mcrt_shot_ex,) where the call needs it — a transparent page, a shadow
    colour other than 0, or ``asked`` (bounds or a crop are wanted); otherwise the calls made before ``_ex`` existed are made
    unchanged: ``"_occ"`` with (mcrt_shot, strength) whenever the floor-occlusion strength is not 0, so the library refuses one
    that is negative, above 1 or NaN, and ``""`` with (mcrt_shot,)."""
    sh = shot if shot is not None else abi.Shot()
    if asked or sh.needs_ex():
        return "_ex", (sh.to_c_ex(),)
    s, o = sh.to_c(), float(sh.floorOcclusion)
    return ("_occ", (s, o)) if o != 0.0 else ("", (s,))


def _empty_bounds(n: int, w: int, h: int) -> np.ndarray:
    """(n, 4) int32 holding the box of a frame without content, {width, height, 0, 0}."""
    b = np.zeros((n, 4), np.int32)
    b[:, 0], b[:, 1] = w, h
    return b


def _bake_grid(grid) -> int:
    if isinstance(grid, bool) or int(grid) != grid or not 1 <= int(grid) <= abi.BAKE_MAX_GRID:
        raise ValueError(f"grid must be an integer from 1 to {abi.BAKE_MAX_GRID}")
    return int(grid)


def scene_floor(scene) -> float:
    """The smallest y of the scene's (posed, world-space) box vertices (mcrt_scene_floor).  At pose 0: 0.0 for the built-in
    default scene and a 64x32 skin, -0.5 for a 64x64 skin, whose outer leg layers are boxes 0.5 larger than the legs — a plane
    there lies 0.5 below the soles; pass ``ground=0.0`` to ``renderGround`` for a shadow that touches the feet of a standing
    figure.  A scene without a vertex raises ``McrtError``."""
    y = C.c_float()
    check(load().mcrt_scene_floor(_as_desc(scene).ptr, C.byref(y)))
    return float(y.value)


def _ground_heights(descs, ground) -> List[float]:
    """One finite height per scene from ``None`` (its floor), a number, or a sequence of len(descs) numbers."""
    if ground is None:
        heights = [scene_floor(d) for d in descs]
    elif isinstance(ground, (int, float, np.integer, np.floating)):
        heights = [float(ground)] * len(descs)
    else:
        heights = [float(g) for g in ground]
        if len(heights) != len(descs):
            raise ValueError(f"{len(heights)} ground heights for {len(descs)} scenes")
    for g in heights:
        if not np.isfinite(np.float32(g)):
            raise ValueError("ground must be finite")
    return heights


def skin_texel(kind, mesh: int, face: int, tx: int, ty: int) -> Tuple[int, int]:
    """(mesh, face slot, tx, ty) of a scene built by ``MeshBuilder.buildScene`` → the skin image's texel ``(x, y)`` that face
    texel was cut from (mcrt_skin_texel_model).  ``kind``: ``"S64"`` / ``"S32"`` or the skin's height, ``"S64S"`` / ``"slim"`` for
    the slim model.  Out-of-range arguments raise ``ValueError``."""
    x, y = C.c_int(), C.c_int()
    lib = load()
    if lib.mcrt_skin_texel_model(*_skin_kind(kind), int(mesh), int(face) & 7, int(tx), int(ty), C.byref(x), C.byref(y)) != 0:
        raise ValueError(lib.mcrt_last_error().decode("utf-8", "replace"))
    return int(x.value), int(y.value)


def quantize_rgba8(image: np.ndarray) -> np.ndarray:
    """ImageWriter quantiser (image_writer.cpp:18-22): (H, W, 4) float32 → uint8."""
    img = np.ascontiguousarray(image, np.float32)
    out = np.zeros(img.shape, np.uint8)
    load().mcrt_quantize_rgba8(abi.fptr(img), out.ctypes.data_as(C.POINTER(C.c_uint8)), img.size // 4)
    return out


class ImageWriter:
    """The reference's PNG hand-off (src/output/image_writer.h): quantise + write.  The file is an
    uncompressed (zlib-stored) 8-bit RGBA PNG written by the library's own store-only encoder."""

    @staticmethod
    def writePNG(image: np.ndarray, path: str) -> bool:
        """(H, W, 4) float32 → PNG at `path`.  False on failure (empty image, unwritable path), like
        ImageWriter::writePNG (image_writer.cpp:6-28)."""
        img = np.ascontiguousarray(image, np.float32)
        if img.ndim != 3 or img.shape[2] != 4 or img.shape[0] <= 0 or img.shape[1] <= 0:
            return False
        return load().mcrt_write_png_f32(os.fsencode(path), abi.fptr(img), img.shape[1], img.shape[0]) == 0

    @staticmethod
    def writePNG8(rgba8: np.ndarray, path: str) -> bool:
        img = np.ascontiguousarray(rgba8, np.uint8)
        if img.ndim != 3 or img.shape[2] != 4 or img.shape[0] <= 0 or img.shape[1] <= 0:
            return False
        return load().mcrt_write_png_rgba8(os.fsencode(path), img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[1], img.shape[0]) == 0

    @staticmethod
    def encodePNG8(rgba8: np.ndarray) -> bytes:
        img = np.ascontiguousarray(rgba8, np.uint8)
        h, w = img.shape[:2]
        p = img.ctypes.data_as(C.POINTER(C.c_uint8))
        n = load().mcrt_encode_png_rgba8(p, w, h, None, 0)
        buf = (C.c_uint8 * n)()
        got = load().mcrt_encode_png_rgba8(p, w, h, buf, n)
        return bytes(buf[:got])


def render_png(scene, config: Config, path: str, device: int = 0, background: str = "reference", lights=None) -> bool:
    """TileRenderer::render + ImageWriter::writePNG in one call (RGBA8 quantised in the kernel epilogue,
    4 B/pixel copied back).  ``background="transparent"``: the figure alone on a transparent background (straight alpha).
    ``lights``: extra lights, as for ``TileRenderer.render``."""
    mode = abi.background_mode(background)
    c = config.to_c()
    extra, n_extra = abi.light_array(lights)
    if n_extra:
        return load().mcrt_render_png_lights(_as_desc(scene).ptr, C.byref(c), extra, n_extra, mode, os.fsencode(path), device) == 0
    if mode != abi.BACKGROUND_REFERENCE:
        return load().mcrt_render_png_ex(_as_desc(scene).ptr, C.byref(c), mode, os.fsencode(path), device) == 0
    return load().mcrt_render_png(_as_desc(scene).ptr, C.byref(c), os.fsencode(path), device) == 0


def render_shot_png(scene, config: Config, path: str, shot: Optional[abi.Shot] = None, ground: Optional[float] = None, device: int = 0,
                    crop: bool = False) -> bool:
    """``TileRenderer.renderShot`` + ``ImageWriter.writePNG8`` in one call (mcrt_render_shot_png): the finished studio shot as
    a PNG, 4 B/pixel copied back.  ``ground=None``: the scene's floor.  False on failure, like ``render_png``.  With
    ``Shot(page="transparent")`` the file carries the cut-out's alpha, and ``crop=True`` writes its bounds rectangle alone (the
    whole frame where nothing is visible) through mcrt_render_shot_png_ex."""
    variant, shot_args = _shot_variant(shot, crop)
    d = _as_desc(scene)
    g = _ground_heights([d], ground)[0]
    c = config.to_c()
    ex_args = (int(bool(crop)), None) if variant == "_ex" else ()
    return getattr(load(), "mcrt_render_shot_png" + variant)(d.ptr, C.byref(c), *shot_args, g, os.fsencode(path), *ex_args, int(device)) == 0


def shot_scratch_bytes(config: Config, shot: Optional[abi.Shot] = None, n_frames: int = 1, bounds: bool = False) -> int:
    """Bytes of device scratch ``render_shot_batch_device`` / ``DeviceScene.render_shot_device`` need for ``n_frames`` frames
    (mcrt_shot_scratch_bytes; host only): 16 per pixel, + 16 with a reflection, + 4 with a shadow, + 4 with a fading
    reflection, + 4 behind them with ``floorOcclusion`` > 0 (mcrt_shot_scratch_bytes_occ), every plane on a 16-byte boundary.
    0 for a zero-size frame or ``n_frames <= 0``.  A transparent page, a shadow colour and ``bounds`` change nothing of the size
    (mcrt_shot_scratch_bytes_ex); bounds with an opaque page are refused like an invalid shot: 0."""
    c = config.to_c()
    variant, shot_args = _shot_variant(shot, bounds)
    if bounds and shot_args[0].shot.page != abi.PAGE_TRANSPARENT:
        return 0
    return int(getattr(load(), "mcrt_shot_scratch_bytes" + variant)(C.byref(c), *shot_args, int(n_frames)))


SKIN_HEIGHTS = {"S64": 64, "S32": 32, 64: 64, 32: 32}


def _skin_height(kind) -> int:
    if isinstance(kind, bool) or kind not in SKIN_HEIGHTS:
        raise ValueError("kind must be 'S64', 'S32', 64 or 32")
    return SKIN_HEIGHTS[kind]


# a skin kind with its player model: (skin height, model).  "S64S" / "slim": a 64x64 skin on the slim model
SKIN_KINDS = {"S64S": (64, abi.SKIN_SLIM), "slim": (64, abi.SKIN_SLIM)}
SKIN_KINDS.update({k: (h, abi.SKIN_CLASSIC) for k, h in SKIN_HEIGHTS.items()})
SKIN_POOL_TEXELS = {(64, abi.SKIN_CLASSIC): 3264, (32, abi.SKIN_CLASSIC): 2016, (64, abi.SKIN_SLIM): 3136}


def _skin_kind(kind) -> Tuple[int, int]:
    if isinstance(kind, bool) or kind not in SKIN_KINDS:
        raise ValueError("kind must be 'S64', 'S32', 'S64S' ('slim'), 64 or 32")
    return SKIN_KINDS[kind]


def skin_model(image) -> str:
    """``"slim"`` or ``"classic"``: the player model a skin image, (64 | 32, 64, 4) uint8, was painted for, by the rule the common
    skin viewers use (mcrt_skin_model_of) — a heuristic: slim iff the image is 64x64 and the 64 pixels of the inner arms'
    unwraps that a slim figure never reads all have alpha 0."""
    a = np.ascontiguousarray(image, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("skin must be (H, W, 4) uint8")
    lib = load()
    m = lib.mcrt_skin_model_of(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0])
    if m < 0:
        raise ValueError(lib.mcrt_last_error().decode("utf-8", "replace"))
    return "slim" if m == abi.SKIN_SLIM else "classic"


def skin_pool_map(kind) -> np.ndarray:
    """Per texel of the pool of a repaintable scene (``DeviceScene.for_skin``), in pool order, the skin pixel index
    ``y * 64 + x`` it is cut from (mcrt_skin_pool_map_model): 3264 int32 for ``"S64"``, 2016 for ``"S32"``, 3136 for ``"S64S"``."""
    h, model = _skin_kind(kind)
    lib = load()
    out = np.zeros(SKIN_POOL_TEXELS[h, model], np.int32)
    n = lib.mcrt_skin_pool_map_model(h, model, out.ctypes.data_as(abi.c_int32_p), len(out))
    if n != len(out):
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    return out


def cape_texel(face: int, tx: int, ty: int) -> Tuple[int, int]:
    """The cape pixel (x, y) that texel (tx, ty) of face slot ``face`` of a cape mesh is cut from (mcrt_cape_texel)."""
    x, y = C.c_int(), C.c_int()
    check(load().mcrt_cape_texel(int(face), int(tx), int(ty), C.byref(x), C.byref(y)))
    return int(x.value), int(y.value)


def cape_pool_map() -> np.ndarray:
    """Per texel of a cape mesh, in pool order — six faces in slot order, row-major — the cape pixel index ``y * 64 + x`` it is
    cut from (mcrt_cape_pool_map): 372 int32.  In a caped figure's pool these are the LAST 372 texels."""
    lib = load()
    out = np.zeros(CAPE_TEXELS, np.int32)
    if lib.mcrt_cape_pool_map(out.ctypes.data_as(abi.c_int32_p), len(out)) != len(out):
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    return out


def pool_to_cape(values, fill=0) -> np.ndarray:
    """Scatters a pool-order plane of a cape mesh — ``values``: (372,) or (372, c), e.g. the last 372 rows of a caped figure's
    bake — into a cape-shaped image ``(32, 64[, c])`` through ``cape_pool_map``; pixels the unwrap does not read hold ``fill``."""
    pmap = cape_pool_map()
    v = np.asarray(values)
    if v.ndim not in (1, 2) or v.shape[0] != len(pmap):
        raise ValueError(f"values must be ({len(pmap)},) or ({len(pmap)}, c)")
    out = np.full((32 * 64,) + v.shape[1:], fill, v.dtype)
    out[pmap] = v  # (every pixel is used once at most)
    return out.reshape((32, 64) + v.shape[1:])


def _cape_angle(cape_angle) -> float:
    a = float(cape_angle)
    if not (0.0 <= a <= 90.0):
        raise ValueError("cape_angle must be within 0 .. 90 degrees")
    return a


def _view_pose(pose) -> Optional[np.ndarray]:
    if pose is None:
        return None
    p = np.ascontiguousarray(pose, np.float32)
    if p.shape != (12,):
        raise ValueError("pose must hold 12 floats")
    return p


def skin_view_table(kind, pose: Optional[Sequence[float]] = None, look=None, cape_angle: Optional[float] = None) -> bytes:
    """The view-dependent prefix ``[header][mesh table]`` of the blob of ``DeviceScene.for_skin(kind, pose, look)`` — bytes
    ``[0, texel_offset)``, 2496 for ``"S64"`` and ``"S64S"``, 1536 for ``"S32"`` — computed on the host
    (mcrt_skin_view_table_model): what a view change writes into a resident scene, but for the MESH_OPAQUE bits, which are the
    white figure's here.  ``cape_angle``: the prefix of the CAPED figure at that angle instead (mcrt_skin_view_table_cape), 2688 or
    1728 bytes."""
    h, model = _skin_kind(kind)
    p, d = _view_pose(pose), _as_desc(look) if look is not None else None
    lib = load()
    args = (h, model, abi.fptr(p) if p is not None else None, d.ptr if d is not None else None)
    fn = lib.mcrt_skin_view_table_model
    if cape_angle is not None:
        args, fn = args + (_cape_angle(cape_angle),), lib.mcrt_skin_view_table_cape
    n = fn(*args, None, 0)
    buf = C.create_string_buffer(max(n, 1))
    if n <= 0 or fn(*args, buf, n) != n:
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    return buf.raw[:n]


_LOOK_ARRAYS = ("light_position", "light_color", "camera_position", "camera_target", "camera_up", "background_color")
_LOOK_SCALARS = ("light_intensity", "light_radius", "camera_fov")


def orbit_look(yaw_deg: float, pitch_deg: float, distance: float, target=(0.0, 18.0, 0.0), base=None) -> SceneDesc:
    """A look — a description whose light, camera and background count, for ``DeviceScene.for_skin`` and ``set_view`` — with
    the camera on an orbit about ``target`` (yaw 0: the default camera's side, +Z), on a copy of ``base`` (a ``Scene`` /
    ``SceneDesc``; ``None``: the builder's default look).  ``base`` is not modified."""
    import math

    sd = MeshBuilder.buildDefaultScene()
    d = sd.desc
    if base is not None:
        b = _as_desc(base).desc
        for k in _LOOK_ARRAYS:
            for i in range(len(getattr(d, k))):
                getattr(d, k)[i] = getattr(b, k)[i]
        for k in _LOOK_SCALARS:
            setattr(d, k, getattr(b, k))
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    pos = (target[0] + distance * math.cos(pitch) * math.sin(yaw), target[1] + distance * math.sin(pitch),
           target[2] + distance * math.cos(pitch) * math.cos(yaw))
    for k in range(3):
        d.camera_position[k] = pos[k]
        d.camera_target[k] = target[k]
    return sd


def texel_table(scene) -> np.ndarray:
    """Per texel of the scene's texel pool, in pool order, its OWNER face (mcrt_bake_texel_table): (n, 4) int32 rows
    ``mesh, face slot, tx, ty`` — of the faces that reference the texel the one with the lowest mesh index, then the lowest face
    slot — and ``-1, 0, -1, -1`` for a texel no face references.  The planes of a light bake are indexed like this table.  For
    a figure of ``MeshBuilder.buildScene`` / ``DeviceScene.for_skin`` with every part present it agrees with ``skin_pool_map``
    and ``skin_texel``."""
    d = _as_desc(scene)
    lib = load()
    n = lib.mcrt_bake_texel_table(d.ptr, None, 0)
    if n < 0:
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    out = np.zeros((n, 4), np.int32)
    if n and lib.mcrt_bake_texel_table(d.ptr, out.ctypes.data_as(abi.c_int32_p), n) != n:
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    return out


def pool_to_skin(kind, values, fill=0) -> np.ndarray:
    """Scatters a pool-order plane of a repaintable scene (``DeviceScene.for_skin``) or of a builder figure with every part
    present — ``values``: (n,) or (n, c) with n = 3264 for ``"S64"``, 2016 for ``"S32"``, 3136 for ``"S64S"`` — into a skin-shaped image
    ``(skin_height, 64[, c])`` through ``skin_pool_map``.  Where a legacy skin maps two pool texels to one pixel (its mirrored
    left limbs) the lowest pool index wins; pixels no pool texel is cut from hold ``fill``.  Pure numpy."""
    h = _skin_kind(kind)[0]
    pmap = skin_pool_map(kind)
    v = np.asarray(values)
    if v.ndim not in (1, 2) or v.shape[0] != len(pmap):
        raise ValueError(f"values must be ({len(pmap)},) or ({len(pmap)}, c) for this skin kind")
    out = np.full((h * 64,) + v.shape[1:], fill, v.dtype)
    out[pmap[::-1]] = v[::-1]  # assigned last to first: of two texels of one pixel the lowest pool index is written last
    return out.reshape((h, 64) + v.shape[1:])


class DeviceScene:
    """A flattened scene resident in HBM on one device (mcrt_scene).  Renders go to device pointers
    (e.g. ``torch.Tensor.data_ptr()``) on a caller-chosen HIP stream."""

    skin_height = 0  # 64 / 32 for a repaintable scene (for_skin)
    skin_model = "classic"  # "slim" for a repaintable scene of the slim model (for_skin("S64S", ...))
    has_cape = False  # a repaintable scene with a cape mesh (for_skin(..., cape=True))

    def __init__(self, scene, device: int = 0):
        self._desc = _as_desc(scene)
        self._h = C.c_void_p()
        self.device = device
        check(load().mcrt_scene_create(self._desc.ptr, device, C.byref(self._h)))

    @classmethod
    def for_skin(cls, kind, pose: Optional[Sequence[float]] = None, look=None, device: int = 0, cape: bool = False, cape_angle: float = 10.0) -> "DeviceScene":
        """A REPAINTABLE scene (mcrt_scene_create_skin_model): the builder's figure for ``kind`` (``"S64"`` / ``"S32"`` or the skin's
        height, ``"S64S"`` / ``"slim"`` for a 64x64 skin on the slim model) at ``pose`` with every part present — always the full mesh table of ``skin_texel``, 12 or 7 meshes — which
        ``set_skin`` / ``set_skin_device`` / ``set_skins_batch_device`` give a new skin without rebuilding the scene.  ``look``:
        a ``Scene`` / ``SceneDesc`` whose light, camera and background are taken (its meshes are ignored); ``None``: the
        builder's.  White and opaque until the first repaint.  ``cape=True`` (mcrt_scene_create_skin_cape): the cape mesh behind
        the figure as mesh 12 or 7, at ``cape_angle`` degrees, which ``set_cape`` / ``set_cape_device`` / ``set_capes_batch_device``
        paint; transparent — never hit — until then."""
        h, model = _skin_kind(kind)
        self = object.__new__(cls)
        self._desc = _as_desc(look) if look is not None else None
        self._h = C.c_void_p()
        self.device = device
        self.skin_height = h
        self.skin_model = "slim" if model == abi.SKIN_SLIM else "classic"
        p = _view_pose(pose)
        if cape:
            self.has_cape = True
            check(load().mcrt_scene_create_skin_cape(h, model, abi.fptr(p) if p is not None else None, self._desc.ptr if self._desc is not None else None,
                                                     _cape_angle(cape_angle), int(device), C.byref(self._h)))
            return self
        check(load().mcrt_scene_create_skin_model(h, model, abi.fptr(p) if p is not None else None, self._desc.ptr if self._desc is not None else None,
                                            int(device), C.byref(self._h)))
        return self

    def _need_cape(self) -> None:
        if not self.has_cape:
            raise ValueError("this scene has no cape: create it with DeviceScene.for_skin(..., cape=True)")

    def set_cape(self, cape: Optional[np.ndarray]) -> None:
        """Repaint the cape from a host image, (32, 64, 4) uint8, or ``None`` for no cape (transparent); synchronous
        (mcrt_scene_set_cape).  The skin stays as it is."""
        self._need_cape()
        a = _cape_image(cape) if cape is not None else None
        check(load().mcrt_scene_set_cape(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)) if a is not None else None))

    def set_cape_device(self, ptr: int, stream: int = 0) -> None:
        """Repaint the cape from 8192 bytes of RGBA8 in device memory, 4-byte aligned (0: no cape); asynchronous on ``stream``
        (mcrt_scene_set_cape_device).  Ordered against the handle's renders like ``set_skin_device``."""
        self._need_cape()
        check(load().mcrt_scene_set_cape_device(self._h, C.c_void_p(ptr or None), C.c_void_p(stream)))

    def _skin_bytes(self) -> int:
        if not self.skin_height:
            raise ValueError("not a repaintable scene: create it with DeviceScene.for_skin")
        return 64 * self.skin_height * 4

    def set_skin(self, skin: np.ndarray) -> None:
        """Repaint from a host image, (skin_height, 64, 4) uint8; synchronous (mcrt_scene_set_skin)."""
        n = self._skin_bytes()
        a = np.ascontiguousarray(skin, np.uint8)
        if a.shape != (self.skin_height, 64, 4):
            raise ValueError(f"skin must be ({self.skin_height}, 64, 4) uint8")
        assert a.nbytes == n
        check(load().mcrt_scene_set_skin(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_skin_device(self, ptr: int, stream: int = 0) -> None:
        """Repaint from 64 * skin_height * 4 bytes of RGBA8 in device memory, 4-byte aligned; asynchronous on ``stream``
        (mcrt_scene_set_skin_device).  The handle's renders are ordered against it by the library; its layers, ground and
        pick passes by the caller."""
        self._skin_bytes()
        check(load().mcrt_scene_set_skin_device(self._h, C.c_void_p(ptr or None), C.c_void_p(stream)))

    def set_view(self, pose: Optional[Sequence[float]] = None, look=None, cape_angle: Optional[float] = None) -> None:
        """Another pose and / or look for this repaintable scene, synchronously (mcrt_scene_set_view): afterwards it is what
        ``for_skin(kind, pose, look)`` repainted with the current skin would be, bit for bit.  ``None`` keeps the scene's own.
        ``cape_angle`` (a caped scene): another cape angle too (mcrt_scene_set_view_cape)."""
        self._skin_bytes()
        p, d = _view_pose(pose), _as_desc(look) if look is not None else None
        if cape_angle is not None:
            self._need_cape()
            a = C.c_float(_cape_angle(cape_angle))
            check(load().mcrt_scene_set_view_cape(self._h, abi.fptr(p) if p is not None else None, d.ptr if d is not None else None, C.byref(a)))
            return
        check(load().mcrt_scene_set_view(self._h, abi.fptr(p) if p is not None else None, d.ptr if d is not None else None))

    def set_view_device(self, pose: Optional[Sequence[float]] = None, look=None, stream: int = 0, cape_angle: Optional[float] = None) -> None:
        """The same, asynchronous on ``stream`` (mcrt_scene_set_view_device); ``pose`` and ``look`` are read before the call
        returns.  The handle's renders are ordered against it by the library; its layers, ground, reflection, light, bake and
        pick passes by the caller."""
        self._skin_bytes()
        p, d = _view_pose(pose), _as_desc(look) if look is not None else None
        if cape_angle is not None:
            self._need_cape()
            a = C.c_float(_cape_angle(cape_angle))
            check(load().mcrt_scene_set_view_cape_device(self._h, abi.fptr(p) if p is not None else None, d.ptr if d is not None else None, C.byref(a),
                                                         C.c_void_p(stream)))
            return
        check(load().mcrt_scene_set_view_device(self._h, abi.fptr(p) if p is not None else None, d.ptr if d is not None else None, C.c_void_p(stream)))

    def blob(self) -> bytes:
        """The scene's resident blob, downloaded after waiting for the device (mcrt_probe_scene_blob)."""
        lib = load()
        head = C.create_string_buffer(192)
        n = lib.mcrt_probe_scene_blob(self._h, head, 192)
        if n < 192:
            raise McrtError(n, lib.mcrt_last_error().decode("utf-8", "replace"))
        buf = C.create_string_buffer(n)
        if lib.mcrt_probe_scene_blob(self._h, buf, n) != n:
            raise McrtError(abi.MCRT_ERR_HIP, lib.mcrt_last_error().decode("utf-8", "replace"))
        return buf.raw

    def units(self) -> dict:
        """The work units of the last pass of the handle's last render, first lane (mcrt_probe_units), after waiting for the
        device: ``{"records": (n, 4) uint32, "hits": (n,) uint32}``."""
        fn = load().mcrt_probe_units  # bound here: a build selected with MCRT_LIB may predate it
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        n = fn(self._h, None, None, 0)
        if n < 0:
            raise McrtError(n, load().mcrt_last_error().decode("utf-8", "replace"))
        rec, hits = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
        if n and fn(self._h, rec.ctypes.data, hits.ctypes.data, n) != n:
            raise McrtError(abi.MCRT_ERR_HIP, load().mcrt_last_error().decode("utf-8", "replace"))
        return {"records": rec, "hits": hits}

    def close(self):
        if self._h:
            load().mcrt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self) -> None:
        """Wait for the scene's device work; raises if the device flagged an internal inconsistency."""
        check(load().mcrt_scene_check(self._h))

    def tables(self) -> dict:
        """``{"window": bool, "full": bool, "sample": bool}``: the per-device tables this handle holds right now, which its next
        render or pass reads instead of the recurrence or the engine (mcrt_scene_tables)."""
        fn = load().mcrt_scene_tables  # bound here: a build selected with MCRT_LIB may predate it
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
        mask = C.c_int()
        check(fn(self._h, C.byref(mask)))
        return {name: bool(mask.value >> which & 1) for which, name in enumerate(TABLE_NAMES)}

    def set_lanes(self, lanes: int) -> None:
        """0 = automatic split of a render over internal streams, n >= 1 = exactly n (mcrt_scene_set_lanes)."""
        check(load().mcrt_scene_set_lanes(self._h, int(lanes)))

    def set_background(self, mode: str) -> None:
        """``"reference"`` or ``"transparent"`` for every later render of this handle, batches included
        (mcrt_scene_set_background)."""
        m = abi.background_mode(mode)
        check(load().mcrt_scene_set_background(self._h, m))

    def set_extra_lights(self, lights) -> None:
        """Up to three ``abi.Light`` beside the scene's own for every later beauty render of this handle, batches included; an
        empty sequence takes them off (mcrt_scene_set_extra_lights).  The passes that depend on the light refuse the handle
        while it carries any."""
        extra, n = abi.light_array(lights)
        check(load().mcrt_scene_set_extra_lights(self._h, extra, n))

    @property
    def extra_lights(self) -> List[abi.Light]:
        """The handle's extra lights (mcrt_scene_extra_lights)."""
        buf = (abi.McrtLightSource * abi.MAX_EXTRA_LIGHTS)()
        n = int(load().mcrt_scene_extra_lights(self._h, buf, abi.MAX_EXTRA_LIGHTS))
        return [abi.Light(tuple(buf[i].position), tuple(buf[i].color), float(buf[i].radius)) for i in range(n)]

    def owned_pixel_rows(self, config: Config, first: int = 0, step: int = 1) -> int:
        c = config.to_c()
        return int(load().mcrt_owned_pixel_rows(C.byref(c), first, step))

    def render_device(self, config: Config, out_ptr: int, first: int = 0, step: int = 1,
                      layout: int = abi.LAYOUT_FRAME, stream: int = 0) -> None:
        c = config.to_c()
        check(load().mcrt_render_device(self._h, C.byref(c), first, step, layout, C.c_void_p(out_ptr), C.c_void_p(stream)))

    def render_device_ex(self, config: Config, out_f32_ptr: int = 0, out_rgba8_ptr: int = 0, first: int = 0, step: int = 1,
                         layout: int = abi.LAYOUT_FRAME, stream: int = 0) -> None:
        """Render with the quantisation fused into the epilogue: float4 frame and/or RGBA8 plane."""
        c = config.to_c()
        check(load().mcrt_render_device_ex(self._h, C.byref(c), first, step, layout, C.c_void_p(out_f32_ptr or None),
                                           C.c_void_p(out_rgba8_ptr or None), C.c_void_p(stream)))

    def time_render_device(self, config: Config, out_ptr: int, iters: int, first: int = 0, step: int = 1,
                           layout: int = abi.LAYOUT_FRAME, stream: int = 0) -> float:
        """Average ms of one render's whole pipeline on the device, measured with hipEvents on `stream`."""
        c = config.to_c()
        a = C.c_float()
        check(load().mcrt_time_render_device(self._h, C.byref(c), first, step, layout, C.c_void_p(out_ptr),
                                             C.c_void_p(stream), iters, C.byref(a)))
        return float(a.value)

    def _pass_device(self, family: abi.PlaneFamily, config: Config, planes, stream: int, *middle) -> None:
        """One pass of ``family`` into the device planes (``_device_planes``) through its ``_device`` entry.  ``middle``: what
        the entry takes between the config and the planes — a ground height, a bake's grid."""
        c = config.to_c()
        check(getattr(load(), family.entry + "_device")(self._h, C.byref(c), *middle, C.byref(planes), C.c_void_p(stream)))

    def render_layers_device(self, config: Config, depth_ptr: int = 0, normal_ptr: int = 0, albedo_ptr: int = 0, id_ptr: int = 0,
                             stream: int = 0) -> None:
        """The geometry layers of the frame into device memory (mcrt_render_layers_device): width * height pixels per plane —
        depth 4 bytes per pixel, normal, albedo and id 16 — any pointer may be 0, not all.  Asynchronous on ``stream``;
        uses none of the handle's workspace, so it may run beside a render of the handle on another stream."""
        self._pass_device(abi.LAYERS, config, _device_planes(abi.LAYERS, depth_ptr, normal_ptr, albedo_ptr, id_ptr), stream)

    def render_ground_device(self, config: Config, ground: float, visibility_ptr: int = 0, distance_ptr: int = 0, matte_ptr: int = 0,
                             stream: int = 0) -> None:
        """The ground-shadow planes of the frame into device memory (mcrt_render_ground_device): width * height pixels per plane
        — visibility and distance 4 bytes per pixel, matte 1 — any pointer may be 0, not all.  ``ground``: the plane's height
        (``scene_floor`` of the description for the figure's own floor).  Asynchronous on ``stream``; uses none of the handle's
        workspace, so it may run beside a render of the handle on another stream."""
        self._pass_device(abi.GROUND, config, _device_planes(abi.GROUND, visibility_ptr, distance_ptr, matte_ptr), stream, _finite_ground(ground))

    def render_ground_occlusion_device(self, config: Config, ground: float, occlusion_ptr: int = 0, matte_ptr: int = 0, stream: int = 0) -> None:
        """The ground-occlusion planes of the frame into device memory (mcrt_render_ground_occlusion_device): width * height
        pixels per plane — occlusion 4 bytes per pixel, matte 1 — either pointer may be 0, not both.  ``ground``: the plane's
        height.  Asynchronous on ``stream``; uses none of the handle's workspace, so it may run beside a render of the handle on
        another stream."""
        self._pass_device(abi.GROUND_OCCLUSION, config, _device_planes(abi.GROUND_OCCLUSION, occlusion_ptr, matte_ptr), stream, _finite_ground(ground))

    def render_reflection_device(self, config: Config, ground: float, rgba_ptr: int = 0, rgba8_ptr: int = 0, distance_ptr: int = 0,
                                 stream: int = 0) -> None:
        """The ground-reflection planes of the frame into device memory (mcrt_render_reflection_device): width * height pixels
        per plane — rgba 16 bytes per pixel, rgba8 and distance 4 — any pointer may be 0, not all.  ``ground``: the plane's
        height.  Asynchronous on ``stream``; uses none of the handle's workspace, so it may run beside a render of the handle on
        another stream."""
        self._pass_device(abi.REFLECTION, config, _device_planes(abi.REFLECTION, rgba_ptr, rgba8_ptr, distance_ptr), stream, _finite_ground(ground))

    def render_shot_device(self, config: Config, shot: Optional[abi.Shot], ground: float, scratch_ptr: int, scratch_bytes: int,
                           out_f32_ptr: int = 0, out_rgba8_ptr: int = 0, stream: int = 0, bounds_ptr: int = 0) -> None:
        """The studio shot of the frame into device memory (mcrt_render_shot_device): render, ground pass, reflection pass and
        blend, in order on ``stream``, the intermediate planes in the caller's scratch (``shot_scratch_bytes`` bytes, 16-byte
        aligned).  The figure is rendered transparent whatever ``set_background`` says; the handle's mode is untouched.
        ``bounds_ptr``: device memory for 4 int32, the cut-out's box (transparent page only; 0: none)."""
        _need_output(out_f32_ptr, out_rgba8_ptr)
        g = _finite_ground(ground)
        variant, shot_args = _shot_variant(shot, bool(bounds_ptr))
        if variant:  # the batch entries with one handle: there is no single-handle _occ or _ex entry
            render_shot_batch_device([self], config, shot, g, scratch_ptr, scratch_bytes, out_f32_ptr, out_rgba8_ptr, None, stream, bounds_ptr)
            return
        c = config.to_c()
        check(load().mcrt_render_shot_device(self._h, C.byref(c), *shot_args, g, C.c_void_p(scratch_ptr or None), int(scratch_bytes),
                                             C.c_void_p(out_f32_ptr or None), C.c_void_p(out_rgba8_ptr or None), C.c_void_p(stream)))

    def render_light_device(self, config: Config, visibility_ptr: int = 0, occlusion_ptr: int = 0, direct_ptr: int = 0, stream: int = 0) -> None:
        """The light planes of the frame into device memory (mcrt_render_light_device): width * height pixels per plane —
        visibility and occlusion 4 bytes per pixel, direct 16 — any pointer may be 0, not all.  Asynchronous on ``stream``; uses
        none of the handle's workspace, so it may run beside a render of the handle on another stream."""
        self._pass_device(abi.LIGHT, config, _device_planes(abi.LIGHT, visibility_ptr, occlusion_ptr, direct_ptr), stream)

    @property
    def texels(self) -> int:
        """The size of the scene's texel pool (mcrt_scene_texels): the texels per plane of a light bake."""
        n = C.c_int()
        check(load().mcrt_scene_texels(self._h, C.byref(n)))
        return int(n.value)

    def bake_light_device(self, config: Config, grid: int = 1, position_ptr: int = 0, normal_ptr: int = 0, visibility_ptr: int = 0,
                          occlusion_ptr: int = 0, direct_ptr: int = 0, stream: int = 0) -> None:
        """The planes of a light bake into device memory (mcrt_bake_light_device): ``texels`` texels per plane in pool order —
        visibility and occlusion 4 bytes per texel, position, normal and direct 16 — any pointer may be 0, not all.
        Asynchronous on ``stream``; uses none of the handle's workspace, so it may run beside a render of the handle on another
        stream.  Ordering against a repaint of the handle is the caller's job."""
        self._pass_device(abi.BAKE, config, _device_planes(abi.BAKE, position_ptr, normal_ptr, visibility_ptr, occlusion_ptr, direct_ptr), stream, _bake_grid(grid))

    def render_light_multi_device(self, config: Config, visibility_ptrs: Sequence[int] = (), direct_ptrs: Sequence[int] = (), occlusion_ptr: int = 0,
                                  combined_ptr: int = 0, stream: int = 0) -> None:
        """The light planes PER LIGHT of the frame into device memory (mcrt_render_light_multi_device), for a handle with or without
        extra lights: ``visibility_ptrs[k]`` (4 bytes per pixel) and ``direct_ptrs[k]`` (16) take light k's plane — light 0 is the
        scene's own, lights 1.. the handle's extra lights, read at this call; a light the handle lacks gives the miss constants —,
        ``occlusion_ptr`` the occlusion (4) and ``combined_ptr`` the clamped sum of the direct planes (16), which is the beauty
        frame at 1 spp and 0 bounces on every hit pixel.  Any pointer may be 0, not all.  Asynchronous on ``stream``."""
        planes = _multi_device_planes(abi.McrtLightPlanesMulti, visibility_ptrs, direct_ptrs, occlusion=occlusion_ptr, combined=combined_ptr)
        c = config.to_c()
        check(load().mcrt_render_light_multi_device(self._h, C.byref(c), C.byref(planes), C.c_void_p(stream)))

    def bake_light_multi_device(self, config: Config, grid: int = 1, position_ptr: int = 0, normal_ptr: int = 0, visibility_ptrs: Sequence[int] = (),
                                occlusion_ptr: int = 0, direct_ptrs: Sequence[int] = (), combined_ptr: int = 0, stream: int = 0) -> None:
        """The planes of a light bake PER LIGHT into device memory (mcrt_bake_light_multi_device): ``bake_light_device`` with one
        visibility and one direct plane per light, as ``render_light_multi_device`` takes them, and ``combined_ptr``: the mean of
        the sub-samples' clamped sums (16 bytes per texel)."""
        planes = _multi_device_planes(abi.McrtBakePlanesMulti, visibility_ptrs, direct_ptrs, position=position_ptr, normal=normal_ptr,
                                      occlusion=occlusion_ptr, combined=combined_ptr)
        c = config.to_c()
        check(load().mcrt_bake_light_multi_device(self._h, C.byref(c), _bake_grid(grid), C.byref(planes), C.c_void_p(stream)))

    def pick(self, config: Config, xy) -> np.ndarray:
        """What is under the pixels ``xy`` ((n, 2) integers, x then y, inside the frame): a structured array of
        ``abi.SURFACE_DTYPE`` — mesh, face, tx, ty, t, point, normal, albedo — equal to the layers at those pixels
        (mcrt_scene_pick).  Synchronous."""
        a = np.asarray(xy)
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu":
            raise ValueError("xy must be an (n, 2) array of integer pixel coordinates")
        if len(a) and (a.min() < 0 or (a[:, 0] >= config.width).any() or (a[:, 1] >= config.height).any()):
            raise ValueError("a pick coordinate lies outside the frame")
        q = np.ascontiguousarray(a, np.int32)
        out = np.zeros(len(q), abi.SURFACE_DTYPE)
        c = config.to_c()
        check(load().mcrt_scene_pick(self._h, C.byref(c), q.ctypes.data_as(abi.c_int32_p), len(q), out.ctypes.data))
        return out

    # ---- probes (per-function parity tests) ----
    def intersect(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), abi.HIT_DTYPE)
        check(load().mcrt_probe_intersect(self._h, abi.fptr(rays), len(rays), out.ctypes.data))
        return out

    def trace(self, config: Config, rays: np.ndarray, depth: int = 0) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 4), np.float32)
        c = config.to_c()
        check(load().mcrt_probe_trace(self._h, C.byref(c), abi.fptr(rays), len(rays), depth, abi.fptr(out)))
        return out


def render_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, out_f32_ptr: int = 0, out_rgba8_ptr: int = 0,
                        frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """N frames of one config from resident scenes into device memory, one launch sequence (mcrt_render_batch_device).
    Frame i is written at ``out_f32_ptr + i * frame_stride_pixels * 16`` bytes and/or ``out_rgba8_ptr + i *
    frame_stride_pixels * 4``; ``frame_stride_pixels`` defaults to width * height.  Asynchronous on ``stream``."""
    handles = _handles(device_scenes)
    _need_output(out_f32_ptr, out_rgba8_ptr)
    stride = _frame_stride(config, frame_stride_pixels)
    c = config.to_c()
    check(load().mcrt_render_batch_device(_handle_array(handles), len(handles), C.byref(c), C.c_void_p(out_f32_ptr or None), C.c_void_p(out_rgba8_ptr or None),
                                          stride, C.c_void_p(stream)))


def render_layers_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, depth_ptr: int = 0, normal_ptr: int = 0,
                               albedo_ptr: int = 0, id_ptr: int = 0, frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The geometry layers of N resident scenes of one config in one launch (mcrt_render_layers_batch_device): frame i of
    each plane starts ``i * frame_stride_pixels`` pixels on (default width * height).  Asynchronous on ``stream``."""
    _pass_batch_device(abi.LAYERS, device_scenes, config, (depth_ptr, normal_ptr, albedo_ptr, id_ptr), frame_stride_pixels, stream)


def render_ground_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, ground, visibility_ptr: int = 0, distance_ptr: int = 0,
                               matte_ptr: int = 0, frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The ground-shadow planes of N resident scenes of one config in one launch (mcrt_render_ground_batch_device): frame i of
    each plane starts ``i * frame_stride_pixels`` pixels on (default width * height).  ``ground``: one height for all, or N
    heights (a handle may be listed more than once, with different heights).  Asynchronous on ``stream``."""
    _pass_batch_device(abi.GROUND, device_scenes, config, (visibility_ptr, distance_ptr, matte_ptr), frame_stride_pixels, stream, ground)


def render_ground_occlusion_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, ground, occlusion_ptr: int = 0, matte_ptr: int = 0,
                                         frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The ground-occlusion planes of N resident scenes of one config in one launch (mcrt_render_ground_occlusion_batch_device):
    frame i of each plane starts ``i * frame_stride_pixels`` pixels on (default width * height).  ``ground``: one height for
    all, or N heights (a handle may be listed more than once, with different heights).  Asynchronous on ``stream``."""
    _pass_batch_device(abi.GROUND_OCCLUSION, device_scenes, config, (occlusion_ptr, matte_ptr), frame_stride_pixels, stream, ground)


def render_reflection_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, ground, rgba_ptr: int = 0, rgba8_ptr: int = 0,
                                   distance_ptr: int = 0, frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The ground-reflection planes of N resident scenes of one config in one launch (mcrt_render_reflection_batch_device): frame
    i of each plane starts ``i * frame_stride_pixels`` pixels on (default width * height).  ``ground``: one height for all, or N
    heights (a handle may be listed more than once, with different heights).  Asynchronous on ``stream``."""
    _pass_batch_device(abi.REFLECTION, device_scenes, config, (rgba_ptr, rgba8_ptr, distance_ptr), frame_stride_pixels, stream, ground)


def _handles(device_scenes) -> list:
    handles = []
    for s in device_scenes:
        if not isinstance(s, DeviceScene):
            raise TypeError("device_scenes must be DeviceScene objects")
        handles.append(s._h)
    return handles


def _handle_array(handles):
    return (C.c_void_p * max(len(handles), 1))(*[h.value for h in handles])


def _height_array(heights):
    return (C.c_float * max(len(heights), 1))(*heights)


def _need_output(out_f32_ptr: int, out_rgba8_ptr: int) -> None:
    if not out_f32_ptr and not out_rgba8_ptr:
        raise ValueError("give out_f32_ptr and/or out_rgba8_ptr")


def _device_planes(family: abi.PlaneFamily, *ptrs: int):
    """The family's structure of device pointers, one per plane in the family's order, 0 = not wanted; all 0 raises."""
    if not any(ptrs):
        raise ValueError("give at least one of " + ", ".join(f"{k}_ptr" for k in family.names))
    return family.struct(*[p or None for p in ptrs])


def _multi_empty(formats: dict, names, n_lights: int, shape: tuple) -> dict:
    """The host planes of a pass under extra lights, holding the miss values: a per-light member with a leading ``n_lights``."""
    out = {}
    for name in names:
        dtype, comps = formats[name]
        lead = (n_lights,) if name in abi.PER_LIGHT_NAMES else ()
        a = np.zeros(lead + shape + ((comps,) if comps > 1 else ()), dtype)
        if name in abi.MULTI_MISS:
            a[...] = abi.MULTI_MISS[name]
        out[name] = a
    return out


def _multi_host_planes(struct, out: dict, ks):
    """``struct`` with the host addresses of ``out``: row i of a per-light member is light ks[i]'s plane."""
    frame = struct()
    for name, a in out.items():
        if name in abi.PER_LIGHT_NAMES:
            for i, k in enumerate(ks):
                getattr(frame, name)[k] = a[i].ctypes.data
        else:
            setattr(frame, name, a.ctypes.data)
    return frame


def _finite_ground(ground) -> float:
    if not np.isfinite(np.float32(ground)):
        raise ValueError("ground must be finite")
    return float(ground)


def _resident_heights(handles, ground) -> List[float]:
    """``_ground_heights`` for resident scenes, which have no floor of their own to fall back to."""
    if ground is None:
        raise ValueError("ground heights are needed: a resident scene does not keep its description (see scene_floor)")
    return _ground_heights(handles, ground)


def _frame_stride(config: Config, value: Optional[int], name: str = "frame_stride_pixels") -> int:
    """The stride between the frames of a batch, in pixels: ``value``, or width * height for ``None``; never less than that."""
    px = max(config.width, 0) * max(config.height, 0)
    stride = px if value is None else int(value)
    if stride < px:
        raise ValueError(f"{name} {stride} is smaller than width * height = {px}")
    return stride


def _pass_batch_device(family: abi.PlaneFamily, device_scenes, config: Config, ptrs, frame_stride_pixels, stream: int, *ground) -> None:
    """One pass of ``family`` for N resident scenes through its ``_batch_device`` entry.  ``ptrs``: one device pointer per plane in
    the family's order; ``ground``: the heights argument of a pass that has a floor plane, nothing for one that has none."""
    handles = _handles(device_scenes)
    planes = _device_planes(family, *ptrs)
    heights = [_height_array(_resident_heights(handles, g)) for g in ground]
    stride = _frame_stride(config, frame_stride_pixels)
    c = config.to_c()
    check(getattr(load(), family.entry + "_batch_device")(_handle_array(handles), len(handles), C.byref(c), *heights, C.byref(planes), stride,
                                                          C.c_void_p(stream)))


def render_shot_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, shot: Optional[abi.Shot], ground, scratch_ptr: int,
                             scratch_bytes: int, out_f32_ptr: int = 0, out_rgba8_ptr: int = 0, frame_stride_pixels: Optional[int] = None,
                             stream: int = 0, bounds_ptr: int = 0) -> None:
    """The studio shots of N resident scenes of one config (mcrt_render_shot_batch_device): one batched render, one ground and
    one reflection launch and one blend, in order on ``stream``; frame i lands ``i * frame_stride_pixels`` pixels on (default
    width * height) in ``out_f32_ptr`` (16 B/pixel) and / or ``out_rgba8_ptr`` (4 B/pixel).  ``ground``: one height for all, or
    N heights.  ``scratch_ptr``: device memory, 16-byte aligned, ``shot_scratch_bytes(config, shot, N)`` bytes.  With
    ``shot.floorOcclusion`` > 0 the ground-occlusion pass runs between the reflection and the blend
    (mcrt_render_shot_batch_device_occ).  ``bounds_ptr``: device memory for N x 4 int32, the cut-outs' boxes, valid in stream
    order behind the call (transparent page only; 0: none).  A transparent page, a shadow colour or bounds take
    mcrt_render_shot_batch_device_ex."""
    handles = _handles(device_scenes)
    _need_output(out_f32_ptr, out_rgba8_ptr)
    heights = _resident_heights(handles, ground)
    stride = _frame_stride(config, frame_stride_pixels)
    variant, shot_args = _shot_variant(shot, bool(bounds_ptr))
    c = config.to_c()
    ex_args = (C.c_void_p(bounds_ptr or None),) if variant == "_ex" else ()
    check(getattr(load(), "mcrt_render_shot_batch_device" + variant)(
        _handle_array(handles), len(handles), C.byref(c), *shot_args, _height_array(heights), C.c_void_p(scratch_ptr or None), int(scratch_bytes),
        C.c_void_p(out_f32_ptr or None), C.c_void_p(out_rgba8_ptr or None), stride, *ex_args, C.c_void_p(stream)))


def composite_shot_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, shot: Optional[abi.Shot], figure_ptr: int,
                                visibility_ptr: int = 0, reflection_ptr: int = 0, reflection_distance_ptr: int = 0, out_f32_ptr: int = 0,
                                out_rgba8_ptr: int = 0, in_stride_pixels: Optional[int] = None, out_stride_pixels: Optional[int] = None,
                                stream: int = 0, occlusion_ptr: int = 0, bounds_ptr: int = 0) -> None:
    """The studio shot's blend alone, on device planes the caller already has (mcrt_composite_shot_batch_device): the
    transparent figure (required, 16 B/pixel), the ground pass's visibility (0: none, no shadow), the reflection pass's rgba
    (0: no mirror image) and distance (0 only with ``shot.reflectionFade == 0``).  Frame i of the inputs starts
    ``i * in_stride_pixels`` pixels on, of the outputs ``i * out_stride_pixels`` (default width * height).  With
    ``shot.floorOcclusion`` > 0 the blend takes the ground-occlusion pass's plane at ``occlusion_ptr`` (4 B/pixel; 0: none)
    through mcrt_composite_shot_batch_device_occ.  ``bounds_ptr``: as for ``render_shot_batch_device``; a transparent page, a
    shadow colour or bounds take mcrt_composite_shot_batch_device_ex."""
    handles = _handles(device_scenes)
    if not figure_ptr:
        raise ValueError("figure_ptr is required")
    _need_output(out_f32_ptr, out_rgba8_ptr)
    in_stride = _frame_stride(config, in_stride_pixels, "in_stride_pixels")
    out_stride = _frame_stride(config, out_stride_pixels, "out_stride_pixels")
    variant, shot_args = _shot_variant(shot, bool(bounds_ptr))
    c = config.to_c()
    planes = abi.McrtShotInputs(figure_ptr, visibility_ptr or None, reflection_ptr or None, reflection_distance_ptr or None)
    shot_c, *strength = shot_args  # (here the _occ form takes its strength behind the occlusion plane, not behind the shot)
    occ_args = (C.c_void_p(occlusion_ptr or None), *strength) if variant else ()
    ex_args = (C.c_void_p(bounds_ptr or None),) if variant == "_ex" else ()
    check(getattr(load(), "mcrt_composite_shot_batch_device" + variant)(
        _handle_array(handles), len(handles), C.byref(c), shot_c, C.byref(planes), *occ_args, in_stride, C.c_void_p(out_f32_ptr or None),
        C.c_void_p(out_rgba8_ptr or None), out_stride, *ex_args, C.c_void_p(stream)))


def render_light_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, visibility_ptr: int = 0, occlusion_ptr: int = 0,
                              direct_ptr: int = 0, frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The light planes of N resident scenes of one config in one launch per kernel (mcrt_render_light_batch_device): frame i of
    each plane starts ``i * frame_stride_pixels`` pixels on (default width * height).  A handle may be listed more than once.
    Asynchronous on ``stream``."""
    _pass_batch_device(abi.LIGHT, device_scenes, config, (visibility_ptr, occlusion_ptr, direct_ptr), frame_stride_pixels, stream)


def bake_light_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, grid: int = 1, position_ptr: int = 0, normal_ptr: int = 0,
                            visibility_ptr: int = 0, occlusion_ptr: int = 0, direct_ptr: int = 0, texel_stride: Optional[int] = None,
                            stream: int = 0) -> None:
    """The light bakes of N resident scenes in one launch per kernel (mcrt_bake_light_batch_device): frame i of each plane starts
    ``i * texel_stride`` texels on (default: the largest ``texels`` of the scenes, which may differ).  A handle may be listed more
    than once.  Asynchronous on ``stream``."""
    handles = _handles(device_scenes)
    planes = _device_planes(abi.BAKE, position_ptr, normal_ptr, visibility_ptr, occlusion_ptr, direct_ptr)
    g = _bake_grid(grid)
    if texel_stride is None:
        texel_stride = max([s.texels for s in device_scenes], default=0)
    if int(texel_stride) < 0:
        raise ValueError("texel_stride must be >= 0")
    c = config.to_c()
    check(load().mcrt_bake_light_batch_device(_handle_array(handles), len(handles), C.byref(c), g, C.byref(planes), int(texel_stride), C.c_void_p(stream)))


def _multi_device_planes(struct, visibility_ptrs, direct_ptrs, **single):
    """The structure of device pointers of a pass under extra lights: up to ``abi.MAX_LIGHTS`` pointers per per-light member (light
    k's plane at index k, 0 = not wanted), one per other member; all 0 raises."""
    planes = struct()
    for name, ptrs in (("visibility", visibility_ptrs), ("direct", direct_ptrs)):
        ptrs = tuple(int(p or 0) for p in ptrs)
        if len(ptrs) > abi.MAX_LIGHTS:
            raise ValueError(f"{name}_ptrs takes at most {abi.MAX_LIGHTS} pointers, one per light")
        for k, p in enumerate(ptrs):
            getattr(planes, name)[k] = p or None
    for name, p in single.items():
        setattr(planes, name, int(p or 0) or None)
    if not any(visibility_ptrs) and not any(direct_ptrs) and not any(single.values()):
        raise ValueError("give at least one of visibility_ptrs, direct_ptrs, " + ", ".join(f"{k}_ptr" for k in single))
    return planes


def render_light_multi_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, visibility_ptrs: Sequence[int] = (),
                                    direct_ptrs: Sequence[int] = (), occlusion_ptr: int = 0, combined_ptr: int = 0,
                                    frame_stride_pixels: Optional[int] = None, stream: int = 0) -> None:
    """The per-light light planes of N resident scenes of one config in one launch per kernel
    (mcrt_render_light_multi_batch_device): ``visibility_ptrs[k]`` / ``direct_ptrs[k]`` take light k's plane (0: the scene's own
    light, 1..: the handle's extra lights; a light a handle lacks: the miss constants), ``combined_ptr`` the clamped sum.  Frame i
    of each plane starts ``i * frame_stride_pixels`` pixels on.  The handles may carry different lights and may be listed more
    than once.  Asynchronous on ``stream``."""
    handles = _handles(device_scenes)
    planes = _multi_device_planes(abi.McrtLightPlanesMulti, visibility_ptrs, direct_ptrs, occlusion=occlusion_ptr, combined=combined_ptr)
    stride = _frame_stride(config, frame_stride_pixels)
    c = config.to_c()
    check(load().mcrt_render_light_multi_batch_device(_handle_array(handles), len(handles), C.byref(c), C.byref(planes), stride, C.c_void_p(stream)))


def bake_light_multi_batch_device(device_scenes: Sequence["DeviceScene"], config: Config, grid: int = 1, position_ptr: int = 0, normal_ptr: int = 0,
                                  visibility_ptrs: Sequence[int] = (), occlusion_ptr: int = 0, direct_ptrs: Sequence[int] = (), combined_ptr: int = 0,
                                  texel_stride: Optional[int] = None, stream: int = 0) -> None:
    """The per-light light bakes of N resident scenes in one launch per kernel (mcrt_bake_light_multi_batch_device): the planes of
    ``bake_light_batch_device`` with one visibility and one direct plane per light and ``combined_ptr``, the mean of the
    sub-samples' clamped sums.  Frame i starts ``i * texel_stride`` texels on (default: the largest ``texels`` of the scenes)."""
    handles = _handles(device_scenes)
    planes = _multi_device_planes(abi.McrtBakePlanesMulti, visibility_ptrs, direct_ptrs, position=position_ptr, normal=normal_ptr,
                                  occlusion=occlusion_ptr, combined=combined_ptr)
    g = _bake_grid(grid)
    if texel_stride is None:
        texel_stride = max([s.texels for s in device_scenes], default=0)
    if int(texel_stride) < 0:
        raise ValueError("texel_stride must be >= 0")
    c = config.to_c()
    check(load().mcrt_bake_light_multi_batch_device(_handle_array(handles), len(handles), C.byref(c), g, C.byref(planes), int(texel_stride),
                                                    C.c_void_p(stream)))


def set_skins_batch_device(device_scenes: Sequence["DeviceScene"], ptr: int, skin_stride_bytes: Optional[int] = None, stream: int = 0) -> None:
    """One launch repaints N repaintable scenes that take images of one size — ``"S64"`` and ``"S64S"`` scenes may be mixed —
    (mcrt_scene_set_skins_batch_device): skin i is the RGBA8 image
    at ``ptr + i * skin_stride_bytes`` in device memory (default: the image size, 64 * height * 4).  Asynchronous on ``stream``."""
    handles = _handles(device_scenes)
    n = len(handles)
    if skin_stride_bytes is None:
        skin_stride_bytes = device_scenes[0]._skin_bytes() if n else 64 * 64 * 4
    arr = _handle_array(handles)
    check(load().mcrt_scene_set_skins_batch_device(arr, n, C.c_void_p(ptr or None), int(skin_stride_bytes), C.c_void_p(stream)))


def set_capes_batch_device(device_scenes: Sequence["DeviceScene"], ptr: int, cape_stride_bytes: int = 8192, stream: int = 0) -> None:
    """One launch repaints the capes of N caped scenes (mcrt_scene_set_capes_batch_device): cape i is the 64x32 RGBA8 image at
    ``ptr + i * cape_stride_bytes`` in device memory; a stride of 0: one image for all; ``ptr`` 0: every cape transparent.
    Asynchronous on ``stream``."""
    handles = _handles(device_scenes)
    arr = _handle_array(handles)
    check(load().mcrt_scene_set_capes_batch_device(arr, len(handles), C.c_void_p(ptr or None), int(cape_stride_bytes), C.c_void_p(stream)))


def set_views_batch_device(device_scenes: Sequence["DeviceScene"], poses=None, looks=None, stream: int = 0, cape_angles=None) -> None:
    """One launch gives N repaintable scenes of one image size their views (mcrt_scene_set_views_batch_device): ``poses`` — N
    poses of 12 floats, or ``None``: every scene keeps its own; ``looks`` — N entries, each a ``Scene`` / ``SceneDesc`` or
    ``None`` (that scene keeps its look), or ``None`` for all.  Asynchronous on ``stream``; the arguments are read before the
    call returns.  ``cape_angles`` (caped scenes): N cape angles, or ``None``: every scene keeps its own."""
    handles = _handles(device_scenes)
    n = len(handles)
    angles = None
    if cape_angles is not None:
        angles = np.ascontiguousarray(cape_angles, np.float32)
        if angles.shape != (n,):
            raise ValueError(f"cape_angles must hold {n} floats: one angle per scene")
    p = None
    if poses is not None:
        p = np.ascontiguousarray(poses, np.float32)
        if p.shape != (n, 12):
            raise ValueError(f"poses must be ({n}, 12) floats: one pose per scene")
    descs = None
    if looks is not None:
        looks = list(looks)
        if len(looks) != n:
            raise ValueError(f"looks must hold {n} entries: one look (or None) per scene")
        descs = [_as_desc(k) if k is not None else None for k in looks]
    arr = _handle_array(handles)
    look_arr = None
    if descs is not None:
        ptrs = [d.ptr if d is not None else None for d in descs]  # (kept alive until the call has returned)
        look_arr = (C.POINTER(abi.McrtSceneDesc) * max(n, 1))(*[C.cast(q, C.POINTER(abi.McrtSceneDesc)) if q is not None else C.POINTER(abi.McrtSceneDesc)() for q in ptrs])
    if angles is not None:
        check(load().mcrt_scene_set_views_cape_batch_device(arr, n, p.ctypes.data_as(C.c_void_p) if p is not None and n else None, look_arr,
                                                            angles.ctypes.data_as(C.c_void_p) if n else None, C.c_void_p(stream)))
        return
    check(load().mcrt_scene_set_views_batch_device(arr, n, p.ctypes.data_as(C.c_void_p) if p is not None and n else None, look_arr, C.c_void_p(stream)))


class SkinBatch:
    """The farm case: ``n`` repaintable scenes of one skin kind, pose and look resident on ``device``, and a skin buffer there.
    ``render(skins, config)`` gives the frames of ``m <= n`` skins with ONE upload (the images, 16 KB each), one repaint launch,
    one ``render_batch_device`` call and one download — what ``TileRenderer.renderBatch([MeshBuilder.buildScene(s, pose) ...])``
    returns, bit for bit, without building, flattening and uploading a scene per skin.  Device memory through torch.
    ``slim=True`` (``"S64"`` only): every slot also keeps a scene of the slim model, and ``render`` / ``shots`` / ``layers`` take
    ``models`` — ``None``: all classic; ``"auto"``: ``skin_model`` of each image; or one of ``"classic"`` / ``"slim"`` per skin —
    and repaint the chosen scenes of a mixed batch in the same ONE launch."""

    def __init__(self, n: int, kind, pose: Optional[Sequence[float]] = None, look=None, device: int = 0, slim: bool = False, cape: bool = False,
                 cape_angle: float = 10.0):
        import torch

        self.kind_height = _skin_height(kind)
        if slim and self.kind_height != 64:
            raise ValueError("the slim model exists for 64x64 skins only")
        self.device = int(device)
        self.cape = bool(cape)
        self._torch = torch
        self.scenes: List[DeviceScene] = []
        self.slim_scenes: List[DeviceScene] = []  # slot i's scene of the slim model (slim=True), else empty
        try:
            for _ in range(int(n)):
                self.scenes.append(DeviceScene.for_skin(self.kind_height, pose, look, device, cape=self.cape, cape_angle=cape_angle))
            for _ in range(int(n) if slim else 0):
                self.slim_scenes.append(DeviceScene.for_skin("S64S", pose, look, device, cape=self.cape, cape_angle=cape_angle))
        except Exception:
            self.close()
            raise
        self._dev = torch.device("cuda", self.device)
        self._skins = torch.zeros((max(int(n), 1), self.kind_height, 64, 4), dtype=torch.uint8, device=self._dev)
        self._staging = torch.zeros(self._skins.shape, dtype=torch.uint8).pin_memory()
        if self.cape:  # the cape images, beside the skins'
            self._capes = torch.zeros((max(int(n), 1),) + CAPE_SHAPE, dtype=torch.uint8, device=self._dev)
            self._cape_staging = torch.zeros(self._capes.shape, dtype=torch.uint8).pin_memory()
        self._out = {}  # (bytes per frame) -> device buffer, pinned host buffer
        self._mode = None

    def close(self) -> None:
        for s in self.scenes + self.slim_scenes:
            s.close()
        self.scenes, self.slim_scenes = [], []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_extra_lights(self, lights) -> None:
        """The same extra lights (``DeviceScene.set_extra_lights``) for every scene of the batch; ``render`` then enqueues each
        frame on its own (``render_batch_device`` sends such frames through the single-frame path), and ``shots`` refuses."""
        for s in self.scenes + self.slim_scenes:
            s.set_extra_lights(lights)

    def set_views(self, poses=None, looks=None, cape_angles=None) -> None:
        """Another pose and / or look for the batch's scenes without rebuilding them (``set_views_batch_device``): ``poses`` —
        one pose of 12 floats for all scenes, or one per scene (n, 12); ``looks`` — one ``Scene`` / ``SceneDesc`` for all, or a
        sequence of n (entries may be ``None``); ``None`` keeps what the scenes have.  On the current torch stream, ahead of the
        next ``render`` / ``layers``.  ``cape_angles`` (a caped batch): one angle for all, or one per scene."""
        n = len(self.scenes)
        if cape_angles is not None:
            if not self.cape:
                raise ValueError("this batch holds no capes: create it with cape=True")
            c = np.asarray(cape_angles, np.float32)
            if c.shape == ():
                c = np.full((n,), c, np.float32)
            elif c.shape != (n,):
                raise ValueError(f"cape_angles must be one angle or ({n},)")
            cape_angles = c
        if poses is not None:
            p = np.ascontiguousarray(poses, np.float32)
            if p.shape == (12,):
                p = np.tile(p, (n, 1))
            elif p.shape != (n, 12):
                raise ValueError(f"poses must be one pose of 12 floats or ({n}, 12)")
            poses = p
        if looks is not None:
            looks = [looks] * n if isinstance(looks, (Scene, SceneDesc)) else list(looks)
            if len(looks) != n:
                raise ValueError(f"looks must be one look or {n} of them")
        if n == 0 or (poses is None and looks is None and cape_angles is None):
            return
        if self.slim_scenes:  # both scenes of every slot, in the one launch
            poses = np.concatenate([poses, poses]) if poses is not None else None
            looks = looks + looks if looks is not None else None
            cape_angles = np.concatenate([cape_angles, cape_angles]) if cape_angles is not None else None
        with self._torch.cuda.device(self._dev):
            set_views_batch_device(self.scenes + self.slim_scenes, poses, looks, stream=self._torch.cuda.current_stream().cuda_stream, cape_angles=cape_angles)

    def _check_skins(self, skins) -> np.ndarray:
        a = np.ascontiguousarray(skins, np.uint8)
        if a.ndim != 4 or a.shape[1:] != (self.kind_height, 64, 4) or len(a) > len(self.scenes):
            raise ValueError(f"skins must be (m <= {len(self.scenes)}, {self.kind_height}, 64, 4) uint8")
        return a

    def _chosen(self, a, models) -> List[DeviceScene]:
        """Slot i's scene for skin i: the classic one, or the slim one where ``models`` says so."""
        m = len(a)
        if models is None:
            return self.scenes[:m]
        names = [skin_model(k) for k in a] if isinstance(models, str) and models == "auto" else list(models)
        if len(names) != m or any(k not in ("classic", "slim") for k in names):
            raise ValueError(f"models must be None, 'auto' or {m} entries 'classic' / 'slim': one per skin")
        if "slim" in names and not self.slim_scenes:
            raise ValueError("this batch holds no slim scenes: create it with slim=True")
        return [self.slim_scenes[i] if k == "slim" else self.scenes[i] for i, k in enumerate(names)]

    def _check_capes(self, capes, m: int) -> Optional[np.ndarray]:
        """The cape images of the ``m`` skins as (m, 32, 64, 4), a ``None`` entry zeros (no cape); ``None`` on a capeless batch."""
        if not self.cape:
            if capes is not None:
                raise ValueError("this batch holds no capes: create it with cape=True")
            return None
        out = np.zeros((m,) + CAPE_SHAPE, np.uint8)
        if capes is not None:
            capes = list(capes)
            if len(capes) != m:
                raise ValueError(f"capes must hold {m} entries: one image (or None) per skin")
            for i, c in enumerate(capes):
                if c is not None:
                    out[i] = _cape_image(c)
        return out

    def _paint(self, skins, stream, models=None, capes=None) -> List[DeviceScene]:
        """Uploads and repaints; returns the scenes that now hold the skins.  Every caller synchronises `stream` before it
        returns (the pinned staging buffer is reused)."""
        torch = self._torch
        a = self._check_skins(skins)
        chosen = self._chosen(a, models)
        m = len(a)
        c = self._check_capes(capes, m)
        if m and c is not None:  # one upload and one launch beside the skins'
            self._cape_staging[:m].numpy()[...] = c
            with torch.cuda.stream(stream):
                self._capes[:m].copy_(self._cape_staging[:m], non_blocking=True)
            set_capes_batch_device(chosen, self._capes.data_ptr(), stream=stream.cuda_stream)
        if m:
            self._staging[:m].numpy()[...] = a
            with torch.cuda.stream(stream):
                self._skins[:m].copy_(self._staging[:m], non_blocking=True)
            set_skins_batch_device(chosen, self._skins.data_ptr(), stream=stream.cuda_stream)
        return chosen

    def _buffers(self, key, shape, dtype):
        torch = self._torch
        got = self._out.get(key)
        if got is None or got[0].shape != shape or got[0].dtype != dtype:
            got = (torch.empty(shape, dtype=dtype, device=self._dev), torch.empty(shape, dtype=dtype).pin_memory())
            self._out[key] = got
        return got

    def render(self, skins, config: Config, rgba8: bool = False, background: str = "reference", models=None, capes=None) -> np.ndarray:
        """``skins``: (m <= n, H, 64, 4) uint8.  Returns (m, height, width, 4) float32, or uint8 with ``rgba8``.  ``capes`` (a
        batch created with ``cape=True``): m entries, each a (32, 64, 4) uint8 cape image or ``None`` for no cape; ``None``: no
        capes at all."""
        torch = self._torch
        mode = abi.background_mode(background)
        w, h, no_frame = _frame(config)
        with torch.cuda.device(self._dev):
            stream = torch.cuda.current_stream()
            if no_frame:  # nothing is painted either (the staging buffer stays idle)
                return _default_frames(len(self._check_skins(skins)), h, w, rgba8)
            chosen = self._paint(skins, stream, models, capes)
            m = len(chosen)
            dtype = torch.uint8 if rgba8 else torch.float32
            if m == 0:
                return _default_frames(0, h, w, rgba8)
            if mode != self._mode:
                for s in self.scenes + self.slim_scenes:
                    s.set_background(background)
                self._mode = mode
            dev, host = self._buffers("frames", (len(self.scenes), h, w, 4), dtype)
            render_batch_device(chosen, config, 0 if rgba8 else dev.data_ptr(), dev.data_ptr() if rgba8 else 0, w * h, stream.cuda_stream)
            with torch.cuda.stream(stream):
                host[:m].copy_(dev[:m], non_blocking=True)
            stream.synchronize()
            return host[:m].numpy().copy()

    def shots(self, skins, config: Config, shot: Optional[abi.Shot] = None, ground=0.0, rgba8: bool = True, bounds: bool = False, models=None, capes=None):
        """The studio shots of the ``m`` skins (``TileRenderer.renderShotBatch`` of the scenes built per skin, bit for bit): one
        upload, one repaint, one ``render_shot_batch_device`` call — render, ground, reflection and blend on the device — and
        one download of 4 B/pixel (16 with ``rgba8=False``).  ``ground``: one height for all (0.0: the soles of the builder's
        standing figure), or ``m`` heights.  The scenes' background mode (``render``'s) is not touched.  ``bounds=True``
        (``Shot(page="transparent")`` only): the pair (images, (m, 4) int32 boxes {x0, y0, x1, y1}), the boxes written by the
        blend and downloaded with the images."""
        torch = self._torch
        w, h, no_frame = _frame(config)
        with torch.cuda.device(self._dev):
            stream = torch.cuda.current_stream()
            if no_frame:  # nothing is painted either
                out = _default_frames(len(self._check_skins(skins)), h, w, rgba8)
                return (out, _empty_bounds(len(out), w, h)) if bounds else out
            a = self._check_skins(skins)
            if ground is None:
                raise ValueError("ground heights are needed: a resident scene does not keep its description")
            heights = _ground_heights(list(range(len(a))), ground)
            need = shot_scratch_bytes(config, shot, len(self.scenes), bounds)  # (raises nothing: an invalid shot is refused by the call below)
            chosen = self._paint(a, stream, models, capes)
            m = len(chosen)
            if m == 0:
                none = _default_frames(0, h, w, rgba8)
                return (none, _empty_bounds(0, w, h)) if bounds else none
            scratch = self._out.get("shot_scratch")
            if scratch is None or scratch.numel() < need:
                scratch = torch.empty((max(need, 16),), dtype=torch.uint8, device=self._dev)
                self._out["shot_scratch"] = scratch
            dev, host = self._buffers("shots", (len(self.scenes), h, w, 4), torch.uint8 if rgba8 else torch.float32)
            box_dev, box_host = self._buffers("shot_bounds", (len(self.scenes), 4), torch.int32) if bounds else (None, None)
            try:
                render_shot_batch_device(chosen, config, shot, heights, scratch.data_ptr(), scratch.numel(), 0 if rgba8 else dev.data_ptr(),
                                         dev.data_ptr() if rgba8 else 0, w * h, stream.cuda_stream, box_dev.data_ptr() if bounds else 0)
                with torch.cuda.stream(stream):
                    host[:m].copy_(dev[:m], non_blocking=True)
                    if bounds:
                        box_host[:m].copy_(box_dev[:m], non_blocking=True)
            finally:
                stream.synchronize()  # (a refused shot too: the repaint reads the pinned staging buffer)
            return (host[:m].numpy().copy(), box_host[:m].numpy().copy()) if bounds else host[:m].numpy().copy()

    def layers(self, skins, config: Config, layers=abi.LAYER_NAMES, models=None, capes=None) -> dict:
        """The geometry layers of the ``m`` skins' frames (``TileRenderer.renderLayersBatch``'s planes) through
        ``render_layers_batch_device``, behind the repaint on the same stream."""
        torch = self._torch
        names = abi.LAYERS.select(layers)
        w, h, no_frame = _frame(config)
        with torch.cuda.device(self._dev):
            stream = torch.cuda.current_stream()
            if no_frame:  # nothing is painted either
                return {k: abi.LAYERS.empty(k, len(self._check_skins(skins)), h, w) for k in names}
            chosen = self._paint(skins, stream, models, capes)
            m = len(chosen)
            if m == 0:
                return {k: abi.LAYERS.empty(k, 0, h, w) for k in names}
            n = len(self.scenes)
            bufs = {}
            for k in names:
                dtype, comps = abi.LAYERS.formats[k]
                shape = (n, h, w) + ((comps,) if comps > 1 else ())
                bufs[k] = self._buffers(k, shape, torch.int32 if dtype is np.int32 else torch.float32)
            render_layers_batch_device(chosen, config, frame_stride_pixels=w * h, stream=stream.cuda_stream,
                                       **{f"{k}_ptr": bufs[k][0].data_ptr() for k in names})
            with torch.cuda.stream(stream):
                for k in names:
                    bufs[k][1][:m].copy_(bufs[k][0][:m], non_blocking=True)
            stream.synchronize()
            return {k: bufs[k][1][:m].numpy().copy() for k in names}


def last_batch_info() -> dict:
    """mcrt_last_batch_info: ``{"batched_frames": ..., "launch_sequences": ...}`` of the last batch call on this thread."""
    f, q = C.c_int(), C.c_int()
    load().mcrt_last_batch_info(C.byref(f), C.byref(q))
    return {"batched_frames": int(f.value), "launch_sequences": int(q.value)}


def _plate_info(symbol: str, device: int) -> dict:
    fn = getattr(load(), symbol)  # bound here: a build selected with MCRT_LIB may predate it
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    n, b, k = C.c_int(), C.c_size_t(), C.c_int()
    check(fn(int(device), C.byref(n), C.byref(b), C.byref(k)))
    return {"plates": int(n.value), "bytes": int(b.value), "builds": int(k.value)}


def bg_plate_info(device: int = 0) -> dict:
    """mcrt_bg_plate_info: ``{"plates": ..., "bytes": ..., "builds": ...}`` — the background plates kept on ``device``, their
    bytes, and how many were built there since the process began (include/mcrt.h, "Background plates")."""
    return _plate_info("mcrt_bg_plate_info", device)


def draw_plate_info(device: int = 0) -> dict:
    """mcrt_draw_plate_info: ``{"plates": ..., "bytes": ..., "builds": ...}`` — the draw plates kept on ``device``, their
    bytes, and how many were built there since the process began (include/mcrt.h, "Draw plates")."""
    return _plate_info("mcrt_draw_plate_info", device)


def sample_table_info(device: int = 0) -> dict:
    """mcrt_sample_table_info: ``{"bytes": ..., "builds": ...}`` — the bytes of the sample table kept on ``device`` (0: none) and
    how often it was built there since the process began (include/mcrt.h, "Sample table")."""
    fn = load().mcrt_sample_table_info  # bound here: a build selected with MCRT_LIB may predate it
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    b, k = C.c_size_t(), C.c_int()
    check(fn(int(device), C.byref(b), C.byref(k)))
    return {"bytes": int(b.value), "builds": int(k.value)}


TABLE_NAMES = ("window", "full", "sample")  # MCRT_TABLE_WINDOW, MCRT_TABLE_FULL, MCRT_TABLE_SAMPLE


def device_tables_info(device: int = 0) -> dict:
    """mcrt_device_tables_info: ``{"window": {"bytes": ..., "builds": ...}, "full": {...}, "sample": {...}}`` — per table kept on
    ``device`` its bytes (0: none) and how often it was built there since the process began (include/mcrt.h)."""
    fn = load().mcrt_device_tables_info  # bound here: a build selected with MCRT_LIB may predate it
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    out = {}
    for which, name in enumerate(TABLE_NAMES):
        b, k = C.c_size_t(), C.c_int()
        check(fn(int(device), which, C.byref(b), C.byref(k)))
        out[name] = {"bytes": int(b.value), "builds": int(k.value)}
    return out


def probe_seed_words(seeds: Sequence[int], which: str = "window", device: int = 0) -> np.ndarray:
    """uint32[n]: the words of the device's window seed table (``which="window"``: seeds in -2^24 .. 2^24-1) or of its table
    of all seeds (``which="full"``: any 32-bit seed) for ``seeds``; the table is built if the device has none (mcrt.h)."""
    if which not in TABLE_NAMES[:2]:
        raise ValueError(f"which must be one of {TABLE_NAMES[:2]}, not {which!r}")
    s = np.asarray(seeds, np.int64).ravel()
    lo, hi = (-(1 << 24), (1 << 24) - 1) if which == "window" else (0, (1 << 32) - 1)
    if len(s) and (s.min() < lo or s.max() > hi):
        raise ValueError(f"a seed outside {lo} .. {hi}")
    s = np.ascontiguousarray((s & 0xFFFFFFFF).astype(np.uint32))
    out = np.zeros(len(s), np.uint32)
    fn = load().mcrt_probe_seed_words  # bound here: a build selected with MCRT_LIB may predate it
    u32_p = C.POINTER(C.c_uint32)
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, u32_p, C.c_int, u32_p]
    check(fn(int(device), TABLE_NAMES.index(which), s.ctypes.data_as(u32_p), len(s), out.ctypes.data_as(u32_p)))
    return out


def unpack_rows_device(config: Config, first: int, step: int, packed_ptr: int, frame_ptr: int, stream: int = 0) -> None:
    c = config.to_c()
    check(load().mcrt_unpack_rows_device(C.byref(c), first, step, C.c_void_p(packed_ptr), C.c_void_p(frame_ptr), C.c_void_p(stream)))


def assemble_frame_device(config: Config, world: int, gathered_ptr: int, rank_stride_pixels: int, frame_ptr: int,
                          stream: int = 0) -> None:
    """All ranks' packed rows (one contiguous [world, packed_rows, W, 4] buffer) → the frame, one launch."""
    c = config.to_c()
    check(load().mcrt_assemble_frame_device(C.byref(c), world, C.c_void_p(gathered_ptr), rank_stride_pixels,
                                            C.c_void_p(frame_ptr), C.c_void_p(stream)))


def quantize_rgba8_device(rgba_ptr: int, out_ptr: int, n_pixels: int, stream: int = 0) -> None:
    check(load().mcrt_quantize_rgba8_device(C.c_void_p(rgba_ptr), C.c_void_p(out_ptr), n_pixels, C.c_void_p(stream)))


def probe_mt_uniform(seeds: Sequence[int], n_draws: int, device: int = 0) -> np.ndarray:
    s = np.asarray(seeds, np.uint32)
    out = np.zeros((len(s), n_draws), np.float32)
    check(load().mcrt_probe_mt_uniform(device, s.ctypes.data_as(C.POINTER(C.c_uint32)), len(s), n_draws, abi.fptr(out)))
    return out


def probe_sample_rows(seeds: Sequence[int], device: int = 0) -> np.ndarray:
    """(n, 8, 4) float32: the rows {cos, sin, sqrt, 0} of the device's sample table for seeds in -2^22 .. 2^22-1 (mcrt.h)."""
    s = np.asarray(seeds, np.int32)
    out = np.zeros((len(s), 8, 4), np.float32)
    fn = load().mcrt_probe_sample_rows  # bound here: a build selected with MCRT_LIB may predate it
    fn.restype, fn.argtypes = C.c_int, [C.c_int, abi.c_int32_p, C.c_int, abi.c_float_p]
    check(fn(device, s.ctypes.data_as(abi.c_int32_p), len(s), abi.fptr(out)))
    return out


def probe_detmath(op: int, x: np.ndarray, y: Optional[np.ndarray] = None, device: int = 0) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    yy = np.ascontiguousarray(y, np.float32) if y is not None else None
    out = np.zeros_like(x)
    check(load().mcrt_probe_detmath(device, op, abi.fptr(x), abi.fptr(yy) if yy is not None else None, x.size, abi.fptr(out)))
    return out


def probe_detmath_range(op: int, lo_bits: int, hi_bits: int, y0: float = 0.0, device: int = 0) -> int:
    bad = C.c_uint64()
    check(load().mcrt_probe_detmath_range(device, op, lo_bits, hi_bits, C.c_float(y0), C.byref(bad)))
    return int(bad.value)


def probe_div_const(d_first: int, d_count: int, two_corrections: bool = False, device: int = 0, mode: Optional[int] = None):
    """(mismatches, a failing divisor or 0): rt::div_frame against the general division, exhaustively (mcrt.h).
    ``mode``: 0 the adopted form, 1 with a second correction, 2 the uncorrected product (the probe's own check: must
    mismatch), 3 rt::sqrt_pos against sqrtf, 4 the device's 1.0f / d against the host's reciprocal the kernels are given."""
    bad, which = C.c_uint64(), C.c_uint32()
    m = (1 if two_corrections else 0) if mode is None else int(mode)
    check(load().mcrt_probe_div_const(device, d_first, d_count, m, C.byref(bad), C.byref(which)))
    return int(bad.value), int(which.value)


def flatten(scene) -> bytes:
    d = _as_desc(scene)
    lib = load()
    n = lib.mcrt_scene_flatten(d.ptr, None, 0)
    if n == 0:
        raise McrtError(abi.MCRT_ERR_INVALID, lib.mcrt_last_error().decode("utf-8", "replace"))
    buf = C.create_string_buffer(n)
    lib.mcrt_scene_flatten(d.ptr, buf, n)
    return buf.raw
