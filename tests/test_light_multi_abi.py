"""The light layers and the light bake under extra lights (mcrt_render_light_multi*, mcrt_bake_light_multi*) without a device: the
symbols, the structures, every argument check that comes before any device work with the planes untouched, and the no-ops.

The device forms are given opaque handle values, or zeroed blocks in which only the first three words of a handle are set —
device, skin_height, n_texels: every case fails, or is a no-op, on a check that does not look further inside a handle."""
import ctypes as C
import os

import numpy as np
import pytest

import bake_checker as B
from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_render_light_multi_device", "mcrt_render_light_multi_batch_device", "mcrt_render_light_multi",
               "mcrt_bake_light_multi_device", "mcrt_bake_light_multi_batch_device", "mcrt_bake_light_multi")
M = abi.MAX_LIGHTS


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**{"width": 16, "height": 8, **kw}).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _block(device=0, skin_height=0, n_texels=0):
    b = (C.c_int32 * 4096)()
    b[0], b[1], b[2] = device, skin_height, n_texels
    return b


def _light_planes(occlusion=True, lights=True):
    p = abi.McrtLightPlanesMulti()
    if lights:
        for k in range(M):
            p.visibility[k], p.direct[k] = 0x1000 * (k + 1), 0x10000 * (k + 1)
        p.combined = 0x200000
    p.occlusion = 0x100000 if occlusion else None
    return p


def _bake_planes(occlusion=True, lights=True, geometry=True):
    p = abi.McrtBakePlanesMulti()
    if geometry:
        p.position, p.normal = 0x300000, 0x400000
    if lights:
        for k in range(M):
            p.visibility[k], p.direct[k] = 0x1000 * (k + 1), 0x10000 * (k + 1)
        p.combined = 0x200000
    p.occlusion = 0x100000 if occlusion else None
    return p


def _invalid(lib, rc):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def test_symbols_structures_and_wrappers(lib, mcrt):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
    assert M == 4 == 1 + abi.MAX_EXTRA_LIGHTS
    assert C.sizeof(abi.McrtLightPlanesMulti) == 10 * 8 and C.sizeof(abi.McrtBakePlanesMulti) == 12 * 8
    assert [f[0] for f in abi.McrtLightPlanesMulti._fields_] == ["visibility", "direct", "occlusion", "combined"]
    assert [f[0] for f in abi.McrtBakePlanesMulti._fields_] == ["position", "normal", "visibility", "occlusion", "direct", "combined"]
    assert abi.McrtLightPlanesMulti.direct.offset == 32 and abi.McrtLightPlanesMulti.occlusion.offset == 64
    assert abi.McrtBakePlanesMulti.visibility.offset == 16 and abi.McrtBakePlanesMulti.occlusion.offset == 48 and abi.McrtBakePlanesMulti.combined.offset == 88
    assert abi.LIGHT_MULTI_NAMES == ("visibility", "direct", "occlusion", "combined")
    assert abi.BAKE_MULTI_NAMES == ("position", "normal", "visibility", "occlusion", "direct", "combined")
    assert list(abi.FAMILIES) == ["layers", "ground", "ground_occlusion", "reflection", "light", "bake"]  # the single-pointer families stay six
    for name in ("render_light_multi_batch_device", "bake_light_multi_batch_device"):
        assert name in mcrt.__all__ and callable(getattr(mcrt, name))
    for fn in (mcrt.TileRenderer.renderLightMulti, mcrt.TileRenderer.bakeLightMulti, mcrt.DeviceScene.render_light_multi_device,
               mcrt.DeviceScene.bake_light_multi_device):
        assert callable(fn)


def test_the_header_declares_the_entry_points():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert "#define MCRT_MAX_LIGHTS (1 + MCRT_MAX_EXTRA_LIGHTS)" in header
    assert "typedef struct mcrt_light_planes_multi {" in header and "typedef struct mcrt_bake_planes_multi {" in header
    assert "light layers and bake under extra lights" in header and "NOT the clamp of the means" in header


BAD_CONFIGS = {"shadow_samples_114": dict(shadowSamples=114)}
BAD_WITH_OCCLUSION = {"ao_samples_0": dict(aoSamples=0), "ao_samples_114": dict(aoSamples=114), "ao_radius_nan": dict(aoRadius=float("nan")),
                      "ao_radius_inf": dict(aoRadius=float("inf"))}
BAD_GRIDS = {"grid_0": 0, "grid_5": 5, "grid_negative": -1}
COMMON = ["n_negative", "null_cfg", "null_array", "null_entry", "null_planes", "all_planes_null", "stride_too_small", "other_device", *BAD_CONFIGS,
          *BAD_WITH_OCCLUSION]


@pytest.mark.parametrize("family", ["light", "bake"])
@pytest.mark.parametrize("case", COMMON + list(BAD_GRIDS))
def test_batch_device_forms_reject_bad_arguments(lib, family, case):
    bake = family == "bake"
    if case in BAD_GRIDS and not bake:
        return  # a frame pass has no grid
    cfg = _cfg()
    planes = _bake_planes() if bake else _light_planes()
    blocks = [_block(0, 0, 100), _block(0, 0, 200)]
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=C.byref(cfg), grid=2, out=C.byref(planes), stride=4096)
    if case == "n_negative":
        a["n"] = -1
    elif case == "null_cfg":
        a["cfg"] = None
    elif case == "null_array":
        a["scenes"] = None
    elif case == "null_entry":
        a["scenes"] = _handles(0x10, None)
    elif case == "null_planes":
        a["out"] = None
    elif case == "all_planes_null":
        planes = abi.McrtBakePlanesMulti() if bake else abi.McrtLightPlanesMulti()
        a["out"] = C.byref(planes)
    elif case == "stride_too_small":  # a bake: below the second scene's 200 texels; a frame pass: below 16 x 8 pixels
        a["scenes"], a["stride"] = _handles(*[C.addressof(b) for b in blocks]), 199 if bake else 127
    elif case == "other_device":
        blocks[1][0] = 1
        a["scenes"] = _handles(*[C.addressof(b) for b in blocks])
    elif case in BAD_GRIDS:
        a["grid"] = BAD_GRIDS[case]
    else:
        cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        a["cfg"] = C.byref(cfg)
    if bake:
        rc = lib.mcrt_bake_light_multi_batch_device(a["scenes"], a["n"], a["cfg"], a["grid"], a["out"], a["stride"], None)
    else:
        rc = lib.mcrt_render_light_multi_batch_device(a["scenes"], a["n"], a["cfg"], a["out"], a["stride"], None)
    _invalid(lib, rc)
    if case == "stride_too_small":
        assert (b"texel_stride" if bake else b"frame_stride_pixels") in lib.mcrt_last_error()
    if case == "other_device":
        assert b"one device" in lib.mcrt_last_error()


@pytest.mark.parametrize("family", ["light", "bake"])
@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "all_planes_null", *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_single_device_forms_reject_bad_arguments(lib, family, case):
    bake = family == "bake"
    cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}.get(case, {}))
    planes = _bake_planes() if bake else _light_planes()
    if case == "all_planes_null":
        planes = abi.McrtBakePlanesMulti() if bake else abi.McrtLightPlanesMulti()
    h = None if case == "null_handle" else C.c_void_p(0x10)
    c = None if case == "null_cfg" else C.byref(cfg)
    out = None if case == "null_planes" else C.byref(planes)
    _invalid(lib, lib.mcrt_bake_light_multi_device(h, c, 1, out, None) if bake else lib.mcrt_render_light_multi_device(h, c, out, None))


def test_without_the_occlusion_plane_the_ao_fields_are_not_read_and_the_no_ops(lib):
    empty = _block()
    one = _handles(C.addressof(empty))
    for kw in BAD_WITH_OCCLUSION.values():
        cfg = _cfg(**kw)
        p = _bake_planes(occlusion=False)
        assert lib.mcrt_bake_light_multi_batch_device(one, 1, C.byref(cfg), 1, C.byref(p), 0, None) == MCRT_OK, kw  # no texel: nothing to do
        p = _bake_planes(lights=False, geometry=False)  # the occlusion plane alone
        _invalid(lib, lib.mcrt_bake_light_multi_batch_device(one, 1, C.byref(cfg), 1, C.byref(p), 0, None))
        zero = _cfg(width=0, **kw)
        q = _light_planes(occlusion=False)
        assert lib.mcrt_render_light_multi_batch_device(_handles(0x10), 1, C.byref(zero), C.byref(q), 0, None) == MCRT_OK, kw  # zero-size frame
        q = _light_planes(lights=False)
        _invalid(lib, lib.mcrt_render_light_multi_batch_device(_handles(0x10), 1, C.byref(zero), C.byref(q), 0, None))
    # hard shadows take any sample count; 113 soft samples are the limit
    for kw, rc in ((dict(shadowSamples=113), MCRT_OK), (dict(shadowSamples=114, softShadows=False), MCRT_OK), (dict(shadowSamples=114), MCRT_ERR_INVALID)):
        cfg, p, q = _cfg(width=0, **kw), _bake_planes(), _light_planes()
        assert lib.mcrt_bake_light_multi_device(C.c_void_p(C.addressof(empty)), C.byref(cfg), 4, C.byref(p), None) == rc, kw
        assert lib.mcrt_render_light_multi_device(C.c_void_p(0x10), C.byref(cfg), C.byref(q), None) == rc, kw
    # zero-size frames and n_frames = 0
    p, q = _bake_planes(), _light_planes()
    for kw in (dict(width=0), dict(height=0), dict(tileSize=0), dict(width=-3)):
        cfg = _cfg(**kw)
        assert lib.mcrt_render_light_multi_device(C.c_void_p(0x10), C.byref(cfg), C.byref(q), None) == MCRT_OK, kw
        assert lib.mcrt_render_light_multi_batch_device(_handles(0x10, 0x10), 2, C.byref(cfg), C.byref(q), 0, None) == MCRT_OK, kw
    cfg = _cfg()
    assert lib.mcrt_render_light_multi_batch_device(None, 0, C.byref(cfg), C.byref(q), 0, None) == MCRT_OK
    assert lib.mcrt_bake_light_multi_batch_device(None, 0, C.byref(cfg), 1, C.byref(p), 0, None) == MCRT_OK
    assert lib.mcrt_bake_light_multi_batch_device(_handles(), 0, C.byref(cfg), 1, C.byref(p), 0, None) == MCRT_OK


def _lights(n, bad=None):
    arr = (abi.McrtLightSource * max(n, 1))()
    for i in range(n):
        arr[i] = abi.Light((1.0 + i, 20.0, 30.0), (0.5, 0.5, 0.5, 1.0), 3.0).to_c()
    if bad == "nan_position":
        arr[0].position[1] = float("nan")
    elif bad == "inf_radius":
        arr[n - 1].radius = float("inf")
    elif bad == "nan_colour":
        arr[0].color[2] = float("nan")
    return arr


HOST_CASES = ["null_desc", "null_cfg", "null_planes", "all_planes_null", "four_lights", "negative_count", "null_lights", "nan_position", "inf_radius",
              "nan_colour", *BAD_CONFIGS, *BAD_WITH_OCCLUSION]


@pytest.mark.parametrize("family", ["light", "bake"])
@pytest.mark.parametrize("case", HOST_CASES + list(BAD_GRIDS))
def test_host_forms_reject_bad_arguments_and_leave_the_planes(mcrt, lib, family, case):
    bake = family == "bake"
    if case in BAD_GRIDS and not bake:
        return
    sd = mcrt.SceneDesc(B.two_boxes())
    cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}.get(case, {}))
    n = 192 if bake else 16 * 8
    keep = []

    def plane(comps):
        keep.append(np.full((n, comps), 7.0, np.float32))
        return keep[-1].ctypes.data

    planes = abi.McrtBakePlanesMulti() if bake else abi.McrtLightPlanesMulti()
    if case != "all_planes_null":
        for k in range(M):
            planes.visibility[k], planes.direct[k] = plane(1), plane(4)
        planes.occlusion, planes.combined = plane(1), plane(4)
        if bake:
            planes.position, planes.normal = plane(4), plane(4)
    d = None if case == "null_desc" else sd.ptr
    c = None if case == "null_cfg" else C.byref(cfg)
    out = None if case == "null_planes" else C.byref(planes)
    lights, n_lights = _lights(2), 2
    if case == "four_lights":
        lights, n_lights = _lights(4), 4
    elif case == "negative_count":
        n_lights = -1
    elif case == "null_lights":
        lights = None
    elif case in ("nan_position", "inf_radius", "nan_colour"):
        lights = _lights(2, case)
    grid = BAD_GRIDS.get(case, 1)
    rc = lib.mcrt_bake_light_multi(d, c, lights, n_lights, grid, out, 0) if bake else lib.mcrt_render_light_multi(d, c, lights, n_lights, out, 0)
    _invalid(lib, rc)
    assert all(np.all(v == 7.0) for v in keep)


def test_the_light_checks_come_right_behind_the_null_checks(mcrt, lib):
    sd = mcrt.SceneDesc(B.two_boxes())
    cfg = _cfg(shadowSamples=114)  # refused too, but behind the lights
    empty_l, empty_b = abi.McrtLightPlanesMulti(), abi.McrtBakePlanesMulti()  # and so is a struct without a plane
    _invalid(lib, lib.mcrt_render_light_multi(sd.ptr, C.byref(cfg), _lights(4), 4, C.byref(empty_l), 0))
    assert b"extra lights" in lib.mcrt_last_error()
    _invalid(lib, lib.mcrt_bake_light_multi(sd.ptr, C.byref(cfg), _lights(4), 4, 9, C.byref(empty_b), 0))
    assert b"extra lights" in lib.mcrt_last_error()
    _invalid(lib, lib.mcrt_render_light_multi(sd.ptr, C.byref(cfg), None, 0, C.byref(empty_l), 0))
    assert b"planes are NULL" in lib.mcrt_last_error()
    # zero-size frames with valid arguments: MCRT_OK, nothing written, no device needed
    cfg = _cfg(width=0)
    keep = np.full(4, 7.0, np.float32)
    p = abi.McrtLightPlanesMulti()
    p.combined = keep.ctypes.data
    assert lib.mcrt_render_light_multi(sd.ptr, C.byref(cfg), _lights(3), 3, C.byref(p), 0) == MCRT_OK and (keep == 7.0).all()


def test_host_forms_without_device_report_no_device(mcrt):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests run these forms
    sd = mcrt.SceneDesc(B.two_boxes())
    for call in (lambda: mcrt.TileRenderer.renderLightMulti(sd, abi.Config(width=16, height=8), lights=[abi.Light((0, 30, 30))]),
                 lambda: mcrt.TileRenderer.bakeLightMulti(sd, abi.Config(), lights=[abi.Light((0, 30, 30))])):
        with pytest.raises(mcrt._lib.McrtError) as e:
            call()
        assert e.value.code == MCRT_ERR_NO_DEVICE


def test_python_wrappers_check_their_arguments_and_shape_empty_results(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.SceneDesc(B.two_boxes())
    for bad in (("direct", "colour"), (), "shadow", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLightMulti(sd, cfg, planes=bad)
        with pytest.raises(ValueError):
            mcrt.TileRenderer.bakeLightMulti(sd, cfg, planes=bad)
    for bad in ((4,), (-1,), ()):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLightMulti(sd, cfg, light_indices=bad)
    with pytest.raises(ValueError):
        mcrt.TileRenderer.renderLightMulti(sd, cfg, lights=[abi.Light((0, 0, 0))] * 4)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.bakeLightMulti(sd, cfg, lights=[(0, 0, 0)])
    with pytest.raises(ValueError):
        mcrt.TileRenderer.bakeLightMulti(sd, cfg, grid=5)
    out = mcrt.TileRenderer.renderLightMulti(sd, abi.Config(width=0, height=5), light_indices=(0, 2))  # no pixel: the miss values, no device
    assert list(out) == list(abi.LIGHT_MULTI_NAMES)
    assert out["visibility"].shape == (2, 5, 0) and out["direct"].shape == (2, 5, 0, 4) and out["combined"].shape == (5, 0, 4)
    full = mcrt.TileRenderer.renderLightMulti(sd, abi.Config(width=4, height=5, tileSize=0), planes=("visibility", "combined"))
    assert (full["visibility"] == 1).all() and full["visibility"].shape == (M, 5, 4) and (full["combined"] == 0).all()
    with pytest.raises(ValueError, match="^give at least one of visibility_ptrs, direct_ptrs, occlusion_ptr, combined_ptr$"):
        mcrt.render_light_multi_batch_device([], cfg)
    with pytest.raises(ValueError):
        mcrt.render_light_multi_batch_device([], cfg, visibility_ptrs=[1, 2, 3, 4, 5])
    with pytest.raises(TypeError, match="^device_scenes must be DeviceScene objects$"):
        mcrt.render_light_multi_batch_device([object()], cfg, combined_ptr=0x1000)
    with pytest.raises(ValueError, match="^frame_stride_pixels 127 is smaller than width \\* height = 128$"):
        mcrt.render_light_multi_batch_device([], cfg, combined_ptr=0x1000, frame_stride_pixels=127)
    mcrt.render_light_multi_batch_device([], cfg, visibility_ptrs=[0, 0, 0x1000])  # no frames: nothing to do
    with pytest.raises(ValueError):
        mcrt.bake_light_multi_batch_device([], cfg)
    with pytest.raises(ValueError):
        mcrt.bake_light_multi_batch_device([], cfg, grid=9, combined_ptr=0x1000)
    with pytest.raises(ValueError, match="^texel_stride must be >= 0$"):
        mcrt.bake_light_multi_batch_device([], cfg, combined_ptr=0x1000, texel_stride=-1)
    mcrt.bake_light_multi_batch_device([], cfg, direct_ptrs=[0x1000])
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_light_multi_device(cfg)
    with pytest.raises(ValueError):
        ds.bake_light_multi_device(cfg, grid=0, combined_ptr=0x1000)
