"""The light layers (mcrt_render_light*) without a device: the symbols, every argument check that comes before any device work,
the no-ops, the sample limits of the shadow term and of the occlusion plane, and the Python wrappers' own checks.

The device forms are given opaque handle values (or zeroed blocks that differ in the device index, the first member of a
handle): every case fails — or is a no-op — on a check that does not look further inside a handle."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_render_light_device", "mcrt_render_light_batch_device", "mcrt_render_light")
W, H = 64, 32


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _planes(visibility=0x1000, occlusion=0x2000, direct=0x3000):
    return abi.McrtLightPlanes(visibility or None, occlusion or None, direct or None)


def _invalid(lib, rc):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def test_symbols_are_exported_and_declared(lib, mcrt):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name
    assert lib.mcrt_abi_version() == 3
    assert C.sizeof(abi.McrtLightPlanes) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in abi.McrtLightPlanes._fields_] == ["visibility", "occlusion", "direct"]
    assert abi.LIGHT_NAMES == ("visibility", "occlusion", "direct") and abi.LIGHT_MAX_SAMPLES == 113
    assert "render_light_batch_device" in mcrt.__all__ and callable(mcrt.render_light_batch_device)
    assert callable(mcrt.TileRenderer.renderLight) and callable(mcrt.TileRenderer.renderLightBatch)
    assert callable(mcrt.DeviceScene.render_light_device)


def test_the_header_declares_the_entry_points():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert "typedef struct mcrt_light_planes {" in header and "#define MCRT_ABI_VERSION 3" in header
    assert "k = 1.0f - ao_intensity * (1.0f - occlusion)" in header  # the recomposition is part of the contract


# refused whatever planes are asked for / refused only with the occlusion plane
BAD_CONFIGS = {"shadow_samples_114": dict(shadowSamples=114)}
BAD_WITH_OCCLUSION = {"ao_samples_0": dict(aoSamples=0), "ao_samples_negative": dict(aoSamples=-4), "ao_samples_114": dict(aoSamples=114),
                      "ao_radius_nan": dict(aoRadius=float("nan")), "ao_radius_inf": dict(aoRadius=float("inf"))}


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "all_planes_null", *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_single_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(width=W, height=H), _planes()
    args = [C.c_void_p(0x10), C.byref(cfg), C.byref(planes), None]
    if case == "null_cfg":
        args[1] = None
    elif case == "null_handle":
        args[0] = None
    elif case == "null_planes":
        args[2] = None
    elif case == "all_planes_null":
        planes = _planes(0, 0, 0)
        args[2] = C.byref(planes)
    else:
        cfg = _cfg(width=W, height=H, **{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        args[1] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_light_device(*args))


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_planes", "all_planes_null", "stride_too_small",
                                  *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_batch_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(width=W, height=H), _planes()
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=C.byref(cfg), out=C.byref(planes), stride=W * H)
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
        planes = _planes(0, 0, 0)
        a["out"] = C.byref(planes)
    elif case == "stride_too_small":
        a["stride"] = W * H - 1
    else:
        cfg = _cfg(width=W, height=H, **{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        a["cfg"] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_light_batch_device(a["scenes"], a["n"], a["cfg"], a["out"], a["stride"], None))


def test_handles_on_different_devices_are_rejected(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    cfg, planes = _cfg(width=W, height=H), _planes()
    arr = _handles(*[C.addressof(b) for b in blocks])
    _invalid(lib, lib.mcrt_render_light_batch_device(arr, 2, C.byref(cfg), C.byref(planes), W * H, None))
    assert b"one device" in lib.mcrt_last_error()


def test_the_limits(lib, mcrt):
    # the limits are checked before the frame's size: a frame of zero size is a no-op once the arguments are accepted
    every, no_occlusion, only_occlusion = _planes(), _planes(occlusion=0), _planes(visibility=0, direct=0)
    cases = [(dict(shadowSamples=113), every, MCRT_OK), (dict(shadowSamples=114), every, MCRT_ERR_INVALID),
             (dict(shadowSamples=114), only_occlusion, MCRT_ERR_INVALID), (dict(shadowSamples=114, softShadows=False), every, MCRT_OK),
             (dict(shadowSamples=100000, softShadows=False), every, MCRT_OK),
             (dict(aoSamples=1), every, MCRT_OK), (dict(aoSamples=113), every, MCRT_OK), (dict(aoSamples=0), every, MCRT_ERR_INVALID),
             (dict(aoSamples=114), only_occlusion, MCRT_ERR_INVALID),
             # without the occlusion plane the AO fields are not read
             (dict(aoSamples=0), no_occlusion, MCRT_OK), (dict(aoSamples=114), no_occlusion, MCRT_OK), (dict(aoRadius=float("nan")), no_occlusion, MCRT_OK),
             (dict(aoRadius=float("-inf")), every, MCRT_ERR_INVALID),
             # ao_radius <= 0 is legal, ao_enabled and ao_intensity are ignored
             (dict(aoRadius=0.0), every, MCRT_OK), (dict(aoRadius=-2.0), every, MCRT_OK), (dict(aoEnabled=True, aoIntensity=float("nan")), every, MCRT_OK)]
    for kw, planes, rc in cases:
        empty = _cfg(width=0, height=H, **kw)
        assert lib.mcrt_render_light_device(C.c_void_p(0x10), C.byref(empty), C.byref(planes), None) == rc, kw
        assert lib.mcrt_render_light_batch_device(_handles(0x10), 1, C.byref(empty), C.byref(planes), 0, None) == rc, kw
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    for kw, planes, rc in cases:
        host = abi.McrtLightPlanes(keep.ctypes.data if planes.visibility else None, keep.ctypes.data if planes.occlusion else None,
                                   keep.ctypes.data if planes.direct else None)
        empty = _cfg(width=8, height=0, **kw)
        assert lib.mcrt_render_light(sd.ptr, C.byref(empty), C.byref(host), 0) == rc, kw
    assert np.all(keep == 7.0)


def test_zero_frames_and_zero_size_are_ok(lib, mcrt):
    cfg, planes = _cfg(width=W, height=H), _planes()
    assert lib.mcrt_render_light_batch_device(_handles(), 0, C.byref(cfg), C.byref(planes), W * H, None) == MCRT_OK
    assert lib.mcrt_render_light_batch_device(None, 0, C.byref(cfg), C.byref(planes), W * H, None) == MCRT_OK
    for empty in (_cfg(width=0, height=H), _cfg(width=W, height=0), _cfg(width=W, height=H, tileSize=0)):
        assert lib.mcrt_render_light_batch_device(_handles(0x10, 0x20), 2, C.byref(empty), C.byref(planes), 0, None) == MCRT_OK
        assert lib.mcrt_render_light_device(C.c_void_p(0x10), C.byref(empty), C.byref(planes), None) == MCRT_OK
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtLightPlanes(keep.ctypes.data, keep.ctypes.data, None)
    empty = _cfg(width=32, height=0)
    assert lib.mcrt_render_light(sd.ptr, C.byref(empty), C.byref(host), 0) == MCRT_OK
    assert np.all(keep == 7.0)


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_planes", "all_planes_null", *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_host_form_rejects_bad_arguments(mcrt, lib, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = _cfg(width=16, height=8)
    vis, occ, direct = np.full((8, 16), 7.0, np.float32), np.full((8, 16), 7.0, np.float32), np.full((8, 16, 4), 7.0, np.float32)
    planes = abi.McrtLightPlanes(vis.ctypes.data, occ.ctypes.data, direct.ctypes.data)
    d, c, out = sd.ptr, C.byref(cfg), C.byref(planes)
    if case == "null_desc":
        d = None
    elif case == "null_cfg":
        c = None
    elif case == "null_planes":
        out = None
    elif case == "all_planes_null":
        planes = abi.McrtLightPlanes(None, None, None)
        out = C.byref(planes)
    else:
        cfg = _cfg(width=16, height=8, **{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        c = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_light(d, c, out, 0))
    assert np.all(vis == 7.0) and np.all(occ == 7.0) and np.all(direct == 7.0)


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests render the light planes
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderLight(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8))
    assert e.value.code == MCRT_ERR_NO_DEVICE


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    for bad in (("direct", "colour"), (), "shadow", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLight(sd, cfg, planes=bad)
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLightBatch([sd], cfg, planes=bad)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderLightBatch([object()], cfg)
    out = mcrt.TileRenderer.renderLightBatch([], cfg)
    assert {k: (v.shape, v.dtype) for k, v in out.items()} == {
        "visibility": ((0, 8, 16), np.float32), "occlusion": ((0, 8, 16), np.float32), "direct": ((0, 8, 16, 4), np.float32)}
    assert list(mcrt.TileRenderer.renderLightBatch([], cfg, planes=("direct", "visibility"))) == ["visibility", "direct"]
    empty = mcrt.TileRenderer.renderLight(sd, abi.Config(width=0, height=8))  # a frame of zero size: nothing to render
    assert empty["visibility"].shape == (8, 0) and empty["occlusion"].shape == (8, 0) and empty["direct"].shape == (8, 0, 4)
    with pytest.raises(ValueError):
        mcrt.render_light_batch_device([], cfg)  # no plane at all
    with pytest.raises(ValueError):
        mcrt.render_light_batch_device([], cfg, direct_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(TypeError):
        mcrt.render_light_batch_device([object()], cfg, direct_ptr=0x1000)
    mcrt.render_light_batch_device([], cfg, occlusion_ptr=0x1000)  # no frames: nothing to do
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_light_device(cfg)
