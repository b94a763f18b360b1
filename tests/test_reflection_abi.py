"""The ground-reflection pass (mcrt_render_reflection*) without a device: the symbols, every argument check that comes before any
device work, the no-ops, the sample and bounce limits, and the Python wrappers' own checks.

The device forms are given opaque handle values (or zeroed blocks that differ in the device index, the first member of a
handle): every case fails — or is a no-op — on a check that does not look further inside a handle."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_render_reflection_device", "mcrt_render_reflection_batch_device", "mcrt_render_reflection")
W, H = 64, 32


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _heights(*values):
    return (C.c_float * max(len(values), 1))(*values)


def _planes(rgba=0x1000, rgba8=0x2000, distance=0x3000):
    return abi.McrtReflection(rgba or None, rgba8 or None, distance or None)


def _invalid(lib, rc):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name
    assert lib.mcrt_abi_version() == 3
    assert C.sizeof(abi.McrtReflection) == 3 * C.sizeof(C.c_void_p)
    assert [f[0] for f in abi.McrtReflection._fields_] == ["rgba", "rgba8", "distance"]
    assert abi.REFLECTION_NAMES == ("rgba", "rgba8", "distance") and abi.REFLECTION_MAX_BOUNCES == 8


def test_the_header_declares_the_entry_points():
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert "typedef struct mcrt_reflection {" in header and "#define MCRT_ABI_VERSION 3" in header


BAD_CONFIGS = {"samples_114": dict(shadowSamples=114), "bounces_9": dict(maxBounces=9)}


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "all_planes_null", "ground_nan", "ground_inf", *BAD_CONFIGS])
def test_single_device_form_rejects_bad_arguments(lib, case):
    cfg, planes, g = _cfg(width=W, height=H), _planes(), 0.0
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
    elif case == "ground_nan":
        g = float("nan")
    elif case == "ground_inf":
        g = float("-inf")
    else:
        cfg = _cfg(width=W, height=H, **BAD_CONFIGS[case])
        args[1] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_reflection_device(args[0], args[1], g, args[2], args[3]))


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_heights", "null_planes", "all_planes_null",
                                  "stride_too_small", "second_height_nan", "height_inf", *BAD_CONFIGS])
def test_batch_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(width=W, height=H), _planes()
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=C.byref(cfg), g=_heights(0.0, 1.0), out=C.byref(planes), stride=W * H)
    if case == "n_negative":
        a["n"] = -1
    elif case == "null_cfg":
        a["cfg"] = None
    elif case == "null_array":
        a["scenes"] = None
    elif case == "null_entry":
        a["scenes"] = _handles(0x10, None)
    elif case == "null_heights":
        a["g"] = None
    elif case == "null_planes":
        a["out"] = None
    elif case == "all_planes_null":
        planes = _planes(0, 0, 0)
        a["out"] = C.byref(planes)
    elif case == "stride_too_small":
        a["stride"] = W * H - 1
    elif case == "second_height_nan":
        a["g"] = _heights(0.0, float("nan"))
    elif case == "height_inf":
        a["g"] = _heights(float("inf"), 0.0)
    else:
        cfg = _cfg(width=W, height=H, **BAD_CONFIGS[case])
        a["cfg"] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_reflection_batch_device(a["scenes"], a["n"], a["cfg"], a["g"], a["out"], a["stride"], None))


def test_handles_on_different_devices_are_rejected(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    cfg, planes = _cfg(width=W, height=H), _planes()
    arr = _handles(*[C.addressof(b) for b in blocks])
    _invalid(lib, lib.mcrt_render_reflection_batch_device(arr, 2, C.byref(cfg), _heights(0.0, 0.0), C.byref(planes), W * H, None))
    assert b"one device" in lib.mcrt_last_error()


def test_the_limits_are_113_samples_with_soft_shadows_and_8_bounces(lib, mcrt):
    # the limits are checked before the frame's size: a frame of zero size is a no-op once the arguments are accepted
    planes = _planes()
    cases = [(dict(shadowSamples=113), MCRT_OK), (dict(shadowSamples=114), MCRT_ERR_INVALID), (dict(shadowSamples=114, softShadows=False), MCRT_OK),
             (dict(shadowSamples=100000, softShadows=False), MCRT_OK), (dict(maxBounces=8), MCRT_OK), (dict(maxBounces=9), MCRT_ERR_INVALID),
             (dict(maxBounces=0), MCRT_OK), (dict(maxBounces=-3), MCRT_OK)]
    for kw, rc in cases:
        empty = _cfg(width=0, height=H, **kw)
        assert lib.mcrt_render_reflection_device(C.c_void_p(0x10), C.byref(empty), 0.0, C.byref(planes), None) == rc, kw
        assert lib.mcrt_render_reflection_batch_device(_handles(0x10), 1, C.byref(empty), _heights(0.0), C.byref(planes), 0, None) == rc, kw
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtReflection(keep.ctypes.data, None, None)
    for kw, rc in cases:
        empty = _cfg(width=8, height=0, **kw)
        assert lib.mcrt_render_reflection(sd.ptr, C.byref(empty), 0.0, C.byref(host), 0) == rc, kw
    assert np.all(keep == 7.0)


def test_zero_frames_and_zero_size_are_ok(lib, mcrt):
    cfg, planes = _cfg(width=W, height=H), _planes()
    assert lib.mcrt_render_reflection_batch_device(_handles(), 0, C.byref(cfg), None, C.byref(planes), W * H, None) == MCRT_OK
    assert lib.mcrt_render_reflection_batch_device(_handles(), 0, C.byref(cfg), _heights(), C.byref(planes), W * H, None) == MCRT_OK
    for empty in (_cfg(width=0, height=H), _cfg(width=W, height=0), _cfg(width=W, height=H, tileSize=0)):
        assert lib.mcrt_render_reflection_batch_device(_handles(0x10, 0x20), 2, C.byref(empty), _heights(0.0, 2.0), C.byref(planes), 0, None) == MCRT_OK
        assert lib.mcrt_render_reflection_device(C.c_void_p(0x10), C.byref(empty), 0.0, C.byref(planes), None) == MCRT_OK
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtReflection(keep.ctypes.data, None, None)
    empty = _cfg(width=32, height=0)
    assert lib.mcrt_render_reflection(sd.ptr, C.byref(empty), 0.0, C.byref(host), 0) == MCRT_OK
    assert np.all(keep == 7.0)


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_planes", "all_planes_null", "ground_nan", *BAD_CONFIGS])
def test_host_form_rejects_bad_arguments(mcrt, lib, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = _cfg(width=16, height=8)
    rgba = np.full((8, 16, 4), 7.0, np.float32)
    planes = abi.McrtReflection(rgba.ctypes.data, None, None)
    d, c, g, out = sd.ptr, C.byref(cfg), 0.0, C.byref(planes)
    if case == "null_desc":
        d = None
    elif case == "null_cfg":
        c = None
    elif case == "null_planes":
        out = None
    elif case == "all_planes_null":
        planes = abi.McrtReflection(None, None, None)
        out = C.byref(planes)
    elif case == "ground_nan":
        g = float("nan")
    else:
        cfg = _cfg(width=16, height=8, **BAD_CONFIGS[case])
        c = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_reflection(d, c, g, out, 0))
    assert np.all(rgba == 7.0)


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests render the reflection planes
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderReflection(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8))
    assert e.value.code == MCRT_ERR_NO_DEVICE


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    for bad in (("rgba", "colour"), (), "mirror", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderReflection(sd, cfg, planes=bad)
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderReflectionBatch([sd], cfg, planes=bad)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderReflectionBatch([object()], cfg)
    for bad in (float("nan"), [0.0, 1.0], [float("inf")]):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderReflectionBatch([sd], cfg, ground=bad)
    out = mcrt.TileRenderer.renderReflectionBatch([], cfg)
    assert {k: (v.shape, v.dtype) for k, v in out.items()} == {
        "rgba": ((0, 8, 16, 4), np.float32), "rgba8": ((0, 8, 16, 4), np.uint8), "distance": ((0, 8, 16), np.float32)}
    assert list(mcrt.TileRenderer.renderReflectionBatch([], cfg, planes=("distance", "rgba"))) == ["rgba", "distance"]
    empty = mcrt.TileRenderer.renderReflection(sd, abi.Config(width=0, height=8))  # a frame of zero size: nothing to render
    assert empty["rgba"].shape == (8, 0, 4) and empty["rgba8"].shape == (8, 0, 4) and empty["distance"].shape == (8, 0)
    with pytest.raises(ValueError):
        mcrt.render_reflection_batch_device([], cfg, 0.0)  # no plane at all
    with pytest.raises(ValueError):
        mcrt.render_reflection_batch_device([], cfg, 0.0, rgba_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(ValueError):
        mcrt.render_reflection_batch_device([], cfg, None, rgba_ptr=0x1000)  # a resident scene has no floor of its own
    with pytest.raises(TypeError):
        mcrt.render_reflection_batch_device([object()], cfg, 0.0, rgba_ptr=0x1000)
    mcrt.render_reflection_batch_device([], cfg, 0.0, rgba8_ptr=0x1000)  # no frames: nothing to do
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_reflection_device(cfg, 0.0)
    with pytest.raises(ValueError):
        ds.render_reflection_device(cfg, float("nan"), rgba8_ptr=0x1000)
