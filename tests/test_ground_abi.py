"""The ground-shadow pass (mcrt_render_ground*, mcrt_scene_floor) without a device: the symbols, every argument check that comes
before any device work, the no-ops, the sample limit, the Python wrappers' own checks, and mcrt_scene_floor against numpy's
minimum of the scene's vertices.

The device forms are given opaque handle values (or zeroed blocks that differ in the device index, the first member of a
handle): every case fails — or is a no-op — on a check that does not look further inside a handle."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import layers_checker as L
import scenes

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_render_ground_device", "mcrt_render_ground_batch_device", "mcrt_render_ground", "mcrt_scene_floor")
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


def _planes(visibility=0x1000, distance=0x2000, matte=0x3000):
    return abi.McrtGround(visibility or None, distance or None, matte or None)


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
    assert C.sizeof(abi.McrtGround) == 3 * C.sizeof(C.c_void_p)
    assert abi.GROUND_NAMES == ("visibility", "distance", "matte") and abi.GROUND_MAX_SAMPLES == 113


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "all_planes_null", "ground_nan", "ground_inf", "samples_114"])
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
    elif case == "samples_114":
        cfg = _cfg(width=W, height=H, shadowSamples=114)
        args[1] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_ground_device(args[0], args[1], g, args[2], args[3]))


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_heights", "null_planes", "all_planes_null",
                                  "stride_too_small", "second_height_nan", "height_inf", "samples_114"])
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
    elif case == "samples_114":
        cfg = _cfg(width=W, height=H, shadowSamples=114)
        a["cfg"] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_ground_batch_device(a["scenes"], a["n"], a["cfg"], a["g"], a["out"], a["stride"], None))


def test_handles_on_different_devices_are_rejected(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    cfg, planes = _cfg(width=W, height=H), _planes()
    arr = _handles(*[C.addressof(b) for b in blocks])
    _invalid(lib, lib.mcrt_render_ground_batch_device(arr, 2, C.byref(cfg), _heights(0.0, 0.0), C.byref(planes), W * H, None))
    assert b"one device" in lib.mcrt_last_error()


def test_the_sample_limit_is_113_and_only_with_soft_shadows(lib, mcrt):
    # the limit is checked before the frame's size: a frame of zero size is a no-op once the arguments are accepted
    planes = _planes()
    for samples, soft, rc in ((113, True, MCRT_OK), (114, True, MCRT_ERR_INVALID), (114, False, MCRT_OK), (100000, False, MCRT_OK)):
        empty = _cfg(width=0, height=H, shadowSamples=samples, softShadows=soft)
        assert lib.mcrt_render_ground_device(C.c_void_p(0x10), C.byref(empty), 0.0, C.byref(planes), None) == rc, (samples, soft)
        assert lib.mcrt_render_ground_batch_device(_handles(0x10), 1, C.byref(empty), _heights(0.0), C.byref(planes), 0, None) == rc
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtGround(keep.ctypes.data, None, None)
    for samples, soft, rc in ((113, True, MCRT_OK), (114, True, MCRT_ERR_INVALID), (114, False, MCRT_OK)):
        empty = _cfg(width=8, height=0, shadowSamples=samples, softShadows=soft)
        assert lib.mcrt_render_ground(sd.ptr, C.byref(empty), 0.0, C.byref(host), 0) == rc
    assert np.all(keep == 7.0)


def test_zero_frames_and_zero_size_are_ok(lib, mcrt):
    cfg, planes = _cfg(width=W, height=H), _planes()
    assert lib.mcrt_render_ground_batch_device(_handles(), 0, C.byref(cfg), None, C.byref(planes), W * H, None) == MCRT_OK
    assert lib.mcrt_render_ground_batch_device(_handles(), 0, C.byref(cfg), _heights(), C.byref(planes), W * H, None) == MCRT_OK
    for empty in (_cfg(width=0, height=H), _cfg(width=W, height=0), _cfg(width=W, height=H, tileSize=0)):
        assert lib.mcrt_render_ground_batch_device(_handles(0x10, 0x20), 2, C.byref(empty), _heights(0.0, 2.0), C.byref(planes), 0, None) == MCRT_OK
        assert lib.mcrt_render_ground_device(C.c_void_p(0x10), C.byref(empty), 0.0, C.byref(planes), None) == MCRT_OK
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtGround(keep.ctypes.data, None, None)
    empty = _cfg(width=32, height=0)
    assert lib.mcrt_render_ground(sd.ptr, C.byref(empty), 0.0, C.byref(host), 0) == MCRT_OK
    assert np.all(keep == 7.0)


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_planes", "all_planes_null", "ground_nan", "samples_114"])
def test_host_form_rejects_bad_arguments(mcrt, lib, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = _cfg(width=16, height=8)
    vis = np.full((8, 16), 7.0, np.float32)
    planes = abi.McrtGround(vis.ctypes.data, None, None)
    d, c, g, out = sd.ptr, C.byref(cfg), 0.0, C.byref(planes)
    if case == "null_desc":
        d = None
    elif case == "null_cfg":
        c = None
    elif case == "null_planes":
        out = None
    elif case == "all_planes_null":
        planes = abi.McrtGround(None, None, None)
        out = C.byref(planes)
    elif case == "ground_nan":
        g = float("nan")
    elif case == "samples_114":
        cfg = _cfg(width=16, height=8, shadowSamples=114)
        c = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_ground(d, c, g, out, 0))
    assert np.all(vis == 7.0)


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests render the ground planes
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderGround(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8))
    assert e.value.code == MCRT_ERR_NO_DEVICE


def _vertex_floor(sd) -> np.float32:
    d = sd.to_numpy()
    return np.min(np.concatenate([np.asarray(m["triangles"], np.float32).reshape(-1, 3)[:, 1] for m in d["meshes"]]))


def test_scene_floor_of_the_character(mcrt, lib):
    pose0 = mcrt.getBuiltinPoses()[0]
    assert mcrt.scene_floor(mcrt.MeshBuilder.buildDefaultScene()) == 0.0
    assert mcrt.scene_floor(mcrt.MeshBuilder.buildScene(mcrt.synthetic_skin("S32"), pose0)) == 0.0
    # a 64 x 64 skin has outer leg layers, boxes 0.5 larger than the legs on every side: its lowest vertex lies below the soles
    assert mcrt.scene_floor(mcrt.MeshBuilder.buildScene(mcrt.synthetic_skin("S64"), pose0)) == -0.5
    for kind in ("S64", "S32"):
        for pose in (0, 3, 6):
            sd = L.skin_case(kind, pose)
            scenes.assert_bit_equal(np.float32(mcrt.scene_floor(sd)), _vertex_floor(sd), f"{kind} pose {pose}")


@pytest.mark.parametrize("name", L.BOX_CASES)
def test_scene_floor_is_the_vertex_minimum(mcrt, name):
    sd = mcrt.SceneDesc(L.box_scene(name)[0])
    floor = np.float32(mcrt.scene_floor(sd))
    scenes.assert_bit_equal(floor, _vertex_floor(sd), name)
    if name == "posed":  # the rotated arm: no box corner of the un-posed boxes lies there
        assert abs(float(floor) - 21.274969) < 1e-5


def test_scene_floor_rejects_null_and_empty_scenes(mcrt, lib):
    y = C.c_float(-7.0)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    _invalid(lib, lib.mcrt_scene_floor(None, C.byref(y)))
    _invalid(lib, lib.mcrt_scene_floor(sd.ptr, None))
    empty = mcrt.SceneDesc(scenes.simple_scene([]))
    _invalid(lib, lib.mcrt_scene_floor(empty.ptr, C.byref(y)))
    assert y.value == -7.0
    with pytest.raises(mcrt._lib.McrtError):
        mcrt.scene_floor(empty)


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    for bad in (("visibility", "colour"), (), "shadow", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderGround(sd, cfg, planes=bad)
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderGroundBatch([sd], cfg, planes=bad)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderGroundBatch([object()], cfg)
    for bad in (float("nan"), [0.0, 1.0], [float("inf")]):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderGroundBatch([sd], cfg, ground=bad)
    out = mcrt.TileRenderer.renderGroundBatch([], cfg)
    assert {k: (v.shape, v.dtype) for k, v in out.items()} == {
        "visibility": ((0, 8, 16), np.float32), "distance": ((0, 8, 16), np.float32), "matte": ((0, 8, 16), np.uint8)}
    assert list(mcrt.TileRenderer.renderGroundBatch([], cfg, planes=("matte", "visibility"))) == ["visibility", "matte"]
    empty = mcrt.TileRenderer.renderGround(sd, abi.Config(width=0, height=8))  # a frame of zero size: nothing to render
    assert empty["matte"].shape == (8, 0) and empty["distance"].shape == (8, 0)
    with pytest.raises(ValueError):
        mcrt.render_ground_batch_device([], cfg, 0.0)  # no plane at all
    with pytest.raises(ValueError):
        mcrt.render_ground_batch_device([], cfg, 0.0, visibility_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(ValueError):
        mcrt.render_ground_batch_device([], cfg, None, visibility_ptr=0x1000)  # a resident scene has no floor of its own
    with pytest.raises(TypeError):
        mcrt.render_ground_batch_device([object()], cfg, 0.0, visibility_ptr=0x1000)
    mcrt.render_ground_batch_device([], cfg, 0.0, matte_ptr=0x1000)  # no frames: nothing to do
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_ground_device(cfg, 0.0)
    with pytest.raises(ValueError):
        ds.render_ground_device(cfg, float("nan"), matte_ptr=0x1000)
