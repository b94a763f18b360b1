"""Geometry layers and picking (mcrt_render_layers*, mcrt_scene_pick, mcrt_skin_texel) without a device: the symbols, the
argument checks that come before any device work, the Python wrappers' own checks, and mcrt_skin_texel against the scene
builder's textures for every mesh, face and texel of both skin kinds."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import layers_checker

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_render_layers_device", "mcrt_render_layers_batch_device", "mcrt_render_layers", "mcrt_render_layers_batch",
               "mcrt_scene_pick", "mcrt_skin_texel")


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def _handles(*values):
    # opaque handle values: every case that uses them fails on a check that does not look inside a handle
    return (C.c_void_p * max(len(values), 1))(*values)


def _planes(depth=0x1000, normal=0x2000, albedo=0x3000, id=0x4000):
    return abi.McrtLayers(depth or None, normal or None, albedo or None, id or None)


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
    assert C.sizeof(abi.McrtSurface) == 64 == abi.SURFACE_DTYPE.itemsize
    assert C.sizeof(abi.McrtLayers) == 4 * C.sizeof(C.c_void_p)
    assert (abi.ID_BACK, abi.ID_OUTER) == (8, 16)


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_layers", "all_planes_null"])
def test_single_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(width=64, height=32), _planes()
    args = [C.c_void_p(0x10), C.byref(cfg), C.byref(planes), None]
    if case == "null_cfg":
        args[1] = None
    elif case == "null_handle":
        args[0] = None
    elif case == "null_layers":
        args[2] = None
    else:
        planes = _planes(0, 0, 0, 0)
        args[2] = C.byref(planes)
    _invalid(lib, lib.mcrt_render_layers_device(*args))


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_layers", "all_planes_null", "stride_too_small"])
def test_batch_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(width=64, height=32), _planes()
    args = dict(scenes=_handles(0x10, 0x20), n=2, cfg=C.byref(cfg), out=C.byref(planes), stride=64 * 32)
    if case == "n_negative":
        args["n"] = -1
    elif case == "null_cfg":
        args["cfg"] = None
    elif case == "null_array":
        args["scenes"] = None
    elif case == "null_entry":
        args["scenes"] = _handles(0x10, None)
    elif case == "null_layers":
        args["out"] = None
    elif case == "all_planes_null":
        planes = _planes(0, 0, 0, 0)
        args["out"] = C.byref(planes)
    elif case == "stride_too_small":
        args["stride"] = 64 * 32 - 1
    _invalid(lib, lib.mcrt_render_layers_batch_device(args["scenes"], args["n"], args["cfg"], args["out"], args["stride"], None))


def test_handles_on_different_devices_are_rejected(lib):
    # the check reads the handles' device index, the first member of a handle, and nothing else of them: two zeroed blocks
    # that differ in that word stand in for handles on devices 0 and 1
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    cfg, planes = _cfg(width=64, height=32), _planes()
    arr = _handles(*[C.addressof(b) for b in blocks])
    _invalid(lib, lib.mcrt_render_layers_batch_device(arr, 2, C.byref(cfg), C.byref(planes), 64 * 32, None))
    assert b"one device" in lib.mcrt_last_error()


def test_zero_frames_and_zero_size_are_ok(lib, mcrt):
    cfg, planes = _cfg(width=64, height=32), _planes()
    assert lib.mcrt_render_layers_batch_device(_handles(), 0, C.byref(cfg), C.byref(planes), 64 * 32, None) == MCRT_OK
    for empty in (_cfg(width=0, height=32), _cfg(width=64, height=0), _cfg(width=64, height=32, tileSize=0)):
        assert lib.mcrt_render_layers_batch_device(_handles(0x10, 0x20), 2, C.byref(empty), C.byref(planes), 0, None) == MCRT_OK
        assert lib.mcrt_render_layers_device(C.c_void_p(0x10), C.byref(empty), C.byref(planes), None) == MCRT_OK
    # the host forms: nothing is written
    sd = mcrt.MeshBuilder.buildDefaultScene()
    arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtLayers(keep.ctypes.data, None, None, None)
    empty = _cfg(width=32, height=0)
    assert lib.mcrt_render_layers(sd.ptr, C.byref(empty), C.byref(host), 0) == MCRT_OK
    assert lib.mcrt_render_layers_batch(arr, 1, C.byref(empty), C.byref(host), 0) == MCRT_OK
    assert lib.mcrt_render_layers_batch(arr, 0, C.byref(cfg), C.byref(host), 0) == MCRT_OK
    assert np.all(keep == 7.0)


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_entry", "null_layers", "all_planes_null", "null_desc"])
def test_host_forms_reject_bad_arguments(mcrt, lib, case):
    sds = [mcrt.MeshBuilder.buildDefaultScene(), mcrt.MeshBuilder.buildDefaultScene(mcrt.getBuiltinPoses()[1])]
    arr = (C.POINTER(abi.McrtSceneDesc) * 2)(*[d.ptr for d in sds])
    cfg = _cfg(width=16, height=8)
    depth = np.full((2, 8, 16), 7.0, np.float32)
    planes = abi.McrtLayers(depth.ctypes.data, None, None, None)
    n, c, out = 2, C.byref(cfg), C.byref(planes)
    if case == "null_desc":
        _invalid(lib, lib.mcrt_render_layers(None, c, out, 0))
        return
    if case == "n_negative":
        n = -2
    elif case == "null_cfg":
        c = None
    elif case == "null_entry":
        arr[1] = C.POINTER(abi.McrtSceneDesc)()
    elif case == "null_layers":
        out = None
    elif case == "all_planes_null":
        planes = abi.McrtLayers(None, None, None, None)
        out = C.byref(planes)
    _invalid(lib, lib.mcrt_render_layers_batch(arr, n, c, out, 0))
    assert np.all(depth == 7.0)


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests render layers")
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderLayers(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8))
    assert e.value.code == MCRT_ERR_NO_DEVICE


@pytest.mark.parametrize("case", ["null_handle", "null_cfg", "n_negative", "null_xy", "null_out", "x_negative", "x_at_width", "y_at_height",
                                  "second_outside", "zero_size_frame"])
def test_pick_rejects_bad_arguments(lib, case):
    cfg = _cfg(width=64, height=32)
    xy = np.array([[0, 0], [63, 31]], np.int32)
    out = np.zeros(2, abi.SURFACE_DTYPE)
    args = [C.c_void_p(0x10), C.byref(cfg), xy.ctypes.data_as(abi.c_int32_p), 2, out.ctypes.data]
    if case == "null_handle":
        args[0] = None
    elif case == "null_cfg":
        args[1] = None
    elif case == "n_negative":
        args[3] = -1
    elif case == "null_xy":
        args[2] = None
    elif case == "null_out":
        args[4] = None
    elif case == "x_negative":
        xy[0, 0] = -1
    elif case == "x_at_width":
        xy[0, 0] = 64
    elif case == "y_at_height":
        xy[0, 1] = 32
    elif case == "second_outside":
        xy[1] = (63, 32)
    elif case == "zero_size_frame":
        cfg.width = 0
    _invalid(lib, lib.mcrt_scene_pick(*args))
    assert not out.tobytes().strip(b"\0")


def test_pick_of_no_pixels_is_ok(lib):
    cfg = _cfg(width=64, height=32)
    assert lib.mcrt_scene_pick(C.c_void_p(0x10), C.byref(cfg), None, 0, None) == MCRT_OK


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    for bad in (("depth", "colour"), (), "beauty", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLayers(sd, cfg, layers=bad)
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderLayersBatch([sd], cfg, layers=bad)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderLayersBatch([object()], cfg)
    out = mcrt.TileRenderer.renderLayersBatch([], cfg)
    assert {k: (v.shape, v.dtype) for k, v in out.items()} == {
        "depth": ((0, 8, 16), np.float32), "normal": ((0, 8, 16, 4), np.float32), "albedo": ((0, 8, 16, 4), np.float32),
        "id": ((0, 8, 16, 4), np.int32)}
    assert list(mcrt.TileRenderer.renderLayersBatch([], cfg, layers=("id", "depth"))) == ["depth", "id"]
    empty = mcrt.TileRenderer.renderLayers(sd, abi.Config(width=0, height=8))  # a frame of zero size: nothing to render
    assert empty["id"].shape == (8, 0, 4) and empty["depth"].shape == (8, 0)
    with pytest.raises(ValueError):
        mcrt.render_layers_batch_device([], cfg)  # no plane at all
    with pytest.raises(ValueError):
        mcrt.render_layers_batch_device([], cfg, depth_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(TypeError):
        mcrt.render_layers_batch_device([object()], cfg, depth_ptr=0x1000)
    mcrt.render_layers_batch_device([], cfg, id_ptr=0x1000)  # no frames: nothing to do
    # DeviceScene's own checks come before the handle is used
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_layers_device(cfg)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 2), np.float32), [[16, 0]], [[0, 8]], [[-1, 0]]):
        with pytest.raises(ValueError):
            ds.pick(cfg, bad)


@pytest.mark.parametrize("case", ["height", "mesh_64", "mesh_32", "mesh_negative", "face", "face_negative", "tx", "ty", "tx_negative", "null_out"])
def test_skin_texel_rejects_out_of_range_arguments(mcrt, lib, case):
    x, y = C.c_int(-7), C.c_int(-7)
    args = {"height": (48, 0, 0, 0, 0), "mesh_64": (64, 12, 0, 0, 0), "mesh_32": (32, 7, 0, 0, 0), "mesh_negative": (64, -1, 0, 0, 0),
            "face": (64, 0, 6, 0, 0), "face_negative": (64, 0, -1, 0, 0), "tx": (64, 2, 2, 4, 0), "ty": (64, 2, 4, 0, 4),
            "tx_negative": (64, 0, 0, -1, 0), "null_out": (64, 0, 0, 0, 0)}[case]
    if case == "null_out":
        _invalid(lib, lib.mcrt_skin_texel(*args, None, C.byref(y)))
    else:
        _invalid(lib, lib.mcrt_skin_texel(*args, C.byref(x), C.byref(y)))
        assert (x.value, y.value) == (-7, -7)
        kind = {64: "S64", 32: "S32"}.get(args[0], args[0])
        with pytest.raises(ValueError):
            mcrt.skin_texel(kind, *args[1:])


@pytest.mark.parametrize("kind,n_meshes,pose", [("S64", 12, 0), ("S32", 7, 3)])
def test_skin_texel_names_the_texel_the_builder_cut(mcrt, kind, n_meshes, pose):
    skin = layers_checker.unique_skin(kind)
    scene = mcrt.MeshBuilder.buildScene(skin, mcrt.getBuiltinPoses()[pose]).to_numpy()
    assert len(scene["meshes"]) == n_meshes
    expected = skin.astype(np.float32) / np.float32(255.0)  # texel = u8 / 255.0f
    texels = 0
    for m, mesh in enumerate(scene["meshes"]):
        for face in range(6):
            tex = scene["textures"][int(mesh["tri_texture"][2 * face])]
            w, h = tex["width"], tex["height"]
            assert w > 0 and h > 0 and len(tex["pixels"]) == w * h
            for ty in range(h):
                for tx in range(w):
                    sx, sy = mcrt.skin_texel(kind, m, face, tx, ty)
                    assert tex["pixels"][ty * w + tx].tobytes() == expected[sy, sx].tobytes(), (m, face, tx, ty, sx, sy)
                    texels += 1
            with pytest.raises(ValueError):
                mcrt.skin_texel(kind, m, face, w, 0)
            with pytest.raises(ValueError):
                mcrt.skin_texel(kind, m, face, 0, h)
    assert texels == sum(2 * (w * h + w * d + h * d) for w, h, d in ([(8, 8, 8)] * 2 + [(8, 12, 4)] + [(4, 12, 4)] * 4 if kind == "S32"
                                                                    else [(8, 8, 8)] * 2 + [(8, 12, 4)] * 2 + [(4, 12, 4)] * 8))
    assert mcrt.skin_texel(64 if kind == "S64" else 32, 0, 1 | abi.ID_OUTER, 0, 0) == mcrt.skin_texel(kind, 0, 1, 0, 0)  # flags of id.face are ignored
