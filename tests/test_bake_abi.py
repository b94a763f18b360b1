"""The light bake (mcrt_bake_light*) without a device: the symbols, every argument check that comes before any device work with
the planes untouched, the owner table (mcrt_bake_texel_table) on scenes that share a texture and on NULL / EMPTY textures, and
``pool_to_skin``.

The device forms are given opaque handle values, or zeroed blocks in which only the first three words of a handle are set —
device, skin_height, n_texels: every case fails, or is a no-op, on a check that does not look further inside a handle."""
import ctypes as C
import os

import numpy as np
import pytest

import bake_checker as B
import layers_checker as L
import scenes
from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_bake_light_device", "mcrt_bake_light_batch_device", "mcrt_bake_light", "mcrt_bake_texel_table", "mcrt_scene_texels")


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _planes(position=0x1000, normal=0x2000, visibility=0x3000, occlusion=0x4000, direct=0x5000):
    return abi.McrtBakePlanes(position or None, normal or None, visibility or None, occlusion or None, direct or None)


def _block(device=0, skin_height=0, n_texels=0):
    b = (C.c_int32 * 4096)()
    b[0], b[1], b[2] = device, skin_height, n_texels
    return b


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
    assert C.sizeof(abi.McrtBakePlanes) == 5 * C.sizeof(C.c_void_p)
    assert [f[0] for f in abi.McrtBakePlanes._fields_] == ["position", "normal", "visibility", "occlusion", "direct"]
    assert abi.BAKE_NAMES == ("position", "normal", "visibility", "occlusion", "direct") and abi.BAKE_MAX_GRID == 4
    assert {k: c for k, (_, c) in abi.BAKE_FORMATS.items()} == {"position": 4, "normal": 4, "visibility": 1, "occlusion": 1, "direct": 4}
    for name in ("bake_light_batch_device", "texel_table", "pool_to_skin"):
        assert name in mcrt.__all__ and callable(getattr(mcrt, name))
    assert callable(mcrt.TileRenderer.bakeLight) and callable(mcrt.DeviceScene.bake_light_device)
    assert isinstance(mcrt.DeviceScene.texels, property)


def test_the_header_declares_the_entry_points():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert "typedef struct mcrt_bake_planes {" in header and "#define MCRT_ABI_VERSION 3" in header
    assert "the one with the lowest mesh index, then the lowest face" in header  # the owner rule is part of the contract


# refused whatever planes are asked for / refused only with the occlusion plane
BAD_CONFIGS = {"shadow_samples_114": dict(shadowSamples=114)}
BAD_WITH_OCCLUSION = {"ao_samples_0": dict(aoSamples=0), "ao_samples_negative": dict(aoSamples=-4), "ao_samples_114": dict(aoSamples=114),
                      "ao_radius_nan": dict(aoRadius=float("nan")), "ao_radius_inf": dict(aoRadius=float("inf"))}
BAD_GRIDS = {"grid_0": 0, "grid_5": 5, "grid_negative": -1}


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "all_planes_null", *BAD_GRIDS, *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_single_device_form_rejects_bad_arguments(lib, case):
    cfg, planes, grid = _cfg(), _planes(), 1
    args = [C.c_void_p(0x10), C.byref(cfg), grid, C.byref(planes), None]
    if case == "null_cfg":
        args[1] = None
    elif case == "null_handle":
        args[0] = None
    elif case == "null_planes":
        args[3] = None
    elif case == "all_planes_null":
        planes = _planes(0, 0, 0, 0, 0)
        args[3] = C.byref(planes)
    elif case in BAD_GRIDS:
        args[2] = BAD_GRIDS[case]
    else:
        cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        args[1] = C.byref(cfg)
    _invalid(lib, lib.mcrt_bake_light_device(*args))


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_planes", "all_planes_null", "stride_too_small",
                                  "other_device", *BAD_GRIDS, *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_batch_device_form_rejects_bad_arguments(lib, case):
    cfg, planes = _cfg(), _planes()
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
        planes = _planes(0, 0, 0, 0, 0)
        a["out"] = C.byref(planes)
    elif case == "stride_too_small":  # below the second scene's 200 texels
        a["scenes"], a["stride"] = _handles(*[C.addressof(b) for b in blocks]), 199
    elif case == "other_device":
        blocks[1][0] = 1
        a["scenes"] = _handles(*[C.addressof(b) for b in blocks])
    elif case in BAD_GRIDS:
        a["grid"] = BAD_GRIDS[case]
    else:
        cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        a["cfg"] = C.byref(cfg)
    _invalid(lib, lib.mcrt_bake_light_batch_device(a["scenes"], a["n"], a["cfg"], a["grid"], a["out"], a["stride"], None))
    if case == "stride_too_small":
        assert b"texel_stride" in lib.mcrt_last_error()
    if case == "other_device":
        assert b"one device" in lib.mcrt_last_error()


def test_the_limits_and_the_no_ops(lib, mcrt):
    """Scenes without a texel are a no-op once the arguments are accepted: zeroed handle blocks hold 0 texels.  No frame size is
    read: a config of zero width is as good as any."""
    every, no_occlusion, only_occlusion = _planes(), _planes(occlusion=0), _planes(0, 0, 0, 0x4000, 0)
    cases = [(dict(shadowSamples=113), every, MCRT_OK), (dict(shadowSamples=114), every, MCRT_ERR_INVALID),
             (dict(shadowSamples=114), only_occlusion, MCRT_ERR_INVALID), (dict(shadowSamples=114, softShadows=False), every, MCRT_OK),
             (dict(aoSamples=1), every, MCRT_OK), (dict(aoSamples=113), every, MCRT_OK), (dict(aoSamples=0), every, MCRT_ERR_INVALID),
             (dict(aoSamples=114), only_occlusion, MCRT_ERR_INVALID),
             # without the occlusion plane the AO fields are not read
             (dict(aoSamples=0), no_occlusion, MCRT_OK), (dict(aoSamples=114), no_occlusion, MCRT_OK), (dict(aoRadius=float("nan")), no_occlusion, MCRT_OK),
             (dict(aoRadius=float("-inf")), every, MCRT_ERR_INVALID),
             (dict(aoRadius=0.0), every, MCRT_OK), (dict(aoRadius=-2.0), every, MCRT_OK), (dict(aoEnabled=True, aoIntensity=float("nan")), every, MCRT_OK),
             (dict(width=0, height=0, tileSize=0), every, MCRT_OK)]
    empty = _block()
    for kw, planes, rc in cases:
        cfg = _cfg(**kw)
        for grid in (1, 4):
            assert lib.mcrt_bake_light_device(C.c_void_p(C.addressof(empty)), C.byref(cfg), grid, C.byref(planes), None) == rc, kw
            assert lib.mcrt_bake_light_batch_device(_handles(C.addressof(empty)), 1, C.byref(cfg), grid, C.byref(planes), 0, None) == rc, kw
    cfg, planes = _cfg(), _planes()
    assert lib.mcrt_bake_light_batch_device(_handles(), 0, C.byref(cfg), 1, C.byref(planes), 0, None) == MCRT_OK
    assert lib.mcrt_bake_light_batch_device(None, 0, C.byref(cfg), 1, C.byref(planes), 0, None) == MCRT_OK
    n = C.c_int(-1)
    assert lib.mcrt_scene_texels(C.c_void_p(C.addressof(_block(0, 0, 3264))), C.byref(n)) == MCRT_OK and n.value == 3264
    _invalid(lib, lib.mcrt_scene_texels(None, C.byref(n)))
    _invalid(lib, lib.mcrt_scene_texels(C.c_void_p(C.addressof(empty)), None))


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_planes", "all_planes_null", *BAD_GRIDS, *BAD_CONFIGS, *BAD_WITH_OCCLUSION])
def test_host_form_rejects_bad_arguments_and_leaves_the_planes(mcrt, lib, case):
    sd = mcrt.SceneDesc(B.two_boxes())
    cfg = _cfg()
    keep = {k: np.full((192, c) if c > 1 else (192,), 7.0, np.float32) for k, (_, c) in abi.BAKE_FORMATS.items()}
    planes = abi.McrtBakePlanes(**{k: v.ctypes.data for k, v in keep.items()})
    d, c, grid, out = sd.ptr, C.byref(cfg), 1, C.byref(planes)
    if case == "null_desc":
        d = None
    elif case == "null_cfg":
        c = None
    elif case == "null_planes":
        out = None
    elif case == "all_planes_null":
        planes = abi.McrtBakePlanes(None, None, None, None, None)
        out = C.byref(planes)
    elif case in BAD_GRIDS:
        grid = BAD_GRIDS[case]
    else:
        cfg = _cfg(**{**BAD_CONFIGS, **BAD_WITH_OCCLUSION}[case])
        c = C.byref(cfg)
    _invalid(lib, lib.mcrt_bake_light(d, c, grid, out, 0))
    assert all(np.all(v == 7.0) for v in keep.values())


def test_host_form_without_device_reports_no_device(mcrt):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests bake
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.bakeLight(mcrt.SceneDesc(B.two_boxes()), abi.Config())
    assert e.value.code == MCRT_ERR_NO_DEVICE


def test_texel_table_of_scenes_that_share_a_texture(mcrt, lib):
    sd = mcrt.SceneDesc(B.two_boxes(shared=True))
    table = mcrt.texel_table(sd)
    assert table.shape == (64, 4) and table.dtype == np.int32
    ty, tx = np.mgrid[0:8, 0:8]
    # twelve faces reference the one texture: mesh 0's face 0 owns every texel
    assert np.array_equal(table, np.stack([np.zeros(64, int), np.zeros(64, int), tx.ravel(), ty.ravel()], axis=1))
    # a texture shared by LATER faces only: the owner is the lowest (mesh, face) among them
    own, common = L.face_textures(4, 3), L.face_textures(2, 2, seed=3)["top"]
    a = scenes.build_box(dict(own, top=common, bottom=common), (0.0, 10.0, 0.0), (2.0, 2.0, 2.0))
    b = scenes.build_box(common, (5.0, 10.0, 0.0), (2.0, 2.0, 2.0))
    sd = mcrt.SceneDesc(scenes.simple_scene([b, a]))  # mesh 0 = b: it owns the common texture through its face 0
    table = mcrt.texel_table(sd)
    _, meshes, _ = B.parse_blob(mcrt.flatten(sd))
    assert np.array_equal(table, B.owner_table(meshes, len(table)))
    off = int(meshes[1]["tex_off"][4])
    assert off == int(meshes[0]["tex_off"][0]) == int(meshes[1]["tex_off"][5]) and [list(r) for r in table[off:off + 4]] == [[0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 1, 1]]
    sd = mcrt.SceneDesc(scenes.simple_scene([a, b]))  # mesh 0 = a: its top face (slot 4) comes before its bottom face and before b
    table = mcrt.texel_table(sd)
    _, meshes, _ = B.parse_blob(mcrt.flatten(sd))
    assert np.array_equal(table, B.owner_table(meshes, len(table)))
    off = int(meshes[0]["tex_off"][4])
    assert (table[off:off + 4, :2] == (0, 4)).all() and len(table) == 4 * 12 + 4
    # capacity: the count is returned whatever fits, and nothing is written behind the capacity
    part = np.full((10, 4), 99, np.int32)
    assert lib.mcrt_bake_texel_table(sd.ptr, part.ctypes.data_as(abi.c_int32_p), 6) == len(table)
    assert np.array_equal(part[:6], table[:6]) and (part[6:] == 99).all()
    assert lib.mcrt_bake_texel_table(sd.ptr, None, 0) == len(table)
    assert lib.mcrt_bake_texel_table(None, None, 0) == -1 and lib.mcrt_last_error()


def test_texel_table_with_null_empty_and_unreferenced_textures(mcrt):
    sd = mcrt.SceneDesc(L.box_scene("null_and_empty")[0])
    table = mcrt.texel_table(sd)
    _, meshes, _ = B.parse_blob(mcrt.flatten(sd))
    assert len(table) == 2 * 5 * 12 and np.array_equal(table, B.owner_table(meshes, len(table)))
    assert int(meshes[0]["tex_off"][1]) == -1 and int(meshes[1]["tex_off"][1]) == -2  # NULL and EMPTY: no texel of the pool
    assert not ((table[:, 1] == 1) & (table[:, 0] >= 0)).any() and (table[:, 0] >= 0).all()
    # a texture no face references keeps its place in the pool and has no owner: a face takes the texture of its FIRST triangle
    # (intersection.cpp:124-129), so the texture of a second triangle alone is in the pool and on no face
    box = scenes.build_box(L.face_textures(4, 3), (0.0, 10.0, 0.0), (2.0, 2.0, 2.0))
    box.tri_texture[1] = abi.Texture(3, 2, np.ones((6, 4), np.float32))
    sd = mcrt.SceneDesc(scenes.simple_scene([box]))
    table = mcrt.texel_table(sd)
    _, meshes, _ = B.parse_blob(mcrt.flatten(sd))
    assert len(table) == 72 + 6 and np.array_equal(table, B.owner_table(meshes, len(table)))
    orphans = np.flatnonzero(table[:, 0] < 0)
    assert len(orphans) == 6 and [list(r) for r in table[orphans]] == [[-1, 0, -1, -1]] * 6
    assert mcrt.texel_table(scenes.simple_scene([])).shape == (0, 4)


def test_pool_to_skin(mcrt):
    for kind, h, n in (("S64", 64, 3264), ("S32", 32, 2016)):
        pmap = mcrt.skin_pool_map(kind)
        v = np.arange(n, dtype=np.float32)
        img = mcrt.pool_to_skin(kind, v, fill=-1.0)
        assert img.shape == (h, 64) and img.dtype == np.float32
        flat = img.reshape(-1)
        first = {}
        for i, p in enumerate(pmap):
            first.setdefault(int(p), i)  # the lowest pool index of a pixel wins
        assert len(first) == n if kind == "S64" else len(first) < n  # a legacy skin's mirrored limbs share pixels
        for p, i in first.items():
            assert flat[p] == i
        untouched = np.ones(h * 64, bool)
        untouched[pmap] = False
        assert (flat[untouched] == -1.0).all() and untouched.sum() == h * 64 - len(first)
        rgba = mcrt.pool_to_skin(h, np.stack([v, v + 1, v + 2, v + 3], axis=1), fill=0)
        assert rgba.shape == (h, 64, 4) and np.array_equal(rgba[..., 0].reshape(-1)[~untouched], flat[~untouched])
        assert (rgba.reshape(-1, 4)[untouched] == 0).all()
    for bad in (np.zeros(5), np.zeros((3264, 2, 2)), np.zeros(2016)):
        with pytest.raises(ValueError):
            mcrt.pool_to_skin("S64", bad)
    with pytest.raises(ValueError):
        mcrt.pool_to_skin("S16", np.zeros(3264))


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config()
    sd = mcrt.SceneDesc(B.two_boxes())
    for bad in (("direct", "colour"), (), "shadow", (3,)):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.bakeLight(sd, cfg, planes=bad)
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.bakeLight(sd, cfg, grid=bad)
    assert abi.bake_names(("direct", "position")) == ("position", "direct") and abi.bake_names("occlusion") == ("occlusion",)
    with pytest.raises(ValueError):
        mcrt.bake_light_batch_device([], cfg)  # no plane at all
    with pytest.raises(ValueError):
        mcrt.bake_light_batch_device([], cfg, grid=9, direct_ptr=0x1000)
    with pytest.raises(TypeError):
        mcrt.bake_light_batch_device([object()], cfg, direct_ptr=0x1000)
    mcrt.bake_light_batch_device([], cfg, occlusion_ptr=0x1000)  # no frames: nothing to do
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.bake_light_device(cfg)
    with pytest.raises(ValueError):
        ds.bake_light_device(cfg, grid=0, direct_ptr=0x1000)
