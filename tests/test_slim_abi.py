"""The slim player model at the C ABI without a device: the new symbols, every argument check that comes before any device
work, the `_model` entries with MCRT_SKIN_CLASSIC against the entries they extend, and the batch entries' rule — images of one
size — on zeroed blocks that stand in for handles."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import skin_paint_checker as S
import slim_checker as SL

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
CLASSIC, SLIM = 0, 1
NEW_SYMBOLS = ("mcrt_build_skin_scene_model", "mcrt_scene_create_skin_model", "mcrt_skin_texel_model", "mcrt_skin_pool_map_model",
               "mcrt_skin_view_table_model", "mcrt_skin_model_of")
u8_p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _invalid(lib, rc):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def _fake(device=0, skin_height=0, model=0):
    """A zeroed block that stands in for a handle in the checks that come before any device work: device index, skin height,
    (texel count,) model — the handle's first words."""
    block = (C.c_int32 * 8192)()
    block[0], block[1], block[3] = device, skin_height, model
    return block


def _handles(*blocks):
    arr = (C.c_void_p * max(len(blocks), 1))(*[C.addressof(b) for b in blocks])
    arr._keep = blocks
    return arr


def test_symbols_are_exported_declared_and_typed(lib):
    import os
    import re

    from minecraftskin_raytracer_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define MCRT_SKIN_CLASSIC 0\b", header) and re.search(r"#define MCRT_SKIN_SLIM 1\b", header)
    assert "heuristic" in header.lower()
    assert (abi.SKIN_CLASSIC, abi.SKIN_SLIM) == (CLASSIC, SLIM) and lib.mcrt_abi_version() == 3


@pytest.mark.parametrize("model,height", [(2, 64), (-1, 64), (SLIM, 32)])
def test_bad_models_are_invalid_everywhere(lib, model, height):
    image = np.full((height, 64, 4), 255, np.uint8)
    out = C.POINTER(abi.McrtSceneDesc)()
    assert lib.mcrt_build_skin_scene_model(image.ctypes.data_as(u8_p), 64, height, model, None, C.byref(out)) == MCRT_ERR_INVALID
    assert not out
    h = C.c_void_p(0x77)
    _invalid(lib, lib.mcrt_scene_create_skin_model(height, model, None, None, 0, C.byref(h)))
    assert h.value is None  # *out is cleared
    x, y = C.c_int(), C.c_int()
    _invalid(lib, lib.mcrt_skin_texel_model(height, model, 0, 0, 0, 0, C.byref(x), C.byref(y)))
    buf = np.zeros(4000, np.int32)
    _invalid(lib, lib.mcrt_skin_pool_map_model(height, model, buf.ctypes.data_as(abi.c_int32_p), len(buf)))
    assert lib.mcrt_skin_view_table_model(height, model, None, None, None, 0) == 0 and lib.mcrt_last_error()


def test_null_arguments_are_invalid(lib):
    image = np.full((64, 64, 4), 255, np.uint8)
    out = C.POINTER(abi.McrtSceneDesc)()
    assert lib.mcrt_build_skin_scene_model(None, 64, 64, SLIM, None, C.byref(out)) == MCRT_ERR_INVALID
    assert lib.mcrt_build_skin_scene_model(image.ctypes.data_as(u8_p), 64, 64, SLIM, None, None) == MCRT_ERR_INVALID
    _invalid(lib, lib.mcrt_scene_create_skin_model(64, SLIM, None, None, 0, None))
    x = C.c_int()
    _invalid(lib, lib.mcrt_skin_texel_model(64, SLIM, 0, 0, 0, 0, None, C.byref(x)))
    _invalid(lib, lib.mcrt_skin_texel_model(64, SLIM, 0, 0, 0, 0, C.byref(x), None))
    _invalid(lib, lib.mcrt_skin_pool_map_model(64, SLIM, None, 10))
    assert lib.mcrt_skin_model_of(None, 64, 64) == -1 and lib.mcrt_last_error()
    assert lib.mcrt_skin_model_of(image.ctypes.data_as(u8_p), 64, 48) == -1 and lib.mcrt_last_error()
    assert lib.mcrt_skin_model_of(image.ctypes.data_as(u8_p), 32, 64) == -1


def test_a_slim_arm_front_face_is_three_texels_wide(lib):
    x, y = C.c_int(), C.c_int()
    for mesh in SL.ARM_MESHES:
        for face in (0, 1, 4, 5):
            assert lib.mcrt_skin_texel_model(64, SLIM, mesh, face, 2, 0, C.byref(x), C.byref(y)) == MCRT_OK
            _invalid(lib, lib.mcrt_skin_texel_model(64, SLIM, mesh, face, 3, 0, C.byref(x), C.byref(y)))
            assert lib.mcrt_skin_texel_model(64, CLASSIC, mesh, face, 3, 0, C.byref(x), C.byref(y)) == MCRT_OK
        for face in (2, 3):  # the sides keep their four columns
            assert lib.mcrt_skin_texel_model(64, SLIM, mesh, face, 3, 11, C.byref(x), C.byref(y)) == MCRT_OK


@pytest.mark.parametrize("height", [64, 32])
def test_classic_model_entries_equal_the_old_entries(mcrt, lib, height):
    n = 3264 if height == 64 else 2016
    old, new = np.zeros(n + 8, np.int32), np.zeros(n + 8, np.int32)
    assert lib.mcrt_skin_pool_map(height, old.ctypes.data_as(abi.c_int32_p), len(old)) == n
    assert lib.mcrt_skin_pool_map_model(height, CLASSIC, new.ctypes.data_as(abi.c_int32_p), len(new)) == n
    assert np.array_equal(old, new)
    # skin_texel over every (mesh, face, tx, ty), one step beyond each range included
    a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    for mesh in range(-1, 13 if height == 64 else 8):
        for face in range(-1, 7):
            for ty in range(-1, 13):
                for tx in range(-1, 9):
                    r0 = lib.mcrt_skin_texel(height, mesh, face, tx, ty, C.byref(a), C.byref(b))
                    r1 = lib.mcrt_skin_texel_model(height, CLASSIC, mesh, face, tx, ty, C.byref(c), C.byref(d))
                    assert r0 == r1 and (r0 != MCRT_OK or (a.value, b.value) == (c.value, d.value)), (mesh, face, tx, ty)
    # the view table's bytes
    look = S.look_desc(S.LOOK)
    for pose, lk in ((None, None), (mcrt.getBuiltinPoses()[6], look)):
        p = abi.fptr(pose) if pose is not None else None
        q = lk.ptr if lk is not None else None
        size = lib.mcrt_skin_view_table(height, p, q, None, 0)
        assert size == (2496 if height == 64 else 1536) and lib.mcrt_skin_view_table_model(height, CLASSIC, p, q, None, 0) == size
        t0, t1 = C.create_string_buffer(size), C.create_string_buffer(size)
        assert lib.mcrt_skin_view_table(height, p, q, t0, size) == size and lib.mcrt_skin_view_table_model(height, CLASSIC, p, q, t1, size) == size
        assert t0.raw == t1.raw


@pytest.mark.parametrize("name", ["synthetic_S64", "synthetic_S32", "head_overlay_only", "all_transparent", "all_bytes", "inner_hole"])
@pytest.mark.parametrize("pose", [0, 6])
def test_classic_model_builder_equals_the_old_builder(mcrt, lib, name, pose):
    skin, p = np.ascontiguousarray(S.skin(name)), mcrt.getBuiltinPoses()[pose]
    blobs = []
    for build in (lambda out: lib.mcrt_build_skin_scene(skin.ctypes.data_as(u8_p), 64, skin.shape[0], abi.fptr(p), C.byref(out)),
                  lambda out: lib.mcrt_build_skin_scene_model(skin.ctypes.data_as(u8_p), 64, skin.shape[0], CLASSIC, abi.fptr(p), C.byref(out))):
        out = C.POINTER(abi.McrtSceneDesc)()
        assert build(out) == MCRT_OK and out
        blobs.append(mcrt.flatten(mcrt.SceneDesc(_native=out)))
    assert blobs[0] == blobs[1]
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, p)) == blobs[0] == mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, p, model="classic"))


def test_valid_create_skin_model_needs_a_device(mcrt, lib):
    h = C.c_void_p()
    rc = lib.mcrt_scene_create_skin_model(64, SLIM, abi.fptr(mcrt.getBuiltinPoses()[6]), S.look_desc(S.LOOK).ptr, 0, C.byref(h))
    if mcrt.device_count() > 0:
        assert rc == MCRT_OK and h.value
        lib.mcrt_scene_destroy(h)
    else:
        assert rc == MCRT_ERR_NO_DEVICE and h.value is None


# ---- the batch entries: images of one size ---------------------------------------------------------------------------------
def _after_the_checks(mcrt, rc):
    """What a batch call on fake handles ends with once every argument check has passed: the device error on a machine
    without a device — never MCRT_ERR_INVALID.  (With a device the fake handles must not travel further: not called.)"""
    assert mcrt.device_count() <= 0
    assert rc in (MCRT_ERR_NO_DEVICE, abi.MCRT_ERR_HIP), rc


def test_batches_may_mix_the_two_64x64_models(mcrt, lib):
    classic, slim = _fake(0, 64, CLASSIC), _fake(0, 64, SLIM)
    both = _handles(classic, slim)
    assert lib.mcrt_scene_set_skins_batch_device(both, 0, 0x10000, 64 * 64 * 4, None) == MCRT_OK
    assert lib.mcrt_scene_set_views_batch_device(both, 0, None, None, None) == MCRT_OK
    if mcrt.device_count() <= 0:
        _after_the_checks(mcrt, lib.mcrt_scene_set_skins_batch_device(both, 2, 0x10000, 64 * 64 * 4, None))
        _after_the_checks(mcrt, lib.mcrt_scene_set_views_batch_device(both, 2, None, None, None))


def test_batches_refuse_two_image_sizes(lib):
    mixed = _handles(_fake(0, 64, SLIM), _fake(0, 32, CLASSIC))
    _invalid(lib, lib.mcrt_scene_set_skins_batch_device(mixed, 2, 0x10000, 64 * 64 * 4, None))
    _invalid(lib, lib.mcrt_scene_set_views_batch_device(mixed, 2, None, None, None))
    mixed = _handles(_fake(0, 32, CLASSIC), _fake(0, 64, SLIM))
    _invalid(lib, lib.mcrt_scene_set_skins_batch_device(mixed, 2, 0x10000, 64 * 64 * 4, None))
    _invalid(lib, lib.mcrt_scene_set_views_batch_device(mixed, 2, None, None, None))
