"""Capes at the C ABI without a device: the new symbols, every refusal that comes before any device work with its message,
the builder entry with and without a cape, and the batch entries' rule — all caped or all capeless — on zeroed blocks that
stand in for handles."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import cape_checker as CK
import skin_paint_checker as S

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
CLASSIC, SLIM = 0, 1
NEW_SYMBOLS = ("mcrt_build_skin_scene_cape", "mcrt_cape_texel", "mcrt_cape_pool_map", "mcrt_scene_create_skin_cape", "mcrt_scene_set_cape",
               "mcrt_scene_set_cape_device", "mcrt_scene_set_capes_batch_device", "mcrt_skin_view_table_cape", "mcrt_scene_set_view_cape",
               "mcrt_scene_set_view_cape_device", "mcrt_scene_set_views_cape_batch_device")
u8_p = C.POINTER(C.c_uint8)
CAPE_BYTES = 64 * 32 * 4


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _invalid(lib, rc, message):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert message in lib.mcrt_last_error().decode(), lib.mcrt_last_error()


def _fake(device=0, skin_height=0, model=0, cape=0):
    """A zeroed block that stands in for a handle in the checks that come before any device work: device index, skin height,
    (texel count,) model, cape — the handle's first words."""
    block = (C.c_int32 * 8192)()
    block[0], block[1], block[3], block[4] = device, skin_height, model, cape
    return block


def _handles(*blocks):
    arr = (C.c_void_p * max(len(blocks), 1))(*[C.addressof(b) for b in blocks])
    arr._keep = blocks
    return arr


def _after_the_checks(mcrt, rc):
    """What a call on fake handles ends with once every argument check has passed: the device error on a machine without a
    device — never MCRT_ERR_INVALID.  (With a device the fake handles must not travel further: not called.)"""
    assert mcrt.device_count() <= 0
    assert rc in (MCRT_ERR_NO_DEVICE, abi.MCRT_ERR_HIP), rc


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
    assert "---- capes" in header and "does NOT follow" in header
    assert lib.mcrt_abi_version() == 3


@pytest.mark.parametrize("kind", ["S64", "S64S", "S32"])
def test_builder_entry_with_and_without_a_cape(mcrt, lib, kind):
    height, model, n_skin = CK.KINDS[kind]
    skin, p = np.ascontiguousarray(CK.skin(kind)), mcrt.getBuiltinPoses()[6]
    m = SLIM if model == "slim" else CLASSIC

    def build(cape, angle):
        out = C.POINTER(abi.McrtSceneDesc)()
        rc = lib.mcrt_build_skin_scene_cape(skin.ctypes.data_as(u8_p), 64, height, m, abi.fptr(p), cape.ctypes.data_as(u8_p) if cape is not None else None,
                                            angle, C.byref(out))
        assert rc == MCRT_OK and out
        return mcrt.SceneDesc(_native=out)

    today = C.POINTER(abi.McrtSceneDesc)()
    assert lib.mcrt_build_skin_scene_model(skin.ctypes.data_as(u8_p), 64, height, m, abi.fptr(p), C.byref(today)) == MCRT_OK
    today = mcrt.flatten(mcrt.SceneDesc(_native=today))
    assert mcrt.flatten(build(None, 10.0)) == today
    assert mcrt.flatten(build(None, float("nan"))) == today  # without a cape the angle is not read
    assert mcrt.flatten(build(np.ascontiguousarray(CK.cape("transparent")), 10.0)) == today
    caped = build(np.ascontiguousarray(CK.cape("synthetic")), 10.0)
    assert caped.desc.n_meshes == build(None, 10.0).desc.n_meshes + 1
    assert mcrt.flatten(caped) == mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, p, model=model, cape=CK.cape("synthetic"), cape_angle=10.0))
    # an opaque skin and cape: the full table, the blob the checker expects of a repainted handle
    opaque = skin.copy()
    opaque[..., 3] = 255
    full = mcrt.MeshBuilder.buildScene(opaque, p, model=model, cape=CK.cape("all_bytes"), cape_angle=45.0)
    assert full.desc.n_meshes == n_skin + 1
    assert mcrt.flatten(full) == CK.expected_blob(kind, opaque, CK.cape("all_bytes"), p, 45.0)


def test_builder_refusals(lib):
    skin, cape = np.ascontiguousarray(S.skin("synthetic_S64")), np.ascontiguousarray(CK.cape("synthetic"))
    out = C.POINTER(abi.McrtSceneDesc)()
    s, c = skin.ctypes.data_as(u8_p), cape.ctypes.data_as(u8_p)
    _invalid(lib, lib.mcrt_build_skin_scene_cape(None, 64, 64, CLASSIC, None, c, 10.0, C.byref(out)), "NULL argument")
    _invalid(lib, lib.mcrt_build_skin_scene_cape(s, 64, 64, CLASSIC, None, c, 10.0, None), "NULL argument")
    _invalid(lib, lib.mcrt_build_skin_scene_cape(s, 64, 48, CLASSIC, None, c, 10.0, C.byref(out)), "a skin image is 64x64 or 64x32")
    _invalid(lib, lib.mcrt_build_skin_scene_cape(s, 64, 32, SLIM, None, c, 10.0, C.byref(out)), "model must be")
    for angle in (-0.001, 90.001, float("nan"), float("inf"), -float("inf")):
        _invalid(lib, lib.mcrt_build_skin_scene_cape(s, 64, 64, CLASSIC, None, c, angle, C.byref(out)), "cape_angle must be within 0 .. 90 degrees")
    assert not out
    for angle in (0.0, 90.0):
        assert lib.mcrt_build_skin_scene_cape(s, 64, 64, CLASSIC, None, c, angle, C.byref(out)) == MCRT_OK
        lib.mcrt_scene_desc_free(out)


def test_map_refusals(lib):
    x, y = C.c_int(), C.c_int()
    _invalid(lib, lib.mcrt_cape_texel(0, 0, 0, None, C.byref(y)), "NULL argument")
    _invalid(lib, lib.mcrt_cape_texel(0, 0, 0, C.byref(x), None), "NULL argument")
    _invalid(lib, lib.mcrt_cape_texel(6, 0, 0, C.byref(x), C.byref(y)), "face_slot must be 0..5")
    _invalid(lib, lib.mcrt_cape_texel(2, 1, 0, C.byref(x), C.byref(y)), "texel outside the face's region")
    _invalid(lib, lib.mcrt_cape_pool_map(None, 372), "NULL argument")
    short = np.full(16, -7, np.int32)
    assert lib.mcrt_cape_pool_map(short.ctypes.data_as(abi.c_int32_p), 10) == 372  # the count; `capacity` entries written
    assert (short[:10] >= 0).all() and (short[10:] == -7).all()
    # skin_texel keeps refusing the cape's mesh index
    _invalid(lib, lib.mcrt_skin_texel_model(64, CLASSIC, 12, 0, 0, 0, C.byref(x), C.byref(y)), "mesh must be 0..11")
    _invalid(lib, lib.mcrt_skin_texel_model(32, CLASSIC, 7, 0, 0, 0, C.byref(x), C.byref(y)), "mesh must be 0..6")


def test_create_and_view_table_refusals(mcrt, lib):
    h = C.c_void_p(0x77)
    _invalid(lib, lib.mcrt_scene_create_skin_cape(48, CLASSIC, None, None, 10.0, 0, C.byref(h)), "skin_height must be 64 or 32")
    assert h.value is None  # *out is cleared
    _invalid(lib, lib.mcrt_scene_create_skin_cape(32, SLIM, None, None, 10.0, 0, C.byref(h)), "model must be")
    _invalid(lib, lib.mcrt_scene_create_skin_cape(64, CLASSIC, None, None, 10.0, 0, None), "out is NULL")
    for angle in (-1.0, 91.0, float("nan")):
        _invalid(lib, lib.mcrt_scene_create_skin_cape(64, CLASSIC, None, None, angle, 0, C.byref(h)), "cape_angle must be within 0 .. 90 degrees")
        assert lib.mcrt_skin_view_table_cape(64, CLASSIC, None, None, angle, None, 0) == 0
        assert b"cape_angle must be within 0 .. 90 degrees" in lib.mcrt_last_error()
    assert lib.mcrt_skin_view_table_cape(64, 2, None, None, 10.0, None, 0) == 0 and lib.mcrt_skin_view_table_cape(48, CLASSIC, None, None, 10.0, None, 0) == 0
    assert lib.mcrt_skin_view_table_cape(64, SLIM, None, None, 10.0, None, 0) == 2688 and lib.mcrt_skin_view_table_cape(32, CLASSIC, None, None, 10.0, None, 0) == 1728
    rc = lib.mcrt_scene_create_skin_cape(64, SLIM, None, None, 10.0, 0, C.byref(h))
    if mcrt.device_count() > 0:
        assert rc == MCRT_OK and h.value
        lib.mcrt_scene_destroy(h)
    else:
        assert rc == MCRT_ERR_NO_DEVICE and h.value is None


def test_set_cape_refusals(mcrt, lib):
    cape = np.ascontiguousarray(CK.cape("synthetic"))
    capeless, foreign, caped = _fake(0, 64, CLASSIC, 0), _fake(0, 0), _fake(0, 64, CLASSIC, 1)
    for form in (lambda h: lib.mcrt_scene_set_cape(h, cape.ctypes.data_as(u8_p)), lambda h: lib.mcrt_scene_set_cape_device(h, 0x10000, None)):
        _invalid(lib, form(None), "NULL argument")
        _invalid(lib, form(C.addressof(capeless)), "no cape")
        _invalid(lib, form(C.addressof(foreign)), "mcrt_scene_create_skin_cape")
    one = _handles(caped)
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(one, -1, 0x10000, CAPE_BYTES, None), "n must be >= 0")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(None, 1, 0x10000, CAPE_BYTES, None), "NULL argument")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device((C.c_void_p * 1)(None), 1, 0x10000, CAPE_BYTES, None), "NULL scene handle in the batch")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(one, 1, 0x10000, CAPE_BYTES + 2, None), "cape_stride_bytes must be a multiple of 4")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(one, 1, 0x10002, CAPE_BYTES, None), "aligned to 4 bytes")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(one, 1, 0x10000, CAPE_BYTES - 4, None), "cape_stride_bytes is smaller than the cape image")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(_handles(caped, caped), 2, 0x10000, CAPE_BYTES, None), "listed twice")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(_handles(caped, _fake(1, 64, CLASSIC, 1)), 2, 0x10000, CAPE_BYTES, None), "one device")
    _invalid(lib, lib.mcrt_scene_set_capes_batch_device(_handles(caped, _fake(0, 32, CLASSIC, 1)), 2, 0x10000, CAPE_BYTES, None), "images of one size")
    assert lib.mcrt_scene_set_capes_batch_device(one, 0, None, 0, None) == MCRT_OK
    if mcrt.device_count() <= 0:  # accepted: a stride of 0, a NULL image, the two 64x64 models mixed
        both = _handles(caped, _fake(0, 64, SLIM, 1))
        _after_the_checks(mcrt, lib.mcrt_scene_set_capes_batch_device(both, 2, 0x10000, 0, None))
        _after_the_checks(mcrt, lib.mcrt_scene_set_capes_batch_device(both, 2, None, CAPE_BYTES, None))
        _after_the_checks(mcrt, lib.mcrt_scene_set_capes_batch_device(both, 2, 0x10004, CAPE_BYTES + 64, None))


def test_batches_are_all_caped_or_all_capeless(mcrt, lib):
    message = "all have a cape or all have none"
    for a, b in ((_fake(0, 64, CLASSIC, 1), _fake(0, 64, CLASSIC, 0)), (_fake(0, 64, SLIM, 0), _fake(0, 64, CLASSIC, 1)), (_fake(0, 32, CLASSIC, 0), _fake(0, 32, CLASSIC, 1))):
        mixed = _handles(a, b)
        _invalid(lib, lib.mcrt_scene_set_skins_batch_device(mixed, 2, 0x10000, 64 * 64 * 4, None), message)
        _invalid(lib, lib.mcrt_scene_set_views_batch_device(mixed, 2, None, None, None), message)
        _invalid(lib, lib.mcrt_scene_set_views_cape_batch_device(mixed, 2, None, None, None, None), message)
        _invalid(lib, lib.mcrt_scene_set_capes_batch_device(mixed, 2, 0x10000, CAPE_BYTES, None), message)
    if mcrt.device_count() <= 0:  # all caped, the two 64x64 models mixed: accepted
        both = _handles(_fake(0, 64, CLASSIC, 1), _fake(0, 64, SLIM, 1))
        _after_the_checks(mcrt, lib.mcrt_scene_set_skins_batch_device(both, 2, 0x10000, 64 * 64 * 4, None))
        _after_the_checks(mcrt, lib.mcrt_scene_set_views_batch_device(both, 2, None, None, None))


def test_view_cape_angle_refusals(mcrt, lib):
    caped, capeless = _fake(0, 64, CLASSIC, 1), _fake(0, 64, CLASSIC, 0)
    angles = np.array([10.0, 95.0], np.float32)
    _invalid(lib, lib.mcrt_scene_set_views_cape_batch_device(_handles(caped, _fake(0, 64, SLIM, 1)), 2, None, None, angles.ctypes.data, None),
             "cape_angle must be within 0 .. 90 degrees")
    _invalid(lib, lib.mcrt_scene_set_views_cape_batch_device(_handles(capeless), 1, None, None, angles.ctypes.data, None), "a handle without a cape")
    nan = np.array([np.nan], np.float32)
    _invalid(lib, lib.mcrt_scene_set_view_cape(C.addressof(caped), None, None, abi.fptr(nan)), "cape_angle must be within 0 .. 90 degrees")
    _invalid(lib, lib.mcrt_scene_set_view_cape_device(C.addressof(capeless), None, None, abi.fptr(angles), None), "a handle without a cape")
    _invalid(lib, lib.mcrt_scene_set_view_cape(None, None, None, abi.fptr(angles)), "NULL argument")


def test_python_refusals_without_a_handle(mcrt):
    with pytest.raises(ValueError, match="cape_angle must be within 0 .. 90 degrees"):
        mcrt.DeviceScene.for_skin("S64", cape=True, cape_angle=120.0)
    fake = object.__new__(mcrt.DeviceScene)  # a capeless repaintable scene, as far as the Python checks look
    fake._h, fake.skin_height = C.c_void_p(), 64
    for call in (lambda: fake.set_cape(CK.cape("synthetic")), lambda: fake.set_cape(None), lambda: fake.set_cape_device(0x10000),
                 lambda: fake.set_view(cape_angle=10.0), lambda: fake.set_view_device(cape_angle=10.0)):
        with pytest.raises(ValueError, match="this scene has no cape"):
            call()
    fake.has_cape = True
    with pytest.raises(ValueError, match="a cape image is"):
        fake.set_cape(np.zeros((64, 64, 4), np.uint8))
    with pytest.raises(ValueError, match="cape_angle must be within 0 .. 90 degrees"):
        fake.set_view(cape_angle=float("nan"))
    # SkinBatch's own checks (no device is touched by them)
    batch = object.__new__(mcrt.SkinBatch)
    batch.cape, batch.scenes, batch.slim_scenes = False, [], []
    with pytest.raises(ValueError, match="this batch holds no capes"):
        batch._check_capes([None], 1)
    with pytest.raises(ValueError, match="this batch holds no capes"):
        batch.set_views(cape_angles=10.0)
    assert batch._check_capes(None, 3) is None
    batch.cape = True
    assert batch._check_capes(None, 2).shape == (2, 32, 64, 4) and not batch._check_capes(None, 2).any()
    got = batch._check_capes([CK.cape("synthetic"), None], 2)
    assert np.array_equal(got[0], CK.cape("synthetic")) and not got[1].any()
    with pytest.raises(ValueError, match="one image"):
        batch._check_capes([None], 2)
    with pytest.raises(ValueError, match="a cape image is"):
        batch._check_capes([np.zeros((64, 64, 4), np.uint8)], 1)
