"""Skins on resident scenes (mcrt_scene_create_skin, mcrt_scene_set_skin*, mcrt_skin_pool_map, mcrt_probe_scene_blob) without a
device: the symbols, every argument check that comes before any device work, and the pool map against mcrt_skin_texel and
against the flattened pool of a marker skin."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import skin_paint_checker as S

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_scene_create_skin", "mcrt_scene_set_skin_device", "mcrt_scene_set_skins_batch_device", "mcrt_scene_set_skin",
               "mcrt_skin_pool_map", "mcrt_probe_scene_blob")
COUNTS = {"S64": 3264, "S32": 2016}


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _invalid(lib, rc):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def _fake(device=0, skin_height=0):
    """A zeroed block that stands in for a handle in the checks that come before any device work: those read the handle's
    device index and its skin kind, its first two words, and nothing else."""
    block = (C.c_int32 * 8192)()
    block[0], block[1] = device, skin_height
    return block


def _handles(*blocks):
    arr = (C.c_void_p * max(len(blocks), 1))(*[C.addressof(b) if b is not None else None for b in blocks])
    arr._keep = blocks
    return arr


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name


@pytest.mark.parametrize("case", ["null_out", "height_48", "height_0", "height_negative"])
def test_create_skin_rejects_bad_arguments(lib, case):
    h = C.c_void_p(0x77)
    if case == "null_out":
        _invalid(lib, lib.mcrt_scene_create_skin(64, None, None, 0, None))
        return
    height = {"height_48": 48, "height_0": 0, "height_negative": -64}[case]
    _invalid(lib, lib.mcrt_scene_create_skin(height, None, None, 0, C.byref(h)))
    assert h.value is None  # *out is cleared


@pytest.mark.parametrize("kind", [64, 32])
def test_valid_create_skin_needs_a_device(mcrt, lib, kind):
    h = C.c_void_p()
    pose = mcrt.getBuiltinPoses()[6]
    look = S.look_desc(S.LOOK)
    rc = lib.mcrt_scene_create_skin(kind, abi.fptr(pose), look.ptr, 0, C.byref(h))
    if mcrt.device_count() > 0:
        assert rc == MCRT_OK and h.value
        lib.mcrt_scene_destroy(h)
    else:
        assert rc == MCRT_ERR_NO_DEVICE and h.value is None


@pytest.mark.parametrize("case", ["null_handle", "null_image", "not_a_skin_handle"])
def test_single_forms_reject_bad_arguments(lib, case):
    image = np.zeros((64, 64, 4), np.uint8)
    skin_handle, plain = _fake(0, 64), _fake(0, 0)
    handle = {"null_handle": None, "null_image": C.addressof(skin_handle), "not_a_skin_handle": C.addressof(plain)}[case]
    ptr = None if case == "null_image" else image.ctypes.data
    _invalid(lib, lib.mcrt_scene_set_skin_device(handle, ptr, None))
    _invalid(lib, lib.mcrt_scene_set_skin(handle, image.ctypes.data_as(C.POINTER(C.c_uint8)) if ptr else None))
    if case == "not_a_skin_handle":
        assert b"mcrt_scene_create_skin" in lib.mcrt_last_error()


@pytest.mark.parametrize("case", ["n_negative", "null_array", "null_entry", "null_images", "stride_not_multiple_of_4", "stride_too_small_64",
                                  "stride_too_small_32", "not_a_skin_handle", "mixed_kinds", "mixed_devices", "listed_twice",
                                  "images_not_aligned"])
def test_batch_form_rejects_bad_arguments(lib, case):
    a, b = _fake(0, 64), _fake(0, 64)
    args = dict(scenes=_handles(a, b), n=2, skins=0x10000, stride=64 * 64 * 4)
    if case == "n_negative":
        args["n"] = -1
    elif case == "null_array":
        args["scenes"] = None
    elif case == "null_entry":
        args["scenes"] = _handles(a, None)
    elif case == "null_images":
        args["skins"] = None
    elif case == "stride_not_multiple_of_4":
        args["stride"] = 64 * 64 * 4 + 2
    elif case == "stride_too_small_64":  # the size of a 64x32 image given to 64x64 handles
        args["stride"] = 64 * 32 * 4
    elif case == "stride_too_small_32":
        args["scenes"], args["stride"] = _handles(_fake(0, 32), _fake(0, 32)), 64 * 32 * 4 - 4
    elif case == "not_a_skin_handle":
        args["scenes"] = _handles(a, _fake(0, 0))
    elif case == "mixed_kinds":
        args["scenes"] = _handles(a, _fake(0, 32))
    elif case == "mixed_devices":
        args["scenes"] = _handles(a, _fake(1, 64))
    elif case == "listed_twice":
        args["scenes"] = _handles(a, b, a)
        args["n"] = 3
    elif case == "images_not_aligned":
        args["skins"] = 0x10002
    _invalid(lib, lib.mcrt_scene_set_skins_batch_device(args["scenes"], args["n"], args["skins"], args["stride"], None))


def test_no_handles_is_ok(lib):
    assert lib.mcrt_scene_set_skins_batch_device(_handles(), 0, 0x10000, 64 * 64 * 4, None) == MCRT_OK
    assert lib.mcrt_scene_set_skins_batch_device(None, 0, 0x10000, 0, None) == MCRT_OK


def test_blob_probe_rejects_null_arguments(lib):
    buf = C.create_string_buffer(192)
    _invalid(lib, lib.mcrt_probe_scene_blob(None, buf, 192))
    block = _fake()
    _invalid(lib, lib.mcrt_probe_scene_blob(C.addressof(block), None, 0))


@pytest.mark.parametrize("case", ["null_out", "height_48", "height_0"])
def test_pool_map_rejects_bad_arguments(lib, case):
    out = np.full(8, -7, np.int32)
    if case == "null_out":
        _invalid(lib, lib.mcrt_skin_pool_map(64, None, 8))
    else:
        _invalid(lib, lib.mcrt_skin_pool_map(48 if case == "height_48" else 0, out.ctypes.data_as(abi.c_int32_p), 8))
    assert (out == -7).all()


@pytest.mark.parametrize("kind", ["S64", "S32"])
def test_pool_map_follows_skin_texel(mcrt, lib, kind):
    height, n_meshes = (64, 12) if kind == "S64" else (32, 7)
    got = mcrt.skin_pool_map(kind)
    assert got.dtype == np.int32 and len(got) == COUNTS[kind]
    walked = []
    for m in range(n_meshes):
        for face in range(6):
            w = h = 0  # the face's size: the first tx / ty that mcrt_skin_texel refuses
            while True:
                try:
                    mcrt.skin_texel(kind, m, face, w, 0)
                    w += 1
                except ValueError:
                    break
            while True:
                try:
                    mcrt.skin_texel(kind, m, face, 0, h)
                    h += 1
                except ValueError:
                    break
            for ty in range(h):
                for tx in range(w):
                    x, y = mcrt.skin_texel(kind, m, face, tx, ty)
                    walked.append(y * 64 + x)
    assert got.tolist() == walked
    assert got.min() >= 0 and got.max() < 64 * height
    # a short buffer takes the first entries and the count is still returned
    short = np.full(10, -7, np.int32)
    assert lib.mcrt_skin_pool_map(height, short.ctypes.data_as(abi.c_int32_p), 7) == COUNTS[kind]
    assert short[:7].tolist() == walked[:7] and (short[7:] == -7).all()
    assert lib.mcrt_skin_pool_map(height, short.ctypes.data_as(abi.c_int32_p), 0) == COUNTS[kind]


@pytest.mark.parametrize("kind,pose", [("S64", 0), ("S32", 5)])
def test_pool_map_names_the_flattened_pool(mcrt, kind, pose):
    height = 64 if kind == "S64" else 32
    y, x = np.mgrid[0:height, 0:64]
    marker = np.stack([x, y, np.full_like(x, 9), np.full_like(x, 255)], axis=-1).astype(np.uint8)  # r = x, g = y, opaque
    blob = mcrt.flatten(mcrt.MeshBuilder.buildScene(marker, mcrt.getBuiltinPoses()[pose]))
    hdr = np.frombuffer(blob[:192], np.uint32)
    n_texels, texel_off = int(hdr[2]), int(hdr[33])
    assert n_texels == COUNTS[kind]
    pool = np.frombuffer(blob[texel_off:texel_off + 16 * n_texels], np.float32).reshape(n_texels, 4)
    want = (marker.reshape(-1, 4).astype(np.float32) / np.float32(255.0))[mcrt.skin_pool_map(kind)]
    assert pool.tobytes() == want.tobytes()


def test_python_wrappers_check_their_arguments(mcrt):
    for bad in ("S48", 48, True, None):
        with pytest.raises(ValueError):
            mcrt.skin_pool_map(bad)
        with pytest.raises(ValueError):
            mcrt.DeviceScene.for_skin(bad)
    with pytest.raises(ValueError):
        mcrt.DeviceScene.for_skin("S64", pose=[0.0] * 11)
    plain = object.__new__(mcrt.DeviceScene)  # a scene that for_skin did not make
    plain._h = C.c_void_p()
    for call in (lambda: plain.set_skin(np.zeros((64, 64, 4), np.uint8)), lambda: plain.set_skin_device(0x1000)):
        with pytest.raises(ValueError):
            call()
    skinned = object.__new__(mcrt.DeviceScene)
    skinned._h, skinned.skin_height = C.c_void_p(), 32
    with pytest.raises(ValueError):
        skinned.set_skin(np.zeros((64, 64, 4), np.uint8))  # a 64x64 image for a 64x32 scene
    with pytest.raises(TypeError):
        mcrt.set_skins_batch_device([object()], 0x1000)
    mcrt.set_skins_batch_device([], 0x1000)  # no scenes: nothing to do


def test_expected_blob_of_the_checker_is_the_builders_for_an_opaque_skin(mcrt):
    """With no transparent texel the full-table scene IS buildScene's: the checker's texel-by-texel rewrite through skin_texel
    must give the very blob the flattener gives for the builder's scene."""
    pose = mcrt.getBuiltinPoses()[6]
    skin = S.skin("all_opaque")
    assert S.expected_blob(skin, pose) == mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose))
    assert S.expected_blob(skin, pose, S.LOOK) == mcrt.flatten(S.reference_scene(skin, pose, S.LOOK))
    assert S.expected_blob(skin, pose, S.LOOK) != S.expected_blob(skin, pose)
