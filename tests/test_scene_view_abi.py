"""Views of resident scenes (mcrt_scene_set_view*, mcrt_skin_view_table) without a device: the symbols, every argument check
that comes before any device work, and the host half of a view change — the table mcrt_skin_view_table flattens for a pose
and a look — against the flattener's own prefix of the full-table scene (tests/skin_paint_checker.py), byte for byte."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import layers_checker
import skin_paint_checker as S

MCRT_OK, MCRT_ERR_INVALID = 0, 1
NEW_SYMBOLS = ("mcrt_scene_set_view", "mcrt_scene_set_view_device", "mcrt_scene_set_views_batch_device", "mcrt_skin_view_table")
TABLE_BYTES = {"S64": 192 + 12 * 192, "S32": 192 + 7 * 192}
# FlatHeader words that describe the blob's layout: magic, n_meshes, n_texels, mesh / texel offset, blob_bytes, alpha offset / words
LAYOUT_WORDS = (0, 1, 2, 32, 33, 34, 35, 36)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")


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


def opaque_skin(kind) -> np.ndarray:
    a = np.array(S.skin("synthetic_" + kind), np.uint8)
    a[..., 3] = 255
    a.setflags(write=False)
    return a


def expected_table(kind, pose, look) -> bytes:
    blob = S.expected_blob(opaque_skin(kind), pose, look)
    return blob[:int(np.frombuffer(blob[:192], np.uint32)[33])]


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    with open(HEADER, encoding="utf-8") as f:
        header = f.read()
    assert "views of resident scenes" in header
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name
        assert f" {name}(" in header, name
    assert lib.mcrt_abi_version() == 3 and "#define MCRT_ABI_VERSION 3 " in header


@pytest.mark.parametrize("case", ["null_handle", "not_a_skin_handle"])
def test_single_forms_reject_bad_arguments(lib, case):
    plain = _fake(0, 0)
    handle = None if case == "null_handle" else C.addressof(plain)
    pose = np.zeros(12, np.float32)
    for p in (None, abi.fptr(pose)):
        _invalid(lib, lib.mcrt_scene_set_view(handle, p, None))
        _invalid(lib, lib.mcrt_scene_set_view_device(handle, p, None, None))
        if case == "not_a_skin_handle":
            assert b"mcrt_scene_create_skin" in lib.mcrt_last_error()


@pytest.mark.parametrize("case", ["n_negative", "null_array", "null_entry", "not_a_skin_handle", "mixed_kinds", "mixed_devices", "listed_twice"])
def test_batch_form_rejects_bad_arguments(lib, case):
    a, b = _fake(0, 64), _fake(0, 64)
    scenes, n = _handles(a, b), 2
    if case == "n_negative":
        n = -1
    elif case == "null_array":
        scenes = None
    elif case == "null_entry":
        scenes = _handles(a, None)
    elif case == "not_a_skin_handle":
        scenes = _handles(a, _fake(0, 0))
    elif case == "mixed_kinds":
        scenes = _handles(a, _fake(0, 32))
    elif case == "mixed_devices":
        scenes = _handles(a, _fake(1, 64))
    elif case == "listed_twice":
        scenes, n = _handles(a, b, a), 3
    poses = np.zeros((3, 12), np.float32)
    for p in (None, poses.ctypes.data):
        _invalid(lib, lib.mcrt_scene_set_views_batch_device(scenes, n, p, None, None))
    text = lib.mcrt_last_error()
    want = {"n_negative": b"n must be >= 0", "null_array": b"NULL argument", "null_entry": b"NULL scene handle in the batch",
            "not_a_skin_handle": b"mcrt_scene_create_skin", "mixed_kinds": b"one skin kind", "mixed_devices": b"one device", "listed_twice": b"listed twice"}[case]
    assert want in text, text


def test_no_handles_is_ok(lib):
    assert lib.mcrt_scene_set_views_batch_device(_handles(), 0, None, None, None) == MCRT_OK
    assert lib.mcrt_scene_set_views_batch_device(None, 0, None, None, None) == MCRT_OK


def test_view_table_rejects_a_bad_kind_and_honours_the_capacity(mcrt, lib):
    buf = C.create_string_buffer(b"\x5a" * 4096, 4096)
    for h in (48, 0, -64):
        assert lib.mcrt_skin_view_table(h, None, None, buf, 4096) == 0
        assert b"skin_height" in lib.mcrt_last_error()
    assert buf.raw == b"\x5a" * 4096
    assert lib.mcrt_skin_view_table(64, None, None, None, 0) == TABLE_BYTES["S64"]
    assert lib.mcrt_skin_view_table(32, None, None, None, 0) == TABLE_BYTES["S32"]
    assert lib.mcrt_skin_view_table(64, None, None, buf, 100) == TABLE_BYTES["S64"]
    assert buf.raw[:100] == mcrt.skin_view_table("S64")[:100] and buf.raw[100:] == b"\x5a" * (4096 - 100)


@pytest.mark.parametrize("kind", ["S64", "S32"])
def test_view_table_of_the_builtin_poses_is_the_flattened_prefix(mcrt, kind):
    poses = mcrt.getBuiltinPoses()
    assert len(poses) == 7
    base = np.frombuffer(mcrt.skin_view_table(kind, poses[0]), np.uint32)
    seen = set()
    for i, pose in enumerate(poses):
        for look in (None, S.LOOK):
            got = mcrt.skin_view_table(kind, pose, S.look_desc(look))
            assert len(got) == TABLE_BYTES[kind]
            assert got == expected_table(kind, pose, look), f"{kind} pose {i} look {'LOOK' if look else None}"
            words = np.frombuffer(got, np.uint32)
            assert [int(words[w]) for w in LAYOUT_WORDS] == [int(base[w]) for w in LAYOUT_WORDS]
            seen.add(got)
    assert len(seen) == 14
    # no pose and no look: the builder's own — pose 0 is all zeros
    assert mcrt.skin_view_table(kind) == mcrt.skin_view_table(kind, poses[0]) == mcrt.skin_view_table(kind, np.zeros(12, np.float32), None)


def _random_case(rng, i):
    """Random angles in +-180 degrees — some below rotatePoint's 0.01 degree gate, some exactly 0 — and a random look."""
    pose = rng.uniform(-180.0, 180.0, 12).astype(np.float32)
    tiny = rng.random(12) < 0.15
    pose[tiny] = rng.uniform(-0.02, 0.02, 12).astype(np.float32)[tiny]  # either side of the gate
    pose[rng.random(12) < 0.15] = 0.0
    if i % 25 == 0:
        pose[:] = rng.uniform(-0.009, 0.009, 12).astype(np.float32)  # every angle below the gate: an un-posed figure
    yaw, pitch, dist = rng.uniform(-180.0, 180.0), rng.uniform(-85.0, 85.0), rng.uniform(20.0, 90.0)
    target = (float(rng.uniform(-3, 3)), float(rng.uniform(10, 26)), float(rng.uniform(-3, 3)))
    y, p = math.radians(yaw), math.radians(pitch)
    cam = (target[0] + dist * math.cos(p) * math.sin(y), target[1] + dist * math.sin(p), target[2] + dist * math.cos(p) * math.cos(y))
    look = {"light_position": tuple(float(v) for v in rng.uniform(-60.0, 60.0, 3)), "light_color": (1.0, float(rng.uniform(0.5, 1.0)), float(rng.uniform(0.5, 1.0)), 1.0),
            "light_intensity": float(rng.uniform(0.2, 1.5)), "light_radius": float(rng.uniform(0.0, 8.0)), "camera_position": cam, "camera_target": target,
            "camera_up": (0.0, 1.0, 0.0), "camera_fov": float(rng.uniform(15.0, 110.0)),
            "background_color": tuple(float(v) for v in rng.uniform(0.0, 1.0, 3)) + (1.0,)}
    return pose, look


def test_view_table_of_random_views_is_the_flattened_prefix(mcrt):
    rng = np.random.default_rng(20261019)
    base = {k: np.frombuffer(mcrt.skin_view_table(k), np.uint32) for k in ("S64", "S32")}
    below_gate = zeros = 0
    for i in range(500):
        kind = "S64" if i % 2 == 0 else "S32"
        pose, look = _random_case(rng, i)
        below_gate += int(((np.abs(pose) <= 0.01) & (pose != 0)).sum())
        zeros += int((pose == 0).sum())
        got = mcrt.skin_view_table(kind, pose, S.look_desc(look))
        want = mcrt.flatten(S.full_table_scene(opaque_skin(kind), pose, look))
        assert got == want[:TABLE_BYTES[kind]], f"case {i}: {kind} pose {pose.tolist()} look {look}"
        words = np.frombuffer(got, np.uint32)
        assert [int(words[w]) for w in LAYOUT_WORDS] == [int(base[kind][w]) for w in LAYOUT_WORDS], f"case {i}"
    assert below_gate >= 100 and zeros >= 100


def test_orbit_look_is_the_checkers_orbit(mcrt):
    fields = S.LOOK_FIELDS

    def values(sd):
        d = sd.desc
        return [list(getattr(d, k)) if hasattr(getattr(d, k), "__len__") else getattr(d, k) for k in fields]

    for yaw, pitch, dist, target in [(0.0, 0.0, 50.0, None), (135.0, 20.0, 34.0, None), (250.0, -30.0, 30.0, (1.0, 17.5, -2.0)), (-40.0, 60.0, 28.0, (0.0, 18.0, 0.0))]:
        for base in (None, S.LOOK):
            args = (yaw, pitch, dist) + ((target,) if target is not None else ())
            want = layers_checker.orbit(S.apply_look(mcrt.MeshBuilder.buildDefaultScene(), base), *args)
            base_desc = S.look_desc(base)
            before = values(base_desc) if base_desc is not None else None
            got = mcrt.orbit_look(*args, base=base_desc)
            assert values(got) == values(want), (yaw, pitch, dist, target, base is not None)
            if base_desc is not None:
                assert values(base_desc) == before  # a copy: the base is not modified
    # the builder's default look is the repaintable figure's own
    assert mcrt.skin_view_table("S64", None, mcrt.orbit_look(0.0, 0.0, 50.0)) == mcrt.skin_view_table("S64")


def test_python_wrappers_check_their_arguments(mcrt):
    skinned = object.__new__(mcrt.DeviceScene)
    skinned._h, skinned.skin_height = C.c_void_p(), 64
    plain = object.__new__(mcrt.DeviceScene)
    plain._h = C.c_void_p()
    for bad in ([0.0] * 11, np.zeros((2, 12), np.float32)):
        with pytest.raises(ValueError):
            skinned.set_view(bad)
        with pytest.raises(ValueError):
            skinned.set_view_device(bad)
        with pytest.raises(ValueError):
            mcrt.skin_view_table("S64", bad)
    for call in (lambda: plain.set_view(np.zeros(12, np.float32)), lambda: plain.set_view_device(look=None)):
        with pytest.raises(ValueError):
            call()  # a scene that for_skin did not make
    for bad in ("S48", 48, True, None):
        with pytest.raises(ValueError):
            mcrt.skin_view_table(bad)
    with pytest.raises(TypeError):
        skinned.set_view(look=object())
    with pytest.raises(TypeError):
        mcrt.set_views_batch_device([object()])
    with pytest.raises(ValueError):
        mcrt.set_views_batch_device([skinned, skinned], poses=np.zeros((3, 12), np.float32))  # a count mismatch
    with pytest.raises(ValueError):
        mcrt.set_views_batch_device([skinned, skinned], looks=[None])
    mcrt.set_views_batch_device([])  # no scenes: nothing to do
