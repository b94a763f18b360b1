"""The ground-occlusion pass (mcrt_render_ground_occlusion*) and the studio shot's floor-occlusion entries (mcrt_*_occ) without a
device: the symbols, every argument check that comes before any device work with the argument named in mcrt_last_error, the
no-ops, the scratch layout, and abi.Shot's unchanged round trip.

The device forms are given opaque handle values (or zeroed blocks that differ in the device index, the first member of a
handle): every case fails — or is a no-op — on a check that does not look further inside a handle."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID = 0, 1
PASS_SYMBOLS = ("mcrt_render_ground_occlusion_device", "mcrt_render_ground_occlusion_batch_device", "mcrt_render_ground_occlusion")
SHOT_SYMBOLS = ("mcrt_shot_scratch_bytes_occ", "mcrt_render_shot_batch_device_occ", "mcrt_composite_shot_batch_device_occ",
                "mcrt_render_shot_batch_occ", "mcrt_render_shot_png_occ")
W, H = 64, 32


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    kw.setdefault("aoSamples", 8)
    kw.setdefault("aoRadius", 3.0)
    return abi.Config(**kw).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _heights(*values):
    return (C.c_float * max(len(values), 1))(*values)


def _planes(occlusion=0x1000, matte=0x2000):
    return abi.McrtGroundOcclusion(occlusion or None, matte or None)


def _invalid(lib, rc, names=None):
    text = lib.mcrt_last_error()
    assert rc == MCRT_ERR_INVALID, text
    assert text
    if names is not None:
        assert names.encode() in text, (names, text)


# what mcrt_last_error must name, per mistake
NAMES = {"null_cfg": "NULL", "null_handle": "NULL", "null_planes": "NULL", "null_array": "NULL", "null_entry": "NULL scene handle",
         "null_heights": "NULL", "both_planes_null": "both planes", "ground_nan": "ground_y", "ground_inf": "ground_y",
         "second_height_nan": "ground_y", "height_inf": "ground_y", "samples_0": "ao_samples", "samples_negative": "ao_samples",
         "samples_114": "ao_samples", "radius_nan": "ao_radius", "radius_inf": "ao_radius", "n_negative": "n_frames",
         "stride_too_small": "frame_stride_pixels"}
CONFIG_CASES = {"samples_0": dict(aoSamples=0), "samples_negative": dict(aoSamples=-3), "samples_114": dict(aoSamples=114),
                "radius_nan": dict(aoRadius=float("nan")), "radius_inf": dict(aoRadius=float("inf"))}


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in PASS_SYMBOLS + SHOT_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes, name
    assert lib.mcrt_abi_version() == 3
    assert C.sizeof(abi.McrtGroundOcclusion) == 2 * C.sizeof(C.c_void_p)
    assert abi.GROUND_OCCLUSION_NAMES == ("occlusion", "matte") and abi.GROUND_OCCLUSION_MAX_SAMPLES == 113


@pytest.mark.parametrize("case", ["null_cfg", "null_handle", "null_planes", "both_planes_null", "ground_nan", "ground_inf", *CONFIG_CASES])
def test_single_device_form_rejects_bad_arguments(lib, case):
    cfg, planes, g = _cfg(width=W, height=H), _planes(), 0.0
    args = [C.c_void_p(0x10), C.byref(cfg), C.byref(planes), None]
    if case == "null_cfg":
        args[1] = None
    elif case == "null_handle":
        args[0] = None
    elif case == "null_planes":
        args[2] = None
    elif case == "both_planes_null":
        planes = _planes(0, 0)
        args[2] = C.byref(planes)
    elif case == "ground_nan":
        g = float("nan")
    elif case == "ground_inf":
        g = float("-inf")
    else:
        cfg = _cfg(width=W, height=H, **CONFIG_CASES[case])
        args[1] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_ground_occlusion_device(args[0], args[1], g, args[2], args[3]), NAMES[case])


@pytest.mark.parametrize("case", ["n_negative", "null_cfg", "null_array", "null_entry", "null_heights", "null_planes", "both_planes_null",
                                  "stride_too_small", "second_height_nan", "height_inf", *CONFIG_CASES])
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
    elif case == "both_planes_null":
        planes = _planes(0, 0)
        a["out"] = C.byref(planes)
    elif case == "stride_too_small":
        a["stride"] = W * H - 1
    elif case == "second_height_nan":
        a["g"] = _heights(0.0, float("nan"))
    elif case == "height_inf":
        a["g"] = _heights(float("inf"), 0.0)
    else:
        cfg = _cfg(width=W, height=H, **CONFIG_CASES[case])
        a["cfg"] = C.byref(cfg)
    _invalid(lib, lib.mcrt_render_ground_occlusion_batch_device(a["scenes"], a["n"], a["cfg"], a["g"], a["out"], a["stride"], None), NAMES[case])


def test_handles_on_different_devices_are_rejected(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    cfg, planes = _cfg(width=W, height=H), _planes()
    arr = _handles(*[C.addressof(b) for b in blocks])
    _invalid(lib, lib.mcrt_render_ground_occlusion_batch_device(arr, 2, C.byref(cfg), _heights(0.0, 0.0), C.byref(planes), W * H, None), "one device")


@pytest.mark.parametrize("case", ["null_cfg", "null_scene", "null_planes", "both_planes_null", "ground_nan", *CONFIG_CASES])
def test_host_form_rejects_bad_arguments(lib, mcrt, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(W * H, 7.0, np.float32)
    cfg, planes, g = _cfg(width=W, height=H), abi.McrtGroundOcclusion(keep.ctypes.data, None), 0.0
    args = [sd.ptr, C.byref(cfg), C.byref(planes)]
    if case == "null_cfg":
        args[1] = None
    elif case == "null_scene":
        args[0] = None
    elif case == "null_planes":
        args[2] = None
    elif case == "both_planes_null":
        planes = _planes(0, 0)
        args[2] = C.byref(planes)
    elif case == "ground_nan":
        g = float("nan")
    else:
        cfg = _cfg(width=W, height=H, **CONFIG_CASES[case])
        args[1] = C.byref(cfg)
    names = {"null_scene": "NULL", "ground_nan": "ground_y"}.get(case) or NAMES[case]
    _invalid(lib, lib.mcrt_render_ground_occlusion(args[0], args[1], g, args[2], 0), names)
    assert np.all(keep == 7.0)


def test_the_limits_hold_whatever_ao_enabled_says_and_a_radius_below_zero_is_legal(lib):
    # the limits are checked before the frame's size: a frame of zero size is a no-op once the arguments are accepted
    planes = _planes()
    for kw, rc in ((dict(aoSamples=1), MCRT_OK), (dict(aoSamples=113), MCRT_OK), (dict(aoSamples=114), MCRT_ERR_INVALID),
                   (dict(aoSamples=0, aoEnabled=False), MCRT_ERR_INVALID), (dict(aoRadius=0.0), MCRT_OK), (dict(aoRadius=-1.0), MCRT_OK),
                   (dict(aoSamples=8, softShadows=True, shadowSamples=100000), MCRT_OK)):
        empty = _cfg(width=0, height=H, **kw)
        assert lib.mcrt_render_ground_occlusion_device(C.c_void_p(0x10), C.byref(empty), 0.0, C.byref(planes), None) == rc, kw
        assert lib.mcrt_render_ground_occlusion_batch_device(_handles(0x10), 1, C.byref(empty), _heights(0.0), C.byref(planes), 0, None) == rc, kw


@pytest.mark.parametrize("size", [(0, H, 16), (W, 0, 16), (W, H, 0), (-3, H, 16)])
def test_zero_size_frames_and_no_frames_are_no_ops(lib, mcrt, size):
    w, h, tile = size
    cfg, planes = _cfg(width=w, height=h, tileSize=tile), _planes()
    assert lib.mcrt_render_ground_occlusion_device(C.c_void_p(0x10), C.byref(cfg), 0.0, C.byref(planes), None) == MCRT_OK
    assert lib.mcrt_render_ground_occlusion_batch_device(_handles(0x10, 0x20), 2, C.byref(cfg), _heights(0.0, 1.0), C.byref(planes), 0, None) == MCRT_OK
    full = _cfg(width=W, height=H)
    assert lib.mcrt_render_ground_occlusion_batch_device(None, 0, C.byref(full), None, C.byref(planes), 0, None) == MCRT_OK
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    host = abi.McrtGroundOcclusion(keep.ctypes.data, None)
    assert lib.mcrt_render_ground_occlusion(sd.ptr, C.byref(cfg), 0.0, C.byref(host), 0) == MCRT_OK
    assert np.all(keep == 7.0)
    out = mcrt.TileRenderer.renderGroundOcclusion(sd, abi.Config(width=max(w, 0), height=max(h, 0), tileSize=tile), ground=0.0)
    assert set(out) == {"occlusion", "matte"} and out["occlusion"].dtype == np.float32 and out["matte"].dtype == np.uint8


def test_python_wrappers_check_their_own_arguments(mcrt):
    with pytest.raises(ValueError):
        abi.ground_occlusion_names(())
    with pytest.raises(ValueError):
        abi.ground_occlusion_names(("occlusion", "distance"))
    assert abi.ground_occlusion_names("matte") == ("matte",)
    assert abi.ground_occlusion_names(("matte", "occlusion")) == ("occlusion", "matte")
    with pytest.raises(ValueError):
        mcrt.render_ground_occlusion_batch_device([], abi.Config(width=W, height=H), 0.0)
    with pytest.raises(TypeError):
        mcrt.render_ground_occlusion_batch_device([object()], abi.Config(width=W, height=H), 0.0, occlusion_ptr=0x1000)


# ---- the shot's entries ------------------------------------------------------------------------------------------------
def _shot(**kw):
    return abi.Shot(**kw).to_c()


@pytest.mark.parametrize("size", [(64, 32), (33, 17), (1, 1)])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shot", [dict(), dict(shadowStrength=0.0), dict(reflectivity=0.0), dict(reflectionFade=12.0), dict(shadowStrength=0.0, reflectivity=0.0)])
def test_the_scratch_grows_by_one_plane_behind_the_others(lib, size, n, shot):
    w, h = size
    cfg, s = _cfg(width=w, height=h), _shot(**shot)
    base = lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(s), n)
    assert base > 0
    assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(s), 0.0, n) == base
    plane = (n * w * h * 4 + 15) & ~15
    for o in (0.5, 1.0, 1e-6):
        assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(s), o, n) == base + plane, o


def test_the_scratch_size_is_zero_for_what_is_refused(lib):
    cfg, s = _cfg(width=W, height=H), _shot()
    for o in (-0.1, 1.5, float("nan"), float("inf")):
        assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(s), o, 1) == 0, o
    assert lib.mcrt_shot_scratch_bytes_occ(None, C.byref(s), 0.5, 1) == 0
    assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), None, 0.5, 1) == 0
    assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(s), 0.5, 0) == 0
    empty = _cfg(width=0, height=H)
    assert lib.mcrt_shot_scratch_bytes_occ(C.byref(empty), C.byref(s), 0.5, 1) == 0


SHOT_CASES = {"strength_negative": (-0.25, {}, "floor_occlusion"), "strength_above_one": (1.25, {}, "floor_occlusion"),
              "strength_nan": (float("nan"), {}, "floor_occlusion"), "samples_0": (0.5, dict(aoSamples=0), "ao_samples"),
              "samples_114": (0.5, dict(aoSamples=114), "ao_samples"), "radius_nan": (0.5, dict(aoRadius=float("nan")), "ao_radius")}


@pytest.mark.parametrize("case", list(SHOT_CASES))
def test_render_shot_occ_rejects_the_strength_and_the_pass_limits(lib, mcrt, case):
    o, kw, names = SHOT_CASES[case]
    cfg, s = _cfg(width=W, height=H, **kw), _shot()
    rc = lib.mcrt_render_shot_batch_device_occ(_handles(0x10), 1, C.byref(cfg), C.byref(s), o, _heights(0.0), C.c_void_p(0x1000), 1 << 30, C.c_void_p(0x2000),
                                               None, W * H, None)
    _invalid(lib, rc, names)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full((H, W, 4), 9, np.uint8)
    arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    rc = lib.mcrt_render_shot_batch_occ(arr, 1, C.byref(cfg), C.byref(s), o, _heights(0.0), None, keep.ctypes.data_as(C.POINTER(C.c_uint8)), 0)
    _invalid(lib, rc, names)
    assert np.all(keep == 9)
    _invalid(lib, lib.mcrt_render_shot_png_occ(sd.ptr, C.byref(cfg), C.byref(s), o, 0.0, b"/nonexistent/never.png", 0), names)


def test_without_the_term_the_pass_limits_do_not_apply(lib):
    # o == 0: ao_samples / ao_radius are not looked at; a zero-size frame is a no-op once the arguments are accepted
    s = _shot()
    for kw in (dict(aoSamples=0), dict(aoSamples=114), dict(aoRadius=float("nan"))):
        empty = _cfg(width=0, height=H, **kw)
        args = (_handles(0x10), 1, C.byref(empty), C.byref(s))
        tail = (_heights(0.0), C.c_void_p(0x1000), 1 << 30, C.c_void_p(0x2000), None, 0, None)
        assert lib.mcrt_render_shot_batch_device_occ(*args, 0.0, *tail) == MCRT_OK, kw
        _invalid(lib, lib.mcrt_render_shot_batch_device_occ(*args, 0.5, *tail))


@pytest.mark.parametrize("o", [-0.25, 1.25, float("nan")])
def test_composite_occ_rejects_the_strength(lib, o):
    cfg, s = _cfg(width=W, height=H), _shot()
    planes = abi.McrtShotInputs(0x1000, None, None, None)
    rc = lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), 1, C.byref(cfg), C.byref(s), C.byref(planes), C.c_void_p(0x3000), o, W * H, C.c_void_p(0x2000),
                                                  None, W * H, None)
    _invalid(lib, rc, "floor_occlusion")


def test_composite_occ_keeps_the_checks_of_the_blend(lib):
    cfg, s = _cfg(width=W, height=H), _shot()
    planes = abi.McrtShotInputs(0x1000, None, None, None)
    tail = (C.c_void_p(0x3000), 0.5, W * H, C.c_void_p(0x2000), None, W * H, None)
    _invalid(lib, lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), -1, C.byref(cfg), C.byref(s), C.byref(planes), *tail), "n_frames")
    _invalid(lib, lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), 1, None, C.byref(s), C.byref(planes), *tail), "NULL")
    no_figure = abi.McrtShotInputs(None, None, None, None)
    _invalid(lib, lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), 1, C.byref(cfg), C.byref(s), C.byref(no_figure), *tail), "NULL")
    _invalid(lib, lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), 1, C.byref(cfg), C.byref(s), C.byref(planes), C.c_void_p(0x3000), 0.5, W * H - 1,
                                                           C.c_void_p(0x2000), None, W * H, None), "in_stride_pixels")
    empty = _cfg(width=0, height=H)
    assert lib.mcrt_composite_shot_batch_device_occ(_handles(0x10), 1, C.byref(empty), C.byref(s), C.byref(planes), *tail) == MCRT_OK


def test_shot_round_trips_through_to_c_as_before():
    s = abi.Shot()
    assert s.floorOcclusion == 0.0 and list(abi.Shot.__dataclass_fields__)[-1] == "floorOcclusion"
    c = s.to_c()
    assert C.sizeof(c) == 28 and [n for n, _ in abi.McrtShot._fields_] == ["page", "page_color", "shadow_strength", "reflectivity", "reflection_fade"]
    assert (c.page, list(c.page_color)) == (abi.PAGE_REFERENCE, [1.0, 1.0, 1.0])
    assert (c.shadow_strength, c.reflectivity, c.reflection_fade) == (np.float32(0.6), np.float32(0.35), 0.0)
    positional = abi.Shot("color", (0.25, 0.5, 0.75), 0.125, 0.5, 3.0)
    assert positional.floorOcclusion == 0.0
    with_term = abi.Shot("color", (0.25, 0.5, 0.75), 0.125, 0.5, 3.0, floorOcclusion=0.5)
    assert bytes(positional.to_c()) == bytes(with_term.to_c())
    c = positional.to_c()
    assert (c.page, list(c.page_color), c.shadow_strength, c.reflectivity, c.reflection_fade) == (abi.PAGE_COLOR, [0.25, 0.5, 0.75], 0.125, 0.5, 3.0)


def test_python_shot_entries_take_the_new_form_only_with_the_term(mcrt):
    cfg = abi.Config(width=W, height=H, aoSamples=8, aoRadius=3.0)
    base = mcrt.shot_scratch_bytes(cfg, abi.Shot(), 2)
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(floorOcclusion=0.0), 2) == base
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(floorOcclusion=0.5), 2) == base + 2 * W * H * 4
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(floorOcclusion=-0.5), 2) == 0
    # a config outside the pass's limits is fine without the term, refused with it (before any device work)
    from minecraftskin_raytracer_amd._lib import McrtError

    bad = abi.Config(width=0, height=H, aoSamples=0)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    assert mcrt.TileRenderer.renderShot(sd, bad, abi.Shot(), ground=0.0).shape == (H, 0, 4)
    with pytest.raises(McrtError, match="ao_samples"):
        mcrt.TileRenderer.renderShot(sd, bad, abi.Shot(floorOcclusion=0.5), ground=0.0)
    with pytest.raises(McrtError, match="floor_occlusion"):
        mcrt.TileRenderer.renderShot(sd, bad, abi.Shot(floorOcclusion=1.5), ground=0.0)
