"""The shot as a cut-out (mcrt_shot_ex_init, mcrt_shot_scratch_bytes_ex, mcrt_composite_shot_batch_device_ex,
mcrt_render_shot_batch_device_ex, mcrt_render_shot_batch_ex, mcrt_render_shot_png_ex) without a device: the symbols, the struct,
every new refusal with its message before any device work, the refusals the entries share with the ``_occ`` entries, the scratch
sizes, the no-ops, and the rules of the Python ``Shot``.

The device forms are given opaque handle values: every case fails — or is a no-op — on a check that does not look inside a
handle."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_shot_ex_init", "mcrt_shot_scratch_bytes_ex", "mcrt_composite_shot_batch_device_ex", "mcrt_render_shot_batch_device_ex",
               "mcrt_render_shot_batch_ex", "mcrt_render_shot_png_ex")
W, H = 64, 32
PX = W * H
SCRATCH = 0x10000  # an "address": 16-byte aligned, never dereferenced
BOUNDS = 0x300000


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**{"width": W, "height": H, **kw}).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _heights(*values):
    return (C.c_float * max(len(values), 1))(*values)


def _refused(lib, rc, text):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert text.encode() in lib.mcrt_last_error(), lib.mcrt_last_error()


def _raw(page=2, color=(1.0, 1.0, 1.0), s=0.6, k=0.35, fade=0.0, o=0.0, C_=(0.0, 0.0, 0.0)):
    shot = abi.McrtShotEx()
    shot.shot.page = page
    for i in range(3):
        shot.shot.page_color[i] = color[i]
        shot.shadow_color[i] = C_[i]
    shot.shot.shadow_strength, shot.shot.reflectivity, shot.shot.reflection_fade, shot.floor_occlusion = s, k, fade, o
    return shot


# what every _ex entry refuses of the shot itself: name -> (shot, message)
BAD_SHOTS = {
    "page_3": (dict(page=3), "page must be"),
    "page_negative": (dict(page=-1), "page must be"),
    "s_above_one": (dict(s=1.5), "shadow_strength"),
    "s_nan": (dict(s=float("nan")), "shadow_strength"),
    "k_negative": (dict(k=-1.0), "reflectivity"),
    "fade_inf": (dict(fade=float("inf")), "reflection_fade"),
    "page_color_nan_with_the_transparent_page": (dict(color=(1.0, float("nan"), 1.0)), "page_color"),
    "page_color_inf_on_a_page": (dict(page=0, color=(float("inf"), 0.0, 0.0)), "page_color"),
    "o_above_one": (dict(o=1.25), "floor_occlusion"),
    "o_nan": (dict(o=float("nan")), "floor_occlusion"),
    "shadow_color_nan": (dict(C_=(0.0, float("nan"), 0.0)), "shadow_color must be finite"),
    "shadow_color_inf": (dict(C_=(float("-inf"), 0.0, 0.0)), "shadow_color must be finite"),
    "shadow_color_nan_on_a_page": (dict(page=1, C_=(0.0, 0.0, float("nan"))), "shadow_color must be finite"),
}


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert C.sizeof(abi.McrtShotEx) == 44
    assert [n for n, _ in abi.McrtShotEx._fields_] == ["shot", "floor_occlusion", "shadow_color"]
    assert abi.McrtShotEx.floor_occlusion.offset == 28 and abi.McrtShotEx.shadow_color.offset == 32
    assert abi.PAGE_TRANSPARENT == 2 and (abi.PAGE_COLOR, abi.PAGE_REFERENCE) == (0, 1)
    assert lib.mcrt_abi_version() == 3


def test_shot_ex_init_and_the_dataclass_agree(lib):
    s = _raw(page=7, color=(9.0, 9.0, 9.0), s=9.0, k=9.0, fade=9.0, o=9.0, C_=(9.0, 9.0, 9.0))
    lib.mcrt_shot_ex_init(C.byref(s))
    plain = abi.McrtShot()
    lib.mcrt_shot_init(C.byref(plain))
    assert bytes(s.shot) == bytes(plain) and s.floor_occlusion == 0.0 and list(s.shadow_color) == [0.0, 0.0, 0.0]
    assert bytes(abi.Shot().to_c_ex()) == bytes(s)
    lib.mcrt_shot_ex_init(None)  # ignored


def _render_batch(lib, **kw):
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=_cfg(), shot=_raw(), g=_heights(0.0, 1.0), scratch=SCRATCH, bytes=1 << 30, f32=0x100000, u8=0x200000,
             stride=PX, bounds=BOUNDS)
    a.update(kw)
    byref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return lib.mcrt_render_shot_batch_device_ex(a["scenes"], a["n"], byref(a["cfg"]), byref(a["shot"]), a["g"], a["scratch"], a["bytes"], a["f32"], a["u8"],
                                                a["stride"], a["bounds"], None)


def _composite(lib, **kw):
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=_cfg(), shot=_raw(), planes=abi.McrtShotInputs(0x1000, 0x2000, 0x3000, 0x4000), occ=0x5000, in_stride=PX,
             f32=0x100000, u8=0x200000, out_stride=PX, bounds=BOUNDS)
    a.update(kw)
    byref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return lib.mcrt_composite_shot_batch_device_ex(a["scenes"], a["n"], byref(a["cfg"]), byref(a["shot"]), byref(a["planes"]), a["occ"], a["in_stride"],
                                                   a["f32"], a["u8"], a["out_stride"], a["bounds"], None)


@pytest.mark.parametrize("case", list(BAD_SHOTS))
def test_every_entry_point_refuses_a_bad_shot(lib, mcrt, case):
    kw, text = BAD_SHOTS[case]
    shot = _raw(**kw)
    cfg = _cfg()
    for bounds in (BOUNDS, None):
        _refused(lib, _render_batch(lib, shot=shot, bounds=bounds), text)
        _refused(lib, _composite(lib, shot=shot, bounds=bounds), text)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full((H, W, 4), 7, np.uint8)
    out = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    descs = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    _refused(lib, lib.mcrt_render_shot_batch_ex(descs, 1, C.byref(cfg), C.byref(shot), _heights(0.0), None, out, None, 0), text)
    _refused(lib, lib.mcrt_render_shot_png_ex(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0, None, 0), text)
    assert (keep == 7).all()
    assert lib.mcrt_shot_scratch_bytes_ex(C.byref(cfg), C.byref(shot), 1) == 0


@pytest.mark.parametrize("page", [0, 1])
def test_bounds_and_crop_need_the_transparent_page(lib, mcrt, page):
    text = "MCRT_PAGE_TRANSPARENT only"
    shot, cfg = _raw(page=page), _cfg()
    _refused(lib, _render_batch(lib, shot=shot), text)
    _refused(lib, _composite(lib, shot=shot), text)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full((H, W, 4), 7, np.uint8)
    out = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    box = np.full((1, 4), 7, np.int32)
    descs = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    _refused(lib, lib.mcrt_render_shot_batch_ex(descs, 1, C.byref(cfg), C.byref(shot), _heights(0.0), None, out, box.ctypes.data, 0), text)
    _refused(lib, lib.mcrt_render_shot_png_ex(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, b"/nonexistent/shot.png", 1, None, 0), text)
    _refused(lib, lib.mcrt_render_shot_png_ex(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0, box.ctypes.data, 0), text)
    assert (keep == 7).all() and (box == 7).all()
    # without bounds an opaque page is welcome: the next check refuses
    _refused(lib, _render_batch(lib, shot=shot, bounds=None, f32=None, u8=None), "both outputs are NULL")
    _refused(lib, _composite(lib, shot=shot, bounds=None, f32=None, u8=None), "both outputs are NULL")


@pytest.mark.parametrize("page", [2, 3, -1])
def test_the_entries_before_still_refuse_the_page(lib, mcrt, page):
    shot = abi.McrtShot()
    lib.mcrt_shot_init(C.byref(shot))
    shot.page = page
    cfg = _cfg()
    text = "page must be MCRT_PAGE_COLOR or MCRT_PAGE_REFERENCE"
    planes = abi.McrtShotInputs(0x1000, 0x2000, 0x3000, 0x4000)
    args = (_handles(0x10), 1, C.byref(cfg), C.byref(shot))
    _refused(lib, lib.mcrt_render_shot_batch_device(*args, _heights(0.0), SCRATCH, 1 << 30, None, 0x1000, PX, None), text)
    _refused(lib, lib.mcrt_render_shot_batch_device_occ(*args, 0.5, _heights(0.0), SCRATCH, 1 << 30, None, 0x1000, PX, None), text)
    _refused(lib, lib.mcrt_render_shot_device(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, SCRATCH, 1 << 30, None, 0x1000, None), text)
    _refused(lib, lib.mcrt_composite_shot_batch_device(*args, C.byref(planes), PX, 0x5000, None, PX, None), text)
    _refused(lib, lib.mcrt_composite_shot_batch_device_occ(*args, C.byref(planes), None, 0.0, PX, 0x5000, None, PX, None), text)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full((H, W, 4), 7, np.uint8)
    out = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    descs = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    _refused(lib, lib.mcrt_render_shot(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, None, out, 0), text)
    _refused(lib, lib.mcrt_render_shot_batch_occ(descs, 1, C.byref(cfg), C.byref(shot), 0.0, _heights(0.0), None, out, 0), text)
    _refused(lib, lib.mcrt_render_shot_png(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0), text)
    _refused(lib, lib.mcrt_render_shot_png_occ(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, 0.0, b"/nonexistent/shot.png", 0), text)
    assert (keep == 7).all()
    assert lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(shot), 1) == 0 and lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(shot), 0.0, 1) == 0


RENDER_REFUSALS = {
    "n_negative": (dict(n=-1), "n_frames"),
    "null_cfg": (dict(cfg=None), "NULL argument"),
    "null_shot": (dict(shot=None), "NULL argument"),
    "null_array": (dict(scenes=None), "NULL argument"),
    "null_heights": (dict(g=None), "NULL argument"),
    "null_entry": (dict(scenes=_handles(0x10, None)), "NULL scene handle"),
    "second_height_nan": (dict(g=_heights(0.0, float("nan"))), "ground_y must be finite"),
    "both_outputs_null": (dict(f32=None, u8=None), "both outputs are NULL"),
    "handle_twice": (dict(scenes=_handles(0x10, 0x10)), "listed twice"),
    "samples_114": (dict(cfg=_cfg(shadowSamples=114)), "113 shadow samples"),
    "bounces_9": (dict(cfg=_cfg(maxBounces=9)), "at most 8 bounces"),
    "ao_samples_0_with_the_term": (dict(cfg=_cfg(aoSamples=0), shot=_raw(o=0.5)), "ao_samples"),
    "stride_too_small": (dict(stride=PX - 1), "frame_stride_pixels"),
    "scratch_null": (dict(scratch=None), "d_scratch is NULL"),
    "scratch_unaligned": (dict(scratch=SCRATCH + 8), "not 16-byte aligned"),
    "scratch_too_small": (dict(bytes=2 * PX * 36 - 1), "scratch_bytes is smaller than mcrt_shot_scratch_bytes_ex"),
    "scratch_too_small_for_the_occlusion_plane": (dict(bytes=2 * PX * 40 - 1, shot=_raw(o=0.5)), "scratch_bytes is smaller"),
}


@pytest.mark.parametrize("case", list(RENDER_REFUSALS))
def test_render_batch_device_form_refuses(lib, case):
    kw, text = RENDER_REFUSALS[case]
    _refused(lib, _render_batch(lib, **kw), text)


COMPOSITE_REFUSALS = {
    "n_negative": (dict(n=-1), "n_frames"),
    "null_cfg": (dict(cfg=None), "NULL argument"),
    "null_shot": (dict(shot=None), "NULL argument"),
    "null_inputs": (dict(planes=None), "NULL argument"),
    "null_figure": (dict(planes=abi.McrtShotInputs(None, 0x2000, 0x3000, 0x4000)), "NULL argument"),
    "null_array": (dict(scenes=None), "NULL argument"),
    "null_entry": (dict(scenes=_handles(None, 0x20)), "NULL scene handle"),
    "fade_without_distance": (dict(shot=_raw(fade=24.0), planes=abi.McrtShotInputs(0x1000, 0x2000, 0x3000, None)), "reflection_distance"),
    "both_outputs_null": (dict(f32=None, u8=None), "both outputs are NULL"),
    "in_stride_too_small": (dict(in_stride=PX - 1), "in_stride_pixels"),
    "out_stride_too_small": (dict(out_stride=PX - 1), "out_stride_pixels"),
}


@pytest.mark.parametrize("case", list(COMPOSITE_REFUSALS))
def test_composite_device_form_refuses(lib, case):
    kw, text = COMPOSITE_REFUSALS[case]
    _refused(lib, _composite(lib, **kw), text)


def test_the_skipped_passes_limits_do_not_apply(lib):
    """s = k = o = 0 accepts 12 bounces, 200 shadow samples and no ambient-occlusion samples: a frame of zero size is a no-op
    once the arguments are accepted, and the limits are checked before the frame's size."""
    heavy = _cfg(width=0, maxBounces=12, shadowSamples=200, aoSamples=0)
    assert _render_batch(lib, cfg=heavy, shot=_raw(s=0.0, k=0.0, o=0.0), stride=0) == MCRT_OK, lib.mcrt_last_error()
    _refused(lib, _render_batch(lib, cfg=heavy, shot=_raw(k=0.0), stride=0), "113 shadow samples")
    _refused(lib, _render_batch(lib, cfg=_cfg(width=0, maxBounces=12), shot=_raw(s=0.0), stride=0), "at most 8 bounces")
    _refused(lib, _render_batch(lib, cfg=_cfg(width=0, maxBounces=4001), shot=_raw(s=0.0, k=0.0), stride=0), "max_bounces above 4000")


def test_handles_on_different_devices_are_refused(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    arr = _handles(*[C.addressof(b) for b in blocks])
    _refused(lib, _render_batch(lib, scenes=arr), "one device")
    _refused(lib, _composite(lib, scenes=arr), "one device")


def _a16(n):
    return (n + 15) & ~15


def test_scratch_bytes_ex_equals_scratch_bytes_occ(lib, mcrt):
    w, h, n = 33, 17, 3  # 561 pixels: the 1-float planes of three frames end off a 16-byte boundary
    cfg = _cfg(width=w, height=h)
    px = w * h * n
    rgba, one = _a16(px * 16), _a16(px * 4)
    for s, k, fade, o in [(s, k, f, o) for s in (0.0, 0.6) for k in (0.0, 0.35) for f in (0.0, 24.0) for o in (0.0, 0.5)]:
        want = rgba + (rgba if k else 0) + (one if s else 0) + (one if k and fade else 0) + (one if o else 0)
        plain = _raw(page=1, s=s, k=k, fade=fade).shot
        assert lib.mcrt_shot_scratch_bytes_occ(C.byref(cfg), C.byref(plain), o, n) == want, (s, k, fade, o)
        for page, colour in ((2, (0.0, 0.0, 0.0)), (2, (0.5, 0.25, 1.0)), (0, (0.5, 0.25, 1.0)), (1, (0.0, 0.0, 0.0))):
            shot = _raw(page=page, s=s, k=k, fade=fade, o=o, C_=colour)
            assert lib.mcrt_shot_scratch_bytes_ex(C.byref(cfg), C.byref(shot), n) == want, (s, k, fade, o, page)
        py = abi.Shot("transparent", (1, 1, 1), s, k, fade, floorOcclusion=o, shadowColor=(0.5, 0.25, 1.0))
        assert mcrt.shot_scratch_bytes(abi.Config(width=w, height=h), py, n) == want
        assert mcrt.shot_scratch_bytes(abi.Config(width=w, height=h), py, n, bounds=True) == want
    shot = _raw()
    assert lib.mcrt_shot_scratch_bytes_ex(None, C.byref(shot), 1) == 0 and lib.mcrt_shot_scratch_bytes_ex(C.byref(cfg), None, 1) == 0
    assert lib.mcrt_shot_scratch_bytes_ex(C.byref(cfg), C.byref(shot), 0) == 0 and lib.mcrt_shot_scratch_bytes_ex(C.byref(cfg), C.byref(shot), -2) == 0
    for empty in (_cfg(width=0), _cfg(height=0), _cfg(tileSize=0)):
        assert lib.mcrt_shot_scratch_bytes_ex(C.byref(empty), C.byref(shot), 4) == 0


def test_zero_frames_and_zero_size_are_ok_and_write_nothing(lib, mcrt):
    assert _render_batch(lib, scenes=_handles(), n=0, g=None, scratch=None, bytes=0) == MCRT_OK
    assert _composite(lib, scenes=_handles(), n=0) == MCRT_OK
    assert _composite(lib, scenes=None, n=0) == MCRT_OK
    for empty in (_cfg(width=0), _cfg(height=0), _cfg(tileSize=0)):
        assert _render_batch(lib, cfg=empty, stride=0, scratch=None, bytes=0) == MCRT_OK  # no frame: no stride, no scratch
        assert _composite(lib, cfg=empty, in_stride=0, out_stride=0) == MCRT_OK
    # the argument checks still come first
    _refused(lib, _render_batch(lib, cfg=_cfg(width=0), f32=None, u8=None), "both outputs are NULL")
    _refused(lib, _composite(lib, cfg=_cfg(height=0), n=-1), "n_frames")
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    box = np.full((1, 4), 7, np.int32)
    shot, empty = _raw(), _cfg(width=32, height=0)
    descs = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    assert lib.mcrt_render_shot_batch_ex(descs, 1, C.byref(empty), C.byref(shot), _heights(0.0), abi.fptr(keep), None, box.ctypes.data, 0) == MCRT_OK
    assert lib.mcrt_render_shot_batch_ex(descs, 0, C.byref(_cfg()), C.byref(shot), None, abi.fptr(keep), None, box.ctypes.data, 0) == MCRT_OK
    assert (keep == 7.0).all() and (box == 7).all()
    _refused(lib, lib.mcrt_render_shot_png_ex(sd.ptr, C.byref(empty), C.byref(shot), 0.0, b"/nonexistent/shot.png", 1, box.ctypes.data, 0), "empty image")
    assert (box == 7).all()


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_shot", "null_path", "both_outputs_null", "ground_nan", "null_entry", "n_negative"])
def test_host_forms_refuse(mcrt, lib, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg, shot = _cfg(width=16, height=8), _raw()
    keep = np.full((8, 16, 4), 7.0, np.float32)
    box = np.full((2, 4), 7, np.int32)
    descs = (C.POINTER(abi.McrtSceneDesc) * 2)(sd.ptr, None if case == "null_entry" else sd.ptr)
    a = dict(d=descs, n=2, c=C.byref(cfg), s=C.byref(shot), g=_heights(0.0, 0.0), f=abi.fptr(keep))
    text = {"null_desc": "NULL argument", "null_cfg": "NULL argument", "null_shot": "NULL argument", "null_path": "NULL argument",
            "both_outputs_null": "both outputs are NULL", "ground_nan": "ground_y must be finite", "null_entry": "NULL scene description",
            "n_negative": "n_frames"}[case]
    png = dict(d=sd.ptr, c=a["c"], s=a["s"], g=0.0, path=b"/nonexistent/shot.png")
    if case == "null_desc":
        a["d"], png["d"] = None, None
    elif case == "null_cfg":
        a["c"], png["c"] = None, None
    elif case == "null_shot":
        a["s"], png["s"] = None, None
    elif case == "null_path":
        png["path"] = None
    elif case == "both_outputs_null":
        a["f"] = None
    elif case == "ground_nan":
        a["g"], png["g"] = _heights(0.0, float("nan")), float("nan")
    elif case == "n_negative":
        a["n"] = -1
    if case != "null_path":
        _refused(lib, lib.mcrt_render_shot_batch_ex(a["d"], a["n"], a["c"], a["s"], a["g"], a["f"], None, box.ctypes.data, 0), text)
    if case in ("null_desc", "null_cfg", "null_shot", "null_path", "ground_nan"):
        _refused(lib, lib.mcrt_render_shot_png_ex(png["d"], png["c"], png["s"], png["g"], png["path"], 1, box.ctypes.data, 0), text)
    assert (keep == 7.0).all() and (box == 7).all()


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests render cut-outs
    sd, cfg = mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8)
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderShot(sd, cfg, abi.Shot(page="transparent"), bounds=True)
    assert e.value.code == MCRT_ERR_NO_DEVICE
    assert mcrt.render_shot_png(sd, cfg, "/nonexistent/shot.png", abi.Shot(page="transparent"), crop=True) is False


# ---- the Python Shot --------------------------------------------------------------------------------------------------------
def test_the_dataclass_keeps_its_fields():
    names = ["page", "pageColor", "shadowStrength", "reflectivity", "reflectionFade"]
    s = abi.Shot(page="transparent", shadowColor=(0.25, 0.5, 1))
    assert [f.name for f in dataclasses.fields(abi.Shot)] == names and list(dataclasses.asdict(s)) == names
    assert s.shadowColor == (0.25, 0.5, 1.0) and abi.Shot().shadowColor == (0.0, 0.0, 0.0) and s.floorOcclusion == 0.0
    assert s == abi.Shot(page="transparent", shadowColor=(0.25, 0.5, 1.0)) and s != abi.Shot(page="transparent")
    assert "shadowColor" in repr(s) and "shadowColor" not in repr(abi.Shot())
    with pytest.raises(ValueError):
        abi.Shot(shadowColor=(1.0, 0.0))


def test_to_c_and_to_c_ex():
    # the two old pages: to_c as it was, whatever the shadow's colour
    for page in ("reference", "color"):
        a, b = abi.Shot(page, (0.25, 0.5, 0.75), 0.125, 0.5, 3.0), abi.Shot(page, (0.25, 0.5, 0.75), 0.125, 0.5, 3.0, shadowColor=(1.0, 0.5, 0.0))
        assert bytes(a.to_c()) == bytes(b.to_c()) and C.sizeof(a.to_c()) == 28
        assert bytes(b.to_c_ex().shot) == bytes(a.to_c())
    with pytest.raises(ValueError, match="to_c_ex"):
        abi.Shot(page="transparent").to_c()
    for bad in ("white", 1, None):
        with pytest.raises(ValueError):
            abi.Shot(page=bad).to_c()
        with pytest.raises(ValueError):
            abi.Shot(page=bad).to_c_ex()
    c = abi.Shot("transparent", (0.25, 0.5, 0.75), 0.125, 0.5, 3.0, floorOcclusion=0.75, shadowColor=(1.0, 0.5, 0.0)).to_c_ex()
    assert (c.shot.page, list(c.shot.page_color), c.shot.shadow_strength, c.shot.reflectivity, c.shot.reflection_fade) == (2, [0.25, 0.5, 0.75], 0.125, 0.5, 3.0)
    assert c.floor_occlusion == 0.75 and list(c.shadow_color) == [1.0, 0.5, 0.0]


def test_routing_is_by_need(mcrt, monkeypatch):
    """The _ex entries are called only for a transparent page, a shadow colour other than 0, bounds or a crop; otherwise the
    calls made before are made unchanged."""
    from minecraftskin_raytracer_amd import _lib

    real = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not name.startswith("mcrt_") or "shot" not in name:
                return f

            def wrapped(*a):
                calls.append(name)
                return f(*a)

            return wrapped

    monkeypatch.setattr(mcrt.api, "load", lambda: Spy())
    cfg = abi.Config(width=0, height=8)  # a frame of zero size: every call is a no-op behind its argument checks
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cut, tinted, plain, term = abi.Shot(page="transparent"), abi.Shot(shadowColor=(0.0, 0.0, 0.5)), abi.Shot(), abi.Shot(floorOcclusion=0.5)

    def made(f):
        calls.clear()
        f()
        return list(calls)

    assert made(lambda: mcrt.TileRenderer.renderShotBatch([sd], cfg, plain)) == ["mcrt_render_shot_batch"]
    assert made(lambda: mcrt.TileRenderer.renderShotBatch([sd], cfg, term)) == ["mcrt_render_shot_batch_occ"]
    assert made(lambda: mcrt.TileRenderer.renderShotBatch([sd], cfg, abi.Shot(shadowColor=(0.0, -0.0, 0.0)))) == ["mcrt_render_shot_batch"]
    for shot in (cut, tinted):
        assert made(lambda: mcrt.TileRenderer.renderShotBatch([sd], cfg, shot)) == ["mcrt_render_shot_batch_ex"]
    images, boxes = mcrt.TileRenderer.renderShotBatch([sd, sd], cfg, cut, bounds=True)
    assert images.shape == (2, 8, 0, 4) and boxes.dtype == np.int32 and boxes.tolist() == [[0, 8, 0, 0]] * 2
    image, box = mcrt.TileRenderer.renderShot(sd, cfg, cut, bounds=True)
    assert image.shape == (8, 0, 4) and box.tolist() == [0, 8, 0, 0]
    with pytest.raises(mcrt._lib.McrtError, match="MCRT_PAGE_TRANSPARENT only"):
        mcrt.TileRenderer.renderShotBatch([sd], cfg, plain, bounds=True)
    assert made(lambda: mcrt.shot_scratch_bytes(cfg, plain)) == ["mcrt_shot_scratch_bytes"]
    assert made(lambda: mcrt.shot_scratch_bytes(cfg, term)) == ["mcrt_shot_scratch_bytes_occ"]
    assert made(lambda: mcrt.shot_scratch_bytes(cfg, cut)) == ["mcrt_shot_scratch_bytes_ex"]
    assert mcrt.shot_scratch_bytes(abi.Config(width=8, height=8), plain, 1, bounds=True) == 0  # refused like an invalid shot
    assert made(lambda: mcrt.render_shot_batch_device([], cfg, plain, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)) == ["mcrt_render_shot_batch_device"]
    assert made(lambda: mcrt.render_shot_batch_device([], cfg, term, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)) == ["mcrt_render_shot_batch_device_occ"]
    assert made(lambda: mcrt.render_shot_batch_device([], cfg, tinted, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)) == ["mcrt_render_shot_batch_device_ex"]
    assert made(lambda: mcrt.render_shot_batch_device([], cfg, cut, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000, bounds_ptr=BOUNDS)) == [
        "mcrt_render_shot_batch_device_ex"]
    assert made(lambda: mcrt.composite_shot_batch_device([], cfg, plain, 0x1000, out_rgba8_ptr=0x2000)) == ["mcrt_composite_shot_batch_device"]
    assert made(lambda: mcrt.composite_shot_batch_device([], cfg, cut, 0x1000, out_rgba8_ptr=0x2000)) == ["mcrt_composite_shot_batch_device_ex"]
    assert made(lambda: mcrt.composite_shot_batch_device([], cfg, cut, 0x1000, out_rgba8_ptr=0x2000, bounds_ptr=BOUNDS)) == [
        "mcrt_composite_shot_batch_device_ex"]
    with pytest.raises(mcrt._lib.McrtError, match="MCRT_PAGE_TRANSPARENT only"):
        mcrt.composite_shot_batch_device([], cfg, plain, 0x1000, out_rgba8_ptr=0x2000, bounds_ptr=BOUNDS)
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()  # no handle: the library refuses the call it is given

    def refused(f):
        with pytest.raises(mcrt._lib.McrtError, match="NULL"):
            f()

    assert made(lambda: refused(lambda: ds.render_shot_device(cfg, plain, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000))) == ["mcrt_render_shot_device"]
    assert made(lambda: refused(lambda: ds.render_shot_device(cfg, cut, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000, bounds_ptr=BOUNDS))) == [
        "mcrt_render_shot_batch_device_ex"]
    assert made(lambda: mcrt.render_shot_png(sd, cfg, "/nonexistent/shot.png", plain)) == ["mcrt_render_shot_png"]
    assert made(lambda: mcrt.render_shot_png(sd, cfg, "/nonexistent/shot.png", cut)) == ["mcrt_render_shot_png_ex"]
    assert made(lambda: mcrt.render_shot_png(sd, cfg, "/nonexistent/shot.png", plain, crop=True)) == ["mcrt_render_shot_png_ex"]
