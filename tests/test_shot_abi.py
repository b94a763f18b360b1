"""The studio shot (mcrt_shot_init, mcrt_shot_scratch_bytes, mcrt_composite_shot_batch_device, mcrt_render_shot*) without a
device: the symbols, every argument check that comes before any device work with its message, the scratch sizes, the no-ops and
the Python wrappers' own checks.

The device forms are given opaque handle values (or zeroed blocks that differ in the device index, the first member of a
handle): every case fails — or is a no-op — on a check that does not look further inside a handle."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
NEW_SYMBOLS = ("mcrt_shot_init", "mcrt_shot_scratch_bytes", "mcrt_composite_shot_batch_device", "mcrt_render_shot_batch_device",
               "mcrt_render_shot_device", "mcrt_render_shot", "mcrt_render_shot_batch", "mcrt_render_shot_png")
W, H = 64, 32
PX = W * H
SCRATCH = 0x10000  # an "address": 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**{"width": W, "height": H, **kw}).to_c()


def _shot(**kw):
    return abi.Shot(**kw).to_c()


def _handles(*values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _heights(*values):
    return (C.c_float * max(len(values), 1))(*values)


def _refused(lib, rc, text):
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert text.encode() in lib.mcrt_last_error(), lib.mcrt_last_error()


def _raw_shot(page=1, color=(1.0, 1.0, 1.0), s=0.6, k=0.35, fade=0.0):
    shot = abi.McrtShot()
    shot.page = page
    for i in range(3):
        shot.page_color[i] = color[i]
    shot.shadow_strength, shot.reflectivity, shot.reflection_fade = s, k, fade
    return shot


# what every entry point refuses of the shot itself: name -> (shot, message)
BAD_SHOTS = {
    "page_2": (dict(page=2), "page must be"),
    "page_negative": (dict(page=-1), "page must be"),
    "s_negative": (dict(s=-0.01), "shadow_strength"),
    "s_above_one": (dict(s=1.5), "shadow_strength"),
    "s_nan": (dict(s=float("nan")), "shadow_strength"),
    "k_negative": (dict(k=-1.0), "reflectivity"),
    "k_above_one": (dict(k=1.001), "reflectivity"),
    "k_nan": (dict(k=float("nan")), "reflectivity"),
    "fade_negative": (dict(fade=-1.0), "reflection_fade"),
    "fade_inf": (dict(fade=float("inf")), "reflection_fade"),
    "fade_nan": (dict(fade=float("nan")), "reflection_fade"),
    "page_color_nan": (dict(color=(1.0, float("nan"), 1.0)), "page_color"),
    "page_color_inf": (dict(color=(float("inf"), 0.0, 0.0)), "page_color"),
}
# and of the config of a shot that renders: name -> (config, shot, message or None when the shot is accepted)
CONFIG_LIMITS = {
    "bounces_4001": (dict(maxBounces=4001), dict(s=0.0, k=0.0), "max_bounces above 4000"),
    "samples_114": (dict(shadowSamples=114), dict(), "113 shadow samples"),
    "samples_114_shadow_only": (dict(shadowSamples=114), dict(k=0.0), "113 shadow samples"),
    "samples_114_mirror_only": (dict(shadowSamples=114), dict(s=0.0), "113 shadow samples"),
    "samples_114_neither": (dict(shadowSamples=114), dict(s=0.0, k=0.0), None),
    "samples_114_hard_shadows": (dict(shadowSamples=114, softShadows=False), dict(), None),
    "bounces_9": (dict(maxBounces=9), dict(), "at most 8 bounces"),
    "bounces_9_without_mirror": (dict(maxBounces=9), dict(k=0.0), None),
    "bounces_12_samples_200_plain": (dict(maxBounces=12, shadowSamples=200), dict(s=0.0, k=0.0), None),
}


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert C.sizeof(abi.McrtShot) == 7 * 4 and C.sizeof(abi.McrtShotInputs) == 4 * C.sizeof(C.c_void_p)
    assert abi.PAGE_COLOR == 0 and abi.PAGE_REFERENCE == 1


def test_shot_init_and_the_dataclass_agree(lib):
    s = _raw_shot(page=7, color=(9.0, 9.0, 9.0), s=9.0, k=9.0, fade=9.0)
    lib.mcrt_shot_init(C.byref(s))
    assert s.page == abi.PAGE_REFERENCE and list(s.page_color) == [1.0, 1.0, 1.0]
    assert (s.shadow_strength, s.reflectivity, s.reflection_fade) == (np.float32(0.6), np.float32(0.35), 0.0)
    d = abi.Shot().to_c()
    assert bytes(d) == bytes(s)
    lib.mcrt_shot_init(None)  # ignored
    assert abi.Shot(page="color", pageColor=(0.1, 0.2, 0.3)).to_c().page == abi.PAGE_COLOR
    for bad in ("white", 1, None):
        with pytest.raises(ValueError):
            abi.Shot(page=bad).to_c()


def _a16(n):
    return (n + 15) & ~15


def test_scratch_bytes_of_the_four_plane_combinations(lib, mcrt):
    w, h, n = 33, 17, 3  # 561 pixels: the 1-float planes of three frames end off a 16-byte boundary
    cfg = _cfg(width=w, height=h)
    px = w * h * n
    rgba, one = _a16(px * 16), _a16(px * 4)
    assert one != px * 4
    combos = {(0.0, 0.0, 0.0): rgba, (0.6, 0.0, 0.0): rgba + one, (0.0, 0.35, 0.0): 2 * rgba, (0.6, 0.35, 0.0): 2 * rgba + one,
              (0.0, 0.35, 24.0): 2 * rgba + one, (0.6, 0.35, 24.0): 2 * rgba + 2 * one, (0.6, 0.0, 24.0): rgba + one, (0.0, 0.0, 24.0): rgba}
    for (s, k, fade), want in combos.items():
        shot = _raw_shot(s=s, k=k, fade=fade)
        assert lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(shot), n) == want, (s, k, fade)
        assert mcrt.shot_scratch_bytes(abi.Config(width=w, height=h), abi.Shot(shadowStrength=s, reflectivity=k, reflectionFade=fade), n) == want
    # per pixel, on a frame whose planes need no padding: 16, + 4, + 16, + 4
    cfg = _cfg()
    per_px = [lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(_raw_shot(s=s, k=k, fade=f)), 1) // PX
              for s, k, f in ((0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (0.5, 0.5, 0), (0.5, 0.5, 1))]
    assert per_px == [16, 20, 32, 36, 40]
    # nothing to render, nothing to hold
    shot = _raw_shot()
    assert lib.mcrt_shot_scratch_bytes(None, C.byref(shot), 1) == 0 and lib.mcrt_shot_scratch_bytes(C.byref(cfg), None, 1) == 0
    assert lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(shot), 0) == 0 and lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(shot), -2) == 0
    for empty in (_cfg(width=0), _cfg(height=0), _cfg(tileSize=0)):
        assert lib.mcrt_shot_scratch_bytes(C.byref(empty), C.byref(shot), 4) == 0
    assert lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(_raw_shot(page=3)), 1) == 0


def _render_batch(lib, **kw):
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=_cfg(), shot=_raw_shot(), g=_heights(0.0, 1.0), scratch=SCRATCH, bytes=1 << 30, f32=0x100000, u8=0x200000,
             stride=PX)
    a.update(kw)
    byref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return lib.mcrt_render_shot_batch_device(a["scenes"], a["n"], byref(a["cfg"]), byref(a["shot"]), a["g"], a["scratch"], a["bytes"], a["f32"], a["u8"],
                                             a["stride"], None)


RENDER_REFUSALS = {
    "n_negative": (dict(n=-1), "n_frames"),
    "null_cfg": (dict(cfg=None), "NULL argument"),
    "null_shot": (dict(shot=None), "NULL argument"),
    "null_array": (dict(scenes=None), "NULL argument"),
    "null_heights": (dict(g=None), "NULL argument"),
    "null_entry": (dict(scenes=_handles(0x10, None)), "NULL scene handle"),
    "second_height_nan": (dict(g=_heights(0.0, float("nan"))), "ground_y must be finite"),
    "height_inf": (dict(g=_heights(float("-inf"), 0.0)), "ground_y must be finite"),
    "both_outputs_null": (dict(f32=None, u8=None), "both outputs are NULL"),
    "handle_twice": (dict(scenes=_handles(0x10, 0x10)), "listed twice"),
    "stride_too_small": (dict(stride=PX - 1), "frame_stride_pixels"),
    "scratch_null": (dict(scratch=None), "d_scratch is NULL"),
    "scratch_unaligned": (dict(scratch=SCRATCH + 8), "not 16-byte aligned"),
    "scratch_too_small": (dict(bytes=2 * PX * 36 - 1), "scratch_bytes is smaller"),
}


@pytest.mark.parametrize("case", list(RENDER_REFUSALS))
def test_render_batch_device_form_refuses(lib, case):
    kw, text = RENDER_REFUSALS[case]
    _refused(lib, _render_batch(lib, **kw), text)


@pytest.mark.parametrize("case", list(BAD_SHOTS))
def test_every_entry_point_refuses_a_bad_shot(lib, mcrt, case):
    kw, text = BAD_SHOTS[case]
    shot = _raw_shot(**kw)
    _refused(lib, _render_batch(lib, shot=shot), text)
    cfg = _cfg()
    _refused(lib, lib.mcrt_render_shot_device(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, SCRATCH, 1 << 30, None, 0x1000, None), text)
    planes = abi.McrtShotInputs(0x1000, 0x2000, 0x3000, 0x4000)
    _refused(lib, lib.mcrt_composite_shot_batch_device(_handles(0x10), 1, C.byref(cfg), C.byref(shot), C.byref(planes), PX, 0x5000, None, PX, None), text)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full((H, W, 4), 7, np.uint8)
    out = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    _refused(lib, lib.mcrt_render_shot(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, None, out, 0), text)
    _refused(lib, lib.mcrt_render_shot_png(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0), text)
    assert (keep == 7).all()
    assert lib.mcrt_shot_scratch_bytes(C.byref(cfg), C.byref(shot), 1) == 0


@pytest.mark.parametrize("case", list(CONFIG_LIMITS))
def test_config_limits_follow_the_passes_the_shot_runs(lib, mcrt, case):
    cfg_kw, shot_kw, text = CONFIG_LIMITS[case]
    shot = _raw_shot(**shot_kw)
    # a frame of zero size: a no-op once the arguments are accepted — the limits are checked before the frame's size
    empty = _cfg(width=0, **cfg_kw)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(16, 7, np.uint8)
    out = keep.ctypes.data_as(C.POINTER(C.c_uint8))
    rcs = [_render_batch(lib, cfg=empty, shot=shot, stride=0),
           lib.mcrt_render_shot_device(C.c_void_p(0x10), C.byref(empty), C.byref(shot), 0.0, None, 0, None, 0x1000, None),
           lib.mcrt_render_shot(sd.ptr, C.byref(empty), C.byref(shot), 0.0, None, out, 0)]
    for rc in rcs:
        if text is None:
            assert rc == MCRT_OK, lib.mcrt_last_error()
        else:
            _refused(lib, rc, text)
    assert (keep == 7).all()
    if text is not None:  # the PNG form refuses the limit; without one it refuses the empty image
        _refused(lib, lib.mcrt_render_shot_png(sd.ptr, C.byref(empty), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0), text)
    else:
        _refused(lib, lib.mcrt_render_shot_png(sd.ptr, C.byref(empty), C.byref(shot), 0.0, b"/nonexistent/shot.png", 0), "empty image")


def test_single_device_form_refuses(lib):
    cfg, shot = _cfg(), _raw_shot()
    f = lib.mcrt_render_shot_device
    _refused(lib, f(None, C.byref(cfg), C.byref(shot), 0.0, SCRATCH, 1 << 30, None, 0x1000, None), "NULL argument")
    _refused(lib, f(C.c_void_p(0x10), None, C.byref(shot), 0.0, SCRATCH, 1 << 30, None, 0x1000, None), "NULL argument")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), None, 0.0, SCRATCH, 1 << 30, None, 0x1000, None), "NULL argument")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), float("nan"), SCRATCH, 1 << 30, None, 0x1000, None), "ground_y must be finite")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, SCRATCH, 1 << 30, None, None, None), "both outputs are NULL")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, None, 1 << 30, None, 0x1000, None), "d_scratch is NULL")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, SCRATCH + 4, 1 << 30, None, 0x1000, None), "not 16-byte aligned")
    _refused(lib, f(C.c_void_p(0x10), C.byref(cfg), C.byref(shot), 0.0, SCRATCH, PX * 36 - 1, None, 0x1000, None), "scratch_bytes is smaller")


def _composite(lib, **kw):
    a = dict(scenes=_handles(0x10, 0x20), n=2, cfg=_cfg(), shot=_raw_shot(), planes=abi.McrtShotInputs(0x1000, 0x2000, 0x3000, 0x4000), in_stride=PX,
             f32=0x100000, u8=0x200000, out_stride=PX)
    a.update(kw)
    byref = lambda x: None if x is None else C.byref(x)  # noqa: E731
    return lib.mcrt_composite_shot_batch_device(a["scenes"], a["n"], byref(a["cfg"]), byref(a["shot"]), byref(a["planes"]), a["in_stride"], a["f32"], a["u8"],
                                                a["out_stride"], None)


COMPOSITE_REFUSALS = {
    "n_negative": (dict(n=-1), "n_frames"),
    "null_cfg": (dict(cfg=None), "NULL argument"),
    "null_shot": (dict(shot=None), "NULL argument"),
    "null_inputs": (dict(planes=None), "NULL argument"),
    "null_figure": (dict(planes=abi.McrtShotInputs(None, 0x2000, 0x3000, 0x4000)), "NULL argument"),
    "null_array": (dict(scenes=None), "NULL argument"),
    "null_entry": (dict(scenes=_handles(None, 0x20)), "NULL scene handle"),
    "fade_without_distance": (dict(shot=_raw_shot(fade=24.0), planes=abi.McrtShotInputs(0x1000, 0x2000, 0x3000, None)), "reflection_distance"),
    "fade_without_reflection_planes": (dict(shot=_raw_shot(fade=24.0), planes=abi.McrtShotInputs(0x1000, 0x2000, None, None)), "reflection_distance"),
    "both_outputs_null": (dict(f32=None, u8=None), "both outputs are NULL"),
    "in_stride_too_small": (dict(in_stride=PX - 1), "in_stride_pixels"),
    "out_stride_too_small": (dict(out_stride=PX - 1), "out_stride_pixels"),
}


@pytest.mark.parametrize("case", list(COMPOSITE_REFUSALS))
def test_composite_device_form_refuses(lib, case):
    kw, text = COMPOSITE_REFUSALS[case]
    _refused(lib, _composite(lib, **kw), text)


def test_handles_on_different_devices_are_refused(lib):
    blocks = [(C.c_int32 * 4096)() for _ in range(2)]
    blocks[1][0] = 1
    arr = _handles(*[C.addressof(b) for b in blocks])
    _refused(lib, _render_batch(lib, scenes=arr), "one device")
    _refused(lib, _composite(lib, scenes=arr), "one device")


def test_zero_frames_and_zero_size_are_ok(lib, mcrt):
    assert _render_batch(lib, scenes=_handles(), n=0, g=None, scratch=None, bytes=0) == MCRT_OK
    assert _composite(lib, scenes=_handles(), n=0) == MCRT_OK
    assert _composite(lib, scenes=None, n=0) == MCRT_OK
    for empty in (_cfg(width=0), _cfg(height=0), _cfg(tileSize=0)):
        assert _render_batch(lib, cfg=empty, stride=0, scratch=None, bytes=0) == MCRT_OK  # no frame: no stride, no scratch
        assert _composite(lib, cfg=empty, in_stride=0, out_stride=0) == MCRT_OK
        shot = _raw_shot()
        assert lib.mcrt_render_shot_device(C.c_void_p(0x10), C.byref(empty), C.byref(shot), 0.0, None, 0, 0x1000, None, None) == MCRT_OK
    # the argument checks still come first
    _refused(lib, _render_batch(lib, cfg=_cfg(width=0), f32=None, u8=None), "both outputs are NULL")
    _refused(lib, _composite(lib, cfg=_cfg(height=0), n=-1), "n_frames")
    sd = mcrt.MeshBuilder.buildDefaultScene()
    keep = np.full(8, 7.0, np.float32)
    shot, empty = _raw_shot(), _cfg(width=32, height=0)
    assert lib.mcrt_render_shot(sd.ptr, C.byref(empty), C.byref(shot), 0.0, abi.fptr(keep), None, 0) == MCRT_OK
    descs = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    assert lib.mcrt_render_shot_batch(descs, 1, C.byref(empty), C.byref(shot), _heights(0.0), abi.fptr(keep), None, 0) == MCRT_OK
    assert lib.mcrt_render_shot_batch(descs, 0, C.byref(_cfg()), C.byref(shot), None, abi.fptr(keep), None, 0) == MCRT_OK
    assert (keep == 7.0).all()


@pytest.mark.parametrize("case", ["null_desc", "null_cfg", "null_shot", "both_outputs_null", "ground_nan", "null_entry", "null_heights", "n_negative"])
def test_host_forms_refuse(mcrt, lib, case):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg, shot = _cfg(width=16, height=8), _raw_shot()
    keep = np.full((8, 16, 4), 7.0, np.float32)
    a = dict(d=sd.ptr, c=C.byref(cfg), s=C.byref(shot), g=0.0, f=abi.fptr(keep))
    text = "NULL argument"
    if case == "null_desc":
        a["d"] = None
    elif case == "null_cfg":
        a["c"] = None
    elif case == "null_shot":
        a["s"] = None
    elif case == "both_outputs_null":
        a["f"], text = None, "both outputs are NULL"
    elif case == "ground_nan":
        a["g"], text = float("nan"), "ground_y must be finite"
    if case in ("null_entry", "null_heights", "n_negative"):
        descs = (C.POINTER(abi.McrtSceneDesc) * 2)(sd.ptr, None if case == "null_entry" else sd.ptr)
        g = None if case == "null_heights" else _heights(0.0, 0.0)
        text = {"null_entry": "NULL scene description", "null_heights": "NULL argument", "n_negative": "n_frames"}[case]
        _refused(lib, lib.mcrt_render_shot_batch(descs, -1 if case == "n_negative" else 2, a["c"], a["s"], g, a["f"], None, 0), text)
    else:
        _refused(lib, lib.mcrt_render_shot(a["d"], a["c"], a["s"], a["g"], a["f"], None, 0), text)
        if case != "both_outputs_null":
            _refused(lib, lib.mcrt_render_shot_png(a["d"], a["c"], a["s"], a["g"], b"/nonexistent/shot.png", 0), text)
    _refused(lib, lib.mcrt_render_shot_png(sd.ptr, C.byref(cfg), C.byref(shot), 0.0, None, 0), "NULL argument")
    assert (keep == 7.0).all()


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        return  # a HIP device is visible: the GPU tests render shots
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderShot(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8))
    assert e.value.code == MCRT_ERR_NO_DEVICE
    assert mcrt.render_shot_png(mcrt.MeshBuilder.buildDefaultScene(), abi.Config(width=16, height=8), "/nonexistent/shot.png") is False


def test_python_wrappers_check_their_arguments(mcrt):
    cfg = abi.Config(width=16, height=8)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderShotBatch([object()], cfg)
    for bad in (float("nan"), [0.0, 1.0], [float("inf")]):
        with pytest.raises(ValueError):
            mcrt.TileRenderer.renderShotBatch([sd], cfg, ground=bad)
    with pytest.raises(ValueError):
        mcrt.TileRenderer.renderShotBatch([sd], cfg, abi.Shot(page="paper"))
    none = mcrt.TileRenderer.renderShotBatch([], cfg)
    assert none.shape == (0, 8, 16, 4) and none.dtype == np.uint8
    assert mcrt.TileRenderer.renderShotBatch([], cfg, rgba8=False).dtype == np.float32
    empty = mcrt.TileRenderer.renderShot(sd, abi.Config(width=0, height=8))  # a frame of zero size: nothing to render
    assert empty.shape == (8, 0, 4)
    with pytest.raises(mcrt._lib.McrtError):
        mcrt.TileRenderer.renderShot(sd, abi.Config(width=0, height=8), abi.Shot(shadowStrength=2.0))
    with pytest.raises(ValueError):
        mcrt.render_shot_batch_device([], cfg, None, 0.0, SCRATCH, 1 << 20)  # no output
    with pytest.raises(ValueError):
        mcrt.render_shot_batch_device([], cfg, None, None, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)  # a resident scene has no floor of its own
    with pytest.raises(ValueError):
        mcrt.render_shot_batch_device([], cfg, None, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(TypeError):
        mcrt.render_shot_batch_device([object()], cfg, None, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)
    mcrt.render_shot_batch_device([], cfg, None, 0.0, SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)  # no frames: nothing to do
    with pytest.raises(ValueError):
        mcrt.composite_shot_batch_device([], cfg, None, 0, out_f32_ptr=0x1000)  # no figure
    with pytest.raises(ValueError):
        mcrt.composite_shot_batch_device([], cfg, None, 0x1000)  # no output
    with pytest.raises(ValueError):
        mcrt.composite_shot_batch_device([], cfg, None, 0x1000, out_f32_ptr=0x2000, in_stride_pixels=5)
    with pytest.raises(ValueError):
        mcrt.composite_shot_batch_device([], cfg, None, 0x1000, out_f32_ptr=0x2000, out_stride_pixels=5)
    mcrt.composite_shot_batch_device([], cfg, None, 0x1000, out_rgba8_ptr=0x2000)  # no frames: nothing to do
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.render_shot_device(cfg, None, 0.0, SCRATCH, 1 << 20)
    with pytest.raises(ValueError):
        ds.render_shot_device(cfg, None, float("nan"), SCRATCH, 1 << 20, out_rgba8_ptr=0x1000)
