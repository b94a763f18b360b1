"""Transparent background (MCRT_BACKGROUND_TRANSPARENT) on the GPU: every frame bit for bit against the test-side checker
(tests/cpp/transparent_oracle.cpp) on every entry point and execution path, and reference mode unchanged."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import fuzz_cases
import scenes
import transparent_checker
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RENDERS = json.load(open(os.path.join(GOLDEN, "renders.json")))
T = "transparent"


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return transparent_checker.Checker(transparent_checker.build(str(tmp_path_factory.mktemp("transparent_oracle"))))


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _scene(mcrt, case):
    return (mcrt.MeshBuilder.buildDefaultScene(mcrt.getBuiltinPoses()[case["pose"]]) if case["skin"] == "default"
            else scenes.skin_scene(case["skin"], case["pose"]))


def _want(checker, sd, cfg, tiles=None):
    frame, _ = checker.render(sd.ptr, cfg, T, tiles=tiles, threads=transparent_checker.threads())
    return frame


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device(mcrt, ds, cfg, first=0, step=1, layout=abi.LAYOUT_FRAME, rgba8=False):
    rows = ds.owned_pixel_rows(cfg, first, step) if layout == abi.LAYOUT_PACKED else cfg.height
    f32 = torch.zeros((rows, cfg.width, 4), dtype=torch.float32, device="cuda")
    u8 = torch.zeros((rows, cfg.width, 4), dtype=torch.uint8, device="cuda") if rgba8 else None
    ds.render_device_ex(cfg, f32.data_ptr(), u8.data_ptr() if rgba8 else 0, first, step, layout, _stream())
    torch.cuda.synchronize()
    return f32.cpu().numpy(), (u8.cpu().numpy() if rgba8 else None)


def _check(mcrt, img, want, what, img8=None):
    scenes.assert_bit_equal(img, want, what)
    if img8 is not None:
        assert np.array_equal(img8, mcrt.quantize_rgba8(want)), what + " (RGBA8)"


# ---- basic cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RENDERS, ids=[c["name"] for c in RENDERS])
def test_golden_cases_equal_the_checker(mcrt, gpu, checker, case):
    sd, cfg = _scene(mcrt, case), abi.Config(**case["config"])
    want = _want(checker, sd, cfg)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    img8 = mcrt.TileRenderer.renderRGBA8(sd, cfg, background=T)
    _check(mcrt, img, want, case["name"], img8)


# ---- reference mode unchanged ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b4_spp4_pose6", "dof_on", "flat_bg"])
def test_reference_mode_entries_equal_the_existing_ones_and_the_fixtures(mcrt, gpu, lib, tmp_path, name):
    from test_png import decode_png

    case = next(c for c in RENDERS if c["name"] == name)
    g = np.load(os.path.join(GOLDEN, f"render_{name}.npz"))
    sd, cfg = _scene(mcrt, case), abi.Config(**case["config"])
    c, h, w = cfg.to_c(), cfg.height, cfg.width
    nocb = C.cast(None, abi.PROGRESS_FN)
    R = abi.BACKGROUND_REFERENCE
    out = np.zeros((h, w, 4), np.float32)
    assert lib.mcrt_render_ex(sd.ptr, C.byref(c), R, abi.fptr(out), None, nocb, None, None, 0, 0) == 0
    scenes.assert_bit_equal(out, g["image"], "mcrt_render_ex")
    out8 = np.zeros((h, w, 4), np.uint8)
    assert lib.mcrt_render_ex(sd.ptr, C.byref(c), R, None, out8.ctypes.data_as(C.POINTER(C.c_uint8)), nocb, None, None, 0, 0) == 0
    assert np.array_equal(out8, g["rgba8"])
    arr = (C.POINTER(abi.McrtSceneDesc) * 2)(sd.ptr, sd.ptr)
    outb = np.zeros((2, h, w, 4), np.float32)
    assert lib.mcrt_render_batch_ex(arr, 2, C.byref(c), R, abi.fptr(outb), None, 0) == 0
    scenes.assert_bit_equal(outb[1], g["image"], "mcrt_render_batch_ex")
    path = str(tmp_path / "ref.png")
    assert lib.mcrt_render_png_ex(sd.ptr, C.byref(c), R, os.fsencode(path), 0) == 0
    assert np.array_equal(decode_png(open(path, "rb").read()), g["rgba8"])
    # the default path and an explicit "reference"
    scenes.assert_bit_equal(mcrt.TileRenderer.render(sd, cfg), g["image"], "render")
    scenes.assert_bit_equal(mcrt.TileRenderer.render(sd, cfg, background="reference"), g["image"], "render reference")
    assert np.array_equal(mcrt.TileRenderer.renderRGBA8(sd, cfg, background="reference"), g["rgba8"])
    ds = mcrt.DeviceScene(sd)
    try:
        before, _ = _device(mcrt, ds, cfg)
        ds.set_background(T)
        _device(mcrt, ds, cfg)
        ds.set_background("reference")
        after, after8 = _device(mcrt, ds, cfg, rgba8=True)
        scenes.assert_bit_equal(before, g["image"], "render_device")
        scenes.assert_bit_equal(after, g["image"], "render_device after set_background('reference')")
        assert np.array_equal(after8, g["rgba8"])
    finally:
        ds.close()


# ---- fuzz -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(48))
def test_fuzz_cases_equal_the_checker(mcrt, gpu, checker, seed):
    sd, cfg, what = fuzz_cases.make_case(1000 + seed)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == [], what
    scenes.assert_bit_equal(img, _want(checker, sd, cfg), what)


@pytest.mark.parametrize("seed", range(24))
def test_wide_cases_equal_the_checker(mcrt, gpu, checker, seed):
    sd, cfg, what = fuzz_cases.make_wide_case(2000 + seed)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == [], what
    scenes.assert_bit_equal(img, _want(checker, sd, cfg), what)


# ---- special configurations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [dict(maxBounces=0), dict(maxBounces=10),  # 10 bounces: the general variants
                                   dict(maxBounces=2, shadowSamples=200),      # a long per-hit stream: the general variants
                                   dict(maxBounces=3, samplesPerPixel=33), dict(maxBounces=2, samplesPerPixel=40, dofEnabled=True),
                                   dict(maxBounces=2, samplesPerPixel=36, gradientBg=False),
                                   dict(maxBounces=2, samplesPerPixel=8, aoEnabled=True, aoSamples=8)],
                         ids=["bounces0", "bounces10", "shadow200", "spp33", "spp40_dof", "spp36_flat", "ao"])
def test_special_configurations_equal_the_checker(mcrt, gpu, checker, extra):
    kw = dict(width=72, height=56, samplesPerPixel=2, tileSize=16)
    kw.update(extra)
    sd, cfg = scenes.skin_scene("S64", 3), abi.Config(**kw)
    want = _want(checker, sd, cfg)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    _check(mcrt, img, want, str(extra), mcrt.TileRenderer.renderRGBA8(sd, cfg, background=T))


# ---- execution paths ------------------------------------------------------------------------------------------------
PATH_CFG = dict(width=200, height=170, maxBounces=3, samplesPerPixel=4, tileSize=16)


@pytest.fixture(scope="module")
def path_case(mcrt, checker):
    sd, cfg = scenes.skin_scene("S64", 5), abi.Config(**PATH_CFG)
    return sd, cfg, _want(checker, sd, cfg)


def test_several_passes(mcrt, gpu, path_case, monkeypatch):
    sd, cfg, want = path_case
    monkeypatch.setenv("MCRT_WORKSPACE_MB", "1")  # one tile row per pass
    calls = []
    img = mcrt.TileRenderer.render(sd, cfg, lambda d, t: calls.append(d), background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    assert calls == list(range(1, len(calls) + 1)) and len(calls) == len(mcrt.TileRenderer.generateTiles(cfg.width, cfg.height, cfg.tileSize))
    _check(mcrt, img, want, "several passes", mcrt.TileRenderer.renderRGBA8(sd, cfg, background=T))


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_lanes(mcrt, gpu, path_case, lanes):
    sd, cfg, want = path_case
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_lanes(lanes)
        ds.set_background(T)
        img, img8 = _device(mcrt, ds, cfg, rgba8=True)
        _check(mcrt, img, want, f"{lanes} lanes", img8)
        ds.check()
    finally:
        ds.close()


def test_packed_shard(mcrt, gpu, path_case):
    sd, cfg, want = path_case
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_background(T)
        ts = cfg.tileSize
        for first, step in ((0, 3), (1, 3), (2, 3)):
            packed, packed8 = _device(mcrt, ds, cfg, first, step, abi.LAYOUT_PACKED, rgba8=True)
            for j, ty in enumerate(range(first, (cfg.height + ts - 1) // ts, step)):
                rows = min(ts, cfg.height - ty * ts)
                w = want[ty * ts:ty * ts + rows]
                _check(mcrt, packed[j * ts:j * ts + rows], w, f"shard ({first}, {step}) tile row {ty}", packed8[j * ts:j * ts + rows])
    finally:
        ds.close()


@pytest.mark.parametrize("gather", [False, True])
def test_replicated_ranks(mcrt, gpu, path_case, gather):
    sd, cfg, want = path_case
    img = mcrt.TileRenderer.render(sd, cfg, device=[0, 0], gather=gather, background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    img8 = mcrt.TileRenderer.renderRGBA8(sd, cfg, device=[0, 0], gather=gather, background=T)
    _check(mcrt, img, want, f"ranks [0, 0], gather={gather}", img8)


# ---- full size ------------------------------------------------------------------------------------------------------
def test_metric_frame_whole(mcrt, gpu, checker):
    sd, cfg = scenes.skin_scene("S64", 0), abi.Config(width=1920, height=1080, maxBounces=4, samplesPerPixel=4)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    want = _want(checker, sd, cfg)
    scenes.assert_bit_equal(img, want, "1080p / 4 bounces / 4 spp")
    assert (img[..., 3] == 0).mean() > 0.8  # most of the frame is transparent


def test_gui_defaults_figure_row_and_corners(mcrt, gpu, checker):
    cfg = abi.Config(width=1920, height=1080, maxBounces=4, samplesPerPixel=64, aoEnabled=True, aoSamples=16, dofEnabled=True, aperture=0.3)
    sd = scenes.skin_scene("S64", 0)
    img = mcrt.TileRenderer.render(sd, cfg, background=T)
    assert mcrt.TileRenderer.lastErrors() == []
    ts, cols, rows = cfg.tileSize, (cfg.width + 31) // 32, (cfg.height + 31) // 32
    mid = rows // 2
    alpha = img[..., 3]
    row_tiles = [(tx * ts, mid * ts, ts, min(ts, cfg.height - mid * ts)) for tx in range(cols)
                 if alpha[mid * ts:(mid + 1) * ts, tx * ts:(tx + 1) * ts].any()]  # the figure's tiles of the middle row
    assert 0 < len(row_tiles) <= 24, len(row_tiles)
    corners = [(0, 0, ts, ts), ((cols - 1) * ts, 0, cfg.width - (cols - 1) * ts, ts),
               (0, (rows - 1) * ts, ts, cfg.height - (rows - 1) * ts),
               ((cols - 1) * ts, (rows - 1) * ts, cfg.width - (cols - 1) * ts, cfg.height - (rows - 1) * ts)]
    tiles = row_tiles + corners
    want = _want(checker, sd, cfg, tiles=tiles)
    for (x, y, w, h) in tiles:
        scenes.assert_bit_equal(img[y:y + h, x:x + w], want[y:y + h, x:x + w], f"GUI defaults tile ({x}, {y})")
    for (x, y, w, h) in corners:
        assert np.all(img[y:y + h, x:x + w] == 0.0)


# ---- batches --------------------------------------------------------------------------------------------------------
def test_batch_of_skins_and_poses(mcrt, gpu, checker):
    cfg = abi.Config()  # 256x256, 3 bounces, 1 spp, tile 32
    sds = [scenes.skin_scene("S64" if i % 2 == 0 else "S32", i % 7) for i in range(8)]
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg, background=T)
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 8, "launch_sequences": 1}
    imgs8 = mcrt.TileRenderer.renderBatch(sds, cfg, rgba8=True, background=T)
    for i, sd in enumerate(sds):
        single = mcrt.TileRenderer.render(sd, cfg, background=T)
        scenes.assert_bit_equal(imgs[i], single, f"frame {i} vs single render")
        assert np.array_equal(imgs8[i], mcrt.quantize_rgba8(single))
    for i in (0, 5):
        scenes.assert_bit_equal(imgs[i], _want(checker, sds[i], cfg), f"frame {i} vs checker")


@pytest.mark.parametrize("spp", [1, 16])  # 16 spp: the modes differ in the draws layout too (bg_in_plan)
def test_mixed_mode_device_batch(mcrt, gpu, checker, spp):
    cfg = abi.Config(width=64, height=48, maxBounces=3, samplesPerPixel=spp, tileSize=16)
    modes = ["reference", T, T, "reference", T]
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in range(len(modes))]
    try:
        for h, m in zip(handles, modes):
            h.set_background(m)
        px = cfg.width * cfg.height
        f32 = torch.zeros((len(handles), px, 4), dtype=torch.float32, device="cuda")
        u8 = torch.zeros((len(handles), px, 4), dtype=torch.uint8, device="cuda")
        mcrt.render_batch_device(handles, cfg, f32.data_ptr(), u8.data_ptr(), px, _stream())
        torch.cuda.synchronize()
        assert mcrt.last_batch_info() == {"batched_frames": len(handles), "launch_sequences": 2}  # one sequence per mode
        for i, h in enumerate(handles):
            single, single8 = _device(mcrt, h, cfg, rgba8=True)
            frame = f32[i].cpu().numpy().reshape(cfg.height, cfg.width, 4)
            scenes.assert_bit_equal(frame, single, f"frame {i} ({modes[i]}) vs its single render")
            assert np.array_equal(u8[i].cpu().numpy().reshape(cfg.height, cfg.width, 4), single8)
            h.check()
        scenes.assert_bit_equal(f32[1].cpu().numpy().reshape(cfg.height, cfg.width, 4), _want(checker, scenes.skin_scene("S64", 1), cfg), "vs checker")
    finally:
        for h in handles:
            h.close()


# ---- graph replay ---------------------------------------------------------------------------------------------------
def test_alternating_modes_on_one_handle(mcrt, gpu, checker, oracle):
    """Six renders of one handle, the modes alternating: both parameter sets pass their fourth sighting and are replayed
    from recorded graphs; the mode is part of the recorded parameters, so no frame replays the other mode's launches."""
    sd, cfg = scenes.skin_scene("S64", 6), abi.Config(width=96, height=64, maxBounces=3, samplesPerPixel=4, tileSize=16)
    want = {T: _want(checker, sd, cfg), "reference": oracle.render(sd.ptr, cfg)}
    ds = mcrt.DeviceScene(sd)
    try:
        for k in range(12):
            mode = T if k % 2 else "reference"
            ds.set_background(mode)
            img, _ = _device(mcrt, ds, cfg)
            scenes.assert_bit_equal(img, want[mode], f"render {k} ({mode})")
        ds.check()
    finally:
        ds.close()


# ---- PNG ------------------------------------------------------------------------------------------------------------
def test_transparent_png(mcrt, gpu, tmp_path):
    from test_png import decode_png

    sd, cfg = scenes.skin_scene("S64", 2), abi.Config(width=160, height=120, maxBounces=2, samplesPerPixel=4)
    path = str(tmp_path / "figure.png")
    assert mcrt.render_png(sd, cfg, path, background=T)
    plane = mcrt.TileRenderer.renderRGBA8(sd, cfg, background=T)
    img = decode_png(open(path, "rb").read())
    assert np.array_equal(img, plane)
    for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1)):
        assert img[y, x, 3] == 0
    assert (img[..., 3] == 255).any()
