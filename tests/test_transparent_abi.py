"""Transparent background (MCRT_BACKGROUND_TRANSPARENT) without a device: the new symbols, the argument checks that come
before any device work, the Python keyword, and the self-test of the test-side checker (tests/cpp/transparent_oracle.cpp)
against the CPU oracle."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import fuzz_cases
import scenes
import transparent_checker
from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RENDERS = json.load(open(os.path.join(GOLDEN, "renders.json")))
NEW_SYMBOLS = ("mcrt_scene_set_background", "mcrt_render_ex", "mcrt_render_batch_ex", "mcrt_render_png_ex")
BAD = (-1, 2, 99)


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    return transparent_checker.Checker(transparent_checker.build(str(tmp_path_factory.mktemp("transparent_oracle"))))


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def test_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    header = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\bint " + name + r"\(", header), name
    assert re.search(r"#define MCRT_BACKGROUND_REFERENCE 0\b", header)
    assert re.search(r"#define MCRT_BACKGROUND_TRANSPARENT 1\b", header)
    assert (abi.BACKGROUND_REFERENCE, abi.BACKGROUND_TRANSPARENT) == (0, 1)
    assert lib.mcrt_abi_version() == 3


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("size", [(32, 24), (0, 24), (32, 0)], ids=["frame", "zero_width", "zero_height"])
def test_bad_background_is_invalid_everywhere(mcrt, lib, bad, size):
    w, h = size
    cfg = _cfg(width=w, height=h)
    sd = mcrt.MeshBuilder.buildDefaultScene()
    out = np.zeros((max(h, 1), max(w, 1), 4), np.float32)
    assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), bad, abi.fptr(out), None, C.cast(None, abi.PROGRESS_FN), None, None, 0, 0) == MCRT_ERR_INVALID
    assert lib.mcrt_last_error()
    out8 = np.zeros((max(h, 1), max(w, 1), 4), np.uint8)
    assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), bad, None, out8.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(None, abi.PROGRESS_FN), None,
                              None, 0, 0) == MCRT_ERR_INVALID
    arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    assert lib.mcrt_render_batch_ex(arr, 1, C.byref(cfg), bad, abi.fptr(out), None, 0) == MCRT_ERR_INVALID
    assert lib.mcrt_render_png_ex(sd.ptr, C.byref(cfg), bad, b"/nonexistent/never_written.png", 0) == MCRT_ERR_INVALID
    # an opaque handle value: the mode is checked before the handle is looked into
    assert lib.mcrt_scene_set_background(C.c_void_p(0x10), bad) == MCRT_ERR_INVALID
    assert np.all(out == 0.0) and np.all(out8 == 0)


def test_set_background_null_handle(lib):
    for mode in (abi.BACKGROUND_REFERENCE, abi.BACKGROUND_TRANSPARENT):
        assert lib.mcrt_scene_set_background(None, mode) == MCRT_ERR_INVALID


def test_render_ex_needs_exactly_one_output(mcrt, lib):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    out = np.zeros((24, 32, 4), np.float32)
    out8 = np.zeros((24, 32, 4), np.uint8)
    nocb = C.cast(None, abi.PROGRESS_FN)
    for size in ((32, 24), (0, 24)):
        cfg = _cfg(width=size[0], height=size[1])
        for mode in (abi.BACKGROUND_REFERENCE, abi.BACKGROUND_TRANSPARENT):
            assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), mode, None, None, nocb, None, None, 0, 0) == MCRT_ERR_INVALID
            assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), mode, abi.fptr(out), out8.ctypes.data_as(C.POINTER(C.c_uint8)), nocb, None,
                                      None, 0, 0) == MCRT_ERR_INVALID
    assert lib.mcrt_render_ex(None, C.byref(_cfg()), 0, abi.fptr(out), None, nocb, None, None, 0, 0) == MCRT_ERR_INVALID


def test_zero_size_frames_are_ok_like_the_existing_entries(mcrt, lib):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = _cfg(width=0, height=24)
    out = np.full((4,), 7.0, np.float32)
    nocb = C.cast(None, abi.PROGRESS_FN)
    for mode in (abi.BACKGROUND_REFERENCE, abi.BACKGROUND_TRANSPARENT):
        assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), mode, abi.fptr(out), None, nocb, None, None, 0, 0) == MCRT_OK
        arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
        assert lib.mcrt_render_batch_ex(arr, 1, C.byref(cfg), mode, abi.fptr(out), None, 0) == MCRT_OK
        # as mcrt_render_png: an empty image is refused (writePNG rejects it)
        assert lib.mcrt_render_png_ex(sd.ptr, C.byref(cfg), mode, b"/nonexistent/never_written.png", 0) == MCRT_ERR_INVALID
    assert np.all(out == 7.0)


def test_valid_arguments_reach_the_device(mcrt, lib, tmp_path):
    """With a valid mode the call goes on to the device: MCRT_ERR_NO_DEVICE where none is visible (no CPU fallback)."""
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = _cfg(width=32, height=24, tileSize=16)
    want = MCRT_ERR_NO_DEVICE if mcrt.device_count() <= 0 else MCRT_OK
    out = np.zeros((24, 32, 4), np.float32)
    out8 = np.zeros((24, 32, 4), np.uint8)
    nocb = C.cast(None, abi.PROGRESS_FN)
    arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    for mode in (abi.BACKGROUND_REFERENCE, abi.BACKGROUND_TRANSPARENT):
        assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), mode, abi.fptr(out), None, nocb, None, None, 0, 0) == want
        assert lib.mcrt_render_ex(sd.ptr, C.byref(cfg), mode, None, out8.ctypes.data_as(C.POINTER(C.c_uint8)), nocb, None, None, 0, 0) == want
        assert lib.mcrt_render_batch_ex(arr, 1, C.byref(cfg), mode, abi.fptr(out), None, 0) == want
        assert lib.mcrt_render_png_ex(sd.ptr, C.byref(cfg), mode, os.fsencode(str(tmp_path / "t.png")), 0) == want


@pytest.mark.parametrize("bad", ["opaque", "Transparent", "", None, 1])
def test_python_keyword_rejects_bad_values_before_the_library(mcrt, monkeypatch, bad):
    from minecraftskin_raytracer_amd import api

    def no_library():
        raise AssertionError("the library was called")

    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = abi.Config(width=16, height=8)
    monkeypatch.setattr(api, "load", no_library)
    with pytest.raises(ValueError):
        mcrt.TileRenderer.render(sd, cfg, background=bad)
    with pytest.raises(ValueError):
        mcrt.TileRenderer.renderRGBA8(sd, cfg, background=bad)
    with pytest.raises(ValueError):
        mcrt.TileRenderer.renderBatch([sd], cfg, background=bad)
    with pytest.raises(ValueError):
        mcrt.render_png(sd, cfg, "/nonexistent/never_written.png", background=bad)
    ds = object.__new__(mcrt.DeviceScene)  # no handle: the mode is checked first
    ds._h = C.c_void_p()
    with pytest.raises(ValueError):
        ds.set_background(bad)


# ---- checker self-test: reference mode is the oracle bit for bit; transparent mode keeps properties 1 and 2 -------------
def _scene(mcrt, case):
    return (mcrt.MeshBuilder.buildDefaultScene(mcrt.getBuiltinPoses()[case["pose"]]) if case["skin"] == "default"
            else scenes.skin_scene(case["skin"], case["pose"]))


def _check_against_oracle(checker, oracle, sd, cfg, what):
    ref = oracle.render(sd.ptr, cfg)
    t = transparent_checker.threads()
    mine, n_ref = checker.render(sd.ptr, cfg, "reference", threads=t)
    scenes.assert_bit_equal(mine, ref, f"{what}: checker (reference mode) vs oracle")
    frame, n = checker.render(sd.ptr, cfg, "transparent", threads=t)
    assert np.array_equal(n, n_ref), what
    S = max(1, cfg.samplesPerPixel)
    assert n.min() >= 0 and n.max() <= S
    full, none = n == S, n == 0
    scenes.assert_bit_equal(frame[full], ref[full], f"{what}: property 1 (every sample hits)")
    assert np.all(scenes.bits(frame[none]) == 0), f"{what}: property 2 (no hit: (0,0,0,0))"
    return int(full.sum()), int(none.sum()), int((~(full | none)).sum())


@pytest.mark.parametrize("case", RENDERS, ids=[c["name"] for c in RENDERS])
def test_checker_equals_oracle_on_golden_cases(mcrt, oracle, checker, case):
    cfg = abi.Config(**case["config"])
    full, none, edge = _check_against_oracle(checker, oracle, _scene(mcrt, case), cfg, case["name"])
    assert full > 0 and none > 0, (full, none, edge)  # the cases show the figure on a background


@pytest.mark.parametrize("seed", range(20))
def test_checker_equals_oracle_on_fuzz_cases(mcrt, oracle, checker, seed):
    sd, cfg, what = fuzz_cases.make_case(seed)
    _check_against_oracle(checker, oracle, sd, cfg, what)
