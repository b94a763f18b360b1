"""Batch entry points (mcrt_render_batch_device / mcrt_render_batch / mcrt_last_batch_info) without a device: the
symbols, the argument checks that come before any device work, and the Python wrappers' shape checks."""
import ctypes as C

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

MCRT_OK, MCRT_ERR_INVALID, MCRT_ERR_NO_DEVICE = 0, 1, 2


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


def _cfg(**kw):
    return abi.Config(**kw).to_c()


def _handles(*values):
    # opaque handle values: every case below fails on a check that does not look inside a handle
    return (C.c_void_p * max(len(values), 1))(*values)


def _descs(mcrt, n):
    ds = [mcrt.MeshBuilder.buildDefaultScene(mcrt.getBuiltinPoses()[i % 7]) for i in range(n)]
    return ds, (C.POINTER(abi.McrtSceneDesc) * max(n, 1))(*[d.ptr for d in ds])


def test_batch_symbols_are_exported_and_declared(lib):
    from minecraftskin_raytracer_amd import _lib

    for name in ("mcrt_render_batch_device", "mcrt_render_batch", "mcrt_last_batch_info"):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTED_SYMBOLS
    f, q = C.c_int(-1), C.c_int(-1)
    assert lib.mcrt_last_batch_info(C.byref(f), C.byref(q)) == MCRT_OK
    assert f.value >= 0 and q.value >= 0


@pytest.mark.parametrize("case", ["n_negative", "null_entry", "both_outputs_null", "stride_too_small", "handle_twice", "bounces_above_4000", "null_cfg"])
def test_device_form_rejects_bad_arguments(lib, case):
    cfg = _cfg(width=64, height=32)
    out = C.c_void_p(0x1000)
    args = dict(scenes=_handles(0x10, 0x20), n=2, cfg=C.byref(cfg), f32=out, u8=None, stride=64 * 32)
    if case == "n_negative":
        args["n"] = -1
    elif case == "null_entry":
        args["scenes"] = _handles(0x10, None)
    elif case == "both_outputs_null":
        args["f32"] = None
    elif case == "stride_too_small":
        args["stride"] = 64 * 32 - 1
    elif case == "handle_twice":
        args["scenes"] = _handles(0x10, 0x20, 0x10)
        args["n"] = 3
    elif case == "bounces_above_4000":
        cfg.max_bounces = 4001
    elif case == "null_cfg":
        args["cfg"] = None
    rc = lib.mcrt_render_batch_device(args["scenes"], args["n"], args["cfg"], args["f32"], args["u8"], args["stride"], None)
    assert rc == MCRT_ERR_INVALID, lib.mcrt_last_error()
    assert lib.mcrt_last_error()


def test_device_form_zero_frames_and_zero_size_are_ok(lib):
    cfg = _cfg(width=64, height=32)
    assert lib.mcrt_render_batch_device(_handles(), 0, C.byref(cfg), C.c_void_p(0x1000), None, 64 * 32, None) == MCRT_OK
    empty = _cfg(width=0, height=32)  # zero-size frames behave like mcrt_render: nothing to do, nothing written
    assert lib.mcrt_render_batch_device(_handles(0x10, 0x20), 2, C.byref(empty), C.c_void_p(0x1000), None, 0, None) == MCRT_OK
    f, q = C.c_int(-1), C.c_int(-1)
    lib.mcrt_last_batch_info(C.byref(f), C.byref(q))
    assert (f.value, q.value) == (0, 0)


@pytest.mark.parametrize("case", ["n_negative", "null_entry", "both_outputs_null", "bounces_above_4000"])
def test_host_form_rejects_bad_arguments(mcrt, lib, case):
    ds, arr = _descs(mcrt, 2)
    cfg = _cfg(width=32, height=32)
    out = np.zeros((2, 32, 32, 4), np.float32)
    f32 = abi.fptr(out)
    n = 2
    if case == "n_negative":
        n = -3
    elif case == "null_entry":
        arr[1] = C.POINTER(abi.McrtSceneDesc)()
    elif case == "both_outputs_null":
        f32 = None
    elif case == "bounces_above_4000":
        cfg.max_bounces = 4001
    assert lib.mcrt_render_batch(arr, n, C.byref(cfg), f32, None, 0) == MCRT_ERR_INVALID
    assert np.all(out[..., :3] == 0.0)


def test_host_form_zero_size_is_ok(mcrt, lib):
    ds, arr = _descs(mcrt, 2)
    cfg = _cfg(width=32, height=0)
    out = np.full((2, 4), 7.0, np.float32)
    assert lib.mcrt_render_batch(arr, 2, C.byref(cfg), abi.fptr(out), None, 0) == MCRT_OK
    assert np.all(out == 7.0)


def test_host_form_without_device_reports_no_device(mcrt, lib):
    if mcrt.device_count() > 0:
        pytest.skip("a HIP device is visible: the GPU tests render batches")
    ds, arr = _descs(mcrt, 3)
    cfg = _cfg(width=32, height=32)
    out = np.zeros((3, 32, 32, 4), np.float32)
    assert lib.mcrt_render_batch(arr, 3, C.byref(cfg), abi.fptr(out), None, 0) == MCRT_ERR_NO_DEVICE
    with pytest.raises(mcrt._lib.McrtError) as e:
        mcrt.TileRenderer.renderBatch(ds, abi.Config(width=32, height=32))
    assert e.value.code == MCRT_ERR_NO_DEVICE


def test_python_wrappers_check_shapes(mcrt):
    cfg = abi.Config(width=16, height=8)
    with pytest.raises(ValueError):
        mcrt.render_batch_device([], cfg, out_f32_ptr=0x1000, frame_stride_pixels=16 * 8 - 1)
    with pytest.raises(ValueError):
        mcrt.render_batch_device([], cfg)  # no output at all
    with pytest.raises(TypeError):
        mcrt.render_batch_device([object()], cfg, out_f32_ptr=0x1000)
    with pytest.raises(TypeError):
        mcrt.TileRenderer.renderBatch([object()], cfg)
    out = mcrt.TileRenderer.renderBatch([], cfg)
    assert out.shape == (0, 8, 16, 4) and out.dtype == np.float32
    out8 = mcrt.TileRenderer.renderBatch([], cfg, rgba8=True)
    assert out8.shape == (0, 8, 16, 4) and out8.dtype == np.uint8
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 0, "launch_sequences": 0}
    assert mcrt.last_batch_info() == mcrt.TileRenderer.lastBatchInfo()
