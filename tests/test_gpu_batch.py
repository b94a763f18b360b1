"""Batches of frames in one launch sequence (mcrt_render_batch / mcrt_render_batch_device) on the GPU: every frame
bit-identical to the committed fixtures, the oracle and single renders of the same scenes; the batched kernels' envelope
and the fall-back to single renders outside it (lastBatchInfo)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import scenes
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RENDERS = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "renders.json")))}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device_batch(mcrt, handles, cfg, stride=None, rgba8=False):
    n, px = len(handles), cfg.width * cfg.height
    stride = px if stride is None else stride
    f32 = torch.zeros((n, stride, 4), dtype=torch.float32, device="cuda")
    u8 = torch.zeros((n, stride, 4), dtype=torch.uint8, device="cuda") if rgba8 else None
    mcrt.render_batch_device(handles, cfg, f32.data_ptr(), u8.data_ptr() if rgba8 else 0, stride, _stream())
    torch.cuda.synchronize()
    return f32, u8


def _single(mcrt, ds, cfg):
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_fixtures_pose0_pose6_bit_for_bit(mcrt, gpu):
    case = RENDERS["b4_spp4"]
    cfg = abi.Config(**case["config"])
    sds = [scenes.skin_scene("S64", 0), scenes.skin_scene("S64", 6)]
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg)
    imgs8 = mcrt.TileRenderer.renderBatch(sds, cfg, rgba8=True)
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 2, "launch_sequences": 1}
    for i, name in enumerate(("b4_spp4", "b4_spp4_pose6")):
        g = np.load(os.path.join(GOLDEN, f"render_{name}.npz"))
        scenes.assert_bit_equal(imgs[i], g["image"], name)
        assert np.array_equal(imgs8[i], g["rgba8"]), name


def test_pose_sheet_default_config_equals_oracle_and_single(mcrt, gpu, oracle):
    cfg = abi.Config()  # the reference's default Config: 256x256, 3 bounces, 1 spp, tile 32
    sds = [scenes.skin_scene("S64", i) for i in range(7)] + [mcrt.MeshBuilder.buildDefaultScene()]
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg)
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 8, "launch_sequences": 1}
    for i, sd in enumerate(sds):
        scenes.assert_bit_equal(imgs[i], oracle.render(sd.ptr, cfg), f"frame {i} vs oracle")
        scenes.assert_bit_equal(imgs[i], mcrt.TileRenderer.render(sd, cfg), f"frame {i} vs render")


def _turntable(mcrt, n, radius=40.0, height=20.0):
    out = []
    for k in range(n):
        sd = scenes.skin_scene("S64", k % 7)
        a = 2.0 * math.pi * k / n
        d = sd.desc
        d.camera_position[0], d.camera_position[1], d.camera_position[2] = radius * math.sin(a), height, radius * math.cos(a)
        out.append(sd)
    return out


@pytest.mark.parametrize("extra", [{}, {"aoEnabled": True}, {"dofEnabled": True, "samplesPerPixel": 2}],
                         ids=["soft_shadows", "ao", "dof"])
def test_turntable_equals_oracle(mcrt, gpu, oracle, extra):
    cfg = abi.Config(width=40, height=32, maxBounces=2, samplesPerPixel=extra.get("samplesPerPixel", 1), tileSize=16,
                     softShadows=True, **{k: v for k, v in extra.items() if k != "samplesPerPixel"})
    sds = _turntable(mcrt, 12)
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg)
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 12, "launch_sequences": 1}
    for i, sd in enumerate(sds):
        scenes.assert_bit_equal(imgs[i], oracle.render(sd.ptr, cfg), f"view {i}")


def test_mixed_posed_unposed_and_hbm_scenes(mcrt, gpu, oracle):
    cfg = abi.Config(width=48, height=40, maxBounces=3, samplesPerPixel=2, tileSize=16)
    unposed = [scenes.skin_scene("S64", 0), mcrt.MeshBuilder.buildDefaultScene()]
    posed = [scenes.skin_scene("S64", 3), scenes.skin_scene("S32", 1)]
    big = mcrt.SceneDesc(scenes.many_boxes())
    for batch in (unposed, unposed + posed, [posed[0], unposed[0], big, unposed[1]]):
        imgs = mcrt.TileRenderer.renderBatch(batch, cfg)
        assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": len(batch), "launch_sequences": 1}
        for i, sd in enumerate(batch):
            scenes.assert_bit_equal(imgs[i], oracle.render(sd.ptr, cfg), f"frame {i} of {len(batch)}")


def test_handle_reuse_and_a_second_stream(mcrt, gpu):
    cfg = abi.Config(width=64, height=48, maxBounces=3, samplesPerPixel=2)
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in (0, 2, 4, 6)]
    other = mcrt.DeviceScene(scenes.skin_scene("S64", 5))
    try:
        before = [_single(mcrt, h, cfg) for h in handles]
        alone = _single(mcrt, other, cfg)
        side = torch.cuda.Stream()
        other_out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        with torch.cuda.stream(side):  # another handle renders on a second stream while the batch runs
            other.render_device(cfg, other_out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, side.cuda_stream)
        f32, u8 = _device_batch(mcrt, handles, cfg, rgba8=True)
        assert mcrt.last_batch_info() == {"batched_frames": 4, "launch_sequences": 1}
        side.synchronize()
        after = [_single(mcrt, h, cfg) for h in handles]
        for i in range(len(handles)):
            frame = f32[i].cpu().numpy().reshape(cfg.height, cfg.width, 4)
            scenes.assert_bit_equal(frame, before[i], f"batch frame {i}")
            scenes.assert_bit_equal(after[i], before[i], f"single render after the batch, handle {i}")
            assert np.array_equal(u8[i].cpu().numpy().reshape(cfg.height, cfg.width, 4), mcrt.quantize_rgba8(before[i]))
        scenes.assert_bit_equal(other_out.cpu().numpy(), alone, "second stream")
        for h in handles + [other]:
            h.check()
    finally:
        for h in handles + [other]:
            h.close()


def test_table_ring_shared_by_renders_and_layers_wraps_without_mixing_frames(mcrt, gpu):
    """Batched renders and batched layers passes draw their parameter tables from ONE ring of eight slots per device.  Twenty
    calls of the two kinds, on two streams, with nothing synchronised in between, take the ring past its eighth slot twice:
    a table overwritten while an earlier call still reads it, or a slot reused without its event, shows as another pose's frame."""
    cfg = abi.Config(width=64, height=48, maxBounces=2, samplesPerPixel=1, tileSize=16)
    px, n_calls, per_call = cfg.width * cfg.height, 20, 3
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in (0, 2, 4, 6)]
    try:
        beauty, depth, ids = [], [], []
        for h in handles:  # what every frame has to equal: single calls, each waited for
            beauty.append(_single(mcrt, h, cfg))
            d = torch.zeros((px,), dtype=torch.float32, device="cuda")
            i4 = torch.zeros((px, 4), dtype=torch.int32, device="cuda")
            h.render_layers_device(cfg, depth_ptr=d.data_ptr(), id_ptr=i4.data_ptr(), stream=_stream())
            torch.cuda.synchronize()
            depth.append(d.cpu().numpy())
            ids.append(i4.cpu().numpy())
        assert any(not np.array_equal(beauty[0], b) for b in beauty[1:])  # the poses differ: a mixed-up frame would show
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        out = []
        for k in range(n_calls):  # every call writes into buffers of its own
            if k % 2 == 0:
                out.append((torch.zeros((per_call, px, 4), dtype=torch.float32, device="cuda"),))
            else:
                out.append((torch.zeros((per_call, px), dtype=torch.float32, device="cuda"),
                            torch.zeros((per_call, px, 4), dtype=torch.int32, device="cuda")))
        torch.cuda.synchronize()  # the buffers are filled; from here to the end nothing waits
        order = [[(k + j) % len(handles) for j in range(per_call)] for k in range(n_calls)]
        for k in range(n_calls):
            hs, st = [handles[i] for i in order[k]], streams[k % 2].cuda_stream
            if k % 2 == 0:
                mcrt.render_batch_device(hs, cfg, out[k][0].data_ptr(), 0, px, st)
            else:
                mcrt.render_layers_batch_device(hs, cfg, depth_ptr=out[k][0].data_ptr(), id_ptr=out[k][1].data_ptr(), stream=st)
        torch.cuda.synchronize()
        for k in range(n_calls):
            for j, i in enumerate(order[k]):
                what = f"call {k}, frame {j} (handle {i})"
                if k % 2 == 0:
                    scenes.assert_bit_equal(out[k][0][j].cpu().numpy().reshape(cfg.height, cfg.width, 4), beauty[i], what)
                else:
                    scenes.assert_bit_equal(out[k][0][j].cpu().numpy(), depth[i], what + " depth")
                    assert np.array_equal(out[k][1][j].cpu().numpy(), ids[i]), what + " id"
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()


def test_frame_stride_leaves_padding_untouched(mcrt, gpu):
    cfg = abi.Config(width=40, height=24, maxBounces=2, samplesPerPixel=1, tileSize=16)
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in (1, 4, 6)]
    try:
        px, stride = cfg.width * cfg.height, cfg.width * cfg.height + 100
        f32 = torch.full((3, stride, 4), -7.0, dtype=torch.float32, device="cuda")
        u8 = torch.full((3, stride, 4), 13, dtype=torch.uint8, device="cuda")
        mcrt.render_batch_device(handles, cfg, f32.data_ptr(), u8.data_ptr(), stride, _stream())
        torch.cuda.synchronize()
        for i, h in enumerate(handles):
            ref = _single(mcrt, h, cfg)
            scenes.assert_bit_equal(f32[i, :px].cpu().numpy().reshape(cfg.height, cfg.width, 4), ref, f"frame {i}")
            assert torch.all(f32[i, px:] == -7.0) and torch.all(u8[i, px:] == 13)
    finally:
        for h in handles:
            h.close()


def test_fallback_multi_pass_frames(mcrt, gpu, monkeypatch):
    cfg = abi.Config(width=128, height=128, maxBounces=4, samplesPerPixel=4)
    monkeypatch.setenv("MCRT_WORKSPACE_MB", "1")  # read at a handle's first render: one tile row per pass
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in (0, 6)]
    try:
        f32, _ = _device_batch(mcrt, handles, cfg)
        assert mcrt.last_batch_info() == {"batched_frames": 0, "launch_sequences": 2}
        for i, h in enumerate(handles):
            scenes.assert_bit_equal(f32[i].cpu().numpy().reshape(cfg.height, cfg.width, 4), _single(mcrt, h, cfg), f"frame {i}")
    finally:
        for h in handles:
            h.close()


def test_fallback_general_variant_config(mcrt, gpu):
    cfg = abi.Config(width=48, height=32, maxBounces=9, samplesPerPixel=1, tileSize=16)  # beyond the flat pipeline's 8
    handles = [mcrt.DeviceScene(scenes.skin_scene("S64", i)) for i in (2, 5, 6)]
    try:
        f32, _ = _device_batch(mcrt, handles, cfg)
        assert mcrt.last_batch_info() == {"batched_frames": 0, "launch_sequences": 3}
        for i, h in enumerate(handles):
            scenes.assert_bit_equal(f32[i].cpu().numpy().reshape(cfg.height, cfg.width, 4), _single(mcrt, h, cfg), f"frame {i}")
    finally:
        for h in handles:
            h.close()


def test_large_batch_splits_into_sequences(mcrt, gpu):
    cfg = abi.Config(width=16, height=16, maxBounces=1, samplesPerPixel=1, tileSize=16)
    sds = [scenes.skin_scene("S64", i % 7) for i in range(300)]
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg)
    assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 300, "launch_sequences": 2}
    for i in (0, 6, 255, 256, 299):
        scenes.assert_bit_equal(imgs[i], mcrt.TileRenderer.render(sds[i], cfg), f"frame {i}")
