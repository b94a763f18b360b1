"""Randomised parity of the BATCHED entries against the CPU oracle, in fixed blocks of tests/batch_fuzz_cases.py; the long sweeps
are tools/gpu_fuzz.py's modes batch and pass-batch, which run the functions of this file.

a  device form   render_batch_device on the drawn batches of the blocks of four, one batch per test.  Its handles are made once
                 and closed at its end.  Before a batch every second handle renders alone at the batch's config (its tile seeds are fresh), the
                 others at the config of the block's previous batch — another width and tile (their seeds are stale, their
                 workspaces re-planned): the table carries frame rows and stale-seed rows.  Outputs start 0 ... 2 pixels into a
                 sentinel-filled allocation, frames 0 ... 100 pixels apart; float, RGBA8 or both.  Every frame bit for bit the
                 oracle's (the transparent checker's in transparent mode), RGBA8 byte for byte the quantised frame, lead and gaps
                 untouched, last_batch_info() as batch_fuzz_cases.expected_batch_info; then one handle alone at the batch's
                 config (the pass counters run on behind a batch); check() on every handle at the end.
b  host form     TileRenderer.renderBatch on a third of the same batches.
c  specials      configs the draws do not reach (background_batch_kernel, four stream waves per tile, 52 draws per pixel, a
                 batch of one), device form; 300 frames through renderBatch, every frame compared, two launch sequences.
d  pass batches  render_layers / ground / reflection_batch_device on 16 scenes under one config, each at its own plane height,
                 one handle listed twice at two heights, a stride gap and sentinels; every plane of every frame against
                 layers_checker / ground_checker / reflection_checker; ids by assert_ids_name_the_surfaces; check().
A failing comparison collects its text and the block goes on; a HIP error raises and ends the block.  That no frame of constants
and no swapped frame can pass is tests/test_batch_fuzz_cases.py's part."""
import numpy as np
import pytest
import torch

import batch_fuzz_cases as B
import ground_checker as G
import layers_checker as L
import reflection_checker as R
import scenes
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = {torch.float32: -12345.0, torch.uint8: 77, torch.int32: -12345}
# plane -> (element type, elements per pixel)
GROUND = {"visibility": (torch.float32, 1), "distance": (torch.float32, 1), "matte": (torch.uint8, 1)}
REFLECTION = {"rgba": (torch.float32, 4), "rgba8": (torch.uint8, 4), "distance": (torch.float32, 1)}
LAYERS = {"depth": (torch.float32, 1), "normal": (torch.float32, 4), "albedo": (torch.float32, 4), "id": (torch.int32, 4)}
PASS_GAP = 37  # pixels between the frames of a pass batch


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Failures(list):
    def compare(self, check, what=""):
        try:
            check()
        except AssertionError as e:
            self.append(f"MISMATCH {what}{str(e)[:600]}")


def _bytes_equal(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ; first (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def another_config(cfg, previous=None):
    """A config of another width AND another tile size than cfg's: the previous batch's where it is one, else a small one."""
    if previous is not None and previous.width != cfg.width and previous.tileSize != cfg.tileSize:
        return previous
    return abi.Config(width=cfg.width + 7, height=cfg.height, tileSize=8 if cfg.tileSize == 16 else 16, maxBounces=1, samplesPerPixel=2)


def _alone(ds, cfg):
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    ds.render_device_ex(cfg, out.data_ptr(), 0, 0, 1, abi.LAYOUT_FRAME, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_beauty_batch(mcrt, handles, case, exp, previous=None, single=0) -> list:
    """One device-form batch on `handles` (one per scene of the case); the mismatches as texts (a HIP error raises)."""
    sds, cfg, background, layout, what = case
    fails = Failures()
    n, px = len(handles), cfg.width * cfg.height
    stride, lead = px + layout["gap"], layout["lead"]
    other = another_config(cfg, previous)
    for i, h in enumerate(handles):
        h.set_background(background)
        _alone(h, cfg if i % 2 == 0 else other)  # fresh seeds / stale seeds and another workspace plan
    want_f, want_u = layout["outputs"] in ("both", "f32"), layout["outputs"] in ("both", "u8")
    total = lead + n * stride
    f = torch.full((total, 4), SENTINEL[torch.float32], dtype=torch.float32, device="cuda") if want_f else None
    u = torch.full((total, 4), SENTINEL[torch.uint8], dtype=torch.uint8, device="cuda") if want_u else None
    mcrt.render_batch_device(handles, cfg, f.data_ptr() + lead * 16 if want_f else 0, u.data_ptr() + lead * 4 if want_u else 0, stride, _stream())
    torch.cuda.synchronize()
    info, info_exp = mcrt.last_batch_info(), B.expected_batch_info(cfg, n)
    if info != info_exp:
        fails.append(f"MISMATCH {what}: last_batch_info() {info}, expected {info_exp}")
    for name, buf in (("float", f), ("rgba8", u)):
        if buf is None:
            continue
        a = buf.cpu().numpy()
        sentinel = SENTINEL[buf.dtype]
        if not (a[:lead] == sentinel).all():
            fails.append(f"MISMATCH {what}: plane {name}: written in front of frame 0")
        for i in range(n):
            at = lead + i * stride
            if not (a[at + px:at + stride] == sentinel).all():
                fails.append(f"MISMATCH {what}: plane {name}: the gap behind frame {i} was written")
            frame = a[at:at + px].reshape(cfg.height, cfg.width, 4)
            if name == "float":
                fails.compare(lambda: scenes.assert_bit_equal(frame, exp[i][0], f"{what}: frame {i} plane float"))
            else:
                fails.compare(lambda: _bytes_equal(frame, mcrt.quantize_rgba8(exp[i][0]), f"{what}: frame {i} plane rgba8"))
    k = single % n
    fails.compare(lambda: scenes.assert_bit_equal(_alone(handles[k], cfg), exp[k][0], f"{what}: handle {k} alone after the batch"))
    return fails


def run_host_batch(mcrt, case, exp) -> list:
    sds, cfg, background, layout, what = case
    fails = Failures()
    rgba8 = layout["outputs"] == "u8"
    imgs = mcrt.TileRenderer.renderBatch(sds, cfg, rgba8=rgba8, background=background)
    info, info_exp = mcrt.TileRenderer.lastBatchInfo(), B.expected_batch_info(cfg, len(sds))
    if info != info_exp:
        fails.append(f"MISMATCH {what} (host form): lastBatchInfo() {info}, expected {info_exp}")
    for i in range(len(sds)):
        if rgba8:
            fails.compare(lambda: _bytes_equal(imgs[i], mcrt.quantize_rgba8(exp[i][0]), f"{what} (host form): frame {i} plane rgba8"))
        else:
            fails.compare(lambda: scenes.assert_bit_equal(imgs[i], exp[i][0], f"{what} (host form): frame {i} plane float"))
    return fails


def _close(handles):
    for h in handles:
        h.close()


def run_beauty_block(mcrt, oracle, seeds, previous=None) -> list:
    """The batches `seeds` on one pool of handles: made once, passed from config to config, checked and closed at the end.
    previous: the config the stale handles of the first batch render at beforehand."""
    cases = [B.beauty_expectation(oracle, s, with_hits=False) for s in seeds]
    pool, fails = [], []
    try:
        for case, _ in cases:
            pool.append([mcrt.DeviceScene(sd) for sd in case[0]])
        for k, (case, exp) in enumerate(cases):
            fails += run_beauty_batch(mcrt, pool[k], case, exp, previous, single=seeds[k])
            previous = case[1]
        for handles in pool:
            for h in handles:
                h.check()
    finally:
        for handles in pool:
            _close(handles)
    return fails


def _pass_planes(spec, n, cfg):
    px = cfg.width * cfg.height
    stride = px + PASS_GAP
    return {k: torch.full((c + n * stride * c,), SENTINEL[t], dtype=t, device="cuda") for k, (t, c) in spec.items()}, stride


def _pass_frames(spec, buf, n, stride, cfg, what, fails) -> list:
    """The n frames of a pass batch as dicts of planes, after the sentinels in front of and between the frames."""
    px, out = cfg.width * cfg.height, [dict() for _ in range(n)]
    for k, (t, c) in spec.items():
        a = buf[k].cpu().numpy()
        if not (a[:c] == SENTINEL[t]).all():
            fails.append(f"MISMATCH {what}: plane {k}: written in front of frame 0")
        for i in range(n):
            at = c + i * stride * c
            if not (a[at + px * c:at + stride * c] == SENTINEL[t]).all():
                fails.append(f"MISMATCH {what}: plane {k}: the gap behind frame {i} was written")
            out[i][k] = a[at:at + px * c].reshape((cfg.height, cfg.width) + ((c,) if c > 1 else ()))
    return out


def _ptrs(spec, buf):
    # every plane starts one pixel into its allocation
    return {f"{k}_ptr": buf[k].data_ptr() + spec[k][1] * buf[k].element_size() for k in spec}


def run_pass_batch(mcrt, batch, ground, reflection, surfaces) -> list:
    """The three batched passes on one set of handles; the mismatches as texts (a HIP error raises)."""
    sds, cfg, heights, _, what = batch
    fails = Failures()
    frames = B.frames_of_pass_batch(batch)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        listed, ys = [handles[i] for i, _ in frames], [y for _, y in frames]
        buf, stride = _pass_planes(GROUND, len(frames), cfg)
        mcrt.render_ground_batch_device(listed, cfg, ys, frame_stride_pixels=stride, stream=_stream(), **_ptrs(GROUND, buf))
        torch.cuda.synchronize()
        for j, got in enumerate(_pass_frames(GROUND, buf, len(frames), stride, cfg, what + " | ground", fails)):
            fails.compare(lambda: G.assert_ground_equal(got, ground[j], f"{what} | ground: frame {j} (handle {frames[j][0]}) plane"))
        buf, stride = _pass_planes(REFLECTION, len(frames), cfg)
        mcrt.render_reflection_batch_device(listed, cfg, ys, frame_stride_pixels=stride, stream=_stream(), **_ptrs(REFLECTION, buf))
        torch.cuda.synchronize()
        for j, got in enumerate(_pass_frames(REFLECTION, buf, len(frames), stride, cfg, what + " | reflection", fails)):
            fails.compare(lambda: R.assert_reflection_equal(got, reflection[j], f"{what} | reflection: frame {j} (handle {frames[j][0]}) plane"))
        buf, stride = _pass_planes(LAYERS, len(handles), cfg)
        mcrt.render_layers_batch_device(handles, cfg, frame_stride_pixels=stride, stream=_stream(), **_ptrs(LAYERS, buf))
        torch.cuda.synchronize()
        for j, got in enumerate(_pass_frames(LAYERS, buf, len(handles), stride, cfg, what + " | layers", fails)):
            for k in ("depth", "normal", "albedo"):
                fails.compare(lambda: scenes.assert_bit_equal(got[k], surfaces[j][k], f"{what} | layers: frame {j} plane {k}"))
            fails.compare(lambda: L.assert_ids_name_the_surfaces(got["id"], surfaces[j], sds[j].to_numpy(), f"{what} | layers: frame {j} plane id"))
        for h in handles:
            h.check()
    finally:
        _close(handles)
    return fails


def _report(fails):
    assert not fails, f"{len(fails)} mismatches:\n" + "\n".join(fails[:40])


# One batch of a block of four per test: a whole block, and a half, take longer than the longest block of
# tests/test_gpu_pass_fuzz.py (the time is the oracle's, on the CPU).  The stale handles render beforehand at the config of the
# block's previous batch all the same.
@gpu_test
@pytest.mark.parametrize("first, k", [(first, k) for first in B.BEAUTY_BLOCKS for k in range(B.BLOCK_SIZE)])
def test_device_form_batch_equals_the_oracle(mcrt, gpu, oracle, first, k):
    previous = B.make_beauty_batch(first + k - 1)[1] if k > 0 else None
    _report(run_beauty_block(mcrt, oracle, [first + k], previous))


@gpu_test
@pytest.mark.parametrize("part", range(4))
def test_host_form_batches_equal_the_oracle(mcrt, gpu, oracle, part):
    fails = []
    for seed in B.host_form_seeds()[part::4]:
        case, exp = B.beauty_expectation(oracle, seed, with_hits=False)
        fails += run_host_batch(mcrt, case, exp)
    _report(fails)


@gpu_test
@pytest.mark.parametrize("name", B.SPECIALS)
def test_special_batch_equals_the_oracle(mcrt, gpu, oracle, name):
    case, exp = B.beauty_expectation(oracle, name, with_hits=False)
    if name == "three-hundred":
        fails = run_host_batch(mcrt, case, exp)
        assert mcrt.TileRenderer.lastBatchInfo() == {"batched_frames": 300, "launch_sequences": 2}
    else:
        handles = [mcrt.DeviceScene(sd) for sd in case[0]]
        try:
            fails = run_beauty_batch(mcrt, handles, case, exp)
            for h in handles:
                h.check()
        finally:
            _close(handles)
    _report(fails)


@gpu_test
def test_regression_far_camera_with_depth_of_field(mcrt, gpu, oracle):
    """Found by the batch sweep (seed 100411, frame 9); no matter of the batched entries: TileRenderer.render of the scene alone
    differed in the same way.  At 66 x 28, 3 spp, 1 x 1 tiles, depth of field with aperture 0.05 and focus distance 10, the camera
    5.7e7 from the origin, the oracle's frame holds 41 pixels with a hit; the device's frame differed from it in one pixel,
    (y, x) = (8, 32): (0.8539324, ...) — all three samples on the background — against the oracle's (0.59441495, 0.6258851,
    0.57059205), where one of the three samples hits a box.  The 1 x 1 tile of that pixel was taken for untouched:
    tile_mesh_mask's lens_pad bounded the displacement of a thin-lens ray for the exact lens only, aperture x |1/z - 1/z_focus|,
    while at this magnitude one ulp of the camera's coordinates (4) is of the order of the focus distance, so lens_ray's rounded
    origin and focus point give directions far outside that bound.  The bound now carries that rounding, and gives up where it
    is no small angle.  The single-frame fuzz never drew depth of field for a scaled scene (make_wide_case has none)."""
    case = B.make_far_camera_dof_batch()
    exp = B.expected_frames(oracle, case[0], case[1], case[2], with_hits=False)
    _report(run_host_batch(mcrt, case, exp))


@gpu_test
@pytest.mark.parametrize("key", list(B.PASS_BATCHES), ids=B.PASS_IDS)
def test_pass_batch_equals_the_oracle(mcrt, gpu, oracle, key):
    _report(run_pass_batch(mcrt, *B.pass_expectation(oracle, key)))
