"""Randomised parity at the limits of the scene tables — 63 / 64 / 65 and up to 200 meshes, rotated meshes in the HBM view and in the
tail beyond mesh 63, texel pools of 65 536 and 65 537 texels, general-variant configs on such scenes — against the CPU oracle, in
fixed blocks of 12 cases of tests/big_scene_cases.py, three blocks per group; the long sweep is tools/gpu_fuzz.py's mode big, which
runs run_big_case of this file.

Per case, on one DeviceScene, every output bit for bit the oracle's (bytes for the 8-bit planes), then check():
  beauty      TileRenderer.render and render_device (every fourth case 1 or 2 pixels off its allocation); every third case both
              also with background="transparent" against tests/transparent_checker.py
  intersect   1 500 random rays aimed at the scene against oracle.intersect: hit, t, point, normal, colour, layer flag
  passes      ground, reflection, layers with 32 picks (test_gpu_pass_fuzz.run_case: the mesh the id plane and the picks name is
              the oracle's, tail meshes included) and the three light planes (test_gpu_light_fuzz.run_case; every other case also
              twice through the batched kernels), under big_scene_cases.pass_config — the passes refuse a general-variant config
Two fixed batches go through render_batch_device, the three batched passes and render_light_batch_device, every frame against the
oracle and against its own single call: a MIXED batch (an un-posed figure, a posed figure, a posed case of 65 meshes, a texels case
of 65 537 texels, a count case of 64 meshes: the HBM view forced on frames that alone take each LDS view) and the posed 64-mesh
scenes of five blocks, which stay in kViewLds at capacity: 384 face entries staged, rotated meshes, mesh 63 in use.

No frame of constants can pass: before a block runs, the ORACLE's census over it (big_scene_cases.CENSUS) must reach half of what
tests/test_big_scene_cases.py pins on the CPU.  MCRT_BUNDLE_DECISIONS=0 / MCRT_REFLECT_CULL=0 in the environment are left as they
are (tools/gpu_fuzz.py): they localise a mismatch by hand.

Measured on one MI355X machine, the whole suite running: 1.7 ... 3.8 s per block of count and posed, 0.9 ... 1.1 s per block of texels,
0.4 and 0.5 s per batch; the time is the oracle's, on the CPU."""
import numpy as np
import pytest
import torch

import batch_fuzz_cases as B
import big_scene_cases as BS
import ground_checker as G
import layers_checker as L
import light_checker as LC
import reflection_checker as R
import scenes
import test_gpu_batch_fuzz as TB
import test_gpu_light_fuzz as TL
import test_gpu_pass_fuzz as TP
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_big_case(mcrt, case, pexp, bexp, i: int, seed: int) -> list:
    """Everything of one case; i: its place in the block or sweep (leads, the transparent frame, the batched light kernels).
    The mismatches as texts (a HIP error raises)."""
    sd, cfg, ground, what = case[:4]
    pc = BS.pass_config(cfg)
    lead = TP.lead_of(i)
    fails = TB.Failures()
    img = mcrt.TileRenderer.render(sd, cfg)
    if mcrt.TileRenderer.lastErrors():
        fails.append(f"MISMATCH {what}: render failed: {mcrt.TileRenderer.lastErrors()}")
    fails.compare(lambda: scenes.assert_bit_equal(img, bexp["frame"], f"{what} | TileRenderer.render"))
    if bexp["transparent"] is not None:
        clear = mcrt.TileRenderer.render(sd, cfg, background="transparent")
        fails.compare(lambda: scenes.assert_bit_equal(clear, bexp["transparent"], f"{what} | TileRenderer.render transparent"))
    ds = mcrt.DeviceScene(sd)
    try:
        px = cfg.width * cfg.height
        out = torch.full((lead + px, 4), SENTINEL, dtype=torch.float32, device="cuda")
        ds.render_device(cfg, out.data_ptr() + lead * 16, stream=_stream())
        torch.cuda.synchronize()
        a = out.cpu().numpy()
        if not (a[:lead] == SENTINEL).all():
            fails.append(f"MISMATCH {what} | render_device: written in front of the frame")
        fails.compare(lambda: scenes.assert_bit_equal(a[lead:].reshape(cfg.height, cfg.width, 4), bexp["frame"], f"{what} | render_device"))
        if bexp["transparent"] is not None:  # the device form on a transparent background, then back
            ds.set_background("transparent")
            out.fill_(SENTINEL)
            ds.render_device(cfg, out.data_ptr() + lead * 16, stream=_stream())
            torch.cuda.synchronize()
            ds.set_background("reference")
            t = out.cpu().numpy()
            if not (t[:lead] == SENTINEL).all():
                fails.append(f"MISMATCH {what} | render_device transparent: written in front of the frame")
            fails.compare(lambda: scenes.assert_bit_equal(t[lead:].reshape(cfg.height, cfg.width, 4), bexp["transparent"], f"{what} | render_device transparent"))
        hits = ds.intersect(bexp["rays"])
        fails.compare(lambda: scenes.assert_hits_equal(hits, bexp["hits"], f"{what} | intersect"))
        fails += [f"MISMATCH {t}" for t in TP.run_case(mcrt, (sd, pc, ground, what), lead, pexp["ground"], pexp["reflection"], pexp["surfaces"], seed, ds=ds)]
        fails += [f"MISMATCH {t}" for t in TL.run_case(mcrt, (sd, pc, what), pexp["light"], TL.lead_of(i), twice=i % 2 == 0, ds=ds)]
        ds.check()
    finally:
        ds.close()
    return fails


@gpu_test
@pytest.mark.parametrize("block", list(BS.BLOCKS), ids=BS.BLOCK_IDS)
def test_block_equals_the_oracle(mcrt, gpu, oracle, block):
    group, first = block
    pexps = BS.check_block(oracle, group, first)
    fails = []
    for i, (case, seed) in enumerate(zip(BS.block_cases(group, first), BS.block_seeds(group, first))):
        fails += run_big_case(mcrt, case, pexps[i], BS.beauty_expectation(oracle, case, i, seed), i, seed)
    assert not fails, f"{len(fails)} mismatches:\n" + "\n".join(fails[:40])


# ---- the two fixed batches ---------------------------------------------------------------------------------------------
def batch_scenes(name) -> list:
    if name == "mixed":
        return [scenes.skin_scene("S64", 0), scenes.skin_scene("S64", 6), BS.make_big_case(BS.seed_with("posed", 36000, 65), "posed")[0],
                BS.make_big_case(BS.seed_with("texels", 36000, 65537), "texels")[0], BS.make_big_case(BS.seed_with("count", 36000, 64), "count")[0]]
    return [BS.make_big_case(BS.seed_with("posed", first, 64), "posed")[0] for first in (36000, 36036, 36072, 36108, 36144)]


BATCH_CONFIG = abi.Config(width=44, height=30, tileSize=16, maxBounces=2, samplesPerPixel=2, shadowSamples=8, aoSamples=5, aoRadius=3.0)
# the views of the frames alone, and of the batch: the weakest
BATCH_VIEWS = {"mixed": (["lds-unposed", "lds", "hbm", "hbm", "lds-unposed"], "hbm"), "sixty-four": (["lds"] * 5, "lds")}


def _light_batch(mcrt, handles, cfg, exps, what, fails):
    px, n = cfg.width * cfg.height, len(handles)
    buf = {k: torch.full((n * px * c,), SENTINEL, dtype=torch.float32, device="cuda") for k, c in TL.COMPONENTS.items()}
    mcrt.render_light_batch_device(handles, cfg, stream=_stream(), **{f"{k}_ptr": buf[k].data_ptr() for k in TL.COMPONENTS})
    torch.cuda.synchronize()
    for j, h in enumerate(handles):
        alone = TL.render(h, cfg)
        for k, c in TL.COMPONENTS.items():
            frame = buf[k].cpu().numpy().reshape(n, -1)[j].reshape(alone[k].shape)
            fails.compare(lambda: scenes.assert_bit_equal(frame, exps[j][k], f"{what} | light batch: frame {j} plane {k}"))
            fails.compare(lambda: scenes.assert_bit_equal(alone[k], exps[j][k], f"{what} | light alone: frame {j} plane {k}"))


@gpu_test
@pytest.mark.parametrize("name", list(BATCH_VIEWS))
def test_fixed_batch_equals_the_oracle_and_its_single_calls(mcrt, gpu, oracle, name):
    sds, cfg = batch_scenes(name), BATCH_CONFIG
    alone, together = BATCH_VIEWS[name]
    views = [B.expected_view(B.flat_header(sd)) for sd in sds]
    assert views == alone and ("hbm" if "hbm" in views else ("lds" if "lds" in views else "lds-unposed")) == together
    assert B.expected_envelope(cfg)
    if name == "sixty-four":  # at capacity: 64 meshes each, rotated ones among them, mesh 63 in use
        hdrs = [B.flat_header(sd) for sd in sds]
        assert all(h["n_meshes"] == 64 and h["posed"] and h["n_meshes"] * 6 == B.K_FACE_LDS_ENTRIES_MAX for h in hdrs)
    what = f"big batch {name}"
    heights = [mcrt.scene_floor(sd) for sd in sds]
    frames = B.expected_frames(oracle, sds, cfg, "reference", with_hits=False)
    ground = [G.expected_ground(oracle, sd, cfg, y) for sd, y in zip(sds, heights)]
    reflection = [R.expected_reflection(oracle, sd, cfg, y) for sd, y in zip(sds, heights)]
    surfaces = [L.expected_surfaces(oracle, sd, cfg.width, cfg.height) for sd in sds]
    light = [LC.expected_light(oracle, sd, cfg) for sd in sds]
    # frames that hold something: hits, shadowed ground, mirror images, tail meshes in the mixed batch
    assert all(int(s["hit"].sum()) > 50 for s in surfaces) and sum(G.counts(e)[1] + G.counts(e)[2] for e in ground) > 100
    assert sum(int(e["hit"].sum()) for e in reflection) > 100
    assert (name == "mixed") == any(int((s["mesh"] >= 64).sum()) > 0 for s in surfaces)
    if name == "sixty-four":  # the last bit of the mask is some pixel's closest hit, and rotated meshes are seen
        assert sum(int((s["mesh"] == 63).sum()) for s in surfaces) > 0
        assert all(int((h["flags"][np.maximum(s["mesh"], 0)] & B.MESH_ROTATED != 0)[s["hit"]].sum()) > 0 for h, s in zip(hdrs, surfaces))
    second = float(np.float32(heights[2] - 1.5))
    ground.append(G.expected_ground(oracle, sds[2], cfg, second))
    reflection.append(R.expected_reflection(oracle, sds[2], cfg, second))
    fails = TB.Failures()
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        case = (sds, cfg, "reference", dict(gap=1, lead=1, outputs="both"), what)
        fails += TB.run_beauty_batch(mcrt, handles, case, frames)
        for j, h in enumerate(handles):  # every frame's own single call
            fails.compare(lambda: scenes.assert_bit_equal(TB._alone(h, cfg), frames[j][0], f"{what}: handle {j} alone"))
        _light_batch(mcrt, handles, cfg, light, what, fails)
        for j, (sd, h) in enumerate(zip(sds, handles)):  # the passes' single calls, on the same handles
            fails += [f"MISMATCH {t}" for t in TP.run_case(mcrt, (sd, cfg, heights[j], f"{what}: handle {j} alone"), 0, ground[j], reflection[j], surfaces[j], j, ds=h)]
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()
    fails += TB.run_pass_batch(mcrt, (sds, cfg, heights, (2, second), what), ground, reflection, surfaces)
    assert not fails, f"{len(fails)} mismatches:\n" + "\n".join(fails[:40])
