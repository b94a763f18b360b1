"""Randomised parity of the scene-only passes — ground shadow, ground reflection, geometry layers and picks — against the CPU
oracle, in fixed blocks of 16 seeds of tests/pass_fuzz_cases.py; the long sweeps are tools/gpu_fuzz.py's modes ground, reflection,
layers, long-shadow and far-plane.

Per case one DeviceScene runs the device form of every pass, then check():
  ground      visibility and distance bit for bit, the matte byte for byte (ground_checker) — groups A (bundle and wide, each case
              also under a light lifted clear above every mesh, so that ground_tile_mask bounds shadows and does not merely keep
              every mesh), B (long shadows: ground points up to 30 000 out, beyond the magnitude FlatHeader::mask_slack is formed
              from) and C (planes 10 ... 10 000 scene heights down)
  reflection  rgba and distance bit for bit, rgba8 byte for byte (reflection_checker) — A, B and C
  layers      depth, normal and albedo bit for bit, hit and mesh exactly; the random textures repeat colours, so the texel the pass
              names, looked up in the scene description, must hold the oracle's albedo (layers_checker.assert_ids_name_the_surfaces);
              picks at 32 random pixels equal the planes — A
Every fourth case renders into planes that start 1 or 2 elements off their allocation (layers: the depth plane; its 16-byte planes
start 1 or 2 pixels in), the elements in front must keep their sentinel; the random widths then take the one-element stores.

No frame of constants can pass: before a block runs, the ORACLE's totals over it are asserted (pass_fuzz_cases.BLOCKS: exactly for
the first block of A and B, to half of the measured totals elsewhere; 100 dark, 100 penumbra and 100 reflected pixels per block
of C; 3275 dark and 504 penumbra pixels beyond 1e3 in B's first block), and at least a third of A's ground cases have the light
clear above every mesh by ground_tile_mask's own criterion."""
import numpy as np
import pytest
import torch

import ground_checker as G
import layers_checker as L
import pass_fuzz_cases as PF
import reflection_checker as R
import scenes
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = {torch.float32: -12345.0, torch.uint8: 77, torch.int32: -12345}
# plane -> (element type, elements per pixel, elements of lead per step: a 16-byte plane moves by whole pixels)
GROUND = {"visibility": (torch.float32, 1, 1), "distance": (torch.float32, 1, 1), "matte": (torch.uint8, 1, 1)}
REFLECTION = {"rgba": (torch.float32, 4, 1), "rgba8": (torch.uint8, 4, 1), "distance": (torch.float32, 1, 1)}
LAYERS = {"depth": (torch.float32, 1, 1), "normal": (torch.float32, 4, 4), "albedo": (torch.float32, 4, 4), "id": (torch.int32, 4, 4)}


def lead_of(i: int) -> int:
    """Every fourth case of a block: 1 or 2 elements off the allocation."""
    return 0 if i % 4 != 3 else 1 + (i // 4) % 2


def _render(spec, cfg, lead, launch) -> dict:
    """Planes of `spec` filled with sentinels, `lead` steps in front of each; launch(**pointers); the frames as numpy arrays."""
    px = cfg.width * cfg.height
    buf = {k: torch.full((lead * step + px * c,), SENTINEL[t], dtype=t, device="cuda") for k, (t, c, step) in spec.items()}
    launch(stream=torch.cuda.current_stream().cuda_stream,
           **{f"{k}_ptr": buf[k].data_ptr() + lead * spec[k][2] * buf[k].element_size() for k in spec})
    torch.cuda.synchronize()
    out = {}
    for k, (t, c, step) in spec.items():
        a = buf[k].cpu().numpy()
        assert (a[:lead * step] == SENTINEL[t]).all(), f"{k}: written in front of the plane"
        out[k] = a[lead * step:].reshape((cfg.height, cfg.width) + ((c,) if c > 1 else ()))
    return out


def _ground(ds, cfg, ground, lead):
    return _render(GROUND, cfg, lead, lambda **kw: ds.render_ground_device(cfg, ground, **kw))


def _reflection(ds, cfg, ground, lead):
    return _render(REFLECTION, cfg, lead, lambda **kw: ds.render_reflection_device(cfg, ground, **kw))


def _layers(ds, cfg, lead):
    return _render(LAYERS, cfg, lead, lambda **kw: ds.render_layers_device(cfg, **kw))


def _check_layers(ds, sd, cfg, got, surf, seed, what):
    for k in ("depth", "normal", "albedo"):
        scenes.assert_bit_equal(got[k], surf[k], f"{what} {k}")
    L.assert_ids_name_the_surfaces(got["id"], surf, sd.to_numpy(), what)
    g = np.random.default_rng(seed ^ 0x91C4)
    xy = np.stack([g.integers(0, cfg.width, 32), g.integers(0, cfg.height, 32)], axis=1).astype(np.int64)
    rec = ds.pick(cfg, xy)
    at = (xy[:, 1], xy[:, 0])
    assert np.array_equal(np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1), got["id"][at]), f"{what} pick id"
    scenes.assert_bit_equal(rec["t"], got["depth"][at], f"{what} pick t")
    scenes.assert_bit_equal(rec["normal"], got["normal"][at], f"{what} pick normal")
    scenes.assert_bit_equal(rec["albedo"], got["albedo"][at], f"{what} pick albedo")
    scenes.assert_bit_equal(rec["point"], surf["point"][at], f"{what} pick point")


def run_case(mcrt, case, lead, ground_exp=None, reflection_exp=None, surfaces=None, seed=0, ds=None) -> list:
    """One DeviceScene (the caller's `ds`, which stays open, or one made and closed here), every pass an expectation is given for,
    check(); the mismatches as texts (a HIP error raises)."""
    sd, cfg, ground, what = case
    failures = []

    def compare(check):
        try:
            check()
        except AssertionError as e:
            failures.append(str(e)[:600])

    own = ds is None
    if own:
        ds = mcrt.DeviceScene(sd)
    try:
        if ground_exp is not None:
            got = _ground(ds, cfg, ground, lead)
            compare(lambda: G.assert_ground_equal(got, ground_exp, what + " | ground"))
        if reflection_exp is not None:
            got_r = _reflection(ds, cfg, ground, lead)
            compare(lambda: R.assert_reflection_equal(got_r, reflection_exp, what + " | reflection"))
        if surfaces is not None:
            got_l = _layers(ds, cfg, lead)
            compare(lambda: _check_layers(ds, sd, cfg, got_l, surfaces, seed, what + " | layers"))
        ds.check()
    finally:
        if own:
            ds.close()
    return failures


@gpu_test
@pytest.mark.parametrize("block", list(PF.BLOCKS), ids=PF.BLOCK_IDS)
def test_block_equals_the_oracle(mcrt, gpu, oracle, block):
    group, first = block
    ground = PF.check_ground_block(oracle, group, first)
    reflection = PF.check_reflection_block(oracle, group, first)
    surfaces = PF.check_surface_block(oracle, group, first) if block in PF.A_BLOCKS else [None] * 16
    failures = []
    for i, case in enumerate(PF.block_cases(group, first)):
        failures += run_case(mcrt, case, lead_of(i), ground[i], reflection[i], surfaces[i], first + i)
    if block in PF.A_BLOCKS:  # the same cases under a light clear above every mesh: the culling branch of ground_tile_mask
        cases, exps = PF.check_lifted_block(oracle, group, first)
        for i, case in enumerate(cases):
            failures += run_case(mcrt, case, lead_of(i + 2), exps[i])
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures)
