"""Randomised parity of the light bake (mcrt_bake_light*) against the CPU oracle, in fixed blocks of 8 seeds
(bake_checker.FUZZ_BLOCKS), at grid 1: the scenes and settings of light_checker.make_light_case — lights near, inside and grazing
boxes, texel grids of every density, textures shared between faces, flat boxes, figures posed with free angles, scenes scaled by
1e-5 ... 1e6 or moved up to 3e6 away, 1 to 113 AO samples at radii from a hundredth of the scene's height to ten times it.

Per case one DeviceScene bakes the five planes in one call, then check(); every plane bit for bit, every texel of every case of a
block, none skipped.  Every fourth case bakes into planes that start 1 or 2 floats off their allocation (the floats in front must
keep their sentinel); every other case also goes through the batched kernels — its scene twice in one call — against its single
call.

No planes of constants can pass: before a block runs, the ORACLE's totals over it — texels, live, penumbra and partly occluded
texels — must be what tests/test_bake_checker.py pins on the CPU."""
import numpy as np
import pytest
import torch

import bake_checker as B
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
COMPONENTS = {k: c for k, (_, c) in abi.BAKE_FORMATS.items()}


def lead_of(i: int) -> int:
    """Every fourth case of a block: 1 or 2 floats off the allocation."""
    return 0 if i % 4 != 3 else 1 + (i // 4) % 2


def bake(ds, cfg, lead=0, grid=1) -> dict:
    n = ds.texels
    buf = {k: torch.full((lead + n * c,), SENTINEL, dtype=torch.float32, device="cuda") for k, c in COMPONENTS.items()}
    ds.bake_light_device(cfg, grid, stream=torch.cuda.current_stream().cuda_stream, **{f"{k}_ptr": buf[k].data_ptr() + lead * 4 for k in COMPONENTS})
    torch.cuda.synchronize()
    out = {}
    for k, c in COMPONENTS.items():
        a = buf[k].cpu().numpy()
        assert (a[:lead] == SENTINEL).all(), f"{k}: written in front of the plane"
        out[k] = a[lead:].reshape((n, c) if c > 1 else (n,))
    return out


def run_case(mcrt, case, exp, lead=0, twice=False, grid=1) -> list:
    """One DeviceScene, the five planes, check(); the mismatches as texts (a HIP error raises)."""
    sd, cfg, what = case
    failures = []
    ds = mcrt.DeviceScene(sd)
    try:
        assert ds.texels == len(exp["table"])
        got = bake(ds, cfg, lead, grid)
        try:
            B.assert_bake_equal(got, exp, what)
        except AssertionError as e:
            failures.append(str(e)[:600])
        if twice and ds.texels:  # the batched kernels: the scene twice in one call
            n = ds.texels
            buf = {k: torch.full((2 * n * c,), SENTINEL, dtype=torch.float32, device="cuda") for k, c in COMPONENTS.items()}
            mcrt.bake_light_batch_device([ds, ds], cfg, grid, texel_stride=n, stream=torch.cuda.current_stream().cuda_stream,
                                         **{f"{k}_ptr": buf[k].data_ptr() for k in COMPONENTS})
            torch.cuda.synchronize()
            for k in COMPONENTS:
                a = buf[k].cpu().numpy().reshape(2, -1)
                for i in range(2):
                    if a[i].tobytes() != np.ascontiguousarray(got[k]).tobytes():
                        failures.append(f"{what}: batch frame {i} plane {k} differs from the single call")
        ds.check()
    finally:
        ds.close()
    return failures


@gpu_test
@pytest.mark.parametrize("block", list(B.FUZZ_BLOCKS), ids=B.FUZZ_BLOCK_IDS)
def test_block_equals_the_oracle(mcrt, gpu, oracle, block):
    group, first = block
    exps = B.block_expectations(oracle, group, first)
    for e in exps:
        B.assert_dead_constants(e)
    total = B.block_totals(exps)
    print(block, "oracle totals (texels, live, penumbra, partly occluded):", total)
    assert total == B.FUZZ_BLOCKS[block], f"{block}: the oracle holds {total}, not {B.FUZZ_BLOCKS[block]}"
    failures = []
    cases = B.block_cases(group, first)
    assert len(cases) == len(exps) == 8
    for i, case in enumerate(cases):
        failures += run_case(mcrt, case, exps[i], lead_of(i), twice=i % 2 == 0)
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures)
