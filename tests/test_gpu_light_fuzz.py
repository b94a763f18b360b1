"""Randomised parity of the light layers (mcrt_render_light*) against the CPU oracle, in fixed blocks of 16 seeds
(light_checker.FUZZ_BLOCKS): the scenes and frames of pass_fuzz_cases.make_pass_case and make_wide_pass_case and of
fuzz_cases.make_bundle_case — lights near, inside and grazing boxes, texel grids of every density, flat boxes, figures posed with
free angles, scenes scaled by 1e-5 ... 1e6 or moved up to 3e6 away — with AO settings drawn per case: 1 to 113 samples, a radius from
a hundredth of the scene's height to ten times it.  The long sweep is tools/gpu_fuzz.py's mode light.

Per case one DeviceScene renders the three planes in one call, then check(); every plane bit for bit, every case of a block, none
skipped.  Every fourth case renders into planes that start 1 or 2 floats off their allocation (the floats in front must keep
their sentinel); every other case also goes through the batched kernels — its scene twice in one call — against its single call.

No frame of constants can pass: before a block runs, the ORACLE's totals over it — hits, penumbra hits, partly occluded hits — must
reach half of what tests/test_light_fuzz_cases.py pins exactly on the CPU."""
import numpy as np
import pytest
import torch

import light_checker as LC
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
COMPONENTS = {"visibility": 1, "occlusion": 1, "direct": 4}


def lead_of(i: int) -> int:
    """Every fourth case of a block: 1 or 2 floats off the allocation."""
    return 0 if i % 4 != 3 else 1 + (i // 4) % 2


def render(ds, cfg, lead=0) -> dict:
    px = cfg.width * cfg.height
    buf = {k: torch.full((lead + px * c,), SENTINEL, dtype=torch.float32, device="cuda") for k, c in COMPONENTS.items()}
    ds.render_light_device(cfg, stream=torch.cuda.current_stream().cuda_stream, **{f"{k}_ptr": buf[k].data_ptr() + lead * 4 for k in COMPONENTS})
    torch.cuda.synchronize()
    out = {}
    for k, c in COMPONENTS.items():
        a = buf[k].cpu().numpy()
        assert (a[:lead] == SENTINEL).all(), f"{k}: written in front of the plane"
        out[k] = a[lead:].reshape((cfg.height, cfg.width) + ((c,) if c > 1 else ()))
    return out


def run_case(mcrt, case, exp, lead=0, twice=False, ds=None) -> list:
    """One DeviceScene (the caller's `ds`, which stays open, or one made and closed here), the three planes, check(); the
    mismatches as texts (a HIP error raises)."""
    sd, cfg, what = case
    failures = []
    own = ds is None
    if own:
        ds = mcrt.DeviceScene(sd)
    try:
        got = render(ds, cfg, lead)
        try:
            LC.assert_light_equal(got, exp, what)
        except AssertionError as e:
            failures.append(str(e)[:600])
        if twice:  # the batched kernels: the scene twice in one call
            px = cfg.width * cfg.height
            buf = {k: torch.full((2 * px * c,), SENTINEL, dtype=torch.float32, device="cuda") for k, c in COMPONENTS.items()}
            mcrt.render_light_batch_device([ds, ds], cfg, stream=torch.cuda.current_stream().cuda_stream, **{f"{k}_ptr": buf[k].data_ptr() for k in COMPONENTS})
            torch.cuda.synchronize()
            for k, c in COMPONENTS.items():
                a = buf[k].cpu().numpy().reshape(2, -1)
                for i in range(2):
                    if a[i].tobytes() != np.ascontiguousarray(got[k]).tobytes():
                        failures.append(f"{what}: batch frame {i} plane {k} differs from the single call")
        ds.check()
    finally:
        if own:
            ds.close()
    return failures


@gpu_test
@pytest.mark.parametrize("block", list(LC.FUZZ_BLOCKS), ids=LC.FUZZ_BLOCK_IDS)
def test_block_equals_the_oracle(mcrt, gpu, oracle, block):
    group, first = block
    exps = LC.block_expectations(oracle, group, first)
    for e in exps:
        LC.assert_miss_constants(e)
    total, pinned = LC.block_totals(exps), LC.FUZZ_BLOCKS[block]
    print(block, "oracle totals (hits, penumbra hits, partly occluded hits):", total, "pinned on the CPU:", pinned)
    assert all(2 * t >= m for t, m in zip(total, pinned)), f"{block}: the oracle holds {total}, less than half of {pinned}"
    assert total[0] >= 1000 and total[1] >= 75 and total[2] >= 500
    failures = []
    cases = LC.block_cases(group, first)
    assert len(cases) == len(exps) == 16
    for i, case in enumerate(cases):
        failures += run_case(mcrt, case, exps[i], lead_of(i), twice=i % 2 == 0)
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures)
