"""Randomised parity of the light layers under extra lights (mcrt_render_light_multi*) against the CPU oracle, in fixed blocks of 16
seeds (light_multi_fuzz_cases.FUZZ_BLOCKS): the cases of the light layers' fuzz with 0 to 3 random lights each — point and disk
lights around the scene, colour channels from -0.5 to 2.

Per case one DeviceScene takes the lights and renders every plane — four visibility, four direct, occlusion, combined — in one
call, then check(); every plane bit for bit, every case of a block, none skipped.  Every fourth case renders into planes that start
1 or 2 floats off their allocation (the floats in front must keep their sentinel); every other case also goes through the batched
kernels — its scene twice in one call — against its single call.

No frame of constants can pass: before a block runs, the ORACLE's totals over it — extra lights, hits, penumbra pairs, hits the
extra lights changed, partly occluded hits — must reach half of what tests/test_light_multi_fuzz_cases.py pins exactly on the CPU."""
import numpy as np
import pytest
import torch

import light_multi_checker as LM
import light_multi_fuzz_cases as F
import scenes
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
MAXL = abi.MAX_LIGHTS
PLANES = tuple(("visibility", k, 1) for k in range(MAXL)) + tuple(("direct", k, 4) for k in range(MAXL)) + (("occlusion", None, 1), ("combined", None, 4))


def lead_of(i: int) -> int:
    """Every fourth case of a block: 1 or 2 floats off the allocation."""
    return 0 if i % 4 != 3 else 1 + (i // 4) % 2


def _args(buf, lead):
    ptr = lambda name, k: buf[(name, k)].data_ptr() + 4 * lead  # noqa: E731
    return dict(visibility_ptrs=[ptr("visibility", k) for k in range(MAXL)], direct_ptrs=[ptr("direct", k) for k in range(MAXL)],
                occlusion_ptr=ptr("occlusion", None), combined_ptr=ptr("combined", None))


def run_case(mcrt, case, exp, lead=0, twice=False) -> list:
    """One DeviceScene with the case's lights, every plane, check(); the mismatches as texts (a HIP error raises)."""
    sd, cfg, lights, what = case
    px = cfg.width * cfg.height
    failures = []
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        stream = torch.cuda.current_stream().cuda_stream
        buf = {(n, k): torch.full((lead + px * c,), SENTINEL, dtype=torch.float32, device="cuda") for n, k, c in PLANES}
        ds.render_light_multi_device(cfg, stream=stream, **_args(buf, lead))
        torch.cuda.synchronize()
        got = {}
        for n, k, c in PLANES:
            a = buf[(n, k)].cpu().numpy()
            assert (a[:lead] == SENTINEL).all(), f"{what}: {n}: written in front of the plane"
            got[(n, k)] = a[lead:]
            want = exp[n] if k is None else exp[n][k]
            try:
                scenes.assert_bit_equal(got[(n, k)].reshape(want.shape), want, f"{what}: {n}{'' if k is None else [k]}")
            except AssertionError as e:
                failures.append(str(e)[:600])
        if twice:  # the batched kernels: the scene twice in one call
            two = {(n, k): torch.full((2 * px * c,), SENTINEL, dtype=torch.float32, device="cuda") for n, k, c in PLANES}
            mcrt.render_light_multi_batch_device([ds, ds], cfg, stream=stream, **_args(two, 0))
            torch.cuda.synchronize()
            for n, k, c in PLANES:
                a = two[(n, k)].cpu().numpy().reshape(2, -1)
                for i in range(2):
                    if a[i].tobytes() != got[(n, k)].tobytes():
                        failures.append(f"{what}: batch frame {i} plane {n}{k} differs from the single call")
        ds.check()
    finally:
        ds.close()
    return failures


@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_block_equals_the_oracle(mcrt, gpu, oracle, block):
    cases, exps = F.block_cases(*block), F.block_expectations(oracle, *block)
    assert len(cases) == len(exps) == 16
    for (_, _, lights, _), e in zip(cases, exps):
        LM.assert_constants(e, len(lights))
    total, pinned = F.block_totals(cases, exps), F.FUZZ_BLOCKS[block]
    print(block, "oracle totals (extra lights, hits, penumbra pairs, changed hits, partly occluded hits):", total, "pinned on the CPU:", pinned)
    assert all(2 * t >= m for t, m in zip(total, pinned)), f"{block}: the oracle holds {total}, less than half of {pinned}"
    assert total[0] >= 10 and total[1] >= 1000 and total[2] >= 50 and total[3] >= 125
    failures = []
    for i, case in enumerate(cases):
        failures += run_case(mcrt, case, exps[i], lead_of(i), twice=i % 2 == 0)
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures)
