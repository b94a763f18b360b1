"""Randomised parity of renders with extra lights against the expectation of tests/extra_lights_checker.py, in fixed blocks of 16
seeds (extra_lights_fuzz_cases.FUZZ_BLOCKS): scenes of boxes and of figures posed with free angles, key lights near, inside and
grazing boxes, and 1 to 3 extra lights inside, below, behind and around the figure, point lights and disks of radius up to 25,
colours up to 2.  The long sweep is tools/gpu_fuzz.py's mode lights.

Per case one DeviceScene renders the frame with its lights, then check(); every frame bit for bit, every case of a block, none
skipped.  Every other case is also rendered through the one-shot form.

No frame of constants can pass: before a block runs, the ORACLE's totals over it — hits, hits the extra lights change, hits over 1
before the clamp, penumbra pairs — must reach half of what tests/test_extra_lights_fuzz_cases.py pins exactly on the CPU."""
import pytest
import torch

import extra_lights_fuzz_cases as F
import scenes
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu


def run_case(mcrt, case, want, one_shot=False) -> list:
    """One DeviceScene, its lights, the frame, check(); the mismatches as texts (a HIP error raises)."""
    sd, cfg, lights, what = case
    failures = []
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        ds.render_device_ex(cfg, out.data_ptr(), 0, 0, 1, abi.LAYOUT_FRAME, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ds.check()
        try:
            scenes.assert_bit_equal(out.cpu().numpy(), want, what)
        except AssertionError as e:
            failures.append(str(e)[:600])
    finally:
        ds.close()
    if one_shot:
        img = mcrt.TileRenderer.render(sd, cfg, lights=lights)
        if mcrt.TileRenderer.lastErrors():
            failures.append(f"{what}: one-shot form: {mcrt.TileRenderer.lastErrors()}")
        try:
            scenes.assert_bit_equal(img, want, what + " (one-shot form)")
        except AssertionError as e:
            failures.append(str(e)[:600])
    return failures


@gpu_test
@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_block_equals_the_checker(mcrt, gpu, oracle, block):
    group, first = block
    exps = F.block_expectations(oracle, group, first)
    total, pinned = F.block_totals(exps), F.FUZZ_BLOCKS[block]
    print(block, "oracle totals (hits, changed hits, hits over 1, penumbra pairs):", total, "pinned on the CPU:", pinned)
    assert all(2 * t >= m for t, m in zip(total, pinned)), f"{block}: the oracle holds {total}, less than half of {pinned}"
    failures = []
    cases = F.block_cases(group, first)
    assert len(cases) == len(exps) == 16
    for i, case in enumerate(cases):
        failures += run_case(mcrt, case, exps[i][0], one_shot=i % 2 == 0)
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures)
