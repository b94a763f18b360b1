"""The generator of the multi-light fuzz cases (light_multi_fuzz_cases.make_case) alone, on the CPU: it is deterministic, the lights
it draws span their ranges, the oracle holds over each fixed block EXACTLY what FUZZ_BLOCKS says (so that
tests/test_gpu_light_multi_fuzz.py compares planes that hold hits, penumbrae and changed sums, not constants), and every block
catches every wrong reading of the definition that a frame can show: a seed per light, ambient on every light, no per-light clamp,
the reverse summation order.  The two others cannot show in a frame, and the blocks say so: the raw normal in hard mode (unit
normals, tests/test_light_multi_checker.py) and `combined` as the clamp of the means (a frame has no sub-samples)."""
import numpy as np
import pytest

import light_checker as LC
import light_multi_checker as LM
import light_multi_fuzz_cases as F

SHOWS_IN_A_FRAME = ("seed_per_light", "ambient_per_light", "no_light_clamp", "reverse_order")


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _differing(a, b) -> int:
    return sum(int((np.ascontiguousarray(a[k]).view(np.uint32) != np.ascontiguousarray(b[k]).view(np.uint32)).sum()) for k in ("visibility", "direct", "combined"))


@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_cases_are_deterministic_and_the_lights_span_their_ranges(mcrt, block):
    group, first = block
    texts, counts, radii, colours = set(), [], [], []
    for seed in range(first, first + 16):
        (sd, cfg, lights, what), (sd2, cfg2, lights2, what2) = F.make_case(group, seed), F.make_case(group, seed)
        assert what == what2 and bytes(cfg.to_c()) == bytes(cfg2.to_c()) and _same(sd.to_numpy(), sd2.to_numpy())
        assert [bytes(l.to_c()) for l in lights] == [bytes(l.to_c()) for l in lights2]
        base = LC.make_light_case(group, seed)
        assert _same(sd.to_numpy(), base[0].to_numpy()) and bytes(cfg.to_c()) == bytes(base[1].to_c())  # the scene and frame are the generator's own
        texts.add(what)
        counts.append(len(lights))
        radii += [l.radius for l in lights]
        colours += [c for l in lights for c in l.color[:3]]
    assert len(texts) == 16 and min(counts) == 0 and max(counts) == 3
    assert all(r == 0.0 or 0.5 <= r <= 12.0 for r in radii) and 0.0 in radii and max(radii) > 6.0
    assert all(-0.5 <= c <= 2.0 for c in colours) and min(colours) < 0.0 and max(colours) > 1.0


@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_the_oracle_holds_the_blocks_totals_and_every_wrong_variant_is_caught(oracle, block):
    cases, exps = F.block_cases(*block), F.block_expectations(oracle, *block)
    assert len(cases) == len(exps) == 16
    for (_, _, lights, _), e in zip(cases, exps):
        LM.assert_constants(e, len(lights))
    total = F.block_totals(cases, exps)
    print(block, "extra lights, hits, penumbra pairs, changed hits, partly occluded hits:", total)
    assert total == F.FUZZ_BLOCKS[block]
    assert total[0] >= 10 and total[1] >= 2000 and total[2] >= 100 and total[3] >= 250 and total[4] >= 1000
    for variant in LM.WRONG_VARIANTS:
        caught = 0
        for (sd, cfg, lights, _), e in zip(cases, exps):
            if lights:
                caught += _differing(LM.expected_light_multi(oracle, sd, cfg, lights, variant=variant), e) > 0
        print(block, variant, "caught by", caught, "cases")
        if variant in SHOWS_IN_A_FRAME:
            assert caught >= 2, f"{block}: {variant} goes unnoticed"
        else:
            assert caught == 0, f"{block}: {variant} was held to be invisible in a frame"
