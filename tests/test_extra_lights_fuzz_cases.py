"""The generator of the extra-lights fuzz cases (extra_lights_fuzz_cases.make_lights_case) alone, on the CPU: it is deterministic,
the lights it draws span what the module says, and the oracle holds over each fixed block EXACTLY what FUZZ_BLOCKS says — so that
tests/test_gpu_extra_lights_fuzz.py compares frames in which the extra lights change hits, saturate some and cast penumbrae."""
import numpy as np
import pytest

import extra_lights_fuzz_cases as F


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_cases_are_deterministic_and_the_lights_span_their_ranges(mcrt, block):
    group, first = block
    texts, counts, radii, colours = set(), [], [], []
    for seed in range(first, first + 16):
        (sd, cfg, lights, what), (sd2, cfg2, lights2, what2) = F.make_lights_case(group, seed), F.make_lights_case(group, seed)
        assert what == what2 and bytes(cfg.to_c()) == bytes(cfg2.to_c()) and _same(sd.to_numpy(), sd2.to_numpy())
        assert [bytes(l.to_c()) for l in lights] == [bytes(l.to_c()) for l in lights2]
        assert cfg.width <= 64 and cfg.height <= 64 and cfg.samplesPerPixel == 1 and 0 <= cfg.maxBounces <= 2
        assert 1 <= len(lights) <= 3
        texts.add(what)
        counts.append(len(lights))
        radii += [l.radius for l in lights]
        colours += [v for l in lights for v in l.color[:3]]
    assert len(texts) == 16 and set(counts) == {1, 2, 3}
    assert min(radii) == 0.0 and 0.0 < min(r for r in radii if r > 0) and max(radii) <= 25.0 and max(radii) > 12.0
    assert min(colours) >= 0.0 and max(colours) <= 2.0 and max(colours) > 1.5 and min(colours) < 0.5


@pytest.mark.parametrize("block", list(F.FUZZ_BLOCKS), ids=F.FUZZ_BLOCK_IDS)
def test_the_oracle_holds_the_blocks_totals(oracle, block):
    exps = F.block_expectations(oracle, *block)
    assert len(exps) == 16
    total = F.block_totals(exps)
    print(block, "hits, changed hits, hits over 1 before the clamp, penumbra pairs:", total)
    assert total == F.FUZZ_BLOCKS[block]
    assert total[0] >= 2000 and total[1] >= 1000 and total[2] >= 30 and total[3] >= 1000
