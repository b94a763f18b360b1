"""The generator of the light layers' fuzz cases (light_checker.make_light_case) alone, on the CPU: it is deterministic, the AO
settings it draws span 1 to 113 samples and a hundredth to ten times the scene's height, the oracle holds over each fixed block
EXACTLY what light_checker.FUZZ_BLOCKS says (so that tests/test_gpu_light_fuzz.py compares frames that hold hits, penumbra and
occlusion, not constants), and every expectation obeys its miss constants."""
import numpy as np
import pytest

import light_checker as LC
import pass_fuzz_cases as PF


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("block", list(LC.FUZZ_BLOCKS), ids=LC.FUZZ_BLOCK_IDS)
def test_cases_are_deterministic_and_the_ao_settings_span_their_ranges(mcrt, block):
    group, first = block
    texts, samples, ratios = set(), [], []
    for seed in range(first, first + 16):
        (sd, cfg, what), (sd2, cfg2, what2) = LC.make_light_case(group, seed), LC.make_light_case(group, seed)
        assert what == what2 and bytes(cfg.to_c()) == bytes(cfg2.to_c()) and _same(sd.to_numpy(), sd2.to_numpy())
        texts.add(what)
        lo, hi = PF.y_range(sd)
        assert 1 <= cfg.aoSamples <= 113 and np.isfinite(cfg.aoRadius) and cfg.aoRadius > 0
        assert not (cfg.softShadows and cfg.shadowSamples > 113)
        samples.append(cfg.aoSamples)
        ratios.append(cfg.aoRadius / (hi - lo))
    assert len(texts) == 16
    assert all(0.0099 < r < 10.01 for r in ratios) and min(ratios) < 0.1 and max(ratios) > 1.0
    assert min(samples) <= 16 and max(samples) >= 64


def test_the_scene_and_frame_of_a_case_are_the_generators_own(mcrt):
    import fuzz_cases

    sd, cfg, what = LC.make_light_case("bundle", 7003)
    psd, pcfg, _, _ = PF.make_pass_case(7003)
    assert _same(sd.to_numpy(), psd.to_numpy()) and (cfg.width, cfg.height, cfg.tileSize, cfg.shadowSamples) == (pcfg.width, pcfg.height, pcfg.tileSize, pcfg.shadowSamples)
    sd, cfg, what = LC.make_light_case("wide", 9003)
    assert _same(sd.to_numpy(), PF.make_wide_pass_case(9003)[0].to_numpy())
    sd, cfg, what = LC.make_light_case("bundle-plain", 21003)
    bsd, bcfg, _ = fuzz_cases.make_bundle_case(21003)
    assert _same(sd.to_numpy(), bsd.to_numpy()) and (cfg.width, cfg.height, cfg.tileSize) == (bcfg.width, bcfg.height, bcfg.tileSize)


@pytest.mark.parametrize("block", list(LC.FUZZ_BLOCKS), ids=LC.FUZZ_BLOCK_IDS)
def test_the_oracle_holds_the_blocks_totals(oracle, block):
    exps = LC.block_expectations(oracle, *block)
    assert len(exps) == 16
    for e in exps:
        LC.assert_miss_constants(e)
    total = LC.block_totals(exps)
    print(block, "hits, penumbra hits, partly occluded hits:", total)
    assert total == LC.FUZZ_BLOCKS[block]
    assert total[0] >= 2000 and total[1] >= 150 and total[2] >= 1000
