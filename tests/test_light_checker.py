"""tests/light_checker.py against the oracle's own render (CPU, no device): the two recomposition identities of include/mcrt.h —
the beauty frame at 1 spp, 0 bounces, no depth of field equals `direct` without ambient occlusion, and clamp(direct.rgb *
(1 - intensity * (1 - occlusion))) with it — on every pixel with a hit, bit for bit, soft and hard; and the counts that keep a
frame of constants from passing any test built on the checker."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import light_checker as LC  # noqa: E402
import scenes  # noqa: E402

# case -> (checker arguments, (hits, dark, penumbra, occlusion < 1, occlusion = 0 or None: not pinned))
CASES = {
    "pose0_default_96x64": (dict(), (551, 68, 32, 182, 10)),
    "pose6_orbit_96x64": (dict(radius=25.0), (1079, 790, 288, 352, None)),
    "pose5_orbit_64x64_t16": (dict(samples=113, ao_samples=113), (1790, 451, 521, 825, None)),
    "pose0_33x17_t7": (dict(), (40, 5, 2, 11, 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_counts_of_the_expectation(name):
    kw, want = CASES[name]
    sd, cfg, exp = LC.skin_expectation(name, **kw)
    got = LC.counts(exp)
    print(name, "hits, dark, penumbra, occlusion < 1, occlusion = 0:", got, "distinct occlusion values:", len(np.unique(exp["occlusion"][exp["hit"]])))
    for g, w in zip(got, want):
        assert w is None or g == w, (got, want)
    LC.assert_miss_constants(exp)
    hit = exp["hit"]
    assert (exp["direct"][hit][:, 3] > 0).all()  # a hit's texel is never fully transparent
    assert ((exp["visibility"] >= 0) & (exp["visibility"] <= 1)).all() and ((exp["occlusion"] >= 0) & (exp["occlusion"] <= 1)).all()
    if name == "pose0_default_96x64":
        v = exp["visibility"][hit]
        assert int((v == 1).sum()) == 451  # the other hits are fully lit
    if name == "pose5_orbit_64x64_t16":
        assert len(np.unique(exp["occlusion"][hit])) == 109


@pytest.mark.parametrize("name", ["pose0_default_96x64", "pose6_orbit_96x64", "pose5_orbit_64x64_t16", "pose0_33x17_t7"])
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_recomposition_against_the_oracles_render(oracle, name, soft):
    kw = dict(CASES[name][0]) if soft else {k: v for k, v in CASES[name][0].items() if k == "radius"}
    sd, cfg, exp = LC.skin_expectation(name, soft=soft, **kw)
    hit = exp["hit"]
    assert hit.sum() >= 40
    plain = oracle.render(sd.ptr, LC.beauty_config(cfg)).reshape(cfg.height, cfg.width, 4)
    scenes.assert_bit_equal(plain[hit], exp["direct"][hit], f"{name}: beauty without AO against direct")
    with_ao = oracle.render(sd.ptr, LC.beauty_config(cfg, ao=True, intensity=0.5)).reshape(cfg.height, cfg.width, 4)
    scenes.assert_bit_equal(with_ao[hit], LC.recompose(exp["direct"], exp["occlusion"], 0.5)[hit], f"{name}: beauty with AO against the recomposition")
    if (exp["occlusion"][hit] < 1).any():  # the two frames differ: the identity with AO is not the one without
        assert not np.array_equal(with_ao[hit], plain[hit])
    if soft and not kw:
        other = LC.skin_expectation(name, soft=False)[2]
        assert not np.array_equal(other["visibility"], exp["visibility"])  # the hard mode is another plane
