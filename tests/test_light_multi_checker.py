"""tests/light_multi_checker.py on the CPU: without extra lights it IS the single-light checkers, its `combined` recomposes the
multi-light beauty frame of tests/extra_lights_checker.py, the GPU suite's cases hold what they are meant to hold, and the wrong
readings of the definition are told apart.

Two of the six wrong readings cannot show everywhere, and why is asserted rather than passed over:

* the raw normal in hard mode: intersectMesh returns unit normals (|N| within 2.5e-7 of 1), and the bake's normals are axis
  vectors or normalised ones, so the shadow origin moves by less than 3e-10 and no plane can differ
  (tests/test_extra_lights_checker.py has the bound on the posed frames; it is asserted here on the frame used).
* `combined` as the clamp of the means: a frame has no sub-samples, and at grid 1 a texel has one, so the two readings are the same
  expression there; at grid 2 under the bright light they differ.
* no per-light clamp changes the direct planes wherever a term left [0, 1], but `combined` only through the lower bound
  (C >= 0, so clamp(C + min(E, 1)) = clamp(C + E)): `bright_front+negative` is its case, as for the beauty frame."""
import numpy as np
import pytest

import bake_checker as B
import extra_lights_checker as X
import layers_checker as L
import light_checker as LC
import light_multi_checker as LM
import scenes
from minecraftskin_raytracer_amd import abi

POSE0 = "pose0_default_96x64"
# (hits, penumbra pixels of the extra disk lights in order, hits whose combined differs from direct[0]) at S = 8
COUNTS = {
    "fill_left+kicker": (551, (36,), 507),
    "three": (551, (36, 87), 534),
    "bright_front": (551, (39,), 551),
    "bright_front+negative": (551, (39, 50), 551),
}


def _differing(a, b) -> int:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    d = a.view(np.uint32) != b.view(np.uint32)
    return int(d.reshape(-1, a.shape[-1]).any(axis=-1).sum()) if a.ndim > 2 and a.shape[-1] == 4 else int(d.sum())


# ---- (a) without extra lights ------------------------------------------------------------------------------------------------
def test_without_lights_the_layers_are_light_checkers():
    sd, cfg, exp = LM.skin_expectation(POSE0)
    _, _, single = LC.skin_expectation(POSE0)
    for k in ("visibility", "direct"):
        scenes.assert_bit_equal(exp[k][0], single[k], k + "[0]")
    scenes.assert_bit_equal(exp["occlusion"], single["occlusion"], "occlusion")
    scenes.assert_bit_equal(exp["combined"], single["direct"], "combined = clamp(D_0) = D_0")
    assert np.array_equal(exp["hit"], single["hit"])
    LM.assert_constants(exp, 0)


def test_without_lights_the_bake_is_bake_checkers():
    sd, cfg, exp = LM.bake_skin_expectation("S64", 0, 2)
    _, _, single = B.skin_expectation("S64", 0, 2)
    for k in ("visibility", "direct"):
        scenes.assert_bit_equal(exp[k][0], single[k], k + "[0]")
    for k in ("position", "normal", "occlusion"):
        scenes.assert_bit_equal(exp[k], single[k], k)
    scenes.assert_bit_equal(exp["combined"], single["direct"], "combined = mean of clamp(D_0,s) = mean of D_0,s")
    assert np.array_equal(exp["table"], single["table"]) and np.array_equal(exp["live"], single["live"])
    LM.assert_bake_constants(exp, 0)


# ---- (b) recomposition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CASES))
def test_combined_recomposes_the_beauty_frame(name):
    key = X.lights_key(X.CASES[name])
    sd, cfg, exp = LM.skin_expectation(POSE0, key, ao_samples=4)
    assert LM.counts(exp, X.CASES[name]) == COUNTS[name]
    LM.assert_exercised(exp, X.CASES[name], 50, 25, name)
    LM.assert_constants(exp, len(X.CASES[name]))
    hit = exp["hit"]
    plain = X.skin_expectation(POSE0, key, bounces=0)[2]
    scenes.assert_bit_equal(exp["combined"][hit], plain[hit], f"{name}: combined vs the beauty frame")
    with_ao = X.skin_expectation(POSE0, key, bounces=0, ao=True)
    intensity = with_ao[1].aoIntensity
    assert (exp["occlusion"][hit] < 1).sum() >= 100
    scenes.assert_bit_equal(LC.recompose(exp["combined"], exp["occlusion"], intensity)[hit], with_ao[2][hit], f"{name}: recomposition with AO")


# ---- (c) the wrong readings ----------------------------------------------------------------------------------------------------
# variant -> (case, the plane it must show in, the light index of a per-light plane or None)
CAUGHT_ON = {
    "seed_per_light": ("three", "visibility", 3),
    "ambient_per_light": ("fill_left+kicker", "direct", 1),
    "no_light_clamp": ("bright_front+negative", "combined", None),
    "reverse_order": ("three", "combined", None),
}


@pytest.mark.parametrize("variant", list(CAUGHT_ON))
def test_wrong_variants_are_each_caught(variant):
    case, plane, k = CAUGHT_ON[variant]
    key = X.lights_key(X.CASES[case])
    want = LM.skin_expectation(POSE0, key)[2]
    wrong = LM.skin_expectation(POSE0, key, variant=variant)[2]
    a, b = (want[plane], wrong[plane]) if k is None else (want[plane][k], wrong[plane][k])
    assert _differing(a, b) >= 25, variant


def test_every_wrong_variant_is_accounted_for():
    assert set(LM.WRONG_VARIANTS) == set(CAUGHT_ON) | {"raw_normal_hard", "clamp_of_means"}


def test_per_light_clamp_shows_in_combined_only_through_its_lower_bound():
    key = X.lights_key(X.CASES["bright_front"])
    want, wrong = LM.skin_expectation(POSE0, key)[2], LM.skin_expectation(POSE0, key, variant="no_light_clamp")[2]
    assert _differing(want["direct"][1], wrong["direct"][1]) >= 100  # the bright light's own plane is clamped at 1
    assert _differing(want["combined"], wrong["combined"]) == 0  # ... and the sum cannot tell


def test_raw_normal_in_hard_mode_cannot_show(oracle):
    key = X.lights_key(X.CASES["three"])
    name = "pose5_orbit_64x64_t16"  # a posed figure: rotated normals
    sd, cfg, want = LM.skin_expectation(name, key, soft=False)
    hits = oracle.intersect(sd.ptr, L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height))
    n = hits["normal"][hits["hit"] != 0].astype(np.float64)
    assert len(n) > 500 and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 2.5e-7
    wrong = LM.skin_expectation(name, key, soft=False, variant="raw_normal_hard")[2]
    for k in abi.LIGHT_MULTI_NAMES:
        assert _differing(want[k], wrong[k]) == 0, k


def test_clamp_of_means_shows_in_a_bake_with_sub_samples_only():
    key = X.lights_key(X.CASES["bright_front"])
    one = LM.bake_skin_expectation("S64", 0, 1, key)[2]
    scenes.assert_bit_equal(LM.bake_skin_expectation("S64", 0, 1, key, variant="clamp_of_means")[2]["combined"], one["combined"], "grid 1: one sub-sample")
    want = LM.bake_skin_expectation("S64", 0, 2, key)[2]
    wrong = LM.bake_skin_expectation("S64", 0, 2, key, variant="clamp_of_means")[2]
    assert _differing(want["combined"], wrong["combined"]) >= 25
    for k in ("visibility", "direct", "occlusion"):
        assert _differing(want[k], wrong[k]) == 0, k
    # a frame has no sub-samples: the reading is not defined there and the checker ignores it
    lk = X.lights_key(X.CASES["bright_front"])
    assert _differing(LM.skin_expectation(POSE0, lk)[2]["combined"], LM.skin_expectation(POSE0, lk, variant="clamp_of_means")[2]["combined"]) == 0


def test_the_other_variants_show_in_a_bake_too():
    key = X.lights_key(X.CASES["three"])
    want = LM.bake_skin_expectation("S64", 0, 1, key)[2]
    LM.assert_bake_exercised(want, X.CASES["three"], 50, 25, "S64 grid 1")
    for variant, plane, k in (("seed_per_light", "visibility", 3), ("ambient_per_light", "direct", 1), ("reverse_order", "combined", None)):
        wrong = LM.bake_skin_expectation("S64", 0, 1, key, variant=variant)[2]
        a, b = (want[plane], wrong[plane]) if k is None else (want[plane][k], wrong[plane][k])
        assert _differing(a, b) >= 25, variant
