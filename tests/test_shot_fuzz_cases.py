"""The CPU twin of tests/test_gpu_shot_fuzz.py: what the blocks of tests/shot_fuzz_cases.py hold, pinned, so that the GPU blocks
cannot be hollow — no device here.

Per block of 8 blend cases: the same seed gives the same case; the census is the pinned one — pixels per class of every quantity,
the classes of s, k, fade and the page, all 16 combinations of the kernel's four alignment flags, every optional input absent and
each output alone, one frame and several, and the pixels at which the arithmetic is at an edge (dR == fade, a quotient that
overflows, a denormal intermediate, a channel on a quantiser boundary, a clamp whose upper bound acts); no expectation holds a
NaN or an infinity; shot_checker.compose equals, bit for bit, the restatement that clamps with sclamp's comparisons on every pixel
and the Python-float restatement on every pixel of every case's first run; and each of ten deliberately wrong blends differs from compose
somewhere in the block — otherwise the block could not catch that defect on the device.

Per block of 4 whole shots: the oracle's totals of shot_checker.classes, pinned and above the floors; every skip form and page
mode; no NaN."""
import numpy as np
import pytest

import scenes
import shot_checker as S
import shot_fuzz_cases as SF

f32 = np.float32
BLEND_FIRSTS, SHOT_FIRSTS = list(SF.BLEND_BLOCKS), list(SF.SHOT_BLOCKS)
_BLOCKS = {}


def _block(first):
    if first not in _BLOCKS:
        _BLOCKS[first] = SF.blend_block(first)
    return _BLOCKS[first]


def _bits_differ(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_the_same_seed_gives_the_same_blend_case(first):
    digests = [SF.case_digest(c)[:16] for c in SF.blend_block(first)]
    assert digests == [SF.case_digest(c)[:16] for c in _block(first)] and len(set(digests)) == SF.BLEND_BLOCK
    assert digests == SF.BLEND_DIGESTS[first]
    for case in _block(first):
        px = case["w"] * case["h"]
        assert 1 <= case["w"] <= 70 and 1 <= case["h"] <= 40 and 1 <= case["n"] <= 6
        assert px <= case["in_stride"] <= px + 7 and px <= case["out_stride"] <= px + 7
        for run in case["runs"]:
            assert all(0 <= v <= 3 for v in run["leads"].values())
            assert "distance" not in run["absent"] or run["shot"].reflectionFade == 0  # the header allows it only there


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_the_blend_blocks_census(first):
    c = SF.blend_census(_block(first))
    print(first, c)
    assert c == SF.BLEND_BLOCKS[first]
    # what the pin must hold, so that a new pin cannot quietly lose it
    for q, names in SF.QUANTITIES.items():
        assert all(c["classes"][q][name] > 0 for name in names), q
    assert c["alignment_combinations"] == list(range(16))
    assert set(c["absent"]) == {"visibility", "reflection", "distance"} and all(c["outputs"].get(k, 0) >= 1 for k in ("f32", "u8", "both"))
    assert c["frames"]["one"] >= 1 and c["frames"]["several"] >= 1
    assert set(c["s"]) == set(SF.STRENGTH) and set(c["k"]) == set(SF.STRENGTH) and set(c["fade"]) == set(SF.FADE)
    assert set(c["pages"]) == set(SF.PAGES)
    assert all(v >= 1 for v in c["edges"].values()), c["edges"]


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_no_expectation_holds_a_nan_or_an_infinity(first):
    for case in _block(first):
        for k in ("F", "vis", "R", "dR"):
            assert not np.isnan(case[k]).any()
        for r, run in enumerate(case["runs"]):
            out = SF.expected_run(case, run)
            assert np.isfinite(out).all(), (case["seed"], r)
            assert (out[..., 3] == 1).all()


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_compose_clamps_like_sclamp(first):
    """Every pixel of every run: compose (numpy's minimum / maximum) against the restatement with sclamp's comparisons, and
    shot_checker.quantize against the quantiser with them.  The sign of a zero is where they could part."""
    for case in _block(first):
        for r, run in enumerate(case["runs"]):
            F, vis, R, dR, shot = SF.run_inputs(case, run)
            out = SF.expected_run(case, run)
            scenes.assert_bit_equal(out, SF.blend(F, vis, R, dR, SF.page_planes(case), shot), f"case {case['seed']} run {r}")
            assert np.array_equal(S.quantize(out), SF.quantize(out)), (case["seed"], r)
        if case["page"].startswith("gradient"):
            scenes.assert_bit_equal(SF.gradient_page(case["cfg"]), S.gradient_plane(case["cfg"]), f"case {case['seed']}: the page")


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_compose_equals_the_scalar_restatement_on_every_pixel_of_the_block(first):
    """Every pixel of run 0 of each case (every plane present): Python floats, one rounding per operation, sclamp's comparisons."""
    compared = 0
    for case in _block(first):
        F, vis, R, dR, shot = SF.run_inputs(case, case["runs"][0])
        page = SF.page_planes(case)
        out = SF.expected_run(case, case["runs"][0]).reshape(-1, 4)
        s, k, fade = (float(f32(v)) for v in (shot.shadowStrength, shot.reflectivity, shot.reflectionFade))
        total = out.shape[0]
        Ff, Rf, pf, vf, df = F.reshape(-1, 4), R.reshape(-1, 4), page.reshape(-1, 3), vis.reshape(-1), dR.reshape(-1)
        for i in range(total):
            want = SF.scalar_pixel([float(x) for x in Ff[i]], float(vf[i]), [float(x) for x in Rf[i]], float(df[i]), [float(x) for x in pf[i]], s, k, fade)
            scenes.assert_bit_equal(out[i], np.asarray(want, f32), f"case {case['seed']} pixel {i}")
            compared += 1
    assert compared == SF.BLEND_BLOCKS[first]["pixels"]


def test_the_page_is_the_oracles_background(mcrt, oracle):
    """The pages of one block's reference cases against oracle.background, pixel by pixel."""
    for case in _block(BLEND_FIRSTS[0]):
        if case["page"] == "color":
            continue
        want = SF.page_planes(case)
        for i in range(min(case["n"], 3)):
            sd = mcrt.MeshBuilder.buildDefaultScene()
            for c in range(4):
                sd.desc.background_color[c] = case["backgrounds"][i % 3][c]
            scenes.assert_bit_equal(S.page_plane(oracle, sd, case["cfg"], case["shot"]), want[i], f"case {case['seed']} frame {i}")


@pytest.mark.parametrize("mutation", list(SF.MUTATIONS))
@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_a_wrong_blend_differs_somewhere_in_the_block(first, mutation):
    pixels = 0
    for case in _block(first):
        for run in case["runs"]:
            out = SF.expected_run(case, run)
            if mutation in SF.FLOAT_MUTATIONS:
                if run["outputs"] != "u8":  # a run that writes floats
                    pixels += int(_bits_differ(out, SF.expected_run(case, run, mutation)).sum())
            elif run["outputs"] != "f32":
                pixels += int((SF.quantize(out) != SF.quantize(out, mutation)).any(axis=-1).sum())
    print(f"block {first}: {SF.MUTATIONS[mutation]}: {pixels} pixels differ")
    assert pixels >= 1, SF.MUTATIONS[mutation]


def test_the_unmutated_restatement_is_not_a_mutation():
    case = _block(BLEND_FIRSTS[0])[4]
    run = case["runs"][0]
    F, vis, R, dR, shot = SF.run_inputs(case, run)
    scenes.assert_bit_equal(SF.blend(F, vis, R, dR, SF.page_planes(case), shot, mutation=None), S.compose(F, vis, R, dR, SF.page_planes(case), shot), "blend")


def test_make_planes_without_a_place_draws_from_the_same_classes():
    """What the stride test of the GPU suite draws: vectorised, any two to four classes per plane, NaN-free."""
    g = np.random.default_rng(3)
    p = SF.make_planes(g, 1, 37, 53, 24.0)
    assert p["F"].shape == (1, 37, 53, 4) and p["dR"].dtype == f32
    for q in SF.QUANTITIES:
        assert 2 <= len(np.unique(p["classes"][q])) <= 4
    out = S.compose(p["F"], p["vis"], p["R"], p["dR"], np.asarray((0.5, 0.25, 1.0), f32), S.SHOT)
    assert np.isfinite(out).all()


# ---- whole shots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", SHOT_FIRSTS)
def test_the_shot_blocks_census(oracle, first):
    cases, exps, c = SF.shot_block_expectations(oracle, first)
    print(first, c)
    assert c == SF.SHOT_BLOCKS[first]
    assert all(got >= floor for got, floor in zip(c["classes"], SF.FLOORS)), c["classes"]  # the oracle alone: no block is hollow
    assert set(c["skips"]) == set(SF.SKIPS) and set(c["pages"]) == set(SF.SHOT_PAGES)
    for case, per_call in zip(cases, exps):
        assert 1 <= len(case["scenes"]) <= 4 and case["cfg"].width <= 48 and case["cfg"].height <= 40 and case["cfg"].samplesPerPixel <= 2
        assert 0 <= case["cfg"].maxBounces <= 8 and 1 <= case["cfg"].shadowSamples <= 113
        for call, per_scene in zip(case["calls"], per_call):
            assert (call["shot"].shadowStrength == 0) == (call["skip"] in ("s = 0", "s = k = 0"))
            assert (call["shot"].reflectivity == 0) == (call["skip"] in ("k = 0", "s = k = 0"))
            assert len(SF.refusals(case, call)) == (0 if call["deep"] is None else 3 if "shadowSamples" in call["deep"] else 2)
            for exp in per_scene:
                assert np.isfinite(exp["out"]).all() and (exp["rgba8"][..., 3] == 255).all()


def test_the_oracle_holds_every_shot_cases_census(oracle):
    """What a GPU test of one case asserts before it touches the device."""
    assert list(SF.SHOT_CASES) == [first + k for first in SHOT_FIRSTS for k in range(SF.SHOT_BLOCK)]
    for first in SHOT_FIRSTS:
        cases, exps, _ = SF.shot_block_expectations(oracle, first)
        for case, per_call in zip(cases, exps):
            assert SF.shot_case_digest(case, per_call) == SF.SHOT_CASES[case["seed"]], case["seed"]


def test_the_same_seed_gives_the_same_shot_case():
    for seed in range(SHOT_FIRSTS[0], SHOT_FIRSTS[0] + SF.SHOT_BLOCK):
        assert SF.case_digest(SF.make_shot_case(seed)) == SF.case_digest(SF.make_shot_case(seed))
    assert len({SF.case_digest(SF.make_shot_case(s)) for s in range(8)}) == 8


def test_the_launch_limits_are_read_from_the_source():
    assert SF.layers_grid() * SF.block_lanes() == 2097152 and SF.layers_batch_max_frames() == 4096 and SF.batch_max_frames() == 256
