"""The CPU twin of tests/test_gpu_cutout_fuzz.py: what the blocks of tests/cutout_fuzz_cases.py hold, pinned, so that the GPU blocks
cannot be hollow — no device here.

Per block of 8 blend cases: the same seed gives the same case; the census is the pinned one and meets the conditions a pin must
not lose — every class of all seven quantities, of s, k, fade, o, C and the page, all 16 alignment combinations, every optional
input absent and each output alone, runs with and without bounds, each of the blend's three branches on at least 2 % of the
transparent cases' pixels, 50 pixels whose out.a is a positive denormal, a frame whose box a denormal alpha alone decides; no
expectation holds a NaN or an infinity; cutout_checker.compose_ex equals, bit for bit, the restatement with sclamp's comparisons on
every pixel of every run and the Python-float restatement on every pixel of every case's first run; and each of the deliberately
wrong blends and boxes differs from compose_ex / bounds_of somewhere in the block — otherwise the block could not catch that
defect on the device.

Per block of 4 whole cut-outs: the oracle's totals of cutout_checker.classes, pinned and above the floors; every form, page and
kind; and the header's "over any page": the cut-out over the page against the opaque shot of the same settings."""
import numpy as np
import pytest

import cutout_checker as X
import cutout_fuzz_cases as CF
import scenes
import shot_fuzz_cases as SF

f32 = np.float32
BLEND_FIRSTS, SHOT_FIRSTS = list(CF.BLEND_BLOCKS), list(CF.SHOT_BLOCKS)
BOUND = 16 * 2.0 ** -24
_BLOCKS = {}


def _block(first):
    if first not in _BLOCKS:
        _BLOCKS[first] = CF.blend_block(first)
    return _BLOCKS[first]


def _bits_differ(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=-1)


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_the_same_seed_gives_the_same_blend_case(first):
    digests = [CF.case_digest(c)[:16] for c in CF.blend_block(first)]
    assert digests == [CF.case_digest(c)[:16] for c in _block(first)] and len(set(digests)) == CF.BLEND_BLOCK
    assert digests == CF.BLEND_DIGESTS[first]
    for case in _block(first):
        px = case["w"] * case["h"]
        assert 1 <= case["w"] <= 70 and 1 <= case["h"] <= 40 and 1 <= case["n"] <= 6
        assert px <= case["in_stride"] <= px + 7 and px <= case["out_stride"] <= px + 7
        for run in case["runs"]:
            shot = run["shot"]
            assert all(0 <= v <= 3 for v in run["leads"].values())
            assert "distance" not in run["absent"] or shot.reflectionFade == 0  # the header allows it only there
            assert not run["bounds"] or shot.page == "transparent"  # and the boxes only here
            assert 0 <= shot.floorOcclusion <= 1 and np.isfinite(shot.shadowColor).all()
            if case["page_class"] == "opaque, black shadow, o > 0":  # the shot that takes the _occ entry
                assert not shot.needs_ex() and shot.floorOcclusion > 0
            elif case["page_class"] != "transparent":
                assert shot.page != "transparent" and any(c != 0 for c in shot.shadowColor)


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_the_blend_blocks_census(first):
    c = CF.blend_census(_block(first))
    print(first, c)
    assert c == CF.BLEND_BLOCKS[first]
    # what the pin must hold, so that a new pin cannot quietly lose it
    for q, names in CF.QUANTITIES.items():
        assert all(c["classes"][q][name] > 0 for name in names), q
    assert c["alignment_combinations"] == list(range(16))
    assert set(c["absent"]) == {"visibility", "reflection", "distance", "occlusion"} and all(c["outputs"].get(k, 0) >= 1 for k in ("f32", "u8", "both"))
    assert c["frames"]["one"] >= 1 and c["frames"]["several"] >= 1 and c["bounds"]["with"] >= 5 and c["bounds"]["without"] >= 5
    assert set(c["s"]) == set(SF.STRENGTH) and set(c["k"]) == set(SF.STRENGTH) and set(c["fade"]) == set(SF.FADE)
    assert set(c["o"]) == set(CF.OCCLUSION) and set(c["C"]) == set(CF.COLOUR)
    assert set(c["pages"]) == set(CF.PAGES) and c["pages"]["transparent"] >= 5
    assert sum(c["branches"].values()) == c["cutout_pixels"]
    # 2 % each, of the pixels that reach the three branches at all: the transparent cases' (the shares then add up to 100 %)
    assert all(50 * c["branches"][b] >= c["cutout_pixels"] for b in CF.BRANCHES), c["branches"]
    assert c["edges"]["a denormal positive out.a"] >= 50 and c["boxes"]["set by a denormal alpha alone"] >= 1
    assert all(v >= 1 for v in c["edges"].values()), c["edges"]


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_no_expectation_holds_a_nan_or_an_infinity(first):
    for case in _block(first):
        for k in ("F", "vis", "R", "dR", "occ"):
            assert not np.isnan(case[k]).any()
        for r, run in enumerate(case["runs"]):
            out = CF.expected_run(case, run)
            assert np.isfinite(out).all(), (case["seed"], r)
            assert case["page_class"] == "transparent" or (out[..., 3] == 1).all()


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_compose_ex_clamps_and_branches_like_the_restatement(first):
    """Every pixel of every run, all four channels: compose_ex (numpy's minimum / maximum) against the restatement with sclamp's
    comparisons; cutout_checker.quantize against the quantiser with them."""
    for case in _block(first):
        for r, run in enumerate(case["runs"]):
            F, vis, R, dR, occ, shot = CF.run_inputs(case, run)
            out = CF.expected_run(case, run)
            scenes.assert_bit_equal(out, CF.blend_ex(F, vis, R, dR, occ, CF.page_planes(case), shot), f"case {case['seed']} run {r}")
            assert np.array_equal(X.quantize(out), SF.quantize(out)), (case["seed"], r)
            if run["bounds"]:
                assert np.array_equal(CF.expected_boxes(case, run), CF.box(out))


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_compose_ex_equals_the_scalar_restatement_on_every_pixel_of_the_block(first):
    """Every pixel of run 0 of each case (every plane present): Python floats, one rounding per operation."""
    compared = 0
    for case in _block(first):
        F, vis, R, dR, occ, shot = CF.run_inputs(case, case["runs"][0])
        cutout = shot.page == "transparent"
        page = np.zeros(F.shape[:-1] + (3,), f32) if cutout else CF.page_planes(case)
        out = CF.expected_run(case, case["runs"][0]).reshape(-1, 4)
        s, k, fade, o = (float(f32(v)) for v in (shot.shadowStrength, shot.reflectivity, shot.reflectionFade, shot.floorOcclusion))
        C = [float(f32(c)) for c in shot.shadowColor]
        Ff, Rf, pf, vf, df, of = F.reshape(-1, 4), R.reshape(-1, 4), page.reshape(-1, 3), vis.reshape(-1), dR.reshape(-1), occ.reshape(-1)
        for i in range(out.shape[0]):
            want = CF.scalar_pixel_ex([float(x) for x in Ff[i]], float(vf[i]), [float(x) for x in Rf[i]], float(df[i]), float(of[i]),
                                      [float(x) for x in pf[i]], s, k, fade, o, C, cutout)
            scenes.assert_bit_equal(out[i], np.asarray(want, f32), f"case {case['seed']} pixel {i}")
            compared += 1
    assert compared == CF.BLEND_BLOCKS[first]["pixels"]


@pytest.mark.parametrize("mutation", list(CF.MUTATIONS) + list(CF.BOX_MUTATIONS))
@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_a_wrong_model_differs_somewhere_in_the_block(first, mutation):
    """The hollowing check: were the device to compute one of these, the block's comparison would report it."""
    found = 0
    for case in _block(first):
        for run in case["runs"]:
            if mutation in CF.BOX_MUTATIONS:
                if run["bounds"]:
                    found += int((CF.expected_boxes(case, run) != CF.expected_boxes(case, run, mutation)).any(axis=-1).sum())
            elif run["outputs"] != "u8":  # a run that writes floats
                found += int(_bits_differ(CF.expected_run(case, run), CF.expected_run(case, run, mutation)).sum())
    what = {**CF.MUTATIONS, **CF.BOX_MUTATIONS}[mutation]
    print(f"block {first}: {what}: {found} {'frames' if mutation in CF.BOX_MUTATIONS else 'pixels'} differ")
    assert found >= 1, what


def _unit(a):
    return ((a >= 0) & (a <= 1)).reshape(a.shape[:3] + (-1,)).all(axis=-1)


@pytest.mark.parametrize("first", BLEND_FIRSTS)
def test_the_blend_cases_over_their_page_are_the_opaque_shot(first):
    """The header's "over any page" at the value classes: every run of the block's transparent cases, composited in float64
    over the case's page colour (cutout_checker.over), against the opaque blend of the same planes and settings — within
    16 * 2^-24 on the pixels whose inputs (F, vis, R, occ and C) all lie in [0, 1], in the channels whose page value does; the
    distance is any."""
    compared, worst = 0, 0.0
    for case in _block(first):
        if case["page_class"] != "transparent":
            continue
        for run in case["runs"]:
            F, vis, R, dR, occ, shot = CF.run_inputs(case, run)
            pg = np.asarray(shot.pageColor, f32)
            inside = _unit(F) & _unit(case["vis"]) & _unit(case["R"]) & _unit(case["occ"])
            channels = (pg >= 0) & (pg <= 1)
            if not (channels.any() and all(0 <= c <= 1 for c in shot.shadowColor)):
                continue
            cut = CF.expected_run(case, run)
            opaque = X.compose_ex(F, vis, R, dR, occ, pg, CF.with_shot(shot, page="color"))
            diff = np.abs(X.over(cut, pg) - opaque[..., :3])[..., channels][inside]
            compared += int(inside.sum())
            worst = max(worst, float(diff.max()) if diff.size else 0.0)
    print(f"block {first}: {compared} pixels compared, largest difference {worst / 2.0 ** -24:.2f} * 2^-24")
    assert compared > 0 and worst <= BOUND, (compared, worst / 2.0 ** -24)


def test_the_unmutated_restatements_are_no_mutations():
    case = _block(BLEND_FIRSTS[0])[4]
    for run in case["runs"]:
        scenes.assert_bit_equal(CF.expected_run(case, run, mutation="none of them"), CF.expected_run(case, run), "blend_ex")
        assert np.array_equal(CF.box(CF.expected_run(case, run), "none of them"), CF.box(CF.expected_run(case, run)))


def test_the_slim_layout_leaves_the_other_kinds_alone():
    """resident_fuzz_cases.layout's third key: the slim model's pool, from slim_checker's tables; make_skin draws a 64 x 64 skin
    with it.  (The pinned digests of tests/test_resident_fuzz_cases.py hold the two other kinds where they were.)"""
    import resident_fuzz_cases as RF
    import slim_checker as SL

    lay = RF.layout("slim")
    assert len(lay["pool"]) == SL.N_TEXELS["slim"] == 3136 and set(lay["mesh"].tolist()) == set(range(12)) and set(lay["face"].tolist()) == set(range(6))
    assert len(np.unique(lay["pool"])) == len(lay["pool"])  # a 64 x 64 skin: no two texels share a pixel
    skin = RF.make_skin(np.random.default_rng(5), "slim")
    assert skin.shape == (64, 64, 4) and skin.dtype == np.uint8


# ---- whole cut-outs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", SHOT_FIRSTS)
def test_the_shot_blocks_census(oracle, first):
    cases, exps, c = CF.shot_block_expectations(oracle, first)
    print(first, c)
    assert c == CF.SHOT_BLOCKS[first]
    assert all(got >= floor for got, floor in zip(c["classes"], CF.FLOORS)), c["classes"]  # the oracle alone: no block is hollow
    assert set(c["forms"]) == set(CF.FORMS) and set(c["pages"]) == set(CF.CALL_PAGES) and c["kinds"].get("slim", 0) >= 1
    assert c["floor occlusion"] == {"o = 0": 4, "o > 0": 4} and c["skips"].get("s = k = 0", 0) >= 1
    for case, per_call in zip(cases, exps):
        cfg = case["cfg"]
        assert 1 <= len(case["scenes"]) <= 4 and cfg.width <= 48 and cfg.height <= 40
        assert 0 <= cfg.maxBounces <= 8 and 1 <= cfg.shadowSamples <= 113 and 1 <= cfg.aoSamples <= 8 and 1 <= cfg.aoRadius <= 4
        assert (case["calls"][0]["o"] > 0) != (case["calls"][1]["o"] > 0)
        for call, per_scene in zip(case["calls"], per_call):
            shot = call["shot"]
            assert shot.needs_ex() and (shot.page == "transparent") == (call["page"] == "transparent")
            assert call["form"] not in ("png crop", "farm") or shot.page == "transparent"
            assert len(CF.refusals(case, call)) == (3 if call["deep"] is None else 6)
            for exp in per_scene:
                assert np.isfinite(exp["out"]).all()
                if call["deep"] is not None:  # s = k = o = 0: the transparent render itself
                    assert (shot.shadowStrength, shot.reflectivity, shot.floorOcclusion) == (0, 0, 0)
                    assert exp["out"].tobytes() == exp["F"].tobytes()


def test_the_oracle_holds_every_shot_cases_census(oracle):
    """What a GPU test of one case asserts before it touches the device."""
    assert list(CF.SHOT_CASES) == [first + k for first in SHOT_FIRSTS for k in range(CF.SHOT_BLOCK)]
    for first in SHOT_FIRSTS:
        cases, exps, _ = CF.shot_block_expectations(oracle, first)
        for case, per_call in zip(cases, exps):
            assert CF.shot_case_digest(case, per_call) == CF.SHOT_CASES[case["seed"]], case["seed"]


def test_the_same_seed_gives_the_same_shot_case():
    for seed in range(SHOT_FIRSTS[0], SHOT_FIRSTS[0] + CF.SHOT_BLOCK):
        assert SF.case_digest(CF.make_shot_case(seed)) == SF.case_digest(CF.make_shot_case(seed))
    assert len({SF.case_digest(CF.make_shot_case(s)) for s in range(8)}) == 8


@pytest.mark.parametrize("first", SHOT_FIRSTS)
def test_the_cutout_over_a_page_is_the_opaque_shot(oracle, first):
    """The header's "over any page", on the oracle's planes: every call of the block on the transparent page, composited in
    float64 over a page (the call's own page colour), against the opaque blend of the same planes and settings — within
    16 * 2^-24 on the pixels whose inputs all lie in [0, 1] (the oracle's planes do; the count says how many were compared)."""
    cases, exps, _ = CF.shot_block_expectations(oracle, first)
    compared, worst = 0, 0.0
    for case, per_call in zip(cases, exps):
        for call, per_scene in zip(case["calls"], per_call):
            shot = call["shot"]
            pg = np.asarray(shot.pageColor, f32)
            for exp in per_scene:
                planes = (exp["F"], exp["vis"], exp["R"], exp["dR"], exp["occ"])
                inside = np.ones(exp["vis"].shape, bool)
                for a in (exp["F"], exp["vis"][..., None], exp["R"], exp["occ"][..., None]):
                    inside &= ((a >= 0) & (a <= 1)).all(axis=-1)
                cut = X.compose_ex(*planes, None, CF.with_shot(shot, page="transparent"))
                opaque = X.compose_ex(*planes, pg, CF.with_shot(shot, page="color"))
                diff = np.abs(X.over(cut, pg) - opaque[..., :3])[inside]
                compared += int(inside.sum())
                worst = max(worst, float(diff.max()) if diff.size else 0.0)
    print(f"block {first}: {compared} pixels compared, largest difference {worst / 2.0 ** -24:.2f} * 2^-24")
    assert compared > 0 and worst <= BOUND, (compared, worst / 2.0 ** -24)


def test_the_shared_grids_constants_are_read_from_the_source():
    assert CF.bounds_groups() == 2048 and SF.block_lanes() == 256
