"""The generators of tests/pass_fuzz_cases.py alone, on the CPU: they are deterministic, the oracle holds over each fixed block
what pass_fuzz_cases.BLOCKS says (so that the GPU tests of tests/test_gpu_pass_fuzz.py compare frames that hold shadow, penumbra,
mirror images and hits, not constants), every expectation obeys its miss constants, and the plane of group A moves with the
scene: f = 0 is mcrt_scene_floor."""
import numpy as np
import pytest

import pass_fuzz_cases as PF


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("group", list(PF.GROUPS))
def test_cases_are_deterministic(mcrt, group):
    first = {"bundle": 7000, "wide": 9000, "bundle-lifted": 7000, "wide-lifted": 9000, "long-shadow": 12000, "far-plane": 15000}[group]
    texts = set()
    for seed in range(first, first + 6):
        (sd, cfg, g, what), (sd2, cfg2, g2, what2) = PF.GROUPS[group](seed), PF.GROUPS[group](seed)
        assert what == what2 and g == g2 and np.isfinite(np.float32(g)) and float(np.float32(g)) == g
        assert bytes(cfg.to_c()) == bytes(cfg2.to_c())
        assert _same(sd.to_numpy(), sd2.to_numpy())
        texts.add(what)
    assert len(texts) == 6


@pytest.mark.parametrize("wide", [False, True])
def test_the_plane_of_group_a_moves_with_the_scene(mcrt, wide):
    floors = 0
    for seed in range(9000 if wide else 7000, (9000 if wide else 7000) + 48):
        sd, cfg, g, what = PF.make_pass_case(seed, wide)
        lo, hi = PF.y_range(sd)
        assert mcrt.scene_floor(sd) == lo, what
        assert cfg.maxBounces >= 1 and 17 <= cfg.width < 57 and 13 <= cfg.height < 41
        assert g in [float(np.float32(lo + c * (hi - lo))) for c in (0.0, -0.02, -0.5, 0.15, 0.4, 1.1)], what
        if g == lo:
            floors += 1
        lifted = PF.make_pass_case(seed, wide, lift_light=True)
        assert lifted[2] == g and bytes(lifted[1].to_c()) == bytes(cfg.to_c())
        a, b = sd.to_numpy(), lifted[0].to_numpy()
        assert b["light_position"][1] >= a["light_position"][1] and b["light_position"][1] > hi
        b["light_position"][1] = a["light_position"][1]
        assert _same(a, b)  # nothing but the light's height differs
    assert floors >= 8


def test_long_shadow_lights_are_below_the_figures_top(mcrt):
    for seed in range(12000, 12048):
        sd, cfg, g, what = PF.make_long_shadow_case(seed)
        s = sd.to_numpy()
        assert s["light_position"][1] < PF.y_range(sd)[1] and g <= 0.0, what
        assert not PF.light_clear_above_every_mesh(sd, cfg, g)
        out = float(np.hypot(s["camera_target"][0], s["camera_target"][2]))
        assert 10 ** 2.29 < out < 10 ** 4.51


def test_far_planes_lie_ten_to_ten_thousand_heights_down(mcrt):
    for seed in range(15000, 15048):
        sd, cfg, g, what = PF.make_far_plane_case(seed)
        lo, hi = PF.y_range(sd)
        s = sd.to_numpy()
        assert 9.99 * (hi - lo) < lo - g < 10001 * (hi - lo), what
        assert s["light_position"][1] > hi and s["camera_position"][1] > hi and s["camera_target"][1] < lo
        assert PF.mask_slack(s) < 0.05  # a scene at scale 1: the plane's height is no part of the magnitude


@pytest.mark.parametrize("block", list(PF.BLOCKS), ids=PF.BLOCK_IDS)
def test_the_oracle_holds_the_blocks_totals(oracle, block):
    PF.check_ground_block(oracle, *block)
    PF.check_reflection_block(oracle, *block)
    if block in PF.A_BLOCKS:
        PF.check_surface_block(oracle, *block)
        PF.check_lifted_block(oracle, *block)


@pytest.mark.parametrize("name", ["outer_back_face", "null_and_empty", "posed", "pose6_orbit_96x64"])
def test_the_id_check_accepts_the_decoded_ids_and_no_others(oracle, name):
    """layers_checker.assert_ids_name_the_surfaces — ids checked against the albedo, for textures that repeat colours — on
    scenes whose texels all differ, where expected_layers decodes the ids from the colours: it accepts those ids, and neither
    a neighbouring texel, another face, a flipped flag nor another mesh."""
    import layers_checker as L
    from minecraftskin_raytracer_amd import abi

    sd, cfg, exp = L.box_expectation(name) if name in L.BOX_CASES else L.skin_expectation(name)
    surf = L.expected_surfaces(oracle, sd, cfg.width, cfg.height)
    scene_np = sd.to_numpy()
    for k in ("depth", "normal", "albedo", "point", "hit"):
        assert np.array_equal(surf[k], exp[k])
    L.assert_ids_name_the_surfaces(exp["id"], surf, scene_np, name)
    y, x = np.argwhere(exp["hit"] & (exp["id"][..., 2] >= 0))[0]
    for field, change in ((0, 1), (1, 1), (1, abi.ID_BACK), (1, abi.ID_OUTER), (2, 1), (3, 1)):
        ids = exp["id"].copy()
        ids[y, x, field] = ids[y, x, field] ^ change
        with pytest.raises(AssertionError):
            L.assert_ids_name_the_surfaces(ids, surf, scene_np, name)
    ids = exp["id"].copy()
    ids[~exp["hit"]] = (0, 0, 0, 0)
    if not exp["hit"].all():
        with pytest.raises(AssertionError):
            L.assert_ids_name_the_surfaces(ids, surf, scene_np, name)
