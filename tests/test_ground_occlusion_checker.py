"""The ground-occlusion checker (tests/ground_occlusion_checker.py) on the CPU: it catches deliberately wrong passes, its
expectations hold the conditions the GPU tests rely on, and its blend is shot_checker's where the term is absent."""
import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import ground_checker as G
import ground_occlusion_checker as GO
import layers_checker as L
import scenes
import shot_checker as S

f32 = np.float32
CASE = "pose5_orbit_64x64_t16"

# each a pass with ONE mistake (the keyword arguments of expected_ground_occlusion)
MISTAKES = {
    "seed_summed_right_to_left": dict(right_to_left=True),
    "the_shadow_seed_constants": dict(constants=GO.SHADOW_SEED),
    "origin_on_the_plane": dict(on_plane=True),
    "normal_pointing_down": dict(normal=(0.0, -1.0, 0.0)),
    "radius_one_ulp_larger": dict(radius_scale=float(f32(1.0) + f32(2.0 ** -23))),
    "one_sample_more": dict(extra_samples=1),
    "not_reached_is_zero": dict(not_reached=0.0),
}


@pytest.fixture(scope="module")
def truth(mcrt):
    return GO.skin_expectation(CASE)


# Where each mistake is asked.  The issue names one case for all seven: CASE at ground_y = 0, 8 samples, radius 3.  Four of them
# change the expectation there.  Three cannot, for reasons that lie in the reference and not in any pass, so each is asked on
# the nearest case that can show it, and the reason is asserted beside it:
#   seed_summed_right_to_left   at ground_y = 0 the middle term P.y * 19349663 is +0, and x + (0 + z) is (x + 0) + z bit for
#                               bit: 0 of 4096 pixels differ.  Asked at ground_y = -0.5 (75 pixels differ).
#   origin_on_the_plane         0 of 4096 pixels of CASE differ at ground_y = 0 (measured with the oracle).  Asked on
#                               pose6_orbit_96x64 at ground_y = 0 (41 pixels differ).
#   radius_one_ulp_larger       computeAO counts a sample iff t < radius: an ulp matters only to a sample whose t lies in
#                               [radius, radius + 2.4e-7), and none of the 207 * 8 rays of CASE at radius 3 does (nor of any
#                               other skin case at ground_y 0, -0.5, 0.25, 6).  Asked on CASE at ground_y = 0 with the radius ON
#                               such a step, found by bisection over float32 (the largest radius below 3 at which one pixel's
#                               count has not yet grown).
ELSEWHERE = {"seed_summed_right_to_left", "origin_on_the_plane", "radius_one_ulp_larger"}


def _differs(a: dict, b: dict) -> int:
    return int((scenes.bits(a["occlusion"]) != scenes.bits(b["occlusion"])).sum())


@pytest.mark.parametrize("mistake", [m for m in MISTAKES if m not in ELSEWHERE and m != "not_reached_is_zero"])
def test_a_wrong_pass_differs_from_the_expectation(oracle, truth, mistake):
    sd, cfg, exp = truth
    wrong = GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, **MISTAKES[mistake])
    assert _differs(wrong, exp) >= 1, mistake


def test_not_reached_zero_differs(oracle, truth):
    # every pixel of CASE reaches the plane (its camera looks down from 60 degrees), so no value of "not reached" can show
    # there; pose3_orbit_70x50 looks up from below the plane and reaches it nowhere
    sd, cfg, exp = truth
    assert exp["reached"].all()
    assert _differs(GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, only=np.zeros_like(exp["reached"]), not_reached=0.0),
                    GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, only=np.zeros_like(exp["reached"]))) == 0
    bsd, bcfg, below = GO.skin_expectation("pose3_orbit_70x50")
    assert not below["reached"].any()
    wrong = GO.expected_ground_occlusion(oracle, bsd, bcfg, 0.0, not_reached=0.0)
    assert _differs(wrong, below) == bcfg.width * bcfg.height


def test_the_seed_summed_right_to_left_differs(oracle, truth):
    sd, cfg, exp = truth
    a, b, c = (f32(k) for k in GO.AO_SEED)
    assert f32(0.0) * b == 0  # the plane's height times its constant: nothing to associate at ground_y = 0
    assert _differs(GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, right_to_left=True), exp) == 0
    fsd, fcfg, floor = GO.skin_expectation(CASE, -0.5)
    wrong = GO.expected_ground_occlusion(oracle, fsd, fcfg, -0.5, right_to_left=True)
    assert (wrong["seed"] != floor["seed"]).any() and _differs(wrong, floor) >= 1


def test_the_origin_on_the_plane_differs(oracle):
    sd, cfg, exp = GO.skin_expectation("pose6_orbit_96x64")
    assert _differs(GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, on_plane=True), exp) >= 1


def test_a_radius_one_ulp_larger_differs(oracle, truth):
    sd, cfg, exp = truth
    ulp = float(f32(1.0) + f32(2.0 ** -23))
    assert _differs(GO.expected_ground_occlusion(oracle, sd, cfg, 0.0, radius_scale=ulp), exp) == 0  # no t within an ulp of 3
    # one partly occluded pixel; its count as a function of the radius is a step function: bisect to a step below 3
    y, x = np.argwhere((exp["occlusion"] < 1) & (exp["occlusion"] > 0))[0]
    rays = L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height)
    _, _, P, _ = G.plane_points(rays, 0.0)
    i = int(y) * cfg.width + int(x)
    seed = int(exp["seed"][y, x])
    ao = lambda r: oracle.ao(sd.ptr, P[i], GO.UP, 8, float(r), seed)
    lo, hi = np.array([f32(1e-3)]).view(np.uint32)[0], np.array([f32(3.0)]).view(np.uint32)[0]
    as_float = lambda bits: float(np.array([bits], np.uint32).view(f32)[0])
    assert ao(as_float(lo)) > ao(as_float(hi))
    while hi - lo > 1:  # positive floats order as their bits
        mid = (int(lo) + int(hi)) // 2
        if ao(as_float(mid)) == ao(as_float(lo)):
            lo = mid
        else:
            hi = mid
    radius = as_float(lo)  # the sample's t itself: t < radius fails, t < the next float holds
    on_step = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, aoSamples=8, aoRadius=radius)
    only = np.zeros((cfg.height, cfg.width), bool)
    only[y, x] = True
    right = GO.expected_ground_occlusion(oracle, sd, on_step, 0.0, only=only)
    wrong = GO.expected_ground_occlusion(oracle, sd, on_step, 0.0, only=only, radius_scale=ulp)
    assert wrong["occlusion"][y, x] < right["occlusion"][y, x]


# (occlusion < 1, occlusion == 0, < 1 beside the figure) at ground_y = 0, 8 samples, radius 3
COUNTS = {"pose6_orbit_96x64": (152, 7, 50), "pose5_orbit_64x64_t16": (207, 25, 73)}


@pytest.mark.parametrize("name", list(COUNTS))
def test_the_expectations_hold_occluded_pixels(oracle, mcrt, name):
    sd, cfg, exp = GO.skin_expectation(name)
    below, zero = GO.counts(exp)
    beside = int(((exp["occlusion"] < 1) & GO.beside_the_figure(oracle, sd, cfg)).sum())
    print(f"{name}: occlusion < 1: {below}, == 0: {zero}, < 1 beside the figure: {beside}")
    assert (below, zero, beside) == COUNTS[name]
    assert below >= 100 and zero >= 5 and beside >= 40
    assert np.array_equal(exp["matte"], GO.matte_of(exp["occlusion"]))
    assert (exp["matte"][exp["occlusion"] == 1] == 0).all() and (exp["matte"][exp["occlusion"] == 0] == 255).all()
    values = np.unique(exp["occlusion"])
    assert set(values.tolist()) <= {float(f32(1.0) - f32(k) / f32(8.0)) for k in range(9)}


def test_the_plane_at_zero_cuts_the_outer_leg_boxes(mcrt):
    # the 64x64 skin's outer leg layers reach below the soles: at ground_y = 0 ray origins lie inside boxes
    sd, _, _ = GO.skin_expectation(CASE)
    assert mcrt.scene_floor(sd) < -0.25


def test_a_radius_of_zero_occludes_nothing(oracle, mcrt):
    sd, cfg, _ = GO.skin_expectation(CASE)
    for radius in (0.0, -1.0):
        c = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, aoSamples=8, aoRadius=radius)
        near = GO.skin_expectation(CASE)[2]["occlusion"] < 1
        exp = GO.expected_ground_occlusion(oracle, sd, c, 0.0, only=near)
        assert (exp["occlusion"] == 1).all() and (exp["matte"] == 0).all()


def test_the_seed_sum_is_formed_in_float32_left_to_right():
    P = np.array([[1.25, 0.0, -3.5], [100.0, 7.0, 33.0]], f32)
    a, b, c = (f32(k) for k in GO.AO_SEED)
    want = np.array([(p[0] * a + p[1] * b) + p[2] * c for p in P], f32)
    assert np.array_equal(GO.seed_sums(P), want)
    assert GO.seed_sums(P).dtype == f32


def test_compose_is_the_shot_checkers_without_the_term():
    rng = np.random.default_rng(7)
    shape = (5, 9)
    F = rng.random(shape + (4,), dtype=f32)
    vis, R, dR = rng.random(shape, dtype=f32), rng.random(shape + (4,), dtype=f32), rng.random(shape, dtype=f32) * f32(30.0)
    occ = rng.random(shape, dtype=f32)
    page = rng.random(shape + (3,), dtype=f32)
    for fade in (0.0, 12.0):
        plain = abi.Shot(shadowStrength=0.6, reflectivity=0.35, reflectionFade=fade)
        want = S.compose(F, vis, R, dR, page, plain)
        assert np.array_equal(scenes.bits(GO.compose(F, vis, R, dR, None, page, plain)), scenes.bits(want))
        assert np.array_equal(scenes.bits(GO.compose(F, vis, R, dR, occ, page, plain)), scenes.bits(want))  # o = 0: occ plays no part
        term = abi.Shot(shadowStrength=0.6, reflectivity=0.35, reflectionFade=fade, floorOcclusion=0.5)
        assert np.array_equal(scenes.bits(GO.compose(F, vis, R, dR, None, page, term)), scenes.bits(want))  # no plane: occ = 1
        got = GO.compose(F, vis, R, dR, occ, page, term)
        assert (scenes.bits(got) != scenes.bits(want)).any()
        # by hand, for one pixel
        y, x = 2, 3
        sh = f32(0.6) * (f32(1) - vis[y, x])
        f = f32(1) if fade == 0 else np.clip(f32(1) - dR[y, x] / f32(fade), f32(0), f32(1))
        ar = (f32(0.35) * R[y, x, 3]) * f
        oc = f32(0.5) * (f32(1) - occ[y, x])
        keep = ((f32(1) - sh) * (f32(1) - oc)) * (f32(1) - ar)
        r = F[y, x, 0] * F[y, x, 3] + (page[y, x, 0] * keep + R[y, x, 0] * ar) * (f32(1) - F[y, x, 3])
        assert scenes.bits(np.array([got[y, x, 0]]))[0] == scenes.bits(np.array([f32(r)]))[0]
