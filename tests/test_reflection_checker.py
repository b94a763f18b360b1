"""tests/reflection_checker.py pinned on the CPU, so that the GPU tests' expectation cannot go vacuous: the counts of reached
pixels, reflected hits, chains with a second-level hit and level-1 hits in the penumbra that the compiled reference's oracle gave
for two frames, and the checker's own float32 helpers against the oracle's."""
import numpy as np

import reflection_checker as R
import layers_checker as L

f32 = np.float32


def test_pose0_at_the_floor_has_the_measured_counts(oracle):
    sd, cfg, exp = R.skin_expectation("pose0_default_96x64")
    assert cfg.shadowSamples == 8 and cfg.softShadows and cfg.maxBounces == 3
    assert R.counts(exp) == (3072, 136, 34, 5)
    R.assert_miss_constants(exp)
    hit = exp["hit"]
    assert (exp["rgba"][hit][:, 3] > 0).all() and (exp["rgba"][hit][:, :3].max(axis=1) > 0).all()
    assert np.array_equal(exp["rgba8"], oracle.quantize(exp["rgba"]).reshape(exp["rgba8"].shape))
    assert len(np.unique(exp["rgba8"][hit], axis=0)) >= 50  # a picture, not a flat colour
    # the colour is traceRay at depth 1, not at depth 0 and not level 1 alone
    rays = L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height)
    reached, _, P, _ = R.G.plane_points(rays, 0.0)
    rr = R.reflect_rays(rays[:, 3:], P, R.UP)[hit.reshape(-1)]
    assert not np.array_equal(oracle.trace(sd.ptr, cfg, rr, 0, cfg.maxBounces), exp["rgba"][hit])
    assert not np.array_equal(oracle.trace(sd.ptr, cfg, rr, 1, 1), exp["rgba"][hit])


def test_pose6_under_a_wide_light_has_the_measured_penumbra():
    _, _, exp = R.skin_expectation("pose6_orbit_96x64", radius=25.0)
    reached, hits, second, pen = R.counts(exp)
    assert (hits, pen) == (137, 50)
    R.assert_miss_constants(exp)


def test_no_bounce_means_no_hit():
    _, _, exp = R.skin_expectation("pose0_default_96x64", bounces=0)
    assert R.counts(exp) == (3072, 0, 0, 0)
    R.assert_miss_constants(exp)


def test_the_reflection_ray_of_the_floor_mirrors_the_direction(oracle):
    sd = L.skin_case("S64", 0)
    rays = L.pixel_rays(oracle, sd.ptr, 16, 8)
    reached, _, P, _ = R.G.plane_points(rays, 0.0)
    rr = R.reflect_rays(rays[reached, 3:], P[reached], R.UP)
    assert rr.dtype == f32 and reached.sum() == 64
    assert np.array_equal(rr[:, 1], P[reached][:, 1] + f32(1e-3)) and np.array_equal(rr[:, [0, 2]], P[reached][:, [0, 2]])
    d = rays[reached, 3:]
    assert (rr[:, 4] > 0).all() and np.allclose(rr[:, 3:] * [1, -1, 1], d, atol=1e-6)
    assert np.array_equal(R.normalize(np.array([[1e-9, 0, 0], [3, 0, 4]], f32)), np.array([[0, 0, 0], [f32(3) * (f32(1) / f32(5)), 0, f32(4) * (f32(1) / f32(5))]], f32))
