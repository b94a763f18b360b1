"""tests/shot_checker.py itself, on the CPU: the numpy restatement of the studio shot's blend against a hand-computed frame and
against a scalar restatement that rounds after every operation, the consequences include/mcrt.h lists as part of the contract,
the page plane against the oracle's background, and the oracle's counts for the cases of the GPU suite."""
import struct
import warnings

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

import scenes
import shot_checker as S

f32 = np.float32
FLT_MAX = S.FLT_MAX


def _planes(rng, shape, alphas="mixed"):
    """NaN-free synthetic planes: figure alphas from {0, 1, random}, visibilities with exact 0 and 1, reflections with misses
    ((0, 0, 0, 0), FLT_MAX)."""
    F = rng.random(shape + (4,), dtype=f32)
    pick = rng.integers(0, 3, shape)
    F[..., 3] = np.where(pick == 0, f32(0), np.where(pick == 1, f32(1), F[..., 3]))
    if alphas == "opaque":
        F[..., 3] = 1
    F[F[..., 3] == 0] = 0
    vis = rng.integers(0, 9, shape).astype(f32) / f32(8)
    R = rng.random(shape + (4,), dtype=f32)
    dR = (rng.random(shape, dtype=f32) * f32(40)).astype(f32)
    miss = rng.random(shape) < 0.4
    R[miss] = 0
    dR[miss] = FLT_MAX
    return F, vis, R, dR


def test_hand_computed_frame():
    # every constant is a dyadic rational: each operation below is exact, so the expectation is plain arithmetic
    shot = abi.Shot(page="color", pageColor=(1.0, 1.0, 1.0), shadowStrength=0.5, reflectivity=0.5, reflectionFade=4.0)
    F = np.array([[[0.25, 0.5, 0.75, 1.0], [0.0, 0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.5, 0.5]]], f32)
    vis = np.array([[0.0, 0.5], [1.0, 0.0]], f32)
    R = np.array([[[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]], [[0.5, 0.25, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]]], f32)
    dR = np.array([[1.0, FLT_MAX], [2.0, FLT_MAX]], f32)
    # (0, 0) F.a = 1: F.rgb, whatever lies under it
    # (0, 1) sh = 0.5 * 0.5 = 0.25, ar = 0, keep = 0.75: white * 0.75
    # (1, 0) sh = 0, f = 1 - 2 / 4 = 0.5, ar = (0.5 * 1) * 0.5 = 0.25, keep = 0.75: 0.75 + R.c * 0.25
    # (1, 1) sh = 0.5, f = clamp(1 - FLT_MAX / 4) = 0, ar = 0, keep = 0.5, floor 0.5: F.c * 0.5 + 0.5 * 0.5
    want = np.array([[[0.25, 0.5, 0.75, 1.0], [0.75, 0.75, 0.75, 1.0]], [[0.875, 0.8125, 1.0, 1.0], [0.75, 0.25, 0.5, 1.0]]], f32)
    out = S.compose(F, vis, R, dR, np.asarray(shot.pageColor, f32), shot)
    scenes.assert_bit_equal(out, want, "2 x 2")
    want8 = np.array([[[64, 128, 191, 255], [191, 191, 191, 255]], [[223, 207, 255, 255], [191, 64, 128, 255]]], np.uint8)
    assert np.array_equal(S.quantize(out), want8)


def _r(x: float) -> float:
    """round a double to the nearest float32 (the sum or product of two float32 values is exact enough in a double for this
    to be the correctly rounded float32 result)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def _scalar(F, vis, R, dR, pg, s, k, fade):
    sh = _r(s * _r(1.0 - vis))
    f = 1.0
    if fade > 0:
        q = dR / fade
        q = float("inf") if abs(q) > float(FLT_MAX) * (1 + 2.0 ** -25) else _r(q)
        f = min(max(_r(1.0 - q), 0.0), 1.0)
    ar = _r(_r(k * R[3]) * f)
    keep = _r(_r(1.0 - sh) * _r(1.0 - ar))
    under = _r(1.0 - F[3])
    return [_r(_r(F[c] * F[3]) + _r(_r(_r(pg[c] * keep) + _r(R[c] * ar)) * under)) for c in range(3)] + [1.0]


@pytest.mark.parametrize("fade", [0.0, 0.5, 24.0])
def test_compose_equals_a_scalar_restatement(fade):
    rng = np.random.default_rng(7)
    F, vis, R, dR = _planes(rng, (9, 7))
    shot = abi.Shot(page="color", pageColor=(0.91, 0.89, 0.86), shadowStrength=0.6, reflectivity=0.35, reflectionFade=fade)
    pg = np.asarray(shot.pageColor, f32)
    out = S.compose(F, vis, R, dR, pg, shot)
    s, k = float(f32(0.6)), float(f32(0.35))
    want = np.array([[_scalar([float(x) for x in F[y, x_]], float(vis[y, x_]), [float(x) for x in R[y, x_]], float(dR[y, x_]), [float(x) for x in pg],
                              s, k, float(f32(fade))) for x_ in range(7)] for y in range(9)], f32)
    scenes.assert_bit_equal(out, want, f"fade {fade}")


def test_an_opaque_figure_pixel_keeps_its_rgb():
    rng = np.random.default_rng(11)
    F, vis, R, dR = _planes(rng, (16, 16), alphas="opaque")
    out = S.compose(F, vis, R, dR, np.asarray((0.3, 0.6, 0.9), f32), abi.Shot(page="color", reflectionFade=10.0))
    scenes.assert_bit_equal(out[..., :3], F[..., :3], "F.a == 1")
    assert (out[..., 3] == 1).all()


def test_without_shadow_and_reflection_it_is_figure_over_page():
    rng = np.random.default_rng(13)
    F, vis, R, dR = _planes(rng, (16, 16))
    page = rng.random((16, 16, 3), dtype=f32)
    out = S.compose(F, vis, R, dR, page, abi.Shot(shadowStrength=0.0, reflectivity=0.0, reflectionFade=5.0))
    want = F[..., :3] * F[..., 3:] + page * (f32(1) - F[..., 3:])
    assert want.dtype == f32
    scenes.assert_bit_equal(out[..., :3], want, "s = k = 0")
    beside = F[..., 3] == 0
    scenes.assert_bit_equal(out[beside][:, :3], page[beside], "the bare page")


@pytest.mark.parametrize("fade", [1e-3, 0.5, 1.0, 24.0, 3e38])
def test_a_reflection_miss_vanishes_without_nan_or_warning(fade):
    shape = (4, 4)
    F = np.zeros(shape + (4,), f32)
    R = np.full(shape + (4,), 0.5, f32)  # even with a colour in R: the distance alone makes it vanish
    dR = np.full(shape, FLT_MAX, f32)
    shot = abi.Shot(page="color", pageColor=(0.5, 0.25, 1.0), shadowStrength=0.0, reflectivity=1.0, reflectionFade=fade)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = S.compose(F, None, R, dR, np.asarray(shot.pageColor, f32), shot)
    assert np.isfinite(out).all()
    scenes.assert_bit_equal(out[..., :3], np.broadcast_to(np.asarray(shot.pageColor, f32), shape + (3,)), f"fade {fade}")


def test_skipping_a_pass_equals_feeding_its_miss_constants():
    rng = np.random.default_rng(17)
    F, vis, R, dR = _planes(rng, (12, 10))
    page = rng.random((12, 10, 3), dtype=f32)
    ones, zeros, far = np.ones((12, 10), f32), np.zeros((12, 10, 4), f32), np.full((12, 10), FLT_MAX, f32)
    for fade in (0.0, 24.0):
        shot = abi.Shot(reflectionFade=fade)
        scenes.assert_bit_equal(S.compose(F, None, R, dR, page, shot), S.compose(F, ones, R, dR, page, shot), "no visibility")
        scenes.assert_bit_equal(S.compose(F, vis, None, None, page, shot), S.compose(F, vis, zeros, far, page, shot), "no reflection")
        # and a shot with s == 0 / k == 0 does not see the planes at all: running the pass changes nothing
        no_shadow, no_mirror = abi.Shot(shadowStrength=0.0, reflectionFade=fade), abi.Shot(reflectivity=0.0, reflectionFade=fade)
        scenes.assert_bit_equal(S.compose(F, vis, R, dR, page, no_shadow), S.compose(F, None, R, dR, page, no_shadow), "s = 0")
        scenes.assert_bit_equal(S.compose(F, vis, R, dR, page, no_mirror), S.compose(F, vis, None, None, page, no_mirror), "k = 0")
    scenes.assert_bit_equal(S.compose(F, vis, R, None, page, abi.Shot()), S.compose(F, vis, R, dR, page, abi.Shot()), "no distance without a fade")


def test_compose_insists_on_float32():
    F = np.zeros((2, 2, 4), np.float64)
    with pytest.raises(AssertionError):
        S.compose(F, None, None, None, np.zeros(3, f32), abi.Shot())


@pytest.mark.parametrize("scale", [1.0, 0.7, 3.0])
def test_page_plane_is_the_oracles_background(mcrt, oracle, scale):
    sd = mcrt.MeshBuilder.buildDefaultScene()
    cfg = abi.Config(width=33, height=17, gradientScale=scale)
    page = S.page_plane(oracle, sd, cfg, abi.Shot())
    assert page.shape == (17, 33, 3) and page.dtype == f32
    u, v = (f32(5) + f32(0.5)) / f32(33), (f32(3) + f32(0.5)) / f32(17)
    scenes.assert_bit_equal(page[3, 5], oracle.background(sd.ptr, cfg, float(u), float(v))[:3], "one pixel")
    scenes.assert_bit_equal(S.gradient_plane(cfg), page, "the vectorised gradient")
    # the gradient off: the scene's colour; a colour page: the shot's
    sd.desc.background_color[0], sd.desc.background_color[1], sd.desc.background_color[2] = 0.125, 0.5, 0.75
    flat = S.page_plane(oracle, sd, abi.Config(width=5, height=3, gradientBg=False), abi.Shot())
    assert (flat == np.array([0.125, 0.5, 0.75], f32)).all()
    own = S.page_plane(oracle, sd, cfg, abi.Shot(page="color", pageColor=(0.2, 0.4, 0.6)))
    assert (own == np.array([0.2, 0.4, 0.6], f32)).all()


def test_the_oracles_counts_of_the_small_cases():
    """The expectation of the two small cases of the GPU suite, and what it holds (tests/test_gpu_shot.py asserts the large
    cases' counts where it computes them)."""
    sd, cfg, exp = S.skin_expectation("pose0_33x17_t7")
    assert S.classes(exp) == (31, 14, 10, 6, 8)
    assert not np.isnan(exp["out"]).any() and (exp["out"][..., 3] == 1).all() and (exp["rgba8"][..., 3] == 255).all()
    opaque = exp["F"][..., 3] == 1
    scenes.assert_bit_equal(exp["out"][opaque][:, :3], exp["F"][opaque][:, :3], "opaque pixels keep the render's rgb")
    bare = (exp["F"][..., 3] == 0) & (exp["vis"] == 1) & (exp["R"][..., 3] == 0)
    assert bare.sum() > 100
    scenes.assert_bit_equal(exp["out"][bare][:, :3], exp["page"][bare], "the bare page")
    one = S.skin_expectation("pose0_1x1")[2]
    assert S.classes(one) == (0, 1, 0, 0, 0)
