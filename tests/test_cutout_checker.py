"""tests/cutout_checker.py without a device: a hand-computed frame, ``compose_ex`` against a scalar restatement that rounds after
every operation, every consequence the header lists on pixels drawn from value classes, the old blend's bits with opaque pages
and a black shadow, deliberately wrong blends, and the pixel classes of the whole-shot cases as the CPU oracle gives them."""
import itertools

import numpy as np
import pytest

import cutout_checker as X
import ground_occlusion_checker as GO
import scenes
from minecraftskin_raytracer_amd import abi

f32 = np.float32
ONE, ZERO = f32(1), f32(0)
ULP = f32(2.0 ** -24)  # 1 - ULP is the float below 1
DENORMAL = f32(1e-40)
BOUND = 16 * 2.0 ** -24


def _shot(page="transparent", s=0.6, k=0.35, fade=0.0, o=0.0, C=(0.0, 0.0, 0.0), color=(1.0, 1.0, 1.0)):
    return abi.Shot(page, color, s, k, fade, floorOcclusion=o, shadowColor=C)


# ---- by hand ----------------------------------------------------------------------------------------------------------------
def test_a_two_by_two_frame_by_hand():
    """s = k = 0.5, C = (0.25, 0.5, 0): nothing; a shadow alone; an opaque figure pixel in the shadow; a half-covered pixel over a
    mirror image."""
    F = np.array([[[0, 0, 0, 0], [0, 0, 0, 0]], [[1, 0.5, 0.25, 1], [0.5, 0.25, 1, 0.5]]], f32)
    vis = np.array([[1, 0], [0, 1]], f32)
    R = np.zeros((2, 2, 4), f32)
    R[1, 1] = (1, 0, 0.5, 0.5)
    shot = _shot(s=0.5, k=0.5, C=(0.25, 0.5, 0.0))
    out = X.compose_ex(F, vis, R, None, None, None, shot)
    assert out[0, 0].tolist() == [0, 0, 0, 0]
    # sh = 0.5, lit = keep = 0.5, dk = 0.5, af = 0.5, fp = C / 2, A = 0.5: out.c = C
    assert out[0, 1].tolist() == [0.25, 0.5, 0, 0.5]
    # u = 0: A = 1, out.c = F.c
    assert out[1, 0].tolist() == [1, 0.5, 0.25, 1]
    # ar = 0.25, keep = 0.75, dk = 0, af = 0.25, fp = R.c / 4 = (0.25, 0, 0.125), u = 0.5, A = 0.625
    want = [f32(0.375) / f32(0.625), f32(0.125) / f32(0.625), f32(0.5625) / f32(0.625), f32(0.625)]
    assert out[1, 1].tolist() == [float(x) for x in want]
    assert X.bounds_of(out[..., 3]).tolist() == [0, 0, 2, 2]
    assert X.quantize(out)[0, 1].tolist() == [64, 128, 0, 128] and X.quantize(out)[0, 0].tolist() == [0, 0, 0, 0]
    # the same frame on a white page: fl = keep + C * dk + R.c * ar, out = F.c * F.a + fl * u
    white = X.compose_ex(F, vis, R, None, None, np.ones(3, f32), X.with_page(shot, "color", (1.0, 1.0, 1.0)))
    assert white[0, 0].tolist() == [1, 1, 1, 1] and white[0, 1].tolist() == [0.625, 0.75, 0.5, 1]
    assert white[1, 0].tolist() == [1, 0.5, 0.25, 1] and white[1, 1].tolist() == [0.75, 0.5, 0.9375, 1]
    assert np.abs(X.over(out, np.ones(3)) - white[..., :3]).max() <= 2.0 ** -24


def test_bounds_of():
    a = np.zeros((5, 7), f32)
    assert X.bounds_of(a).tolist() == [7, 5, 0, 0]
    a[0, 0] = DENORMAL
    assert X.bounds_of(a).tolist() == [0, 0, 1, 1]
    a[4, 6] = 1
    assert X.bounds_of(a).tolist() == [0, 0, 7, 5]
    b = np.zeros((5, 7), f32)
    b[2, 3], b[3, 1] = 0.5, -0.0
    assert X.bounds_of(b).tolist() == [3, 2, 4, 3]


# ---- pixels drawn from value classes ----------------------------------------------------------------------------------------
def _class_pixels(seed=7):
    """Every combination of F.a, vis, R.a and occ classes, with colours in [0, 1] — a (N,) batch of pixels."""
    g = np.random.default_rng(seed)
    alphas = [ZERO, ONE, ONE - ULP, DENORMAL, f32(0.5), ULP, f32(0.25)]
    viss = [ZERO, f32(0.5), ONE - ULP, ONE, DENORMAL]
    ras = [ZERO, f32(0.5), ONE, ULP]
    occs = [ZERO, f32(0.5), ONE, ONE - ULP]
    combos = np.array(list(itertools.product(alphas, viss, ras, occs)), f32)
    n = len(combos)
    F = g.random((n, 4), dtype=f32)
    F[:, 3] = combos[:, 0]
    F[F[:, 3] == 0] = 0  # no figure: the transparent render leaves (0, 0, 0, 0)
    R = g.random((n, 4), dtype=f32)
    R[:, 3] = combos[:, 2]
    R[R[:, 3] == 0] = 0
    dR = (g.random(n, dtype=f32) * f32(40)).astype(f32)
    dR[R[:, 3] == 0] = X.FLT_MAX
    return F, combos[:, 1].copy(), R, dR, combos[:, 3].copy()


STRENGTHS = [ZERO, DENORMAL, ONE - ULP, ONE]
SETTINGS = list(itertools.product(STRENGTHS, STRENGTHS, STRENGTHS))


def _scalar(F, vis, R, dR, occ, page, shot):
    """compose_ex pixel by pixel on float32 scalars, every operation rounded on its own."""
    s, k, fade, o = f32(shot.shadowStrength), f32(shot.reflectivity), f32(shot.reflectionFade), f32(shot.floorOcclusion)
    C = [f32(c) for c in shot.shadowColor]
    colored = any(c != 0 for c in C)
    out = np.empty_like(F)
    for i in range(len(F)):
        sh = f32(s * f32(ONE - vis[i]))
        f = ONE
        if fade > 0:
            with np.errstate(over="ignore"):
                f = min(max(f32(ONE - f32(dR[i] / fade)), ZERO), ONE)
        ar = f32(f32(k * R[i, 3]) * f)
        oc = f32(o * f32(ONE - occ[i]))
        lit = f32(f32(ONE - sh) * f32(ONE - oc))
        keep = f32(lit * f32(ONE - ar))
        dk = f32(f32(ONE - lit) * f32(ONE - ar))
        u = f32(ONE - F[i, 3])
        if shot.page != "transparent":
            for c in range(3):
                fl = f32(page[c] * keep)
                if colored:
                    fl = f32(fl + f32(C[c] * dk))
                fl = f32(fl + f32(R[i, c] * ar))
                out[i, c] = f32(f32(F[i, c] * F[i, 3]) + f32(fl * u))
            out[i, 3] = ONE
            continue
        af = f32(ONE - keep)
        if af == 0:
            out[i] = F[i]
            continue
        A = f32(F[i, 3] + f32(af * u))
        if not A > 0:
            out[i] = 0
            continue
        for c in range(3):
            fp = f32(R[i, c] * ar)
            if colored:
                fp = f32(f32(C[c] * dk) + fp)
            out[i, c] = f32(f32(f32(F[i, c] * F[i, 3]) + f32(fp * u)) / A)
        out[i, 3] = A
    return out


@pytest.mark.parametrize("page", ["transparent", "color"])
def test_compose_ex_equals_the_scalar_restatement(page):
    F, vis, R, dR, occ = _class_pixels()
    pg = np.array([0.93, 0.87, 0.2], f32)
    for (s, k, o), C, fade in zip(SETTINGS[::5] + [(f32(0.6), f32(0.35), f32(0.5))] * 2, itertools.cycle([(0, 0, 0), (0.125, 0.7, 0.3)]),
                                  itertools.cycle([0.0, 24.0, 0.5])):
        shot = _shot(page, s, k, fade, o, C, tuple(pg))
        with np.errstate(under="ignore"):
            got = X.compose_ex(F, vis, R, dR, occ, pg, shot)
            want = _scalar(F, vis, R, dR, occ, pg, shot)
        scenes.assert_bit_equal(got, want, f"{page} s={s} k={k} o={o} C={C} fade={fade}")


def test_opaque_pages_with_a_black_shadow_are_the_old_blend_bit_for_bit():
    F, vis, R, dR, occ = _class_pixels()
    pg = np.array([0.93, 0.87, 0.2], f32)
    with np.errstate(under="ignore"):
        for s, k, o in SETTINGS + [(f32(0.6), f32(0.35), f32(0.5))]:
            for fade in (0.0, 24.0):
                shot = _shot("color", s, k, fade, o, color=tuple(pg))
                scenes.assert_bit_equal(X.compose_ex(F, vis, R, dR, occ, pg, shot), GO.compose(F, vis, R, dR, occ, pg, shot), f"s={s} k={k} o={o}")
                scenes.assert_bit_equal(X.compose_ex(F, vis, None, None, None, pg, shot), GO.compose(F, vis, None, None, None, pg, shot), "absent planes")
        # -0 is a zero too: the C term is not formed
        shot = _shot("color", 0.6, 0.35, 24.0, 0.5, C=(-0.0, 0.0, -0.0), color=tuple(pg))
        scenes.assert_bit_equal(X.compose_ex(F, vis, R, dR, occ, pg, shot), GO.compose(F, vis, R, dR, occ, pg, shot), "C = -0")


def test_the_consequences_on_pixel_classes():
    F, vis, R, dR, occ = _class_pixels()
    worst, worst8 = 0.0, 0
    with np.errstate(under="ignore"):
        # s = k = o = 0, or the planes absent: the transparent render itself
        scenes.assert_bit_equal(X.compose_ex(F, vis, R, dR, occ, None, _shot(s=0.0, k=0.0, o=0.0, fade=24.0, C=(0.3, 0.2, 0.1))), F, "s = k = o = 0")
        scenes.assert_bit_equal(X.compose_ex(F, None, None, None, None, None, _shot(s=1.0, k=1.0, o=1.0, C=(0.3, 0.2, 0.1))), F, "planes absent")
        for (s, k, o), C in itertools.product(SETTINGS + [(f32(0.6), f32(0.35), f32(0.5)), (f32(0.35), ULP, f32(0.6))], [(0.0, 0.0, 0.0), (0.125, 0.7, 0.3)]):
            for fade in (0.0, 24.0):
                shot = _shot("transparent", s, k, fade, o, C)
                out = X.compose_ex(F, vis, R, dR, occ, None, shot)
                assert np.isfinite(out).all(), (s, k, o, C)
                assert (out[..., 3] >= 0).all() and (out[..., 3] <= 1).all() and (out[..., :3] >= 0).all()
                lit, ar, keep, dk = X.terms(vis, R, dR, occ, shot, vis.shape)
                af = ONE - keep
                # a pixel with F.a == 1 holds F.rgb and alpha 1
                full = F[:, 3] == 1
                assert (out[full] == F[full]).all()
                # no figure and nothing on the floor: F, so (0, 0, 0, 0)
                nothing = (F[:, 3] == 0) & (af == 0)
                assert nothing.any() and (out[nothing] == 0).all()
                # where the floor's alpha is 0 the pixel is F, all four channels as they are
                scenes.assert_bit_equal(out[af == 0], F[af == 0], "af == 0")
                # no figure and a black shadow only: (0, 0, 0, af)
                if C == (0.0, 0.0, 0.0):
                    shadow = (F[:, 3] == 0) & (ar == 0) & (af > 0)
                    assert (out[shadow, :3] == 0).all() and (out[shadow, 3] == af[shadow]).all()
                    assert shadow.any() or (s == 0 and o == 0) or (s < 1e-30 and o < 1e-30)
                # over any page
                for pg in ((0.93, 0.87, 0.2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)):
                    opaque = X.compose_ex(F, vis, R, dR, occ, np.asarray(pg, f32), X.with_page(shot, "color", pg))
                    composed = X.over(out, pg)
                    worst = max(worst, float(np.abs(composed - opaque[..., :3]).max()))
                    q = X.quantize(np.concatenate([composed, np.ones((len(F), 1))], axis=-1).astype(f32))
                    worst8 = max(worst8, int(np.abs(q.astype(int) - X.quantize(opaque).astype(int)).max()))
    print(f"over any page: largest difference {worst / 2.0 ** -24:.2f} * 2^-24, {worst8} level(s) in RGBA8")
    assert worst <= BOUND and worst8 <= 1


def test_af_one_ulp_above_zero():
    """s = 1 and vis = 1 - ulp: the floor's alpha is 2^-24, the smallest the blend can produce from keep < 1."""
    F = np.array([[0, 0, 0, 0], [0.5, 0.25, 1, 0.5], [0.5, 0.25, 1, ONE - ULP]], f32)
    vis = np.full(3, ONE - ULP, f32)
    out = X.compose_ex(F, vis, None, None, None, None, _shot(s=1.0, k=0.0))
    assert out[0].tolist() == [0, 0, 0, float(ULP)]
    assert out[1, 3] == f32(0.5) + f32(ULP * f32(0.5)) and np.isfinite(out).all()
    assert X.bounds_of(out[:, 3].reshape(1, 3)).tolist() == [0, 0, 3, 1]
    assert X.quantize(out)[0].tolist() == [0, 0, 0, 0]  # in the box, though its 8-bit alpha is 0: the box is a superset


# ---- deliberately wrong blends ----------------------------------------------------------------------------------------------
def _variant(F, vis, R, dR, occ, shot, kind=None):
    """The transparent blend, vectorised in its own words, with one mistake (kind None: none)."""
    lit, ar, keep, dk = X.terms(vis, R, dR, occ, shot, F.shape[:-1])
    if kind == "dk without (1 - ar)":
        dk = ONE - lit
    C = np.asarray(shot.shadowColor, f32)
    af = ONE - keep
    if kind == "af = sh":
        af = f32(shot.shadowStrength) * (ONE - vis)
    u = ONE - F[..., 3]
    A = F[..., 3] + af * u
    weight = ONE if kind == "C un-weighted" else dk
    fp = C * np.asarray(weight, f32)[..., None] + R[..., :3] * ar[..., None]
    num = F[..., :3] * F[..., 3:4] + fp * u[..., None]
    div = F[..., 3:4] if kind == "division by F.a" else A[..., None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rgb = num if kind == "premultiplied" else num / div
    rgb = np.where((A > 0)[..., None], rgb, ZERO)
    out = np.concatenate([rgb, np.where(A > 0, A, ZERO)[..., None]], axis=-1).astype(f32)
    if kind != "no af == 0 branch":
        out[af == 0] = F[af == 0]
    return out


def test_wrong_blends_differ():
    F, vis, R, dR, occ = _class_pixels()
    shot = _shot(s=0.6, k=0.35, fade=24.0, o=0.5, C=(0.125, 0.7, 0.3))
    with np.errstate(under="ignore"):
        want = X.compose_ex(F, vis, R, dR, occ, None, shot)
        scenes.assert_bit_equal(_variant(F, vis, R, dR, occ, shot), want, "the blend in other words")
        for kind in ("premultiplied", "division by F.a", "af = sh", "dk without (1 - ar)", "C un-weighted"):
            got = _variant(F, vis, R, dR, occ, shot, kind)
            differ = (np.nan_to_num(got, nan=-1.0, posinf=-2.0) != want).any(axis=-1)
            assert differ.sum() >= 10, kind
        # without the af == 0 branch a pixel with a -0 channel or a colour under alpha 0 changes: F must come through as it is
        odd = np.array([[-0.0, 0.5, 0.25, 0.5], [0.3, 0.2, 0.1, 0.0]], f32)
        plain = _shot(s=0.0, k=0.0)
        through = X.compose_ex(odd, None, None, None, None, None, plain)
        scenes.assert_bit_equal(through, odd, "af == 0")
        assert _variant(odd, np.ones(2, f32), np.zeros((2, 4), f32), None, None, plain, "no af == 0 branch").tobytes() != odd.tobytes()
    # alpha quantised without + 0.5
    q = X.quantize(want)
    trunc = (np.clip(want[..., 3], 0, 1) * f32(255)).astype(np.uint8)
    assert (trunc != q[..., 3]).sum() >= 10
    # the bounds: inclusive maxima, and the box of the 8-bit alpha
    a = np.zeros((4, 6), f32)
    a[1, 2], a[2, 4] = 0.5, 0.001  # 0.001 quantises to 0
    ys, xs = np.nonzero(a > 0)
    assert X.bounds_of(a).tolist() == [2, 1, 5, 3]
    assert [xs.min(), ys.min(), xs.max(), ys.max()] != X.bounds_of(a).tolist()
    assert X.bounds_of(X.quantize(np.stack([a] * 4, axis=-1))[..., 3].astype(f32)).tolist() == [2, 1, 3, 2] != X.bounds_of(a).tolist()


# ---- the whole-shot cases, from the oracle on the CPU -----------------------------------------------------------------------
COUNTS = {"pose0_33x17_t7": (31, 14, 10, 8, 498), "pose6_orbit_48x40_t13": (392, 66, 130, 22, 1310), "s32_pose1_40x30_t16": (93, 31, 37, 22, 1017)}
BOUNDS = {"pose0_33x17_t7": [13, 3, 21, 17], "pose6_orbit_48x40_t13": [14, 0, 48, 40], "s32_pose1_40x30_t16": [14, 6, 27, 30]}


@pytest.mark.parametrize("name", list(X.SHOTS))
def test_the_cases_hold_every_pixel_class(name):
    sd, cfg, shot, exp = X.shot_expectation(name)
    got = X.classes(exp, shot)
    print(name, dict(zip(X.CLASSES, got)), exp["bounds"].tolist())
    assert all(c >= f for c, f in zip(got, X.FLOORS)), got
    assert got == COUNTS[name] and exp["bounds"].tolist() == BOUNDS[name]  # any change of the expectation is noticed
    assert np.isfinite(exp["out"]).all()
    assert cfg.width % cfg.tileSize != 0 and cfg.height % cfg.tileSize != 0
    # the box holds every pixel whose 8-bit alpha is above 0
    x0, y0, x1, y1 = exp["bounds"]
    outside = np.ones((cfg.height, cfg.width), bool)
    outside[y0:y1, x0:x1] = False
    assert (exp["rgba8"][outside, 3] == 0).all()
