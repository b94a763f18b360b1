"""Expected values of the studio shot as a cut-out (mcrt_*_ex: transparent page, shadow colour, crop bounds) — a helper, not a test.

``compose_ex`` restates the blend of include/mcrt.h ("the shot as a cut-out") in numpy float32, one rounding per operation, in
the order written there:

    sh   = s * (1 - vis)
    f    = fade > 0 ? clamp(1 - dR / fade, 0, 1) : 1
    ar   = (k * R.a) * f
    oc   = o * (1 - occ)
    lit  = (1 - sh) * (1 - oc)
    keep = lit * (1 - ar)
    dk   = (1 - lit) * (1 - ar)
    opaque pages:      fl.c = (pg.c * keep + C.c * dk) + R.c * ar      (C = 0: pg.c * keep + R.c * ar)
                       out.c = F.c * F.a + fl.c * (1 - F.a),  out.a = 1
    transparent page:  af = 1 - keep,  fp.c = C.c * dk + R.c * ar      (C = 0: R.c * ar),  u = 1 - F.a
                       af == 0: out = F;  else A = F.a + af * u, out.a = A, out.c = A > 0 ? (F.c * F.a + fp.c * u) / A : 0

``bounds_of`` is the box of the pixels with alpha > 0.  ``expected_shot_ex`` takes every input from the CPU oracle alone: F from
the transparent checker, vis from the ground checker, R and dR from the reflection checker, occ from the ground-occlusion
checker, the page from ``oracle.background`` at the pixel centres."""
from __future__ import annotations

import functools

import numpy as np

from minecraftskin_raytracer_amd import abi

import ground_checker as G
import ground_occlusion_checker as GO
import layers_checker as L
import reflection_checker as R_
import shot_checker as S
import transparent_checker as T

f32 = np.float32
FLT_MAX = S.FLT_MAX
ONE, ZERO = f32(1.0), f32(0.0)
CLASSES = ("opaque figure", "figure edge", "shadow only", "reflection beside the figure", "empty")


def _f32(a, what):
    assert isinstance(a, np.ndarray) and a.dtype == f32, f"{what} is {getattr(a, 'dtype', type(a))}, not float32"
    return a


def terms(vis, R, dR, occ, shot: abi.Shot, shape):
    """(lit, ar, keep, dk) of the definition, each of `shape`; an absent input enters with its miss constant."""
    vis = np.ones(shape, f32) if vis is None else _f32(vis, "vis")
    R = np.zeros(shape + (4,), f32) if R is None else _f32(R, "R")
    occ = np.ones(shape, f32) if occ is None else _f32(occ, "occ")
    s, k, fade, o = f32(shot.shadowStrength), f32(shot.reflectivity), f32(shot.reflectionFade), f32(shot.floorOcclusion)
    sh = _f32(s * (ONE - vis), "sh")
    if fade > 0:
        dR = np.full(shape, FLT_MAX, f32) if dR is None else _f32(dR, "dR")
        with np.errstate(over="ignore"):  # FLT_MAX / fade may be inf below fade = 1: 1 - inf = -inf, clamped to 0
            q = _f32(dR / fade, "dR / fade")
        f = _f32(np.minimum(np.maximum(_f32(ONE - q, "1 - q"), ZERO), ONE), "f")
    else:
        f = np.ones(shape, f32)
    ar = _f32(_f32(k * R[..., 3], "k * R.a") * f, "ar")
    oc = _f32(o * _f32(ONE - occ, "1 - occ"), "oc")
    lit = _f32(_f32(ONE - sh, "1 - sh") * _f32(ONE - oc, "1 - oc"), "lit")
    keep = _f32(lit * _f32(ONE - ar, "1 - ar"), "keep")
    dk = _f32(_f32(ONE - lit, "1 - lit") * _f32(ONE - ar, "1 - ar"), "dk")
    return lit, ar, keep, dk


def compose_ex(F, vis, R, dR, occ, page, shot: abi.Shot) -> np.ndarray:
    """F (..., 4), vis (...) or None, R (..., 4) or None, dR (...) or None, occ (...) or None, page (..., 3) or (3,) — not read
    (may be None) with ``shot.page == "transparent"`` —, all float32 → out (..., 4) float32."""
    F = _f32(F, "F")
    shape = F.shape[:-1]
    _, ar, keep, dk = terms(vis, R, dR, occ, shot, shape)
    R = np.zeros(shape + (4,), f32) if R is None else R
    C = np.asarray(shot.shadowColor, f32)
    colored = not bool((C == 0).all())
    under = _f32(ONE - F[..., 3], "1 - F.a")
    out = np.empty(shape + (4,), f32)
    if shot.page != "transparent":
        page = np.broadcast_to(_f32(np.asarray(page, f32), "page"), shape + (3,))
        for c in range(3):
            fl = _f32(page[..., c] * keep, "pg * keep")
            if colored:
                fl = _f32(fl + _f32(C[c] * dk, "C.c * dk"), "pg * keep + C.c * dk")
            fl = _f32(fl + _f32(R[..., c] * ar, "R.c * ar"), "fl")
            out[..., c] = _f32(_f32(F[..., c] * F[..., 3], "F.c * F.a") + _f32(fl * under, "fl * (1 - F.a)"), "out")
        out[..., 3] = ONE
        return out
    af = _f32(ONE - keep, "af")
    A = _f32(F[..., 3] + _f32(af * under, "af * u"), "A")
    through, seen = af == 0, A > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):  # (the quotients of the pixels that take another branch)
        for c in range(3):
            fp = _f32(R[..., c] * ar, "R.c * ar")
            if colored:
                fp = _f32(_f32(C[c] * dk, "C.c * dk") + fp, "fp")
            num = _f32(_f32(F[..., c] * F[..., 3], "F.c * F.a") + _f32(fp * under, "fp * u"), "num")
            out[..., c] = np.where(through, F[..., c], np.where(seen, _f32(num / A, "num / A"), ZERO))
    out[..., 3] = np.where(through, F[..., 3], np.where(seen, A, ZERO))
    return out


def quantize(rgba: np.ndarray) -> np.ndarray:
    return R_.quantize(rgba)


def bounds_of(alpha: np.ndarray) -> np.ndarray:
    """alpha (H, W) → int32 {x0, y0, x1, y1}: minima of x and y, maxima of x + 1 and y + 1 over the pixels with alpha > 0;
    {W, H, 0, 0} without such a pixel."""
    h, w = alpha.shape
    ys, xs = np.nonzero(alpha > 0)
    if len(xs) == 0:
        return np.array([w, h, 0, 0], np.int32)
    return np.array([xs.min(), ys.min(), xs.max() + 1, ys.max() + 1], np.int32)


def over(out, page) -> np.ndarray:
    """The straight-alpha image `out` (..., 4) over `page` (..., 3) or (3,), in float64: out.c * out.a + pg.c * (1 - out.a)."""
    a = out[..., 3:4].astype(np.float64)
    return out[..., :3].astype(np.float64) * a + np.asarray(page, np.float64) * (1.0 - a)


def expected_shot_ex(oracle, sd, cfg, shot: abi.Shot, ground, pass_cfg=None, threads=None) -> dict:
    """{"F", "vis", "R", "dR", "occ" (1.0 everywhere without the term), "page" (None with the transparent page), "out" (H, W, 4)
    float32, "rgba8" (H, W, 4) uint8, "bounds" (4,) int32 — the box of out's alpha} — every input from the CPU oracle.
    pass_cfg: the config of the passes where cfg's is outside their limits (a shot that skips a pass accepts such a config; it
    does not read the pass's plane).  threads: of the transparent checker (default: transparent_checker.threads())."""
    pass_cfg = pass_cfg or cfg
    F, _ = S.transparent_oracle().render(sd.ptr, cfg, "transparent", threads=threads or T.threads())
    vis = G.expected_ground(oracle, sd, pass_cfg, ground)["visibility"]
    refl = R_.expected_reflection(oracle, sd, pass_cfg, ground)
    if shot.floorOcclusion > 0:
        occ = GO.expected_ground_occlusion(oracle, sd, pass_cfg, ground)["occlusion"]
    else:
        occ = np.ones((cfg.height, cfg.width), f32)
    page = None if shot.page == "transparent" else S.page_plane(oracle, sd, cfg, shot)
    out = compose_ex(F, vis, refl["rgba"], refl["distance"], occ, page, shot)
    return {"F": F, "vis": vis, "R": refl["rgba"], "dR": refl["distance"], "occ": occ, "page": page, "out": out, "rgba8": quantize(out),
            "bounds": bounds_of(out[..., 3])}


def classes(exp: dict, shot: abi.Shot) -> tuple:
    """Pixels of an expectation by what they show, in the order of CLASSES: F.a == 1; 0 < F.a < 1; beside the figure (F.a == 0)
    a darkened floor without a mirror image; beside it a mirror image; nothing at all (out.a == 0)."""
    lit, ar, _, _ = terms(exp["vis"], exp["R"], exp["dR"], exp["occ"], shot, exp["vis"].shape)
    a = exp["F"][..., 3]
    beside = a == 0
    return (int((a == 1).sum()), int(((a > 0) & (a < 1)).sum()), int((beside & (lit < 1) & (ar == 0)).sum()), int((beside & (ar > 0)).sum()),
            int((exp["out"][..., 3] == 0).sum()))


# ---- the whole-shot cases: name -> (kind, pose, orbit camera or None, width, height, tile, shot); tiles that do not divide the
# frame; the floor-occlusion term and a shadow colour in one
SHOTS = {
    "pose0_33x17_t7": ("S64", 0, None, 33, 17, 7, abi.Shot(page="transparent", reflectionFade=24.0)),
    "pose6_orbit_48x40_t13": ("S64", 6, (135.0, 20.0, 34.0), 48, 40, 13,
                              abi.Shot(page="transparent", reflectionFade=24.0, floorOcclusion=0.5, shadowColor=(0.125, 0.0625, 0.25))),
    "s32_pose1_40x30_t16": ("S32", 1, None, 40, 30, 16, abi.Shot(page="transparent", shadowStrength=0.75, reflectivity=0.5)),
}
# what the oracle gives for them (tests/test_cutout_checker.py pins the counts), and the floor every class stays above
FLOORS = (20, 10, 8, 5, 40)


def case_config(name) -> abi.Config:
    _, _, _, w, h, tile, _ = SHOTS[name]
    return abi.Config(width=w, height=h, tileSize=tile, samplesPerPixel=4, maxBounces=3, softShadows=True, shadowSamples=8, aoSamples=8, aoRadius=3.0)


@functools.lru_cache(maxsize=None)
def shot_expectation(name, ground=0.0):
    """(scene description, Config, Shot, expectation) of one of SHOTS — computed once per session, never modified."""
    import oraclelib

    kind, pose, camera, _, _, _, shot = SHOTS[name]
    sd = L.skin_case(kind, pose, camera)
    cfg = case_config(name)
    exp = expected_shot_ex(oraclelib.Oracle(), sd, cfg, shot, ground)
    for a in exp.values():
        if a is not None:
            a.setflags(write=False)
    return sd, cfg, shot, exp


def with_page(shot: abi.Shot, page: str, page_color=None) -> abi.Shot:
    """`shot` on another page."""
    return abi.Shot(page, shot.pageColor if page_color is None else page_color, shot.shadowStrength, shot.reflectivity, shot.reflectionFade,
                    floorOcclusion=shot.floorOcclusion, shadowColor=shot.shadowColor)
