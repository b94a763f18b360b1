"""Seeded cases for the studio shot (mcrt_composite_shot_batch_device, mcrt_render_shot*) — generator and model, no
device; a helper, not a test.

make_blend_case(seed)  planes for the blend alone: 1 ... 70 x 1 ... 40 pixels, 1 ... 6 frames, strides of their own, every pixel
                       drawn from CLASSES of values (a seed picks 2 to 4 classes per plane, so that one wave mixes them), a shot
                       from classes of s, k and fade, a page of every kind, and three RUNS over the same planes: two with every
                       plane present whose leads pin two of the sixteen combinations of the kernel's four alignment flags, one
                       with inputs absent and one output alone
blend(...)             the blend restated with rt_core.h's sclamp (v < lo ? lo : (hi < v ? hi : v)) as comparisons — numpy's
                       min / max give a zero whose sign depends on operand order — and, by name, each of MUTATIONS: a
                       deliberately wrong blend
scalar_pixel(...)      one pixel in Python floats rounded after every operation, with sclamp's comparisons
make_shot_case(seed)   whole shots against the CPU oracle alone: 1 to 4 scenes of resident_fuzz_cases.make_skin / make_view, a
                       config of CONFIGS with bounces and shadow samples of its own, heights per frame, and CALLS: each a Shot, a
                       page, a form of the entry points, some under the configs only a skipping shot accepts, with the refusals
                       beside them

Everything expected comes from shot_checker.compose, the CPU oracle and the checkers; nothing here loads the device.

One class is not in the plan this file was written to: a NEGATIVE distance.  With dR >= 0 and fade > 0 the clamp's upper bound
never acts (1 - dR / fade <= 1), so a kernel without it could not be told from a right one; the header bars only NaN, so
dR < 0 is a legal input of the blend, and the census counts it."""
from __future__ import annotations

import dataclasses
import hashlib
import re
import struct

import numpy as np

import minecraftskin_raytracer_amd as M
import resident_fuzz_cases as RF
import shot_checker as S
import skin_paint_checker as P
from minecraftskin_raytracer_amd import abi

f32 = np.float32
FLT_MAX = S.FLT_MAX
FLT_MIN = np.finfo(f32).tiny
DENORM_MIN = np.nextafter(f32(0), f32(1))
BELOW_ONE = np.nextafter(f32(1), f32(0))
ONE, ZERO = f32(1), f32(0)
INF = f32(np.inf)
BLEND_BLOCK, SHOT_BLOCK = 8, 4


def _constant(header, name) -> int:
    return int(re.search(rf"constexpr int {name} = (\d+);", RF._source(header)).group(1))


def layers_grid() -> int:
    """The workgroups a frame of the blend gets at most (launch_shapes.h)."""
    return _constant("launch_shapes.h", "kLayersGrid")


def block_lanes() -> int:
    return _constant("launch_shapes.h", "kBlock")


def layers_batch_max_frames() -> int:
    """The frames one launch of a pass or of the blend takes (kernels.h)."""
    return _constant("kernels.h", "kLayersBatchMaxFrames")


def batch_max_frames() -> int:
    """The frames one launch sequence of the batched render takes (kernels.h)."""
    return _constant("kernels.h", "kBatchMaxFrames")


# ---- classes of values -----------------------------------------------------------------------------------------------------------
ALPHA = ("0", "1", "1 - ulp", "smallest denormal", "FLT_MIN", "FLT_MIN / 2", "0.5", "uniform")
RGB = ("uniform", "+0", "-0", "denormal", "up to 1e18", "down to -1e18")
FIGURE_RGB = RGB + ("quantiser boundary",)  # with F.a = 1: the output is F.rgb exactly
VIS = ("0", "1", "j / S", "1 - ulp", "denormal")
DISTANCE = ("0", "denormal", "fade", "fade - ulp", "fade + ulp", "fade / 2", "uniform * 40", "FLT_MAX", "+inf", "negative")
STRENGTH = ("0", "smallest denormal", "1", "1 - ulp", "uniform")
FADE = ("0", "smallest denormal", "FLT_MIN", "1e-3", "uniform * 60", "3e38")
PAGE_VALUE = ("uniform", "-0", "denormal", "above 1", "negative")
QUANTITIES = {"F.a": ALPHA, "R.a": ALPHA, "F.rgb": FIGURE_RGB, "R.rgb": RGB, "vis": VIS, "dR": DISTANCE}


def _denormals(g, shape):
    bits = g.integers(1, 1 << 23, shape, dtype=np.uint32) | (g.integers(0, 2, shape, dtype=np.uint32) << np.uint32(31))
    return bits.view(f32)


def _alpha(g, name, shape):
    if name == "uniform":
        return g.random(shape, dtype=f32)
    value = {"0": ZERO, "1": ONE, "1 - ulp": BELOW_ONE, "smallest denormal": DENORM_MIN, "FLT_MIN": FLT_MIN, "FLT_MIN / 2": FLT_MIN / f32(2),
             "0.5": f32(0.5)}[name]
    return np.full(shape, value, f32)


def _rgb(g, name, shape):
    if name == "uniform":
        return g.random(shape, dtype=f32)
    if name == "+0":
        return np.zeros(shape, f32)
    if name == "-0":
        return np.full(shape, -0.0, f32)
    if name == "denormal":
        return _denormals(g, shape)
    if name in ("up to 1e18", "down to -1e18"):
        a = np.ldexp(1.0 + g.random(shape), g.integers(0, 60, shape)).astype(f32)  # 1 ... 2^60 = 1.15e18, every step exact
        return a if name == "up to 1e18" else -a
    assert name == "quantiser boundary"
    k = g.integers(0, 255, shape)
    b = ((k + 0.5) / 255.0).astype(f32)  # the float32 nearest to (k + 0.5) / 255, and its two neighbours
    side = g.integers(0, 3, shape)
    return np.where(side == 0, np.nextafter(b, ZERO), np.where(side == 1, b, np.nextafter(b, ONE))).astype(f32)


def _vis(g, name, shape):
    if name == "j / S":
        s = g.integers(1, 114, shape)
        j = (g.random(shape) * (s + 1)).astype(np.int64)
        return (j.astype(f32) / s.astype(f32)).astype(f32)
    if name == "denormal":
        return np.abs(_denormals(g, shape))
    return np.full(shape, {"0": ZERO, "1": ONE, "1 - ulp": BELOW_ONE}[name], f32)


def _distance(g, name, shape, fade):
    fade = f32(fade)
    if name == "uniform * 40":
        return (g.random(shape, dtype=f32) * f32(40)).astype(f32)
    if name == "negative":
        return -(g.random(shape, dtype=f32) * f32(40)).astype(f32)
    if name == "denormal":
        return np.abs(_denormals(g, shape))
    with np.errstate(over="ignore"):
        value = {"0": ZERO, "fade": fade, "fade - ulp": np.nextafter(fade, ZERO), "fade + ulp": np.nextafter(fade, INF), "fade / 2": fade / f32(2),
                 "FLT_MAX": FLT_MAX, "+inf": INF}[name]
    return np.full(shape, value, f32)


def _mix(g, names, forced, extra, shape, draw):
    """A plane whose pixels are drawn from 2 to 4 of the classes `names`: the `forced` ones and `extra` others; → (plane, the
    class index of every pixel)."""
    chosen = list(dict.fromkeys(forced))
    rest = [i for i in range(len(names)) if i not in chosen]
    chosen += [int(i) for i in g.permutation(rest)[:extra]]
    pick = np.asarray(chosen)[g.integers(0, len(chosen), shape)]
    plane = None
    for i in chosen:
        a = draw(names[i])
        plane = a if plane is None else np.where(pick.reshape(pick.shape + (1,) * (a.ndim - pick.ndim)) == i, a, plane)
    return plane.astype(f32), pick


def make_planes(g, n, h, w, fade, j=None) -> dict:
    """F (n, h, w, 4), vis (n, h, w), R (n, h, w, 4), dR (n, h, w) drawn per pixel from the classes, and per quantity the class of
    every pixel.  j: the case's place in its block, which settles two classes of every quantity (a block of eight then holds all
    of them); None: any."""
    shape = (n, h, w)

    def forced(names, also=()):
        if j is None:
            return [int(i) for i in g.permutation(len(names))[:2]]
        return [(2 * j) % len(names), (2 * j + 1) % len(names)] + [names.index(a) for a in also]

    ordinary = j == 4  # the case of a block in which every operation sees values in general position
    extra = lambda names, f: int(g.integers(0, 3)) if len(f) < 4 else 0  # noqa: E731
    out, classes = {}, {}
    planes = {}
    for q, names, draw in (("F.a", ALPHA, lambda a: _alpha(g, a, shape)), ("R.a", ALPHA, lambda a: _alpha(g, a, shape)),
                           ("F.rgb", FIGURE_RGB, lambda a: _rgb(g, a, shape + (3,))), ("R.rgb", RGB, lambda a: _rgb(g, a, shape + (3,))),
                           ("vis", VIS, lambda a: _vis(g, a, shape)), ("dR", DISTANCE, lambda a: _distance(g, a, shape, fade))):
        f = forced(names, ("uniform",) if ordinary and q != "vis" and q != "dR" else ("uniform * 40",) if ordinary and q == "dR" else ())
        f = list(dict.fromkeys(f))
        planes[q], classes[q] = _mix(g, names, f, extra(names, f), shape, draw)
    F = np.concatenate([planes["F.rgb"], planes["F.a"][..., None]], axis=-1)
    F[classes["F.rgb"] == FIGURE_RGB.index("quantiser boundary"), 3] = ONE
    classes["F.a"] = np.where(classes["F.rgb"] == FIGURE_RGB.index("quantiser boundary"), ALPHA.index("1"), classes["F.a"])
    out["F"], out["vis"], out["dR"] = np.ascontiguousarray(F), planes["vis"], planes["dR"]
    out["R"] = np.ascontiguousarray(np.concatenate([planes["R.rgb"], planes["R.a"][..., None]], axis=-1))
    out["classes"] = classes
    return out


def _strength(g, name):
    return float({"0": ZERO, "smallest denormal": DENORM_MIN, "1": ONE, "1 - ulp": BELOW_ONE}.get(name, f32(g.random())))


def _fade(g, name):
    return float({"0": ZERO, "smallest denormal": DENORM_MIN, "FLT_MIN": FLT_MIN, "1e-3": f32(1e-3), "3e38": f32(3e38)}.get(name, f32(g.random() * 60.0 + 0.5)))


def _page_value(g, name):
    return float({"-0": f32(-0.0), "denormal": DENORM_MIN * f32(int(g.integers(1, 1000)))}.get(
        name, f32(g.random()) if name == "uniform" else f32(1.0 + 3.0 * g.random()) if name == "above 1" else f32(-g.random())))


def draw_shot(g, j=None):
    """(Shot without its page, the classes of s, k and fade)"""
    if j is None:
        si, ki, fi = (int(g.integers(len(STRENGTH))), int(g.integers(len(STRENGTH))), int(g.integers(len(FADE))))
    else:
        si, ki = j % 5, (2 * j + 1) % 5
        fi = (0, 1, 2, 3, 4, 5, int(g.integers(1, len(FADE))), 4)[j]
    shot = abi.Shot(shadowStrength=_strength(g, STRENGTH[si]), reflectivity=_strength(g, STRENGTH[ki]), reflectionFade=_fade(g, FADE[fi]))
    return shot, (STRENGTH[si], STRENGTH[ki], FADE[fi])


PAGES = ("color", "gradient", "gradient scale 0", "gradient scale 1e6", "scene colour")
_PAGE_OF_PLACE = ("color", "gradient", "scene colour", "gradient", "color", "gradient scale 0", "scene colour", "gradient scale 1e6")


def draw_page(g, shot, w, h, page=None):
    """(shot with its page, Config of the frame, the page's name)"""
    page = PAGES[int(g.integers(len(PAGES)))] if page is None else page
    colour = tuple(_page_value(g, PAGE_VALUE[int(g.integers(len(PAGE_VALUE)))]) for _ in range(3))
    centre = tuple(float(f32(g.uniform(-0.5, 1.5))) for _ in range(3)) + (1.0,)
    edge = tuple(float(f32(g.uniform(-0.5, 1.5))) for _ in range(3)) + (1.0,)
    scale = {"gradient": float(f32(g.uniform(0.2, 3.0))), "gradient scale 0": 0.0, "gradient scale 1e6": 1e6}.get(page, 1.0)
    cfg = abi.Config(width=w, height=h, gradientBg=page != "scene colour", gradientScale=scale, bgCenter=centre, bgEdge=edge)
    shot = dataclasses.replace(shot, page="color" if page == "color" else "reference", pageColor=colour)
    return shot, cfg, page


def gradient_page(cfg, mutation=None) -> np.ndarray:
    """shot_checker.gradient_plane — and, by name, two wrong ones: "corner" takes the page at the pixel's corner (no + 0.5),
    "transposed" gives pixel (px, py) the coordinates of (py, px) (u and v themselves may change places unnoticed: the gradient
    is symmetric in u - 0.5 and v - 0.5; what shows is the pixel's column taken for its row)."""
    h, w = cfg.height, cfg.width
    half = f32(0.0 if mutation == "corner" else 0.5)
    px, py = np.meshgrid(np.arange(w, dtype=f32), np.arange(h, dtype=f32))
    if mutation == "transposed":
        px, py = py, px
    u, v = (px + half) / f32(w), (py + half) / f32(h)
    cx, cy = u - f32(0.5), v - f32(0.5)
    dist = np.sqrt(cx * cx + cy * cy) * f32(2.0) * f32(cfg.gradientScale)
    dist = sclamp(dist.astype(f32), ZERO, ONE)
    t = (dist * dist).astype(f32)
    out = np.empty((h, w, 3), f32)
    for c in range(3):
        out[..., c] = f32(cfg.bgCenter[c]) * (ONE - t) + f32(cfg.bgEdge[c]) * t
    return out


def page_planes(case, mutation=None) -> np.ndarray:
    """(n, h, w, 3): the page under every pixel of a blend case."""
    cfg, n = case["cfg"], case["n"]
    shape = (n, cfg.height, cfg.width, 3)
    if case["page"] == "color":
        return np.broadcast_to(np.asarray(case["shot"].pageColor, f32), shape).copy()
    if case["page"] == "scene colour":
        per_frame = np.stack([np.asarray(case["backgrounds"][i % len(case["backgrounds"])][:3], f32) for i in range(n)])
        return np.broadcast_to(per_frame[:, None, None, :], shape).copy()
    return np.broadcast_to(gradient_page(cfg, mutation), shape).copy()


# ---- the blend, restated with sclamp, and its mutations --------------------------------------------------------------------------
def sclamp(v, lo, hi):
    """rt_core.h: (v < lo) ? lo : ((hi < v) ? hi : v) — the comparisons, so that a zero keeps the sign the kernel gives it."""
    return np.where(v < lo, lo, np.where(hi < v, hi, v)).astype(f32)


MUTATIONS = {
    "fused": "the last line as fma(F.c, F.a, fl * under): in float64, rounded once",
    "reciprocal": "dR * (1 / fade) in place of the division",
    "fade minus": "(fade - dR) / fade",
    "no upper bound": "the clamp without its upper bound",
    "other grouping": "k * (R.a * f)",
    "flushed": "inputs and results flushed to zero below FLT_MIN",
    "no half": "the quantiser without + 0.5",
    "half to even": "the quantiser rounding half to even",
    "corner": "the page taken at the pixel corner instead of the centre",
    "transposed": "the page's coordinates swapped",
}
FLOAT_MUTATIONS = ("fused", "reciprocal", "fade minus", "no upper bound", "other grouping", "flushed", "corner", "transposed")


def _flush(a):
    return np.where(np.abs(a) < FLT_MIN, np.copysign(ZERO, a), a).astype(f32)


def blend(F, vis, R, dR, page, shot, mutation=None, trace=None) -> np.ndarray:
    """shot_checker.compose's arguments and result.  trace: a list that receives every intermediate."""
    z = _flush if mutation == "flushed" else (lambda a: a)

    def t(a):
        a = z(np.asarray(a, f32))
        assert a.dtype == f32
        if trace is not None:
            trace.append(a)
        return a

    shape = F.shape[:-1]
    F = z(F)
    vis = np.ones(shape, f32) if vis is None else z(vis)
    R = np.zeros(shape + (4,), f32) if R is None else z(R)
    s, k, fade = z(f32(shot.shadowStrength)), z(f32(shot.reflectivity)), z(f32(shot.reflectionFade))
    page = z(np.broadcast_to(np.asarray(page, f32), shape + (3,)))
    with np.errstate(all="ignore"):
        sh = t(s * t(ONE - vis))
        if fade > 0:
            dR = np.full(shape, FLT_MAX, f32) if dR is None else z(dR)
            if mutation == "fade minus":
                x = t(t(fade - dR) / fade)
            elif mutation == "reciprocal":
                x = t(ONE - t(dR * t(ONE / fade)))
            else:
                x = t(ONE - t(dR / fade))
            f = t(np.where(x < ZERO, ZERO, x)) if mutation == "no upper bound" else t(sclamp(x, ZERO, ONE))
        else:
            f = np.ones(shape, f32)
        ar = t(k * t(R[..., 3] * f)) if mutation == "other grouping" else t(t(k * R[..., 3]) * f)
        keep = t(t(ONE - sh) * t(ONE - ar))
        under = t(ONE - F[..., 3])
        out = np.empty(shape + (4,), f32)
        for c in range(3):
            fl = t(t(page[..., c] * keep) + t(R[..., c] * ar))
            below = t(fl * under)
            if mutation == "fused":
                out[..., c] = t((F[..., c].astype(np.float64) * F[..., 3].astype(np.float64) + below.astype(np.float64)).astype(f32))
            else:
                out[..., c] = t(t(F[..., c] * F[..., 3]) + below)
    out[..., 3] = ONE
    return out


def quantize(rgba, mutation=None) -> np.ndarray:
    """(uint8_t)(sclamp(c, 0, 1) * 255.0f + 0.5f), and two wrong quantisers."""
    scaled = (sclamp(rgba, ZERO, ONE) * f32(255.0)).astype(f32)
    if mutation == "no half":
        return scaled.astype(np.uint8)
    if mutation == "half to even":
        return np.rint(scaled).astype(np.uint8)
    return (scaled + f32(0.5)).astype(f32).astype(np.uint8)


def _r(x: float) -> float:
    """A double to the nearest float32; beyond FLT_MAX's rounding range, the infinity."""
    if x != x:
        return x
    if abs(x) >= float(FLT_MAX) * (1 + 2.0 ** -25):
        return float("inf") if x > 0 else float("-inf")
    return struct.unpack("f", struct.pack("f", x))[0]


def _sclamp(v, lo, hi):
    return lo if v < lo else (hi if hi < v else v)


def scalar_pixel(F, vis, R, dR, pg, s, k, fade) -> list:
    """One pixel of the blend in Python floats (doubles), rounded to float32 after every operation: the sum, product and quotient
    of two float32 values, rounded to double and then to float32, is their correctly rounded float32 result."""
    sh = _r(s * _r(1.0 - vis))
    f = 1.0
    if fade > 0:
        q = float("inf") if dR == float("inf") else float("-inf") if dR == float("-inf") else _r(dR / fade)
        f = _sclamp(_r(1.0 - q), 0.0, 1.0)
    ar = _r(_r(k * R[3]) * f)
    keep = _r(_r(1.0 - sh) * _r(1.0 - ar))
    under = _r(1.0 - F[3])
    return [_r(_r(F[c] * F[3]) + _r(_r(_r(pg[c] * keep) + _r(R[c] * ar)) * under)) for c in range(3)] + [1.0]


# ---- blend cases -------------------------------------------------------------------------------------------------------------------
RGBA_PLANES = ("figure", "reflection", "out", "out8")  # the kernel's fig16, ref16, out16, out8_4
_ABSENT_OF_PLACE = (("visibility",), ("reflection",), ("distance",), ("visibility", "reflection"), (), ("distance",), ("visibility",), ("reflection", "distance"))


def make_blend_case(seed: int) -> dict:
    """The planes, the shot, the frame and three runs; seed % 8 is the case's place in its block, which settles what a block
    must not miss: two classes of every quantity, the classes of s, k and fade, the page, two of the sixteen alignment
    combinations, which inputs the third run leaves out and which output it writes."""
    g = np.random.default_rng([0x5407, int(seed)])
    j = int(seed) % BLEND_BLOCK
    w, h = int(g.integers(1, 71)), int(g.integers(1, 41))
    n = 1 if j == 0 else int(g.integers(2, 7)) if j == 1 else int(g.integers(1, 7))
    px = w * h
    shot, shot_classes = draw_shot(g, j)
    shot, cfg, page = draw_page(g, shot, w, h, _PAGE_OF_PLACE[j])
    planes = make_planes(g, n, h, w, shot.reflectionFade, j)
    backgrounds = [tuple(float(f32(v)) for v in g.uniform(0, 1, 3)) + (1.0,) for _ in range(3)]
    runs = []
    for r in range(3):
        if r < 2:  # every plane present: the leads pin combination 2 j + r of the alignment flags (bit b set: plane b aligned)
            combo = 2 * j + r
            leads = {p: 0 if combo >> b & 1 else int(g.integers(1, 4)) for b, p in enumerate(RGBA_PLANES)}
            absent, outputs = (), "both"
        else:
            leads = {p: int(g.integers(0, 4)) for p in RGBA_PLANES}
            absent, outputs = _ABSENT_OF_PLACE[j], ("f32", "u8", "both", "u8", "f32", "both", "u8", "f32")[j]
        leads["visibility"], leads["distance"] = int(g.integers(0, 4)), int(g.integers(0, 4))
        run_shot = dataclasses.replace(shot, reflectionFade=0.0) if "distance" in absent else shot  # (absent only with fade 0)
        runs.append({"leads": leads, "absent": absent, "outputs": outputs, "shot": run_shot})
    return {"seed": int(seed), "w": w, "h": h, "n": n, "in_stride": px + int(g.integers(0, 8)), "out_stride": px + int(g.integers(0, 8)),
            "shot": shot, "shot_classes": shot_classes, "cfg": cfg, "page": page, "backgrounds": backgrounds, "runs": runs, **planes}


def run_inputs(case, run):
    """(F, vis | None, R | None, dR | None, shot) of a run."""
    a = run["absent"]
    return (case["F"], None if "visibility" in a else case["vis"], None if "reflection" in a else case["R"],
            None if "distance" in a else case["dR"], run["shot"])


def expected_run(case, run, mutation=None) -> np.ndarray:
    """(n, h, w, 4) float32 of a run, from shot_checker.compose — or from a mutated blend."""
    F, vis, R, dR, shot = run_inputs(case, run)
    if mutation is None:
        return S.compose(F, vis, R, dR, page_planes(case), shot)
    return blend(F, vis, R, dR, page_planes(case, mutation if mutation in ("corner", "transposed") else None), shot, mutation)


def alignment_flags(run) -> int:
    """The four flags as the kernel forms them: a plane is read or written 16 (4) bytes at a time where its lead is 0."""
    return sum(1 << b for b, p in enumerate(RGBA_PLANES) if run["leads"][p] == 0)


def is_denormal(a):
    return (a != 0) & (np.abs(a) < FLT_MIN)


def blend_census(cases) -> dict:
    """What a block of blend cases holds: pixels per class of every quantity, the classes of s, k, fade and the page, the
    alignment combinations of the runs with all four rgba planes, the absent inputs and lone outputs, the frame counts, and the
    pixels at which the arithmetic is at an edge."""
    classes = {q: {name: 0 for name in names} for q, names in QUANTITIES.items()}
    s_of, k_of, fade_of, pages, combos, absent, outputs = {}, {}, {}, {}, set(), {}, {}
    edges = {"dR == fade": 0, "dR / fade overflows": 0, "a denormal intermediate": 0, "a denormal output": 0, "on a quantiser boundary": 0,
             "the upper bound acts": 0}
    frames = {"one": 0, "several": 0}
    pixels = 0
    for case in cases:
        for q, names in QUANTITIES.items():
            counts = np.bincount(case["classes"][q].reshape(-1), minlength=len(names))
            for name, c in zip(names, counts):
                classes[q][name] += int(c)
        for d, key in ((s_of, case["shot_classes"][0]), (k_of, case["shot_classes"][1]), (fade_of, case["shot_classes"][2]), (pages, case["page"])):
            d[key] = d.get(key, 0) + 1
        frames["one" if case["n"] == 1 else "several"] += 1
        pixels += case["n"] * case["w"] * case["h"]
        for run in case["runs"]:
            if not run["absent"] and run["outputs"] == "both":
                combos.add(alignment_flags(run))
            for a in run["absent"]:
                absent[a] = absent.get(a, 0) + 1
            outputs[run["outputs"]] = outputs.get(run["outputs"], 0) + 1
        run = case["runs"][0]
        fade = f32(run["shot"].reflectionFade)
        trace = []
        out = blend(*run_inputs(case, run)[:4], page_planes(case), run["shot"], trace=trace)
        if fade > 0:
            with np.errstate(all="ignore"):
                q = case["dR"] / fade
            edges["dR == fade"] += int((case["dR"] == fade).sum())
            edges["dR / fade overflows"] += int((np.isinf(q) & np.isfinite(case["dR"])).sum())
            edges["the upper bound acts"] += int((ONE - q > ONE).sum())
        shape = case["F"].shape[:-1]
        any_denormal = np.zeros(shape, bool)
        for a in trace:
            any_denormal |= is_denormal(np.broadcast_to(a, shape))
        edges["a denormal intermediate"] += int(any_denormal.sum())
        edges["a denormal output"] += int(is_denormal(out[..., :3]).any(axis=-1).sum())
        scaled = (sclamp(out[..., :3], ZERO, ONE) * f32(255.0)).astype(f32)
        edges["on a quantiser boundary"] += int((scaled - np.floor(scaled) == f32(0.5)).any(axis=-1).sum())
    return {"classes": classes, "s": dict(sorted(s_of.items())), "k": dict(sorted(k_of.items())), "fade": dict(sorted(fade_of.items())),
            "pages": dict(sorted(pages.items())), "alignment_combinations": sorted(combos), "absent": dict(sorted(absent.items())),
            "outputs": dict(sorted(outputs.items())), "frames": frames, "pixels": pixels, "edges": edges}


def blend_block(first) -> list:
    return [make_blend_case(first + k) for k in range(BLEND_BLOCK)]


def _canon(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if dataclasses.is_dataclass(v):
        return _canon(dataclasses.asdict(v))
    if isinstance(v, dict):
        return tuple((k, _canon(x)) for k, x in sorted(v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_canon(x) for x in v)
    return v


def case_digest(case) -> str:
    """Every plane and argument of a case, as one hash."""
    return hashlib.sha256(repr(_canon(case)).encode()).hexdigest()


# ---- whole shots -------------------------------------------------------------------------------------------------------------------
CONFIGS = {
    "default": abi.Config(width=48, height=32, tileSize=16),
    "hard": abi.Config(width=48, height=40, tileSize=8, softShadows=False),
    "ao": abi.Config(width=40, height=40, tileSize=32, aoEnabled=True, aoSamples=4),  # the tile does not divide the frame
    "spp2": abi.Config(width=40, height=24, tileSize=16, samplesPerPixel=2),  # nor here
    "dof": abi.Config(width=48, height=32, tileSize=32, samplesPerPixel=2, dofEnabled=True, aperture=0.5),
    "flat": abi.Config(width=40, height=24, tileSize=8, gradientBg=False),  # the page is the look's own background colour
}
CONFIG_NAMES = tuple(CONFIGS)
FORMS = ("batch device", "single device", "host", "png")
SKIPS = ("none", "s = 0", "k = 0", "s = k = 0")
SHOT_PAGES = ("color", "gradient", "scene colour")
HEIGHTS = ("0.0", "floor", "through the legs", "above the head", "50 below")


def _skip_shot(g, skip):
    s = 0.0 if skip in ("s = 0", "s = k = 0") else float(f32(g.uniform(0.05, 1.0)))
    k = 0.0 if skip in ("k = 0", "s = k = 0") else float(f32(g.uniform(0.05, 1.0)))
    fade = 0.0 if g.random() < 0.3 else float(f32(g.uniform(5.0, 60.0)))
    return abi.Shot(shadowStrength=s, reflectivity=k, reflectionFade=fade)


def _figure_look(g):
    """An orbit look that keeps the figure in the frame (every fourth look is make_look's own: any distance, any target)."""
    if g.random() < 0.25:
        return RF.make_look(g)
    return RF.make_look(g, distance=float(g.uniform(28.0, 60.0)), centred=True)


def make_shot_case(seed: int) -> dict:
    """seed % 4 is the case's place in its block: its second call skips nothing, the shadow, the reflection, both, in turn, and
    its pages go through the three kinds; place 3 renders under the config without a gradient."""
    g = np.random.default_rng([0x5408, int(seed)])
    j = int(seed) % SHOT_BLOCK
    n = int(g.integers(1, 5))
    name = "flat" if j == 3 else CONFIG_NAMES[int(g.integers(len(CONFIG_NAMES) - 1))]
    cfg = dataclasses.replace(CONFIGS[name], maxBounces=int(g.integers(0, 9)), shadowSamples=int(g.integers(1, 114)))
    scenes = []
    for _ in range(n):
        kind = "S64" if g.random() < 0.65 else "S32"
        skin = RF.make_skin(g, kind)
        pose, look = RF.make_view(g)
        pose = np.zeros(12, f32) if pose is None else pose
        look = _figure_look(g) if look is not None else None
        scenes.append({"kind": kind, "skin": skin, "pose": pose, "look": look, "background": ("reference", "transparent")[int(g.integers(2))],
                       "height": HEIGHTS[int(g.integers(len(HEIGHTS)))], "offset": float(f32(g.uniform(0.0, 1.0)))})
    calls = []
    for c in range(2):
        skip = SKIPS[j] if c == 1 else ("none", "s = 0", "k = 0", "s = k = 0")[int((g.random() < 0.25) + 2 * (g.random() < 0.25))]
        page = SHOT_PAGES[(j + c) % 2] if name != "flat" else ("scene colour", "color")[c]
        shot = _skip_shot(g, skip)
        shot = dataclasses.replace(shot, page="color" if page == "color" else "reference",
                                   pageColor=tuple(float(f32(v)) for v in g.uniform(0.0, 1.0, 3)))
        deep = None  # the configs only a skipping shot accepts
        if c == 1 and skip == "k = 0":
            deep = {"maxBounces": 12}
        elif c == 1 and skip == "s = k = 0":
            deep = {"maxBounces": 12, "shadowSamples": 200, "softShadows": True}
        calls.append({"shot": shot, "skip": skip, "page": page, "form": FORMS[int(g.integers(len(FORMS)))], "deep": deep,
                      "gap": int(g.choice([0, 3, 64]))})
    return {"seed": int(seed), "config": name, "cfg": cfg, "scenes": scenes, "calls": calls}


def call_config(case, call) -> abi.Config:
    return case["cfg"] if call["deep"] is None else dataclasses.replace(case["cfg"], **call["deep"])


def refusals(case, call) -> list:
    """[(Shot, what the error says)]: the shots the call's deep config must refuse."""
    if call["deep"] is None:
        return []
    full = dataclasses.replace(call["shot"], shadowStrength=0.5, reflectivity=0.5)
    if "shadowSamples" in call["deep"]:
        return [(full, "113 shadow samples"), (dataclasses.replace(full, reflectivity=0.0), "113 shadow samples"),
                (dataclasses.replace(full, shadowStrength=0.0), "113 shadow samples")]
    return [(full, "at most 8 bounces"), (dataclasses.replace(full, shadowStrength=0.0), "at most 8 bounces")]


def scene_desc(scene):
    return P.reference_scene(scene["skin"], scene["pose"], scene["look"])


def ground_height(scene, sd) -> float:
    floor = M.scene_floor(sd)
    return {"0.0": 0.0, "floor": floor, "through the legs": floor + 3.0 + 6.0 * scene["offset"], "above the head": floor + 34.0 + 6.0 * scene["offset"],
            "50 below": floor - 50.0}[scene["height"]]


def shot_expectations(oracle, case, threads=None) -> list:
    """Per call, per scene: shot_checker.expected_shot — every plane from the CPU oracle.  Under a deep config the two passes
    the shot skips take the case's own config (theirs is outside the passes' limits, and the shot does not read them)."""
    sds = [scene_desc(s) for s in case["scenes"]]
    heights = [ground_height(s, sd) for s, sd in zip(case["scenes"], sds)]
    out = []
    for call in case["calls"]:
        cfg = call_config(case, call)
        out.append([S.expected_shot(oracle, sd, cfg, call["shot"], gy, pass_cfg=None if call["deep"] is None else case["cfg"], threads=threads)
                    for sd, gy in zip(sds, heights)])
    return out


def shot_census(cases, expectations) -> dict:
    """shot_checker.classes summed over the first call of every case (one count per scene and height), and what the calls are."""
    totals = np.zeros(len(S.CLASSES), np.int64)
    skips, pages, forms, heights, configs = {}, {}, {}, {}, {}
    frames = 0
    for case, exps in zip(cases, expectations):
        configs[case["config"]] = configs.get(case["config"], 0) + 1
        for exp in exps[0]:
            totals += np.asarray(S.classes(exp))
            frames += 1
        for s in case["scenes"]:
            heights[s["height"]] = heights.get(s["height"], 0) + 1
        for call in case["calls"]:
            for d, key in ((skips, call["skip"]), (pages, call["page"]), (forms, call["form"])):
                d[key] = d.get(key, 0) + 1
    return {"classes": tuple(int(t) for t in totals), "frames": frames, "skips": dict(sorted(skips.items())), "pages": dict(sorted(pages.items())),
            "forms": dict(sorted(forms.items())), "heights": dict(sorted(heights.items())), "configs": dict(sorted(configs.items()))}


def shot_block(first) -> list:
    return [make_shot_case(first + k) for k in range(SHOT_BLOCK)]


_SHOT_BLOCKS = {}


def shot_block_expectations(oracle, first):
    """(cases, their expectations, census) of a block, computed once per process."""
    if first not in _SHOT_BLOCKS:
        cases = shot_block(first)
        exps = [shot_expectations(oracle, c) for c in cases]
        _SHOT_BLOCKS[first] = (cases, exps, shot_census(cases, exps))
    return _SHOT_BLOCKS[first]


def shot_case_digest(case, exps) -> str:
    """The census of one case alone, as a short hash."""
    return hashlib.sha256(repr(shot_census([case], [exps])).encode()).hexdigest()[:16]


_SHOT_CASES = {}


def shot_case_expectation(oracle, seed):
    """(case, its expectations, the digest of its census) of one case of a block, computed once per process."""
    if seed not in _SHOT_CASES:
        case = make_shot_case(seed)
        exps = shot_expectations(oracle, case)
        _SHOT_CASES[seed] = (case, exps, shot_case_digest(case, exps))
    return _SHOT_CASES[seed]


_WORKER = []


def worker_shot_expectation(seed: int) -> list:
    """shot_expectations(make_shot_case(seed)) with an oracle of the worker's own: for a pool of processes that never touch the
    device."""
    import oraclelib

    if not _WORKER:
        _WORKER.append(oraclelib.Oracle())
    return shot_expectations(_WORKER[0], make_shot_case(seed), threads=1)


FLOORS = (400, 50, 100, 50, 50)  # per block, in the order of shot_checker.CLASSES

# first seed of a block -> the census (tests/test_shot_fuzz_cases.py pins and explains it)
BLEND_BLOCKS = {0: {'classes': {'F.a': {'0': 1272,
                         '1': 3806,
                         '1 - ulp': 1191,
                         'smallest denormal': 1779,
                         'FLT_MIN': 1802,
                         'FLT_MIN / 2': 1802,
                         '0.5': 832,
                         'uniform': 1318},
                 'R.a': {'0': 1134,
                         '1': 3148,
                         '1 - ulp': 1906,
                         'smallest denormal': 1376,
                         'FLT_MIN': 1141,
                         'FLT_MIN / 2': 1253,
                         '0.5': 920,
                         'uniform': 2924},
                 'F.rgb': {'uniform': 1821,
                           '+0': 1743,
                           '-0': 1876,
                           'denormal': 929,
                           'up to 1e18': 2715,
                           'down to -1e18': 2854,
                           'quantiser boundary': 1864},
                 'R.rgb': {'uniform': 2824, '+0': 2463, '-0': 2322, 'denormal': 3298, 'up to 1e18': 1622, 'down to -1e18': 1273},
                 'vis': {'0': 2502, '1': 2376, 'j / S': 2182, '1 - ulp': 3325, 'denormal': 3417},
                 'dR': {'0': 992,
                        'denormal': 984,
                        'fade': 1760,
                        'fade - ulp': 2429,
                        'fade + ulp': 1924,
                        'fade / 2': 3493,
                        'uniform * 40': 1362,
                        'FLT_MAX': 64,
                        '+inf': 449,
                        'negative': 345}},
     's': {'0': 2, '1': 2, '1 - ulp': 1, 'smallest denormal': 2, 'uniform': 1},
     'k': {'0': 2, '1': 1, '1 - ulp': 2, 'smallest denormal': 2, 'uniform': 1},
     'fade': {'0': 1, '1e-3': 1, '3e38': 1, 'FLT_MIN': 2, 'smallest denormal': 1, 'uniform * 60': 2},
     'pages': {'color': 2, 'gradient': 2, 'gradient scale 0': 1, 'gradient scale 1e6': 1, 'scene colour': 2},
     'alignment_combinations': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
     'absent': {'distance': 3, 'reflection': 3, 'visibility': 3},
     'outputs': {'both': 18, 'f32': 3, 'u8': 3},
     'frames': {'one': 1, 'several': 7},
     'pixels': 13802,
     'edges': {'dR == fade': 1760,
               'dR / fade overflows': 860,
               'a denormal intermediate': 8830,
               'a denormal output': 1954,
               'on a quantiser boundary': 1310,
               'the upper bound acts': 345}},
 8: {'classes': {'F.a': {'0': 879,
                         '1': 3362,
                         '1 - ulp': 953,
                         'smallest denormal': 1141,
                         'FLT_MIN': 1377,
                         'FLT_MIN / 2': 769,
                         '0.5': 1771,
                         'uniform': 1706},
                 'R.a': {'0': 1054,
                         '1': 2394,
                         '1 - ulp': 578,
                         'smallest denormal': 466,
                         'FLT_MIN': 1714,
                         'FLT_MIN / 2': 1548,
                         '0.5': 1645,
                         'uniform': 2559},
                 'F.rgb': {'uniform': 2073,
                           '+0': 2344,
                           '-0': 1597,
                           'denormal': 1730,
                           'up to 1e18': 263,
                           'down to -1e18': 1538,
                           'quantiser boundary': 2413},
                 'R.rgb': {'uniform': 1941, '+0': 2333, '-0': 2377, 'denormal': 3032, 'up to 1e18': 1874, 'down to -1e18': 401},
                 'vis': {'0': 3109, '1': 1082, 'j / S': 2259, '1 - ulp': 2264, 'denormal': 3244},
                 'dR': {'0': 439,
                        'denormal': 1736,
                        'fade': 1804,
                        'fade - ulp': 1713,
                        'fade + ulp': 1406,
                        'fade / 2': 1350,
                        'uniform * 40': 1058,
                        'FLT_MAX': 19,
                        '+inf': 1070,
                        'negative': 1363}},
     's': {'0': 2, '1': 2, '1 - ulp': 1, 'smallest denormal': 2, 'uniform': 1},
     'k': {'0': 2, '1': 1, '1 - ulp': 2, 'smallest denormal': 2, 'uniform': 1},
     'fade': {'0': 1, '1e-3': 1, '3e38': 1, 'FLT_MIN': 1, 'smallest denormal': 2, 'uniform * 60': 2},
     'pages': {'color': 2, 'gradient': 2, 'gradient scale 0': 1, 'gradient scale 1e6': 1, 'scene colour': 2},
     'alignment_combinations': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
     'absent': {'distance': 3, 'reflection': 3, 'visibility': 3},
     'outputs': {'both': 18, 'f32': 3, 'u8': 3},
     'frames': {'one': 2, 'several': 6},
     'pixels': 11958,
     'edges': {'dR == fade': 1723,
               'dR / fade overflows': 333,
               'a denormal intermediate': 8528,
               'a denormal output': 2636,
               'on a quantiser boundary': 1737,
               'the upper bound acts': 1363}}}

# the planes and arguments of the blend blocks' cases, as hashes: the same seed gives the same case
BLEND_DIGESTS = {0: ['c353137e668cd90a',
     '2dba9d56b4a7a86c',
     '546acee71cb28077',
     'cd35b0399288faa9',
     '72a2abfbf93a2846',
     '93304a79ca3350c2',
     '6805490c187429d0',
     'd5e50ea24d304db8'],
 8: ['4e31d7e7aaacfae6',
     '21bd5a54866ac666',
     'dc2988effcd22fb4',
     '71b9c2ad413d74ca',
     'f8b51a9c6a39e438',
     'd01ef85d70b14fc4',
     '3802995366aadf81',
     'ba5e10d99d40aca8']}

SHOT_BLOCKS = {0: {'classes': (1611, 1323, 1325, 810, 145),
     'frames': 11,
     'skips': {'k = 0': 2, 'none': 1, 's = 0': 4, 's = k = 0': 1},
     'pages': {'color': 4, 'gradient': 3, 'scene colour': 1},
     'forms': {'batch device': 1, 'host': 2, 'png': 2, 'single device': 3},
     'heights': {'50 below': 2, 'above the head': 3, 'floor': 3, 'through the legs': 3},
     'configs': {'ao': 1, 'default': 1, 'flat': 1, 'hard': 1}},
 8: {'classes': (725, 618, 766, 431, 84),
     'frames': 9,
     'skips': {'k = 0': 3, 'none': 3, 's = 0': 1, 's = k = 0': 1},
     'pages': {'color': 4, 'gradient': 3, 'scene colour': 1},
     'forms': {'batch device': 3, 'host': 1, 'png': 1, 'single device': 3},
     'heights': {'0.0': 2, '50 below': 4, 'above the head': 1, 'floor': 1, 'through the legs': 1},
     'configs': {'ao': 2, 'default': 1, 'flat': 1}}}

# seed of a block's case -> the digest of the census the CPU oracle gives for it alone: what a GPU test of one case asserts
SHOT_CASES = {0: 'be4d14b5980de157', 1: 'a22285460dce7253', 2: '65dc6ae7b5f496d4', 3: 'd43f6fec9fd3cb67', 8: '0006d0001738c240', 9: '18e7460553e6671c', 10: 'bcc82087862f5bd5', 11: '2ae0b7fb508633f7'}
