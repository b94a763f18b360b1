"""Seeded cases for the shot as a cut-out (mcrt_*_ex: transparent page, shadow colour, floor occlusion, crop bounds) —
generator and model, no device; a helper, not a test.  The twin of tests/shot_fuzz_cases.py, whose helpers it uses.

make_blend_case(seed)  the planes of shot_fuzz_cases.make_planes with two changes — vis is drawn from VIS plus "above 1" and
                       "negative" (the header bars only NaN), and a fifth plane occ from the same seven classes —, a shot from
                       the classes of s, k, fade, o and the shadow colour C, a page (transparent at five of a block's eight
                       places; an opaque colour page and the reference page with a coloured shadow; an opaque page with a black
                       shadow and o > 0, which takes the _occ entry and so shot_body's occlusion multiply), and three RUNS: two
                       with every plane present whose leads pin two of the sixteen alignment combinations, one with inputs
                       absent (the occlusion among them) and one output alone; with the transparent page one full run and every
                       other third run ask for the boxes, which lie behind a lead of 0 ... 3 int32
blend_ex(...)          the blend restated with sclamp's comparisons, all three branches and four channels, and, by name, each of
                       MUTATIONS: a deliberately wrong blend.  box(...) likewise for the bounds and BOX_MUTATIONS
scalar_pixel_ex(...)   one pixel in Python floats rounded after every operation
make_shot_case(seed)   whole cut-outs against the CPU oracle alone: 1 to 4 scenes (S64, S32, slim) of random skins and views, a
                       config, floor heights, two CALLS — each a Shot on the transparent page or on an opaque page with a shadow
                       colour, one with and one without the floor-occlusion term — through a form of the entry points, and the
                       refusals beside them

Everything expected comes from cutout_checker.compose_ex / bounds_of, the CPU oracle and the checkers; nothing here loads the device.

A denormal A is no class: af = 1 - keep is 0 or at least 2^-24 in magnitude, so A = F.a + af * u is 0, or the sum of two values
of which one is at least 2^-48 — a denormal alpha leaves the blend only where af == 0 hands F through."""
from __future__ import annotations

import dataclasses
import hashlib
import re

import numpy as np

import cutout_checker as X
import resident_fuzz_cases as RF
import shot_fuzz_cases as SF
import slim_checker as SL
from minecraftskin_raytracer_amd import abi
from shot_fuzz_cases import BELOW_ONE, DENORM_MIN, FLT_MAX, FLT_MIN, ONE, ZERO, _r, _sclamp, sclamp

f32 = np.float32
BLEND_BLOCK, SHOT_BLOCK = 8, 4

def bounds_groups() -> int:
    """The workgroups a launch with bounds shares among its frames (pass_kernels.hip)."""
    return int(re.search(r"constexpr unsigned kBoundsGroups = (\d+);", RF._source("pass_kernels.hip")).group(1))


# ---- classes of values -----------------------------------------------------------------------------------------------------------
VIS = SF.VIS + ("above 1", "negative")  # of vis and of occ
OCCLUSION = ("0", "smallest denormal", "0.5", "1 - ulp", "1", "uniform")  # of o
COLOUR = ("(0, 0, 0)", "(-0, 0, -0)", "uniform", "(1, 1, 1)", "one channel the smallest denormal", "above 1 and negative", "1e-30")
PAGES = ("transparent", "color, coloured shadow", "reference, coloured shadow", "opaque, black shadow, o > 0")
QUANTITIES = {**SF.QUANTITIES, "vis": VIS, "occ": VIS}
BRANCHES = ("af == 0", "A > 0", "A <= 0")

# what a case's place in its block settles beside the classes of the planes
_PAGE_OF_PLACE = (0, 1, 0, 2, 0, 3, 0, 0)
# (the colours stand where the shadow has weight: s is 0 at places 0 and 5 and the smallest denormal at 1 and 6, so 1 and 6 get theirs from o)
# Place 4, the one whose values are all in general position, has both what shows a wrong dk (0 < ar < 1 beside a colour) and what
# shows (-0, 0, -0) taken for a colour (dk < 0 beside products that are -0): its second run takes the second colour
_COLOUR_OF_PLACE = ("(0, 0, 0)", "uniform", "one channel the smallest denormal", "above 1 and negative", "uniform", None, "1e-30", "(1, 1, 1)")
_SECOND_COLOUR_OF_PLACE = {4: "(-0, 0, -0)"}
_O_OF_PLACE = ("0", "0.5", "smallest denormal", "1 - ulp", "uniform", "1", "uniform", None)
_ABSENT_OF_PLACE = (("visibility",), ("reflection", "occlusion"), ("distance",), ("occlusion",), (), ("distance",), ("visibility", "occlusion"),
                    ("reflection", "distance"))
_BOUNDS_RUN_OF_PLACE = {0: (0, 2), 2: (1,), 4: (0, 2), 6: (1,), 7: (1, 2)}  # the runs of a transparent case that ask for the boxes


def _vis(g, name, shape):
    if name == "above 1":
        return (ONE + g.random(shape, dtype=f32) * f32(3)).astype(f32)
    if name == "negative":
        return (-(g.random(shape, dtype=f32) * f32(3))).astype(f32)
    return SF._vis(g, name, shape)


def _occlusion(g, name) -> float:
    return float({"0": ZERO, "smallest denormal": DENORM_MIN, "0.5": f32(0.5), "1 - ulp": BELOW_ONE, "1": ONE}.get(name, f32(g.random())))


def _colour(g, name) -> tuple:
    if name == "uniform":
        c = g.random(3, dtype=f32)
    elif name == "one channel the smallest denormal":
        c = np.zeros(3, f32)
        c[int(g.integers(3))] = DENORM_MIN
    elif name == "above 1 and negative":
        c = np.array([1.0 + 3.0 * g.random(), -3.0 * g.random(), 1.0 + 3.0 * g.random()], f32)[g.permutation(3)]
    else:
        c = {"(0, 0, 0)": np.zeros(3, f32), "(-0, 0, -0)": np.array([-0.0, 0.0, -0.0], f32), "(1, 1, 1)": np.ones(3, f32), "1e-30": np.full(3, 1e-30, f32)}[name]
    return tuple(float(v) for v in c)


def with_shot(shot: abi.Shot, **changes) -> abi.Shot:
    """`shot` with some settings changed (dataclasses.replace knows neither floorOcclusion nor shadowColor)."""
    kw = {**dataclasses.asdict(shot), "floorOcclusion": shot.floorOcclusion, "shadowColor": shot.shadowColor, **changes}
    return abi.Shot(**kw)


# ---- the blend, restated with sclamp, and its mutations --------------------------------------------------------------------------
MUTATIONS = {
    "fused": "the numerator as fma(F.c, F.a, fp.c * u): rounded once (the opaque pages: the last line likewise)",
    "reciprocal": "num * (1 / A) in place of the division",
    "A from keep": "A formed as 1 - u * keep",
    "dk regrouped": "dk formed as (1 - ar) - keep",
    "oc regrouped": "oc formed as o - o * occ",
    "no through": "no af == 0 branch: the pixel goes through the division",
    "no guard": "no A > 0 guard",
    "flushed": "inputs and results flushed to zero below FLT_MIN",
    "minus zero colour": "(-0, 0, -0) treated as a colour",
}
BOX_MUTATIONS = {
    "8-bit alpha": "the box taken from the 8-bit alpha",
    "no + 1": "the box's maxima without the + 1",
    "transposed": "the box transposed",
}


def blend_ex(F, vis, R, dR, occ, page, shot, mutation=None, trace=None) -> np.ndarray:
    """cutout_checker.compose_ex's arguments and result.  trace: a list that receives every intermediate."""
    z = SF._flush if mutation == "flushed" else (lambda a: a)

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
    s, k, fade, o = (z(f32(v)) for v in (shot.shadowStrength, shot.reflectivity, shot.reflectionFade, shot.floorOcclusion))
    C = z(np.asarray(shot.shadowColor, f32))
    colored = bool((C != 0).any()) or (mutation == "minus zero colour" and bool(np.signbit(C).any()))
    cutout = shot.page == "transparent"
    with np.errstate(all="ignore"):
        sh = t(s * t(ONE - vis))
        if fade > 0:
            dR = np.full(shape, FLT_MAX, f32) if dR is None else z(dR)
            f = t(sclamp(t(ONE - t(dR / fade)), ZERO, ONE))
        else:
            f = np.ones(shape, f32)
        ar = t(t(k * R[..., 3]) * f)
        lit = t(ONE - sh)
        if occ is not None and o > 0:  # (multiplied in only where there is an occlusion plane; o = 0: oc = +-0, 1 - oc = 1)
            oc = t(o - t(o * z(occ))) if mutation == "oc regrouped" else t(o * t(ONE - z(occ)))
            lit = t(lit * t(ONE - oc))
        keep = t(lit * t(ONE - ar))
        dk = t(t(ONE - ar) - keep) if mutation == "dk regrouped" else t(t(ONE - lit) * t(ONE - ar))
        u = t(ONE - F[..., 3])
        out = np.empty(shape + (4,), f32)
        if not cutout:
            page = z(np.broadcast_to(np.asarray(page, f32), shape + (3,)))
            for c in range(3):
                fl = t(page[..., c] * keep)
                if colored:
                    fl = t(fl + t(C[c] * dk))
                below = t(t(fl + t(R[..., c] * ar)) * u)
                if mutation == "fused":
                    out[..., c] = t((F[..., c].astype(np.float64) * F[..., 3].astype(np.float64) + below.astype(np.float64)).astype(f32))
                else:
                    out[..., c] = t(t(F[..., c] * F[..., 3]) + below)
            out[..., 3] = ONE
            return out
        af = t(ONE - keep)
        A = t(ONE - t(u * keep)) if mutation == "A from keep" else t(F[..., 3] + t(af * u))
        through = np.zeros(shape, bool) if mutation == "no through" else af == 0
        seen = np.ones(shape, bool) if mutation == "no guard" else A > 0
        for c in range(3):
            fp = t(R[..., c] * ar)
            if colored:
                fp = t(t(C[c] * dk) + fp)
            below = t(fp * u)
            if mutation == "fused":
                num = t((F[..., c].astype(np.float64) * F[..., 3].astype(np.float64) + below.astype(np.float64)).astype(f32))
            else:
                num = t(t(F[..., c] * F[..., 3]) + below)
            q = t(num * t(ONE / A)) if mutation == "reciprocal" else t(num / A)
            out[..., c] = np.where(through, F[..., c], np.where(seen, q, ZERO))
        out[..., 3] = np.where(through, F[..., 3], np.where(seen, A, ZERO))
    return out


def box(out, mutation=None) -> np.ndarray:
    """(n, 4) int32: cutout_checker.bounds_of of every frame of out (n, h, w, 4) — or one of BOX_MUTATIONS."""
    boxes = []
    for frame in out:
        alpha = X.quantize(frame)[..., 3].astype(f32) if mutation == "8-bit alpha" else frame[..., 3]
        b = X.bounds_of(alpha)
        if mutation == "no + 1" and b[2] > 0:
            b = b - np.array([0, 0, 1, 1], np.int32)
        if mutation == "transposed":
            b = b[[1, 0, 3, 2]]
        boxes.append(b)
    return np.stack(boxes).astype(np.int32)


def _q(a, b):
    """a / b of two floats as the float32 division gives it, b != 0 or not."""
    with np.errstate(all="ignore"):
        return float(f32(a) / f32(b))


def scalar_pixel_ex(F, vis, R, dR, occ, pg, s, k, fade, o, C, cutout) -> list:
    """One pixel of the blend in Python floats (doubles), rounded to float32 after every operation (the sum and product of two
    float32 values, rounded to double and then to float32, is their correctly rounded float32 result; the quotients are numpy's
    float32 divisions of two scalars).  occ: None where the blend has no occlusion plane."""
    sh = _r(s * _r(1.0 - vis))
    f = 1.0
    if fade > 0:
        f = _sclamp(_r(1.0 - _q(dR, fade)), 0.0, 1.0)
    ar = _r(_r(k * R[3]) * f)
    lit = _r(1.0 - sh)
    if occ is not None and o > 0:
        lit = _r(lit * _r(1.0 - _r(o * _r(1.0 - occ))))
    keep = _r(lit * _r(1.0 - ar))
    dk = _r(_r(1.0 - lit) * _r(1.0 - ar))
    u = _r(1.0 - F[3])
    colored = any(c != 0 for c in C)
    if not cutout:
        out = []
        for c in range(3):
            fl = _r(pg[c] * keep)
            if colored:
                fl = _r(fl + _r(C[c] * dk))
            out.append(_r(_r(F[c] * F[3]) + _r(_r(fl + _r(R[c] * ar)) * u)))
        return out + [1.0]
    af = _r(1.0 - keep)
    if af == 0:
        return list(F)
    A = _r(F[3] + _r(af * u))
    if not A > 0:
        return [0.0, 0.0, 0.0, 0.0]
    out = []
    for c in range(3):
        fp = _r(R[c] * ar)
        if colored:
            fp = _r(_r(C[c] * dk) + fp)
        out.append(_q(_r(_r(F[c] * F[3]) + _r(fp * u)), A))
    return out + [A]


# ---- blend cases -------------------------------------------------------------------------------------------------------------------
def _forced(j, names, shift):
    return [(2 * j + shift) % len(names), (2 * j + shift + 1) % len(names)]


def make_blend_case(seed: int) -> dict:
    """The planes, the shot, the frame and three runs; seed % 8 is the case's place in its block, which settles what a block
    must not miss: two classes of every quantity, the classes of s, k, fade, o and C, the page, two of the sixteen alignment
    combinations, which inputs the third run leaves out, which output it writes and which runs ask for the boxes."""
    g = np.random.default_rng([0xC0707, int(seed)])
    j, block = int(seed) % BLEND_BLOCK, int(seed) // BLEND_BLOCK
    w, h = int(g.integers(1, 71)), int(g.integers(1, 41))
    if j == 0:  # the place whose pixels all go through untouched holds the denormal alphas: a frame that has room for them
        w, h = int(g.integers(36, 71)), int(g.integers(21, 41))
    n = 1 if j == 0 else int(g.integers(2, 7)) if j == 1 else int(g.integers(1, 7))
    px = w * h
    shot, shot_classes = SF.draw_shot(g, j)
    page = PAGES[_PAGE_OF_PLACE[j]]
    reference = ("gradient", "scene colour")[block % 2]
    shot, cfg, page_kind = SF.draw_page(g, shot, w, h, reference if page.startswith("reference") else "color")
    planes = SF.make_planes(g, n, h, w, shot.reflectionFade, j)
    shape = (n, h, w)
    extra = lambda: int(g.integers(0, 3))  # noqa: E731
    planes["vis"], planes["classes"]["vis"] = SF._mix(g, VIS, _forced(j, VIS, 0), extra(), shape, lambda a: _vis(g, a, shape))
    planes["occ"], planes["classes"]["occ"] = SF._mix(g, VIS, _forced(j, VIS, 3), extra(), shape, lambda a: _vis(g, a, shape))
    o_class = _O_OF_PLACE[j] or OCCLUSION[int(g.integers(len(OCCLUSION)))]
    c_class = _COLOUR_OF_PLACE[j] or COLOUR[block % 2]  # place 5: a black shadow, of either spelling
    shot = with_shot(shot, page="transparent" if page == "transparent" else shot.page, floorOcclusion=_occlusion(g, o_class),
                     shadowColor=_colour(g, c_class))
    if j == 0:
        # Place 0 blends nothing (s = 0, k the smallest denormal, o = 0): out = F.  Its frame's top row is empty but for one
        # pixel whose alpha is the smallest denormal, so the box's y0 is decided by that pixel alone.  Its alphas are drawn again,
        # from four classes of which two are denormal
        F, cls = planes["F"], planes["classes"]["F.a"]
        alpha, again = SF._mix(g, SF.ALPHA, [SF.ALPHA.index(a) for a in ("0", "1", "smallest denormal", "FLT_MIN / 2")], 0, shape, lambda a: SF._alpha(g, a, shape))
        boundary = planes["classes"]["F.rgb"] == SF.FIGURE_RGB.index("quantiser boundary")  # (those keep F.a = 1)
        F[..., 3], cls[...] = np.where(boundary, ONE, alpha), np.where(boundary, SF.ALPHA.index("1"), again)
        F[0, 0, :, 3], cls[0, 0, :] = ZERO, SF.ALPHA.index("0")
        x = int(g.integers(w))
        F[0, 0, x, 3], cls[0, 0, x] = DENORM_MIN, SF.ALPHA.index("smallest denormal")
    backgrounds = [tuple(float(f32(v)) for v in g.uniform(0, 1, 3)) + (1.0,) for _ in range(3)]
    runs = []
    for r in range(3):
        if r < 2:  # every plane present: the leads pin combination 2 j + r of the alignment flags (bit b set: plane b aligned)
            combo = 2 * j + r
            leads = {p: 0 if combo >> b & 1 else int(g.integers(1, 4)) for b, p in enumerate(SF.RGBA_PLANES)}
            absent, outputs = (), "both"
        else:
            leads = {p: int(g.integers(0, 4)) for p in SF.RGBA_PLANES}
            absent, outputs = _ABSENT_OF_PLACE[j], ("f32", "u8", "both", "u8", "f32", "both", "u8", "f32")[j]
        for p in ("visibility", "distance", "occlusion", "boxes"):
            leads[p] = int(g.integers(0, 4))
        run_shot = with_shot(shot, reflectionFade=0.0) if "distance" in absent else shot  # (absent only with fade 0)
        colour = _SECOND_COLOUR_OF_PLACE.get(j, c_class) if r == 1 else c_class
        if colour != c_class:
            run_shot = with_shot(run_shot, shadowColor=_colour(g, colour))
        runs.append({"leads": leads, "absent": absent, "outputs": outputs, "shot": run_shot, "C": colour,
                     "bounds": page == "transparent" and r in _BOUNDS_RUN_OF_PLACE[j]})
    return {"seed": int(seed), "w": w, "h": h, "n": n, "in_stride": px + int(g.integers(0, 8)), "out_stride": px + int(g.integers(0, 8)),
            "shot": shot, "o": shot.floorOcclusion, "C": shot.shadowColor, "shot_classes": shot_classes + (o_class,), "cfg": cfg,
            "page": page_kind, "page_class": page, "backgrounds": backgrounds, "runs": runs, **planes}


def run_inputs(case, run):
    """(F, vis | None, R | None, dR | None, occ | None, shot) of a run."""
    a = run["absent"]
    return (case["F"], None if "visibility" in a else case["vis"], None if "reflection" in a else case["R"], None if "distance" in a else case["dR"],
            None if "occlusion" in a else case["occ"], run["shot"])


def page_planes(case):
    return None if case["page_class"] == "transparent" else SF.page_planes(case)


def expected_run(case, run, mutation=None) -> np.ndarray:
    """(n, h, w, 4) float32 of a run, from cutout_checker.compose_ex — or from a mutated blend."""
    F, vis, R, dR, occ, shot = run_inputs(case, run)
    if mutation is None:
        return X.compose_ex(F, vis, R, dR, occ, page_planes(case), shot)
    return blend_ex(F, vis, R, dR, occ, page_planes(case), shot, mutation)


def expected_boxes(case, run, mutation=None) -> np.ndarray:
    """(n, 4) int32 of a run that asks for the boxes, from cutout_checker.bounds_of — or from a mutated box."""
    return box(expected_run(case, run), mutation)


def blend_census(cases) -> dict:
    """What a block of blend cases holds.  The branches, the denormal alphas and the boxes are those of every case's first run
    that takes them: the transparent cases' run 0 for the pixels, their first run with bounds for the frames."""
    classes = {q: {name: 0 for name in names} for q, names in QUANTITIES.items()}
    of = {key: {} for key in ("s", "k", "fade", "o", "C", "pages")}
    combos, absent, outputs, bounds = set(), {}, {}, {"with": 0, "without": 0}
    branches = {b: 0 for b in BRANCHES}
    edges = {"a denormal positive out.a": 0, "a denormal intermediate": 0, "a denormal output": 0, "on a quantiser boundary": 0}
    boxes = {"empty": 0, "the whole frame": 0, "set by a denormal alpha alone": 0, "other": 0}
    frames = {"one": 0, "several": 0}
    pixels = cutout_pixels = 0
    for case in cases:
        for q, names in QUANTITIES.items():
            for name, c in zip(names, np.bincount(case["classes"][q].reshape(-1), minlength=len(names))):
                classes[q][name] += int(c)
        for key, value in zip(("s", "k", "fade", "o", "pages"), case["shot_classes"] + (case["page_class"],)):
            of[key][value] = of[key].get(value, 0) + 1
        frames["one" if case["n"] == 1 else "several"] += 1
        pixels += case["n"] * case["w"] * case["h"]
        for run in case["runs"]:
            if not run["absent"] and run["outputs"] == "both":
                combos.add(SF.alignment_flags(run))
            for a in run["absent"]:
                absent[a] = absent.get(a, 0) + 1
            outputs[run["outputs"]] = outputs.get(run["outputs"], 0) + 1
            bounds["with" if run["bounds"] else "without"] += 1
            of["C"][run["C"]] = of["C"].get(run["C"], 0) + 1  # (per run: a case's second run may have a colour of its own)
        run = case["runs"][0]
        trace = []
        F, vis, R, dR, occ, shot = run_inputs(case, run)
        out = blend_ex(F, vis, R, dR, occ, page_planes(case), shot, trace=trace)
        shape = F.shape[:-1]
        any_denormal = np.zeros(shape, bool)
        for a in trace:
            any_denormal |= SF.is_denormal(np.broadcast_to(a, shape))
        edges["a denormal intermediate"] += int(any_denormal.sum())
        edges["a denormal output"] += int(SF.is_denormal(out).any(axis=-1).sum())
        scaled = (sclamp(out, ZERO, ONE) * f32(255.0)).astype(f32)
        edges["on a quantiser boundary"] += int((scaled - np.floor(scaled) == f32(0.5)).any(axis=-1).sum())
        if case["page_class"] != "transparent":
            continue
        cutout_pixels += case["n"] * case["w"] * case["h"]
        _, ar, keep, _ = X.terms(vis, R, dR, occ if shot.floorOcclusion > 0 else None, shot, shape)
        af = ONE - keep
        A = F[..., 3] + af * (ONE - F[..., 3])
        branches["af == 0"] += int((af == 0).sum())
        branches["A > 0"] += int(((af != 0) & (A > 0)).sum())
        branches["A <= 0"] += int(((af != 0) & ~(A > 0)).sum())
        edges["a denormal positive out.a"] += int(((out[..., 3] > 0) & (out[..., 3] < FLT_MIN)).sum())
        first = next(r for r in case["runs"] if r["bounds"])
        alpha = expected_run(case, first)[..., 3]
        for a in alpha:
            b, normal = X.bounds_of(a).tolist(), X.bounds_of(np.where(a < FLT_MIN, ZERO, a)).tolist()
            boxes["empty" if b[2] == 0 else "set by a denormal alpha alone" if b != normal else "the whole frame" if b == [0, 0, case["w"], case["h"]]
                  else "other"] += 1
    return {"classes": classes, **{key: dict(sorted(d.items())) for key, d in of.items()}, "alignment_combinations": sorted(combos),
            "absent": dict(sorted(absent.items())), "outputs": dict(sorted(outputs.items())), "bounds": bounds, "frames": frames, "pixels": pixels,
            "cutout_pixels": cutout_pixels, "branches": branches, "edges": edges, "boxes": boxes}


def blend_block(first) -> list:
    return [make_blend_case(first + k) for k in range(BLEND_BLOCK)]


def case_digest(case) -> str:
    """Every plane and argument of a case, as one hash (o and C stand beside the Shot, whose fields do not hold them)."""
    return SF.case_digest({k: v for k, v in case.items() if k != "runs"} | {"runs": [dict(r, o=r["shot"].floorOcclusion, C=r["shot"].shadowColor) for r in case["runs"]]})


# ---- whole cut-outs ----------------------------------------------------------------------------------------------------------------
KINDS = ("S64", "S32", "slim")
FORMS = ("batch device", "single device", "host", "png", "png crop", "farm")
CALL_PAGES = ("transparent", "color, coloured shadow", "reference, coloured shadow")
DEEP = {"maxBounces": 12, "shadowSamples": 200, "aoSamples": 200, "softShadows": True}  # what only a shot with s = k = o = 0 accepts
FLOORS = (400, 50, 50, 50, 50)  # per block, in the order of cutout_checker.CLASSES


def _floor_look(g):
    """An orbit look from above the floor, so that the shadow, the occlusion and the mirror image are in the frame."""
    look = RF.make_look(g, distance=float(g.uniform(22.0, 45.0)), centred=True)
    look["camera_position"] = RF._orbit(float(g.uniform(-180, 180)), float(g.uniform(10.0, 40.0)), float(g.uniform(22.0, 45.0)), look["camera_target"])
    return look


def make_shot_case(seed: int) -> dict:
    """seed % 4 is the case's place in its block, and 2 * place + call a call's slot, which settles its page and its form (place
    2 takes the cropped file and the farm, the other slots go through the four other forms, a block on each time).  Place 1 has
    a slim scene first; the second call of place 3 is the shot that blends nothing (s = k = o = 0 on the transparent page) under
    DEEP.  The first call skips nothing, so that the oracle's census of it shows every class; of the two calls one has the
    floor-occlusion term."""
    g = np.random.default_rng([0xC0708, int(seed)])
    j, block = int(seed) % SHOT_BLOCK, int(seed) // SHOT_BLOCK
    n = int(g.integers(1, 5))
    name = SF.CONFIG_NAMES[int(g.integers(len(SF.CONFIG_NAMES)))]
    cfg = dataclasses.replace(SF.CONFIGS[name], maxBounces=int(g.integers(0, 9)), shadowSamples=int(g.integers(1, 114)), aoSamples=int(g.integers(1, 9)),
                              aoRadius=float(f32(g.uniform(1.0, 4.0))))
    scenes = []
    for i in range(n):
        kind = "slim" if (j == 1 and i == 0) else KINDS[int(g.choice(3, p=[0.5, 0.0, 0.5] if j == 2 else [0.5, 0.2, 0.3]))]  # (place 2: the farm's)
        skin = RF.make_skin(g, kind)
        pose, look = RF.make_view(g)
        pose = np.zeros(12, f32) if pose is None else pose
        if look is not None:
            look = _floor_look(g) if g.random() < 0.7 else SF._figure_look(g)
        scenes.append({"kind": kind, "skin": skin, "pose": pose, "look": look, "background": ("reference", "transparent")[int(g.integers(2))],
                       "height": SF.HEIGHTS[int(g.integers(len(SF.HEIGHTS)))], "offset": float(f32(g.uniform(0.0, 1.0)))})
    all_64 = all(s["kind"] != "S32" for s in scenes)
    with_o = 0 if j == 3 else (j + block) % 2  # the call that has the floor-occlusion term
    calls = []
    for c in range(2):
        bare = j == 3 and c == 1
        skip = "s = k = 0" if bare else "none" if c == 0 else SF.SKIPS[j]
        slot = 2 * j + c
        page = CALL_PAGES[(0, 1, 2, 0, 0, 0, 1 + block % 2, 0)[slot]]
        shot = SF._skip_shot(g, skip)
        colour = tuple(float(f32(v)) for v in g.uniform(0.05, 1.0, 3))
        if page == "transparent" and g.random() < 0.5:
            colour = (0.0, 0.0, 0.0)
        o = float(f32(g.uniform(0.1, 1.0))) if c == with_o else 0.0
        shot = abi.Shot("transparent" if page == "transparent" else "color" if page.startswith("color") else "reference",
                        tuple(float(f32(v)) for v in g.uniform(0.0, 1.0, 3)), shot.shadowStrength, shot.reflectivity, shot.reflectionFade,
                        floorOcclusion=o, shadowColor=colour)
        form = FORMS[slot] if slot in (4, 5) else FORMS[((slot if slot < 4 else slot - 6) + block) % 4]  # (place 2: the crop and the farm)
        if form == "farm" and not all_64:
            form = "batch device"
        calls.append({"shot": shot, "o": o, "C": colour, "skip": skip, "page": page, "form": form,
                      "deep": dict(DEEP) if bare else None, "gap": int(g.choice([0, 3, 64]))})
    return {"seed": int(seed), "config": name, "cfg": cfg, "scenes": scenes, "calls": calls}


def call_config(case, call) -> abi.Config:
    return case["cfg"] if call["deep"] is None else dataclasses.replace(case["cfg"], **call["deep"])


def refusals(case, call) -> list:
    """[(Config, Shot, with bounds, what the error says)]: what must be refused beside the call, with nothing written."""
    cfg, shot = call_config(case, call), call["shot"]
    on_a_page = with_shot(shot, page="color", shadowColor=(0.25, 0.5, 0.125))
    out = [(cfg, on_a_page, True, "MCRT_PAGE_TRANSPARENT only"),
           (dataclasses.replace(case["cfg"], aoSamples=114), with_shot(shot, floorOcclusion=0.5), False, "113 ao_samples"),
           (cfg, with_shot(shot, shadowColor=(0.5, float("inf"), 0.5)), False, "shadow_color must be finite")]
    if call["deep"] is not None:  # the limits the bare shot was let past hold for every shot that runs a pass
        out += [(cfg, with_shot(shot, shadowStrength=0.5), shot.page == "transparent", "113 shadow samples"),
                (cfg, with_shot(shot, reflectivity=0.5), False, "113 shadow samples"), (cfg, with_shot(shot, floorOcclusion=0.5), False, "113 ao_samples")]
    return out


def scene_desc(scene):
    if scene["kind"] == "slim":
        return SL.reference_scene(scene["skin"], scene["pose"], scene["look"])
    return SF.scene_desc(scene)


def shot_expectations(oracle, case, threads=None) -> list:
    """Per call, per scene: cutout_checker.expected_shot_ex — every plane from the CPU oracle.  Under DEEP the passes the shot
    skips take the case's own config."""
    sds = [scene_desc(s) for s in case["scenes"]]
    heights = [SF.ground_height(s, sd) for s, sd in zip(case["scenes"], sds)]
    return [[X.expected_shot_ex(oracle, sd, call_config(case, call), call["shot"], gy, pass_cfg=None if call["deep"] is None else case["cfg"], threads=threads)
             for sd, gy in zip(sds, heights)] for call in case["calls"]]


def shot_census(cases, expectations) -> dict:
    """cutout_checker.classes summed over the first call of every case, and what the calls and scenes are."""
    totals = np.zeros(len(X.CLASSES), np.int64)
    of = {key: {} for key in ("skips", "pages", "forms", "kinds", "heights", "configs", "floor occlusion", "boxes")}
    frames = 0
    for case, exps in zip(cases, expectations):
        of["configs"][case["config"]] = of["configs"].get(case["config"], 0) + 1
        for exp in exps[0]:
            totals += np.asarray(X.classes(exp, case["calls"][0]["shot"]))
            frames += 1
        for s in case["scenes"]:
            for key, value in (("heights", s["height"]), ("kinds", s["kind"])):
                of[key][value] = of[key].get(value, 0) + 1
        for call, per_scene in zip(case["calls"], exps):
            for key, value in (("skips", call["skip"]), ("pages", call["page"]), ("forms", call["form"]), ("floor occlusion", "o > 0" if call["o"] > 0 else "o = 0")):
                of[key][value] = of[key].get(value, 0) + 1
            if call["page"] == "transparent":
                for exp in per_scene:
                    b = exp["bounds"].tolist()
                    value = "empty" if b[2] == 0 else "the whole frame" if b == [0, 0, case["cfg"].width, case["cfg"].height] else "inside"
                    of["boxes"][value] = of["boxes"].get(value, 0) + 1
    return {"classes": tuple(int(t) for t in totals), "frames": frames, **{key: dict(sorted(d.items())) for key, d in of.items()}}


def shot_block(first) -> list:
    return [make_shot_case(first + k) for k in range(SHOT_BLOCK)]


_SHOT_BLOCKS, _SHOT_CASES, _WORKER = {}, {}, []


def shot_case_digest(case, exps) -> str:
    """The census of one case alone, as a short hash."""
    return hashlib.sha256(repr(shot_census([case], [exps])).encode()).hexdigest()[:16]


def shot_case_expectation(oracle, seed):
    """(case, its expectations, the digest of its census) of one case, computed once per process."""
    if seed not in _SHOT_CASES:
        case = make_shot_case(seed)
        exps = shot_expectations(oracle, case)
        _SHOT_CASES[seed] = (case, exps, shot_case_digest(case, exps))
    return _SHOT_CASES[seed]


def shot_block_expectations(oracle, first):
    """(cases, their expectations, census) of a block, computed once per process."""
    if first not in _SHOT_BLOCKS:
        got = [shot_case_expectation(oracle, first + k) for k in range(SHOT_BLOCK)]
        cases, exps = [c for c, _, _ in got], [e for _, e, _ in got]
        _SHOT_BLOCKS[first] = (cases, exps, shot_census(cases, exps))
    return _SHOT_BLOCKS[first]


def worker_shot_expectation(seed: int) -> list:
    """shot_expectations(make_shot_case(seed)) with an oracle of the worker's own: for a pool of processes that never touch the
    device."""
    import oraclelib

    if not _WORKER:
        _WORKER.append(oraclelib.Oracle())
    return shot_expectations(_WORKER[0], make_shot_case(seed), threads=1)


# first seed of a block -> the census (tests/test_cutout_fuzz_cases.py pins and explains it)
BLEND_BLOCKS = {0: {'classes': {'F.a': {'0': 536,
                         '1': 4841,
                         '1 - ulp': 2667,
                         'smallest denormal': 1396,
                         'FLT_MIN': 1967,
                         'FLT_MIN / 2': 547,
                         '0.5': 2217,
                         'uniform': 2474},
                 'R.a': {'0': 1229,
                         '1': 1272,
                         '1 - ulp': 736,
                         'smallest denormal': 738,
                         'FLT_MIN': 494,
                         'FLT_MIN / 2': 1166,
                         '0.5': 5520,
                         'uniform': 5490},
                 'F.rgb': {'uniform': 4023,
                           '+0': 892,
                           '-0': 4173,
                           'denormal': 1548,
                           'up to 1e18': 1250,
                           'down to -1e18': 615,
                           'quantiser boundary': 4144},
                 'R.rgb': {'uniform': 3350, '+0': 3799, '-0': 3523, 'denormal': 3457, 'up to 1e18': 1125, 'down to -1e18': 1391},
                 'vis': {'0': 6013, '1': 1392, 'j / S': 716, '1 - ulp': 1072, 'denormal': 843, 'above 1': 1306, 'negative': 5303},
                 'dR': {'0': 912,
                        'denormal': 3642,
                        'fade': 691,
                        'fade - ulp': 376,
                        'fade + ulp': 536,
                        'fade / 2': 699,
                        'uniform * 40': 2977,
                        'FLT_MAX': 2743,
                        '+inf': 3203,
                        'negative': 866},
                 'occ': {'0': 875, '1': 659, 'j / S': 5921, '1 - ulp': 6143, 'denormal': 1193, 'above 1': 971, 'negative': 883}},
     's': {'0': 2, '1': 2, '1 - ulp': 1, 'smallest denormal': 2, 'uniform': 1},
     'k': {'0': 2, '1': 1, '1 - ulp': 2, 'smallest denormal': 2, 'uniform': 1},
     'fade': {'0': 1, '1e-3': 1, '3e38': 2, 'FLT_MIN': 1, 'smallest denormal': 1, 'uniform * 60': 2},
     'o': {'0': 1, '0.5': 1, '1': 2, '1 - ulp': 1, 'smallest denormal': 1, 'uniform': 2},
     'C': {'(-0, 0, -0)': 1,
           '(0, 0, 0)': 6,
           '(1, 1, 1)': 3,
           '1e-30': 3,
           'above 1 and negative': 3,
           'one channel the smallest denormal': 3,
           'uniform': 5},
     'pages': {'color, coloured shadow': 1, 'opaque, black shadow, o > 0': 1, 'reference, coloured shadow': 1, 'transparent': 5},
     'alignment_combinations': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
     'absent': {'distance': 3, 'occlusion': 3, 'reflection': 2, 'visibility': 2},
     'outputs': {'both': 18, 'f32': 3, 'u8': 3},
     'bounds': {'with': 8, 'without': 16},
     'frames': {'one': 3, 'several': 5},
     'pixels': 16645,
     'cutout_pixels': 4710,
     'branches': {'af == 0': 1347, 'A > 0': 2974, 'A <= 0': 389},
     'edges': {'a denormal positive out.a': 463, 'a denormal intermediate': 6009, 'a denormal output': 1233, 'on a quantiser boundary': 3077},
     'boxes': {'empty': 0, 'the whole frame': 9, 'set by a denormal alpha alone': 1, 'other': 0}},
 8: {'classes': {'F.a': {'0': 2666,
                         '1': 3446,
                         '1 - ulp': 397,
                         'smallest denormal': 1191,
                         'FLT_MIN': 2247,
                         'FLT_MIN / 2': 3056,
                         '0.5': 1275,
                         'uniform': 1047},
                 'R.a': {'0': 1313,
                         '1': 1382,
                         '1 - ulp': 1433,
                         'smallest denormal': 416,
                         'FLT_MIN': 4518,
                         'FLT_MIN / 2': 3056,
                         '0.5': 2087,
                         'uniform': 1120},
                 'F.rgb': {'uniform': 2331,
                           '+0': 1999,
                           '-0': 858,
                           'denormal': 1569,
                           'up to 1e18': 3492,
                           'down to -1e18': 2803,
                           'quantiser boundary': 2273},
                 'R.rgb': {'uniform': 4688, '+0': 3512, '-0': 929, 'denormal': 953, 'up to 1e18': 2880, 'down to -1e18': 2363},
                 'vis': {'0': 2019, '1': 2190, 'j / S': 1988, '1 - ulp': 494, 'denormal': 2781, 'above 1': 4262, 'negative': 1591},
                 'dR': {'0': 1069,
                        'denormal': 1422,
                        'fade': 1340,
                        'fade - ulp': 1063,
                        'fade + ulp': 2638,
                        'fade / 2': 3352,
                        'uniform * 40': 982,
                        'FLT_MAX': 2200,
                        '+inf': 659,
                        'negative': 600},
                 'occ': {'0': 3294, '1': 3123, 'j / S': 1831, '1 - ulp': 3406, 'denormal': 2265, 'above 1': 832, 'negative': 574}},
     's': {'0': 2, '1': 2, '1 - ulp': 1, 'smallest denormal': 2, 'uniform': 1},
     'k': {'0': 2, '1': 1, '1 - ulp': 2, 'smallest denormal': 2, 'uniform': 1},
     'fade': {'0': 1, '1e-3': 1, '3e38': 2, 'FLT_MIN': 1, 'smallest denormal': 1, 'uniform * 60': 2},
     'o': {'0': 1, '0.5': 2, '1': 1, '1 - ulp': 1, 'smallest denormal': 1, 'uniform': 2},
     'C': {'(-0, 0, -0)': 4,
           '(0, 0, 0)': 3,
           '(1, 1, 1)': 3,
           '1e-30': 3,
           'above 1 and negative': 3,
           'one channel the smallest denormal': 3,
           'uniform': 5},
     'pages': {'color, coloured shadow': 1, 'opaque, black shadow, o > 0': 1, 'reference, coloured shadow': 1, 'transparent': 5},
     'alignment_combinations': [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
     'absent': {'distance': 3, 'occlusion': 3, 'reflection': 2, 'visibility': 2},
     'outputs': {'both': 18, 'f32': 3, 'u8': 3},
     'bounds': {'with': 8, 'without': 16},
     'frames': {'one': 4, 'several': 4},
     'pixels': 15325,
     'cutout_pixels': 13662,
     'branches': {'af == 0': 3532, 'A > 0': 7718, 'A <= 0': 2412},
     'edges': {'a denormal positive out.a': 1164, 'a denormal intermediate': 10270, 'a denormal output': 2628, 'on a quantiser boundary': 2183},
     'boxes': {'empty': 0, 'the whole frame': 11, 'set by a denormal alpha alone': 1, 'other': 0}}}

# the planes and arguments of the blend blocks' cases, as hashes: the same seed gives the same case
BLEND_DIGESTS = {0: ['0fa7e953e638104b',
     'cb2ca56fd73c6358',
     'fe9443c51e3ae846',
     '9c99766ae9bd9bdc',
     'fdad6822a592ceb1',
     '4da5aed4f7693b0d',
     '9cc41f98c3a60155',
     '3d72bd84f1f7a597'],
 8: ['847a1b37cdb12d85',
     '615e0128ad4d4bf6',
     'ffd8e4febf5be52a',
     '2752880c7e4ac73f',
     'e84e0f3cd81eccbe',
     '504d5413a0df8d5c',
     '111c9690651f34d6',
     'e300268c74565794']}

SHOT_BLOCKS = {0: {'classes': (647, 1144, 316, 85, 3251),
     'frames': 10,
     'skips': {'k = 0': 1, 'none': 5, 's = 0': 1, 's = k = 0': 1},
     'pages': {'color, coloured shadow': 2, 'reference, coloured shadow': 1, 'transparent': 5},
     'forms': {'batch device': 2, 'farm': 1, 'host': 1, 'png': 1, 'png crop': 1, 'single device': 2},
     'kinds': {'S32': 2, 'S64': 3, 'slim': 5},
     'heights': {'0.0': 3, '50 below': 1, 'above the head': 5, 'floor': 1},
     'configs': {'default': 1, 'flat': 2, 'spp2': 1},
     'floor occlusion': {'o = 0': 4, 'o > 0': 4},
     'boxes': {'inside': 11}}}

# seed of a block's case -> the digest of the census the CPU oracle gives for it alone: what a GPU test of one case asserts
SHOT_CASES = {0: 'f629620e8205b5fa', 1: '20e86912e458f36c', 2: '50213ec9f6ad9656', 3: 'e7b1d1a42599d866'}
