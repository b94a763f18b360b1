"""Fuzz cases of the light layers under extra lights — a helper, not a test: the cases of light_checker.make_light_case (the scenes
and frames of pass_fuzz_cases and fuzz_cases, AO settings drawn per case), each with 0 to 3 extra lights drawn from a generator of
its own: a position around the scene at 0.8 to 4 times its size from its centre, radius 0 (a point light, three cases in ten) or
0.5 to 12, colour channels -0.5 to 2 — so terms above 1 and below 0 both occur.  Expectations: tests/light_multi_checker.py."""
from __future__ import annotations

import numpy as np

from minecraftskin_raytracer_amd import abi

import extra_lights_fuzz_cases as XF
import light_checker as LC
import light_multi_checker as LM

f32 = np.float32


def make_case(group: str, seed: int):
    """→ (scene description, Config, lights, description)"""
    sd, cfg, what = LC.make_light_case(group, seed)
    g = np.random.default_rng(seed ^ 0x4D17)
    lo, hi = XF._bounds(sd)
    centre, size = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3)
    lights = []
    for _ in range(int(g.integers(0, 4))):
        d = g.normal(size=3)
        pos = centre + d / max(np.linalg.norm(d), 1e-30) * g.uniform(0.8, 4.0) * np.linalg.norm(size)
        radius = 0.0 if g.random() < 0.3 else float(f32(g.uniform(0.5, 12.0)))
        colour = tuple(float(f32(v)) for v in g.uniform(-0.5, 2.0, 3)) + (1.0,)
        lights.append(abi.Light(tuple(float(f32(v)) for v in pos), colour, radius))
    text = "; ".join(f"{np.round(l.position, 2).tolist()} r {l.radius:.3g} c {np.round(l.color[:3], 2).tolist()}" for l in lights)
    return sd, cfg, tuple(lights), f"multi [{text}]; {what}"


# What the ORACLE holds over a block, measured on the CPU: (extra lights, hits, (hit, extra disk light) pairs in the penumbra, hits
# whose combined differs from direct[0], hits with occlusion < 1).  tests/test_light_multi_fuzz_cases.py pins every block exactly;
# the GPU run asks for at least half of each total.
FUZZ_BLOCKS = {
    ("bundle", 41000): (22, 3514, 491, 1673, 1766),
    ("wide", 43000): (13, 3041, 126, 290, 2127),
}
FUZZ_BLOCK_IDS = [f"{g}-{s}" for g, s in FUZZ_BLOCKS]
_CACHE = {}


def block_cases(group, first, count=16) -> list:
    return [make_case(group, seed) for seed in range(first, first + count)]


def block_expectations(oracle, group, first) -> list:
    """the expectations of a block, computed once per session and never modified"""
    key = (group, first)
    if key not in _CACHE:
        _CACHE[key] = [LM._frozen(LM.expected_light_multi(oracle, sd, cfg, lights)) for sd, cfg, lights, _ in block_cases(group, first)]
    return _CACHE[key]


def case_counts(exp, lights) -> tuple:
    hits, pen, changed = LM.counts(exp, lights)
    return len(lights), hits, sum(pen), changed, int((exp["hit"] & (exp["occlusion"] < 1)).sum())


def block_totals(cases, exps) -> tuple:
    return tuple(int(v) for v in np.sum([case_counts(e, c[2]) for c, e in zip(cases, exps)], axis=0))
