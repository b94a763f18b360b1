"""Fuzz cases of renders with extra lights — a helper, not a test: the scenes of fuzz_cases.make_bundle_case and
pass_fuzz_cases.make_pass_case (lights near, inside and grazing boxes, texel grids of every density, figures posed with free
angles) at frames of at most 64 x 64 and one sample per pixel, each with 1 to 3 extra lights drawn from a generator of its own:
inside the figure's bounds, below it, behind it as the camera sees it, or around it; radius 0 (a point light, two cases in
five) to 25; colour channels 0 to 2.  Expectations: tests/extra_lights_checker.py."""
from __future__ import annotations

import numpy as np

from minecraftskin_raytracer_amd import abi

import extra_lights_checker as X

f32 = np.float32
GROUPS = ("bundle-plain", "bundle")


def _bounds(sd):
    v = np.concatenate([np.asarray(m["triangles"], np.float64).reshape(-1, 3) for m in sd.to_numpy()["meshes"] if len(m["triangles"])])
    return v.min(axis=0), v.max(axis=0)


def make_lights_case(group: str, seed: int):
    """→ (scene description, Config, lights, description)"""
    import fuzz_cases
    import pass_fuzz_cases as P

    if group == "bundle-plain":
        sd, c, what = fuzz_cases.make_bundle_case(seed)
    else:
        sd, c, _, what = P.make_pass_case(seed)
    g = np.random.default_rng(seed ^ 0xE7A0)
    lo, hi = _bounds(sd)
    centre, size = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3)
    cam = np.array(list(sd.desc.camera_position), np.float64)
    away = centre - cam
    away /= max(np.linalg.norm(away), 1e-30)
    lights = []
    for _ in range(int(g.integers(1, 4))):
        where = int(g.integers(0, 4))
        if where == 0:  # inside the figure's bounds
            pos = centre + g.uniform(-0.45, 0.45, 3) * size
        elif where == 1:  # below it
            pos = centre + np.array([g.uniform(-1, 1) * size[0], -g.uniform(0.6, 2.5) * size[1], g.uniform(-1, 1) * size[2]])
        elif where == 2:  # behind it, as the camera sees it
            pos = centre + away * g.uniform(0.7, 3.0) * np.linalg.norm(size) + g.normal(size=3) * 0.2 * size
        else:  # around it
            d = g.normal(size=3)
            pos = centre + d / max(np.linalg.norm(d), 1e-30) * g.uniform(0.8, 4.0) * np.linalg.norm(size)
        radius = 0.0 if g.random() < 0.4 else float(f32(g.uniform(0.0, 25.0)))
        colour = tuple(float(f32(v)) for v in g.uniform(0.0, 2.0, 3)) + (1.0,)
        lights.append(abi.Light(tuple(float(f32(v)) for v in pos), colour, radius))
    cfg = abi.Config(width=min(int(c.width), 64), height=min(int(c.height), 64), tileSize=c.tileSize, softShadows=c.softShadows,
                     shadowSamples=min(int(c.shadowSamples), 64), maxBounces=int(g.integers(0, 3)), samplesPerPixel=1)
    text = "; ".join(f"{np.round(l.position, 2).tolist()} r {l.radius:.3g} c {np.round(l.color[:3], 2).tolist()}" for l in lights)
    return sd, cfg, tuple(lights), f"lights {group} seed {seed}: {cfg.width}x{cfg.height} b{cfg.maxBounces} [{text}]; {what}"


# What the ORACLE holds over a block, measured on the CPU: (primary hits, hits the extra lights changed, hits whose sum exceeds 1
# before the final clamp, penumbra (hit, extra light) pairs).  tests/test_extra_lights_fuzz_cases.py pins every block exactly; the
# GPU run asks for at least half of each total.
FUZZ_BLOCKS = {
    ("bundle-plain", 31000): (15882, 9463, 120, 4626),
    ("bundle", 33000): (3024, 1262, 36, 1701),
}
FUZZ_BLOCK_IDS = [f"{g}-{s}" for g, s in FUZZ_BLOCKS]
_CACHE = {}


def block_cases(group, first, count=16) -> list:
    return [make_lights_case(group, seed) for seed in range(first, first + count)]


def block_expectations(oracle, group, first) -> list:
    """[(frame, counts)] of a block, computed once per session and never modified"""
    key = (group, first)
    if key not in _CACHE:
        out = []
        for sd, cfg, lights, _ in block_cases(group, first):
            frame, counts = X.expected_frame(oracle, sd, cfg, lights)
            frame.setflags(write=False)
            out.append((frame, counts))
        _CACHE[key] = out
    return _CACHE[key]


def block_totals(exps) -> tuple:
    return tuple(int(v) for v in np.sum([c for _, c in exps], axis=0))


# ---- the long sweep (tools/gpu_fuzz.py, mode lights) -------------------------------------------------------------------
def sweep_case(seed: int):
    """The sweep's case of a seed: the two groups in turn."""
    return make_lights_case(GROUPS[seed % 2], seed)


def worker_sweep_expectation(seed: int) -> tuple:
    """For a worker process that never uses the device: (expected frame, counts) of sweep_case(seed)."""
    import oraclelib

    sd, cfg, lights, _ = sweep_case(seed)
    return X.expected_frame(oraclelib.Oracle(), sd, cfg, lights)
