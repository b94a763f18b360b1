"""Expected values of the light layers (mcrt_render_light & co), from the CPU oracle alone — a helper, not a test.

Per pixel the ray is ``layers_checker.pixel_rays`` and ``oracle.intersect`` gives the hit.  For a hit, as include/mcrt.h defines
the pass:

    visibility  soft shadows with more than one sample: ``oracle.soft_shadow(point, normal, S, seed)`` with the seed of the sum
                p.x * 12345.0f + p.y * 67890.0f + p.z * 11111.0f + 0.0f * 99999.0f, formed here in numpy float32 left to right and
                cast by ``oracle.seed_cast`` (computeSoftShadow takes the one isInShadow ray itself when the light's radius is below
                1e-4); otherwise shade()'s own test, ``oracle.in_shadow(point, normalize(normal), light) ? 0 : 1``
    occlusion   ``oracle.ao(point, normal, A, radius, seed)`` with the seed of p.x * 73856093.0f + p.y * 19349663.0f + p.z * 83492791.0f
    direct      ``oracle.shade(hit, normalize(origin - point), visibility)``

and at a miss 1.0, 1.0 and zeros."""
from __future__ import annotations

import functools

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import ground_checker as G
import layers_checker as L
import reflection_checker as R

f32 = np.float32
PLANES = ("visibility", "occlusion", "direct")


def shadow_sums(p: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        s = ((p[:, 0] * f32(12345.0) + p[:, 1] * f32(67890.0)) + p[:, 2] * f32(11111.0)) + f32(0.0) * f32(99999.0)
    assert s.dtype == f32
    return s


def ao_sums(p: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        s = (p[:, 0] * f32(73856093.0) + p[:, 1] * f32(19349663.0)) + p[:, 2] * f32(83492791.0)
    assert s.dtype == f32
    return s


def expected_at(oracle, sd, cfg, rays: np.ndarray, planes=PLANES) -> dict:
    """The expectation of the pixels whose camera rays are `rays` (n, 6), flat: visibility (n,), occlusion (n,), direct (n, 4)
    and hit (n,) bool.  planes: occlusion is computed only when it is named (the other two always)."""
    n = len(rays)
    hits = oracle.intersect(sd.ptr, rays)
    hit = hits["hit"] != 0
    idx = np.flatnonzero(hit)
    vis = np.ones(n, f32)
    occ = np.ones(n, f32)
    direct = np.zeros((n, 4), f32)
    p = hits["point"][idx].astype(f32)
    nrm = hits["normal"][idx].astype(f32)
    S = G.samples_of(cfg)
    if cfg.softShadows and cfg.shadowSamples > 1:
        sums = shadow_sums(p)
        v = [oracle.soft_shadow(sd.ptr, p[i], nrm[i], S, oracle.seed_cast(float(sums[i]))) for i in range(len(idx))]
    else:
        unit = R.normalize(nrm)
        light = np.array(list(sd.desc.light_position), f32)
        v = [0.0 if oracle.in_shadow(sd.ptr, p[i], unit[i], light) else 1.0 for i in range(len(idx))]
    vis[idx] = np.array(v, f32)
    with np.errstate(all="ignore"):
        view = R.normalize(rays[idx, :3].astype(f32) - p)
    for j, i in enumerate(idx):
        direct[i] = oracle.shade(sd.ptr, hits[i], view[j], None, float(vis[i]))
    if "occlusion" in planes:
        asum = ao_sums(p)
        occ[idx] = np.array([oracle.ao(sd.ptr, p[i], nrm[i], int(cfg.aoSamples), float(cfg.aoRadius), oracle.seed_cast(float(asum[i])))
                             for i in range(len(idx))], f32)
    return {"visibility": vis, "occlusion": occ, "direct": direct, "hit": hit}


def expected_light(oracle, sd, cfg, planes=PLANES) -> dict:
    """{"visibility", "occlusion" (H, W) float32, "direct" (H, W, 4) float32, "hit" (H, W) bool}"""
    w, h = cfg.width, cfg.height
    flat = expected_at(oracle, sd, cfg, L.pixel_rays(oracle, sd.ptr, w, h), planes)
    return {k: v.reshape((h, w) + v.shape[1:]) for k, v in flat.items()}


def counts(exp: dict) -> tuple:
    """(hits, dark hits, penumbra hits, hits with occlusion < 1, hits with occlusion 0) of an expectation."""
    v, o, h = exp["visibility"], exp["occlusion"], exp["hit"]
    return int(h.sum()), int((h & (v == 0)).sum()), int((h & (v > 0) & (v < 1)).sum()), int((h & (o < 1)).sum()), int((h & (o == 0)).sum())


def assert_miss_constants(exp: dict):
    miss = ~exp["hit"]
    assert (exp["visibility"][miss] == 1.0).all() and (exp["occlusion"][miss] == 1.0).all() and (exp["direct"][miss] == 0).all()


def recompose(direct: np.ndarray, occlusion: np.ndarray, intensity) -> np.ndarray:
    """k = 1.0f - ao_intensity * (1.0f - occlusion); rgb = clamp(direct.rgb * k, 0, 1); a = direct.a — in float32."""
    k = f32(1.0) - f32(intensity) * (f32(1.0) - occlusion.astype(f32))
    out = direct.astype(f32).copy()
    out[..., :3] = np.clip(out[..., :3] * k[..., None], f32(0.0), f32(1.0))
    assert out.dtype == f32
    return out


def beauty_config(cfg, ao=False, intensity=0.5):
    """The beauty frame the recomposition speaks of: 1 spp, no depth of field, 0 bounces, the same shadow and AO settings."""
    return abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, maxBounces=0, samplesPerPixel=1, softShadows=cfg.softShadows,
                      shadowSamples=cfg.shadowSamples, aoEnabled=ao, aoSamples=cfg.aoSamples, aoRadius=cfg.aoRadius, aoIntensity=intensity)


def _frozen(exp: dict) -> dict:
    for a in exp.values():
        a.setflags(write=False)
    return exp


def config(w, h, tile, soft=True, samples=8, ao_samples=8, ao_radius=3.0):
    return abi.Config(width=w, height=h, tileSize=tile, softShadows=soft, shadowSamples=samples, aoSamples=ao_samples, aoRadius=ao_radius)


@functools.lru_cache(maxsize=None)
def skin_expectation(name, soft=True, samples=8, ao_samples=8, ao_radius=3.0, light=None, radius=None, tile=None, planes=PLANES):
    """(scene description, Config, expectation) of one of layers_checker.SKIN_CASES — computed once per session, never modified."""
    import oraclelib

    kind, pose, camera, w, h, t = L.SKIN_CASES[name]
    sd = G.set_light(L.skin_case(kind, pose, camera), light, radius)
    cfg = config(w, h, tile or t, soft, samples, ao_samples, ao_radius)
    return sd, cfg, _frozen(expected_light(oraclelib.Oracle(), sd, cfg, planes))


@functools.lru_cache(maxsize=None)
def box_expectation(name):
    import oraclelib

    sc, w, h, tile = L.box_scene(name)
    sd = M.SceneDesc(sc)
    cfg = config(w, h, tile)
    return sd, cfg, _frozen(expected_light(oraclelib.Oracle(), sd, cfg))


def assert_light_equal(got: dict, exp: dict, what=""):
    """Bit for bit (as uint32), for the planes `got` holds."""
    import scenes

    for k in got:
        scenes.assert_bit_equal(got[k], exp[k], f"{what} {k}")


# ---- the fixed blocks of 16 seeds of the suite (tests/test_gpu_light_fuzz.py, tests/test_light_fuzz_cases.py) ------------
def make_light_case(group: str, seed: int):
    """A case of pass_fuzz_cases / fuzz_cases with AO settings drawn per case from a generator of its own: 1 to 113 samples, a
    radius from a hundredth of the scene's height to ten times it (log-uniform).  → (scene description, Config, description)"""
    import fuzz_cases
    import pass_fuzz_cases as P

    if group == "bundle-plain":  # the bundle cases under their own frame size and tile size
        sd, c, what = fuzz_cases.make_bundle_case(seed)
    else:
        sd, c, _, what = P.GROUPS[group](seed)
    g = np.random.default_rng(seed ^ 0xA0CC)
    lo, hi = P.y_range(sd)
    height = max(hi - lo, 1e-30)
    a = int(g.integers(1, 114))
    r = float(f32(height * 10.0 ** g.uniform(-2.0, 1.0)))
    cfg = abi.Config(width=c.width, height=c.height, tileSize=c.tileSize, softShadows=c.softShadows, shadowSamples=min(int(c.shadowSamples), 113),
                     aoSamples=a, aoRadius=r)
    return sd, cfg, f"light {group} seed {seed}: A {a} radius {r!r}; {what}"


# what the ORACLE holds over a block, measured on the CPU: (hits, penumbra hits, hits with occlusion < 1).
# tests/test_light_fuzz_cases.py pins every block exactly; the GPU run asks for at least half of each total.
FUZZ_BLOCKS = {
    ("bundle", 7000): (3859, 968, 1792),
    ("bundle", 7016): (4601, 407, 2485),
    ("wide", 9000): (2983, 917, 1271),
    ("wide", 9016): (2549, 189, 1763),
    ("bundle-plain", 21000): (8000, 257, 3497),
    ("bundle-plain", 21016): (18916, 2933, 7259),
}
FUZZ_BLOCK_IDS = [f"{g}-{s}" for g, s in FUZZ_BLOCKS]
_CACHE = {}


def block_cases(group, first, count=16) -> list:
    return [make_light_case(group, seed) for seed in range(first, first + count)]


def block_expectations(oracle, group, first) -> list:
    key = (group, first)
    if key not in _CACHE:
        _CACHE[key] = [_frozen(expected_light(oracle, sd, cfg)) for sd, cfg, _ in block_cases(group, first)]
    return _CACHE[key]


def block_totals(exps) -> tuple:
    c = np.sum([counts(e) for e in exps], axis=0)
    return int(c[0]), int(c[2]), int(c[3])


# ---- the long sweep (tools/gpu_fuzz.py, mode light) ----------------------------------------------------------------------
SWEEP_GROUPS = ("bundle", "wide", "bundle-plain")


def sweep_case(seed: int):
    """The sweep's case of a seed: the three groups in turn."""
    return make_light_case(SWEEP_GROUPS[seed % 3], seed)


def worker_sweep_expectation(seed: int) -> dict:
    """For a worker process that never uses the device: the expectation of sweep_case(seed)."""
    import oraclelib

    sd, cfg, _ = sweep_case(seed)
    return expected_light(oraclelib.Oracle(), sd, cfg)
