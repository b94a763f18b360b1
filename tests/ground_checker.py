"""Expected values of the ground-shadow planes (mcrt_render_ground & co), from the CPU oracle alone — a helper, not a test.

Per pixel the ray is ``layers_checker.pixel_rays`` (``oracle.camera_ray`` at the pixel centre).  Everything after it is formed
here in numpy float32, one rounding per operation, exactly as include/mcrt.h defines the pass:

    t = (g - o.y) / d.y                       reached iff d.y != 0 and t > 0 and t <= FLT_MAX
    P = (o.x + d.x * t, g, o.z + d.z * t)
    seed = seed_cast(P.x * 12345 + P.y * 67890 + P.z * 11111)          summed left to right
    visibility = oracle.soft_shadow(P, (0, 1, 0), S, seed)             S = shadowSamples if softShadows and > 1 else 1

and 1.0 / FLT_MAX / 0 for visibility / distance / matte where the ray does not reach the plane."""
from __future__ import annotations

import functools

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import layers_checker as L

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
PLANES = ("visibility", "distance", "matte")
UP = np.array([0.0, 1.0, 0.0], f32)


def samples_of(cfg) -> int:
    return int(cfg.shadowSamples) if cfg.softShadows and cfg.shadowSamples > 1 else 1


def plane_points(rays: np.ndarray, ground_y) -> tuple:
    """rays (n, 6) float32 → (reached (n,) bool, t (n,) float32, P (n, 3) float32, seed sums (n,) float32)."""
    g = f32(ground_y)
    o, d = rays[:, :3].astype(f32), rays[:, 3:].astype(f32)
    with np.errstate(all="ignore"):
        t = (g - o[:, 1]) / d[:, 1]
        reached = (d[:, 1] != 0) & (t > 0) & (t <= FLT_MAX)
        P = np.stack([o[:, 0] + d[:, 0] * t, np.full(len(t), g, f32), o[:, 2] + d[:, 2] * t], axis=1)
        sums = (P[:, 0] * f32(12345.0) + P[:, 1] * f32(67890.0)) + P[:, 2] * f32(11111.0)
    assert t.dtype == f32 and P.dtype == f32 and sums.dtype == f32
    return reached, t, P, sums


def matte_of(visibility: np.ndarray) -> np.ndarray:
    """(uint8_t)(clamp(1.0f - visibility, 0, 1) * 255.0f + 0.5f), in float32."""
    a = np.clip(f32(1.0) - visibility.astype(f32), f32(0.0), f32(1.0)) * f32(255.0) + f32(0.5)
    assert a.dtype == f32
    return a.astype(np.uint8)


def visibility_at(oracle, sd, P: np.ndarray, sums: np.ndarray, samples: int) -> np.ndarray:
    """oracle.soft_shadow at the points P (n, 3) with the seeds of the sums (n,)."""
    out = np.empty(len(P), f32)
    for i in range(len(P)):
        out[i] = oracle.soft_shadow(sd.ptr, P[i], UP, samples, oracle.seed_cast(float(sums[i])))
    return out


def expected_ground(oracle, sd, cfg, ground_y, only=None) -> dict:
    """{"visibility", "distance" (H, W) float32, "matte" (H, W) uint8, "reached" (H, W) bool, "seed" (H, W) uint32}.
    only: a (H, W) bool mask of the pixels whose visibility is wanted (the others keep 1.0) — for large frames."""
    w, h = cfg.width, cfg.height
    rays = L.pixel_rays(oracle, sd.ptr, w, h)
    reached, t, P, sums = plane_points(rays, ground_y)
    vis = np.ones(w * h, f32)
    want = reached if only is None else (reached & only.reshape(-1))
    idx = np.flatnonzero(want)
    vis[idx] = visibility_at(oracle, sd, P[idx], sums[idx], samples_of(cfg))
    seeds = np.zeros(w * h, np.uint32)
    for i in np.flatnonzero(reached):
        seeds[i] = oracle.seed_cast(float(sums[i]))
    return {"visibility": vis.reshape(h, w), "distance": np.where(reached, t, FLT_MAX).astype(f32).reshape(h, w),
            "matte": matte_of(vis).reshape(h, w), "reached": reached.reshape(h, w), "seed": seeds.reshape(h, w)}


def counts(exp: dict) -> tuple:
    """(reached, dark, penumbra) pixels of an expectation."""
    v, r = exp["visibility"], exp["reached"]
    return int(r.sum()), int((r & (v == 0)).sum()), int((r & (v > 0) & (v < 1)).sum())


def _frozen(exp: dict) -> dict:
    for a in exp.values():
        a.setflags(write=False)
    return exp


def set_light(sd, position=None, radius=None):
    if position is not None:
        for k in range(3):
            sd.desc.light_position[k] = position[k]
    if radius is not None:
        sd.desc.light_radius = radius
    return sd


@functools.lru_cache(maxsize=None)
def skin_expectation(name, ground_y=0.0, soft=True, samples=8):
    """(scene description, Config, expectation) of one of layers_checker.SKIN_CASES — computed once per session, never modified."""
    import oraclelib

    kind, pose, camera, w, h, tile = L.SKIN_CASES[name]
    sd = L.skin_case(kind, pose, camera)
    cfg = abi.Config(width=w, height=h, tileSize=tile, softShadows=soft, shadowSamples=samples)
    return sd, cfg, _frozen(expected_ground(oraclelib.Oracle(), sd, cfg, ground_y))


@functools.lru_cache(maxsize=None)
def orbit_expectation(pose, camera, w, h, light=None, radius=None, ground_y=0.0, soft=True, samples=8, tile=32):
    """The unique S64 skin at a built-in pose on an orbit camera (yaw, pitch, distance), optionally with another light."""
    import oraclelib

    sd = set_light(L.skin_case("S64", pose, camera), light, radius)
    cfg = abi.Config(width=w, height=h, tileSize=tile, softShadows=soft, shadowSamples=samples)
    return sd, cfg, _frozen(expected_ground(oraclelib.Oracle(), sd, cfg, ground_y))


@functools.lru_cache(maxsize=None)
def box_expectation(name):
    """One of layers_checker.BOX_CASES at its own floor (mcrt_scene_floor)."""
    import oraclelib

    sc, w, h, tile = L.box_scene(name)
    sd = M.SceneDesc(sc)
    cfg = abi.Config(width=w, height=h, tileSize=tile)
    floor = M.scene_floor(sd)
    return sd, cfg, floor, _frozen(expected_ground(oraclelib.Oracle(), sd, cfg, floor))


def assert_ground_equal(got: dict, exp: dict, what=""):
    """Bit for bit, for the planes `got` holds."""
    import scenes

    for k in got:
        if k == "matte":
            bad = np.argwhere(got[k] != exp[k])
            assert len(bad) == 0, f"{what} matte: {len(bad)} pixels differ; first (y, x) = {tuple(bad[0])}: {got[k][tuple(bad[0])]} vs {exp[k][tuple(bad[0])]}"
        else:
            scenes.assert_bit_equal(got[k], exp[k], f"{what} {k}")
