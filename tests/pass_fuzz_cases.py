"""Seeded random cases for the scene-only passes — geometry layers, ground shadow, ground reflection — of the HIP-vs-oracle
parity sweep (tools/gpu_fuzz.py, modes ground / reflection / layers / long-shadow / far-plane) and its fixed-seed run
(tests/test_gpu_pass_fuzz.py, tests/test_pass_fuzz_cases.py).  Every new draw comes from a generator of its own, so the seeds of
fuzz_cases.py keep their meaning.

A  make_pass_case        the scenes of fuzz_cases.make_bundle_case / make_wide_case (lights near, inside and grazing boxes, texel
                         grids of every density, flat boxes, scenes scaled by 1e-5 ... 1e6 or moved up to 3e6 away) under a plane
                         at the scene's floor, a hair below it, well below it, through the scene or above it
B  make_long_shadow_case the figure under a light below its top, so that its shadow never ends, seen along that shadow through a
                         narrow lens: ground points 200 ... 30 000 from the origin, where one ulp of a coordinate is larger than
                         FlatHeader::mask_slack, whose magnitude knows the camera, the light and the vertices only
C  make_far_plane_case   a figure or boxes at scale 1, the plane 10 ... 10 000 scene heights below them (the plane's height is no
                         part of that magnitude either), the light clear above, the camera above and tilted down at the shadow
                         or zoomed in on the scene's mirror image

Each returns (scene description, Config, ground height, description)."""
from __future__ import annotations

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import fuzz_cases

f32 = np.float32
K_MASK_SLACK = 4e-5  # flat_scene.h: kMaskSlack


def y_range(sd) -> tuple:
    """(least, greatest) y over all meshes' world triangles, as floats."""
    ys = [np.asarray(m["triangles"], f32).reshape(-1, 3)[:, 1] for m in sd.to_numpy()["meshes"] if len(m["triangles"])]
    ys = np.concatenate(ys)
    return float(ys.min()), float(ys.max())


def make_pass_case(seed: int, wide: bool = False, lift_light: bool = False):
    """lift_light: the same case with its light raised clear above every mesh (a draw of its own: the case without it keeps its
    meaning) — the drawn lights are almost never there, and ground_tile_mask bounds a mesh's shadow under such a light only."""
    sd, bcfg, what = fuzz_cases.make_bundle_case(seed, wide)
    g = np.random.default_rng(seed ^ 0xF100)
    f = [0.0, 0.0, -0.02, -0.5, 0.15, 0.4, 1.1][g.integers(0, 7)]
    width = int(g.integers(17, 57))
    height = int(g.integers(13, 41))
    lo, hi = y_range(sd)
    ground = float(f32(lo + f * (hi - lo)))
    cfg = abi.Config(width=width, height=height, tileSize=bcfg.tileSize, softShadows=bcfg.softShadows, shadowSamples=bcfg.shadowSamples,
                     maxBounces=max(1, bcfg.maxBounces))
    lifted = ""
    if lift_light:
        gl = np.random.default_rng(seed ^ 0x11F7)
        base = max(hi, ground)
        # (the mask asks for a clearance of 64 slacks — of 7.7e3 for a scene moved 3e6 away)
        ly = (base + ((hi - lo) + (base - ground)) * gl.uniform(0.5, 3.0) + 1.1 * float(sd.desc.light_radius) + 1e-3 * max(abs(lo), abs(hi), abs(ground))
              + 80.0 * mask_slack(sd.to_numpy()))
        sd.desc.light_position[1] = max(float(ly), float(sd.desc.light_position[1]))  # raised, never lowered
        lifted = f" light lifted to y = {float(sd.desc.light_position[1])!r}"
    return sd, cfg, ground, f"pass seed {seed}{' wide' if wide else ''}{lifted}: plane {ground!r} (f {f}) {width}x{height}; {what}"


def make_wide_pass_case(seed: int):
    return make_pass_case(seed, wide=True)


def _place(sd, light, radius, cam, target, fov=None):
    d = sd.desc
    for k in range(3):
        d.light_position[k] = float(light[k])
        d.camera_position[k] = float(cam[k])
        d.camera_target[k] = float(target[k])
    d.light_radius = float(radius)
    if fov is not None:
        d.camera_fov = float(fov)
    return sd


def make_long_shadow_case(seed: int):
    g = np.random.default_rng(seed ^ 0x10E5)
    kind = ["S64", "S64", "S32"][g.integers(0, 3)]
    pose = int(g.integers(0, len(M.getBuiltinPoses())))
    sd = M.MeshBuilder.buildScene(M.synthetic_skin(kind, seed=int(g.integers(1, 1 << 30))), M.getBuiltinPoses()[pose])
    a = g.uniform(0, 2 * np.pi)
    r = g.uniform(12, 70)
    ly = g.uniform(2, 28)
    light = (r * np.sin(a), ly, r * np.cos(a))  # below the figure's top: the shadow never ends
    radius = float([0.0, 0.05, 0.5, 3.0, 3.0][g.integers(0, 5)])
    ground = float([0.0, 0.0, -0.5, -3.0][g.integers(0, 4)])
    D = 10.0 ** g.uniform(2.3, 4.5)
    sa = a + np.pi + g.uniform(-0.05, 0.05)
    ca = a + g.uniform(-0.5, 0.5)
    dist = g.uniform(30, 80)
    ch = g.uniform(3, 40)
    cam = (dist * np.sin(ca), ch, dist * np.cos(ca))
    target = (D * np.sin(sa), ground, D * np.cos(sa))  # a ground point 200 ... 30 000 out along the shadow
    fov = g.uniform(2, 30)
    _place(sd, light, radius, cam, target, fov)
    width = int(g.integers(40, 97))
    height = int(g.integers(24, 65))
    tile = int([8, 16, 32][g.integers(0, 3)])
    samples = int([2, 3, 8, 8, 16][g.integers(0, 5)])
    cfg = abi.Config(width=width, height=height, tileSize=tile, shadowSamples=samples)
    what = (f"long-shadow seed {seed}: {kind} pose {pose} light {np.round(light, 3).tolist()} r {radius} plane {ground} target {D:.1f} out "
            f"camera {np.round(cam, 3).tolist()} fov {fov:.2f} {width}x{height} tile {tile} S {samples}")
    return sd, cfg, ground, what


def make_far_plane_case(seed: int):
    import scenes

    g = np.random.default_rng(seed ^ 0xFA70)
    if g.random() < 0.5:
        meshes, _ = fuzz_cases._box_scene(g)
        sd = M.SceneDesc(scenes.simple_scene(meshes))
        what = f"boxes x{len(meshes)}"
    else:
        kind = ["S64", "S64", "S32"][g.integers(0, 3)]
        pose = int(g.integers(0, len(M.getBuiltinPoses())))
        sd = M.MeshBuilder.buildScene(M.synthetic_skin(kind, seed=int(g.integers(1, 1 << 30))), M.getBuiltinPoses()[pose])
        what = f"{kind} pose {pose}"
    v = np.concatenate([np.asarray(m["triangles"], np.float64).reshape(-1, 3) for m in sd.to_numpy()["meshes"]])
    blo, bhi = v.min(axis=0), v.max(axis=0)
    centre, H = 0.5 * (blo + bhi), max(float(bhi[1] - blo[1]), 1e-3)
    span = max(float(bhi[0] - blo[0]), float(bhi[2] - blo[2]), H)
    depth = H * 10.0 ** g.uniform(1, 4)  # 10 ... 10 000 scene heights
    ground = float(f32(blo[1] - depth))
    lift = span * g.uniform(0.6, 3.0)  # the light's height above the scene's top
    light = np.asarray([centre[0] + span * g.uniform(-0.7, 0.7), bhi[1] + lift, centre[2] + span * g.uniform(-0.7, 0.7)])
    radius = float([0.0, 0.01, 0.05, 0.05, 0.2, 0.5][g.integers(0, 6)] * span)
    # the shadow of the scene's bounds on the plane, thrown from the light's centre
    corners = np.asarray([[(blo, bhi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
    s = (light[1] - ground) / (light[1] - corners[:, 1])
    foot = light[None, :] + (corners - light[None, :]) * s[:, None]
    fc = 0.5 * (foot.min(axis=0) + foot.max(axis=0))
    fr = 0.5 * float(np.linalg.norm(foot.max(axis=0) - foot.min(axis=0)))
    ang = g.uniform(0, 2 * np.pi)
    cam = np.asarray([centre[0] + span * g.uniform(0.5, 4) * np.sin(ang), bhi[1] + span * g.uniform(0.5, 6), centre[2] + span * g.uniform(0.5, 4) * np.cos(ang)])
    if g.random() < 0.4:  # zoomed in on the scene's mirror image in the plane (it lies within the shadow's directions)
        target = np.asarray([centre[0], 2.0 * ground - centre[1], centre[2]])
        size = 0.5 * float(np.linalg.norm(bhi - blo)) * g.uniform(1.0, 3.0)
        view = "mirror image"
    else:  # the shadow, from within it to all of it with lit ground around
        target = np.asarray([fc[0] + fr * g.uniform(-0.6, 0.6), ground, fc[2] + fr * g.uniform(-0.6, 0.6)])
        size = fr * g.uniform(0.3, 2.0)
        view = "shadow"
    fov = float(np.clip(np.degrees(2.0 * np.arctan(size / np.linalg.norm(target - cam))), 1e-3, 120.0))
    _place(sd, light, radius, cam, target, fov)
    width = int(g.integers(24, 65))
    height = int(g.integers(16, 49))
    tile = int([8, 16, 32][g.integers(0, 3)])
    samples = int([2, 3, 8, 8, 16][g.integers(0, 5)])
    cfg = abi.Config(width=width, height=height, tileSize=tile, shadowSamples=samples, maxBounces=int([1, 2, 3][g.integers(0, 3)]))
    what = (f"far-plane seed {seed}: {what} plane {ground!r} ({depth / H:.0f} heights down) light {np.round(light, 3).tolist()} r {radius:.4f} "
            f"camera {np.round(cam, 3).tolist()} at the {view} fov {fov:.4f} {width}x{height} tile {tile} S {samples} bounces {cfg.maxBounces}")
    return sd, cfg, ground, what


def make_lifted_case(seed: int):
    return make_pass_case(seed, lift_light=True)


def make_wide_lifted_case(seed: int):
    return make_pass_case(seed, wide=True, lift_light=True)


GROUPS = {"bundle": make_pass_case, "wide": make_wide_pass_case, "bundle-lifted": make_lifted_case, "wide-lifted": make_wide_lifted_case, "long-shadow": make_long_shadow_case, "far-plane": make_far_plane_case}


# ---- what a case exercises, from the scene description alone ---------------------------------------------------------
def mask_slack(scene_np) -> float:
    """FlatHeader::mask_slack as flatten.cpp forms it: kMaskSlack x the largest coordinate of camera, light and vertices."""
    mag = max(float(np.abs(scene_np["camera_position"]).max()), float(np.abs(scene_np["light_position"]).max()), abs(float(scene_np["light_radius"])))
    for m in scene_np["meshes"]:
        for k in ("triangles", "localTriangles"):
            if len(m[k]):
                mag = max(mag, float(np.abs(np.asarray(m[k], np.float64)).max()))
        if m["hasRotation"]:
            mag = max(mag, float(np.abs(m["pivot"]).max()))
    return K_MASK_SLACK * mag


def light_clear_above_every_mesh(sd, cfg, ground) -> bool:
    """ground_tile_mask's own criterion for bounding a mesh's shadow, for every mesh of the scene: with low = L.y - Rb the lowest
    light sample, h = low - (g + 1e-3) and c = low - (the top of the mesh's bound), c > 0.01 h and c > 64 mask_slack (which
    is > 0) — the culling branch of the mask runs for that mesh, not its fall-back 'keep the mesh'.  The bound of a posed mesh is
    its padded sphere.  (Per TILE the kernel asks besides that the four corner rays reach the plane with |d.y| >= 1e-2; that is
    a matter of the camera and is not restated here.)"""
    s = sd.to_numpy()
    slack = mask_slack(s)
    S = int(cfg.shadowSamples) if cfg.softShadows and cfg.shadowSamples > 1 else 1
    R = float(s["light_radius"]) if S > 1 and not float(s["light_radius"]) < 1e-4 else 0.0
    low = float(s["light_position"][1]) - (R * 1.001 + slack)
    h = low - (float(ground) + 1e-3)
    if not np.isfinite(slack) or not h > 0 or not 0 < len(s["meshes"]) < 64:
        return False
    for m in s["meshes"]:
        v = np.asarray(m["triangles"], np.float64).reshape(-1, 3)
        if not len(v):
            continue
        top = float(v[:, 1].max())
        if m["hasRotation"]:
            loc = np.asarray(m["localTriangles"], np.float64).reshape(-1, 3)
            r = 0.5 * float(np.linalg.norm(loc.max(axis=0) - loc.min(axis=0))) * 1.01 + 25.0 * slack
            top = float(np.unique(v, axis=0).mean(axis=0)[1]) + r
        c = low - top
        if not (c > 0.01 * h and c > 64.0 * slack):
            return False
    return True


def far_counts(oracle, sd, cfg, ground, exp, beyond=1e3) -> tuple:
    """(dark, penumbra) pixels of a ground expectation whose plane point has max(|P.x|, |P.z|) > beyond."""
    import ground_checker as G
    import layers_checker as L

    _, _, P, _ = G.plane_points(L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height), ground)
    with np.errstate(all="ignore"):
        far = (np.maximum(np.abs(P[:, 0]), np.abs(P[:, 2])) > f32(beyond)).reshape(cfg.height, cfg.width)
    v, r = exp["visibility"], exp["reached"]
    return int((r & far & (v == 0)).sum()), int((r & far & (v > 0) & (v < 1)).sum())


# ---- the fixed blocks of 16 seeds of the suite -----------------------------------------------------------------------
# What the ORACLE holds over a block, measured on the CPU: ground (reached, dark, penumbra), reflection (hits, chains with a
# second-level hit, level-1 hits in the penumbra), layer hits, and for the A groups the ground totals of the same cases under
# the lifted light.  exact: the block's totals are asserted as they stand; otherwise every total must reach half of what is
# written here.  A frame of constants passes neither.
BLOCKS = {
    ("bundle", 7000): dict(exact=True, ground=(12701, 2241, 3017), reflection=(691, 456, 65), layers=3859, lifted=(12701, 571, 534)),
    ("bundle", 7016): dict(exact=False, ground=(12159, 3619, 2027), reflection=(1238, 932, 143), layers=4601, lifted=(12159, 1078, 155)),
    ("bundle", 7032): dict(exact=False, ground=(12728, 2246, 2491), reflection=(1817, 217, 500), layers=3192, lifted=(12728, 503, 89)),
    ("wide", 9000): dict(exact=True, ground=(10351, 851, 830), reflection=(166, 81, 34), layers=2983, lifted=(10351, 176, 68)),
    ("wide", 9016): dict(exact=False, ground=(12037, 1452, 598), reflection=(542, 508, 4), layers=2549, lifted=(12037, 583, 23)),
    ("wide", 9032): dict(exact=False, ground=(10182, 2431, 93), reflection=(442, 315, 47), layers=3699, lifted=(10182, 720, 0)),
    # far: (dark, penumbra, cases that hold either) at plane points with max(|P.x|, |P.z|) > 1e3; no floor is claimed for the
    # reflection: the mirrored figure lies near the camera, off these frames
    ("long-shadow", 12000): dict(exact=True, ground=(24507, 11383, 3287), reflection=(0, 0, 0), far=(3275, 504, 15)),
    ("long-shadow", 12016): dict(exact=False, ground=(31971, 20065, 2471), reflection=(66, 15, 2), far=(3352, 638, 12)),
    ("long-shadow", 12032): dict(exact=False, ground=(28121, 16683, 1108), reflection=(0, 0, 0), far=(5497, 234, 15)),
    # every block: at least 100 dark, 100 penumbra and 100 reflected hits besides
    ("far-plane", 15000): dict(exact=False, ground=(22638, 3023, 4517), reflection=(540, 215, 5)),
    ("far-plane", 15016): dict(exact=False, ground=(21826, 4440, 2844), reflection=(617, 93, 5)),
    ("far-plane", 15032): dict(exact=False, ground=(20786, 1701, 2266), reflection=(413, 4, 1)),
}
BLOCK_IDS = [f"{g}-{s}" for g, s in BLOCKS]
A_BLOCKS = [k for k in BLOCKS if k[0] in ("bundle", "wide")]
A_BLOCK_IDS = [f"{g}-{s}" for g, s in A_BLOCKS]


def assert_floor(total, measured, exact, what):
    total, measured = tuple(int(t) for t in np.atleast_1d(total)), tuple(int(m) for m in np.atleast_1d(measured))
    print(what, "oracle totals", total, "measured", measured, "(exact)" if exact else "(floor: half)")
    if exact:
        assert total == measured, f"{what}: the oracle holds {total}, not {measured}: the generator differs"
    else:
        assert all(2 * t >= m for t, m in zip(total, measured)), f"{what}: the oracle holds {total}, less than half of {measured}"


def block_cases(group, first, count=16) -> list:
    return [GROUPS[group](seed) for seed in range(first, first + count)]


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        exps = make()
        for e in exps:
            for a in e.values():
                a.setflags(write=False)
        _CACHE[key] = exps
    return _CACHE[key]


def ground_expectations(oracle, group, first) -> list:
    """The block's ground expectations, computed once per session and never modified."""
    import ground_checker as G

    return _cached(("ground", group, first), lambda: [G.expected_ground(oracle, sd, cfg, g) for sd, cfg, g, _ in block_cases(group, first)])


def reflection_expectations(oracle, group, first) -> list:
    import reflection_checker as R

    return _cached(("reflection", group, first), lambda: [R.expected_reflection(oracle, sd, cfg, g) for sd, cfg, g, _ in block_cases(group, first)])


def surface_expectations(oracle, group, first) -> list:
    import layers_checker as L

    return _cached(("layers", group, first), lambda: [L.expected_surfaces(oracle, sd, cfg.width, cfg.height) for sd, cfg, _, _ in block_cases(group, first)])


def check_ground_block(oracle, group, first) -> list:
    """The block's ground expectations after their floors: the totals of BLOCKS, the miss constants, for B the far pixels, for
    C the 100 dark and penumbra pixels."""
    import ground_checker as G

    spec, cases, exps = BLOCKS[(group, first)], block_cases(group, first), ground_expectations(oracle, group, first)
    for e in exps:
        miss = ~e["reached"]
        assert (e["visibility"][miss] == 1.0).all() and (e["distance"][miss] == G.FLT_MAX).all() and (e["matte"][miss] == 0).all()
        assert (e["matte"] == G.matte_of(e["visibility"])).all()
    total = np.sum([G.counts(e) for e in exps], axis=0)
    assert_floor(total, spec["ground"], spec["exact"], f"{group} {first} ground (reached, dark, penumbra)")
    if "far" in spec:
        far = np.asarray([far_counts(oracle, sd, cfg, g, e) for (sd, cfg, g, _), e in zip(cases, exps)])
        assert_floor((far[:, 0].sum(), far[:, 1].sum(), (far.sum(axis=1) > 0).sum()), spec["far"], spec["exact"],
                     f"{group} {first} ground beyond 1e3 (dark, penumbra, cases)")
    if group == "far-plane":
        assert total[1] >= 100 and total[2] >= 100
    return exps


def check_reflection_block(oracle, group, first) -> list:
    import reflection_checker as R

    spec, exps = BLOCKS[(group, first)], reflection_expectations(oracle, group, first)
    for e in exps:
        R.assert_miss_constants(e)
    total = np.sum([R.counts(e)[1:] for e in exps], axis=0)
    assert_floor(total, spec["reflection"], spec["exact"], f"{group} {first} reflection (hits, second-level, penumbra hits)")
    if group == "far-plane":
        assert total[0] >= 100
    return exps


def check_surface_block(oracle, group, first) -> list:
    spec, exps = BLOCKS[(group, first)], surface_expectations(oracle, group, first)
    assert_floor(sum(int(e["hit"].sum()) for e in exps), spec["layers"], spec["exact"], f"{group} {first} layer hits")
    return exps


def check_lifted_block(oracle, group, first) -> tuple:
    """(cases, expectations) of an A block under the lifted light, after their floor, and after the count of ground cases —
    these and the block's own — whose light is clear above every mesh: at least a third."""
    import ground_checker as G

    spec, cases = BLOCKS[(group, first)], block_cases(group + "-lifted", first)
    exps = ground_expectations(oracle, group + "-lifted", first)
    assert_floor(np.sum([G.counts(e) for e in exps], axis=0), spec["lifted"], False, f"{group} {first} ground under the lifted light")
    clear = sum(light_clear_above_every_mesh(sd, cfg, g) for sd, cfg, g, _ in cases + block_cases(group, first))
    print(f"{group} {first}: the light is clear above every mesh in {clear} of {2 * len(cases)} ground cases")
    assert 3 * clear >= 2 * len(cases)
    return cases, exps
