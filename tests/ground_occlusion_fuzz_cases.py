"""Seeded random cases for the ground-occlusion pass (mcrt_render_ground_occlusion & co) of the HIP-vs-oracle parity sweep
(tools/gpu_fuzz.py, mode ground_occlusion) and its fixed-seed run (tests/test_gpu_ground_occlusion_fuzz.py,
tests/test_ground_occlusion_fuzz_cases.py).  Every draw comes from a generator of its own, so the seeds of the other generators
keep their meaning.

make_case(seed)  -> (scene description, Config, ground height, description, classes)
make_batch(seed) -> (scene descriptions, Config, ground heights, description): 2 ... 5 scenes of make_case under ONE config, each at
                    its own plane

A case draws
  scene    a skin (S64 / S32, a built-in pose, free pose angles or none) or a many-mesh box scene of big_scene_cases — its count group
           (un-posed boxes: 48, 62 ... 66, 70 meshes, null textures among them) or its posed group (63, 64, 65, 80 meshes, a posed
           figure among boxes) — a third of the box scenes with an EMPTY texture (0 x 0) put on one face
  scale    1, or 10^-3 ... 10^3: vertices, pivots, camera, light, plane and radius alike
  plane    at the scene's lowest vertex, below it, inside the scene, above it
  camera   on an orbit about the scene's middle: above the plane looking down, below the plane looking up, or grazing it (at the
           plane's height within a hundredth of the scene's height, looking along it)
  A        1, 2, 3, 8, 64, 113
  radius   0, tiny (a thousandth of the scene's height), the reference's 3 (scaled), larger than the scene
  frame    1 ... 96 pixels a side (at most 32 x 24 where the radius is large or A >= 64, which keeps the oracle quick), tiles of 4, 7, 8,
           16, 32

`classes` names what the case is, for the coverage self-test.  No device is used here."""
from __future__ import annotations

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import big_scene_cases as BIG

f32 = np.float32
A_VALUES = (1, 2, 3, 8, 64, 113)
RADII = ("zero", "tiny", "three", "large")
PLANES = ("at the floor", "below the scene", "inside the scene", "above the scene")
CAMERAS = ("above the plane", "below the plane", "grazing the plane")
SCENES = ("skin un-posed", "skin posed", "boxes un-posed", "boxes posed")
TILES = (4, 7, 8, 16, 32)
COUNT_SLOTS = (0, 1, 2, 3, 4, 5, 6)  # big_scene_cases.COUNTS: 48, 62, 63, 64, 65, 66, 70
POSED_SLOTS = (1, 2, 3, 4)           # big_scene_cases.POSED_COUNTS: 63, 64, 65, 80
# every class the first 200 seeds must hit (tests/test_ground_occlusion_fuzz_cases.py)
CLASSES = (SCENES + PLANES + CAMERAS + tuple(f"A = {a}" for a in A_VALUES) + tuple(f"radius {r}" for r in RADII) +
           ("more than 64 meshes", "at most 64 meshes of a box scene", "null texture", "empty texture", "scale below 0.1", "scale above 10",
            "odd width", "width not a multiple of 4", "a side of at most 4 pixels", "a side of 90 or more", "tile 4", "tile 32", "tile 7"))


def _skin(g):
    kind = ["S64", "S64", "S32"][g.integers(0, 3)]
    skin = M.synthetic_skin(kind, seed=int(g.integers(1, 1 << 30)))
    r = g.random()
    if r < 0.3:
        pose, name = np.zeros(12, f32), "no pose"
    elif r < 0.6:
        i = int(g.integers(1, len(M.getBuiltinPoses())))
        pose, name = np.asarray(M.getBuiltinPoses()[i], f32), f"built-in pose {i}"
    else:
        pose = np.where(g.random(12) < 0.5, g.uniform(-120, 120, 12), 0.0).astype(f32)
        name = f"pose {np.round(pose, 1).tolist()}"
    sc = abi.scene_from_numpy(M.MeshBuilder.buildScene(skin, pose).to_numpy())
    posed = any(m.hasRotation and (abs(m.rotX) > 0.01 or abs(m.rotZ) > 0.01) for m in sc.meshes)
    return sc, f"{kind} {name}", "skin posed" if posed else "skin un-posed"


def _boxes(g):
    if g.random() < 0.5:
        slot, group, table = int(g.choice(COUNT_SLOTS)), "count", BIG.COUNTS
    else:
        slot, group, table = int(g.choice(POSED_SLOTS)), "posed", BIG.POSED_COUNTS
    sub = 3 * (len(table) * int(g.integers(0, 1000)) + slot)
    sd, _, _, _ = BIG.make_big_case(sub, group)
    sc = abi.scene_from_numpy(sd.to_numpy())
    assert len(sc.meshes) == table[slot]
    return sc, f"big {group} seed {sub} ({len(sc.meshes)} meshes)", "boxes posed" if group == "posed" else "boxes un-posed"


def _bounds(sc) -> tuple:
    v = np.concatenate([np.asarray(m.triangles, np.float64).reshape(-1, 3) for m in sc.meshes if len(m.triangles)])
    return v.min(axis=0), v.max(axis=0)


def _scale_scene(sc, scale: float) -> None:
    s32 = f32(scale)
    for m in sc.meshes:
        m.triangles = (np.asarray(m.triangles, f32) * s32).astype(f32)
        if m.localTriangles is not None:
            m.localTriangles = (np.asarray(m.localTriangles, f32) * s32).astype(f32)
        m.pivot = tuple(float(f32(x) * s32) for x in m.pivot)
    sc.light_position = tuple(float(f32(x) * s32) for x in sc.light_position)
    sc.light_radius = float(f32(sc.light_radius) * s32)


def make_case(seed: int):
    g = np.random.default_rng(seed ^ 0x60CC0000)
    classes = set()
    sc, what, scene_class = _skin(g) if g.random() < 0.5 else _boxes(g)
    classes.add(scene_class)
    boxes = scene_class.startswith("boxes")
    if boxes:
        classes.add("more than 64 meshes" if len(sc.meshes) > 64 else "at most 64 meshes of a box scene")
        if g.random() < 0.34:  # a TextureRegion without pixels on one face of one mesh
            which = int(g.integers(0, len(sc.meshes)))
            m = sc.meshes[which]
            empty = abi.Texture(0, 0, np.zeros((0, 4), f32))
            face = int(g.integers(0, 6))
            tex = list(m.tri_texture)
            tex[2 * face] = tex[2 * face + 1] = empty
            m.tri_texture = tex
            what += f", an empty texture on a face of mesh {which}"
    if any(t is None for m in sc.meshes for t in m.tri_texture):
        classes.add("null texture")
    if any(t is not None and (t.width <= 0 or t.height <= 0 or len(t.pixels) == 0) for m in sc.meshes for t in m.tri_texture):
        classes.add("empty texture")
    scale = 1.0 if g.random() < 0.55 else float(10.0 ** g.uniform(-3, 3))
    if scale != 1.0:
        _scale_scene(sc, scale)
    if scale < 0.1:
        classes.add("scale below 0.1")
    if scale > 10:
        classes.add("scale above 10")
    lo, hi = _bounds(sc)
    H = max(float(hi[1] - lo[1]), 1e-6)
    middle = 0.5 * (lo + hi)
    span = float(max(hi[0] - lo[0], hi[2] - lo[2], H))
    plane = PLANES[int(g.integers(0, 4))]
    classes.add(plane)
    ground = float(f32({"at the floor": lo[1], "below the scene": lo[1] - g.uniform(0.02, 0.4) * H, "inside the scene": lo[1] + g.uniform(0.05, 0.6) * H,
                        "above the scene": hi[1] + g.uniform(0.01, 0.2) * H}[plane]))
    # A, radius and the frame
    A = int(A_VALUES[int(g.integers(0, len(A_VALUES)))])
    rclass = RADII[int(g.integers(0, 4))]
    radius = float(f32({"zero": 0.0, "tiny": 1e-3 * H, "three": 3.0 * scale, "large": g.uniform(1.2, 2.5) * max(H, span)}[rclass]))
    classes.update({f"A = {A}", f"radius {rclass}"})
    heavy = rclass == "large" or A >= 64
    r = g.random()
    if r < 0.12:
        w, h = int(g.integers(1, 5)), int(g.integers(1, 9))
    elif r < 0.24 and not heavy:
        w, h = int(g.integers(90, 97)), int(g.integers(40, 97))
    else:
        w, h = int(g.integers(9, 33 if heavy else 72)), int(g.integers(7, 25 if heavy else 56))
    tile = int(TILES[int(g.integers(0, len(TILES)))])
    if w % 2:
        classes.add("odd width")
    if w % 4:
        classes.add("width not a multiple of 4")
    if min(w, h) <= 4:
        classes.add("a side of at most 4 pixels")
    if max(w, h) >= 90:
        classes.add("a side of 90 or more")
    if tile in (4, 7, 32):
        classes.add(f"tile {tile}")
    # the camera, on an orbit about the middle of the scene
    camera = CAMERAS[int(g.choice([0, 0, 0, 1, 2]))]
    classes.add(camera)
    yaw, dist = g.uniform(0, 2 * np.pi), g.uniform(1.2, 2.6) * max(span, H)
    if camera == "above the plane":
        pitch = g.uniform(0.15, 1.4)
        cy = max(middle[1] + dist * np.sin(pitch), ground + 0.05 * H)
        target = (middle[0], min(middle[1], cy - 0.02 * H) if g.random() < 0.5 else ground, middle[2])
    elif camera == "below the plane":
        pitch = 0.0
        cy = ground - g.uniform(0.05, 1.5) * H
        target = (middle[0], max(middle[1], ground + 0.2 * H), middle[2])
    else:
        pitch = 0.0
        cy = ground + g.uniform(-0.01, 0.01) * H
        target = (middle[0], cy + g.uniform(-0.01, 0.01) * H, middle[2])
    horizontal = dist * (np.cos(pitch) if camera == "above the plane" else 1.0)
    sc.camera_position = (float(middle[0] + horizontal * np.sin(yaw)), float(cy), float(middle[2] + horizontal * np.cos(yaw)))
    sc.camera_target = tuple(float(x) for x in target)
    sc.camera_up = (0.0, 1.0, 0.0)
    sc.camera_fov = float(g.uniform(25, 75))
    cfg = abi.Config(width=w, height=h, tileSize=tile, aoSamples=A, aoRadius=radius)
    what = (f"ground-occlusion seed {seed}: {what} scale {scale:.4g} plane {ground!r} ({plane}) camera {np.round(sc.camera_position, 4).tolist()} ({camera}) "
            f"fov {sc.camera_fov:.1f} A {A} radius {radius!r} ({rclass}) {w}x{h} tile {tile}")
    return M.SceneDesc(sc), cfg, ground, what, classes


def make_batch(seed: int):
    g = np.random.default_rng(seed ^ 0x60CD0000)
    n = int(g.integers(2, 6))
    first = int(g.integers(0, 1 << 20))
    cases = [make_case(first + 13 * i) for i in range(n)]
    _, cfg, _, _, _ = cases[0]
    w, h = min(cfg.width, 40), min(cfg.height, 30)
    shared = abi.Config(width=w, height=h, tileSize=cfg.tileSize, aoSamples=min(cfg.aoSamples, 8) if n > 3 else cfg.aoSamples, aoRadius=cfg.aoRadius)
    what = f"ground-occlusion batch seed {seed}: cases {[first + 13 * i for i in range(n)]} under A {shared.aoSamples} radius {shared.aoRadius!r} {w}x{h} tile {shared.tileSize}"
    return [c[0] for c in cases], shared, [c[2] for c in cases], what
