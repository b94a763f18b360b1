"""Seeded random cases at the limits of the scene tables: many-mesh scenes around 64 meshes (the width of the candidate masks, the
end of tile culling, of the whole-bundle shadow decisions and of the first-pass groups, the start of the per-ray tail loops),
rotated meshes in every scene view, texel pools around 65 536 texels (the end of the staged alpha words), and the "general"
kernel variants on such scenes.  For tools/gpu_fuzz.py (mode big), tests/test_gpu_big_scene_fuzz.py, tests/test_big_scene_cases.py
and tests/test_oracle_vs_ref.py.  Every draw comes from a generator of its own: the seeds of the other generators keep their meaning.

make_big_case(seed, group) -> (scene description, Config, ground height, description)

count   n boxes, n = COUNTS[(seed // 3) % 12]: random sizes and positions in a volume roughly the figure's, with the ingredients of
        fuzz_cases._box_scene — nested, touching, IDENTICAL and flat boxes, null textures, texel grids of every alpha density, outer
        layers from a hair's breadth to a wide shell.  The mesh order is shuffled; then these are put in place (SPECIALS in the
        description names their indices):
          K L U I   a cluster in front of the volume, towards the camera: an inner box I, two IDENTICAL shells L and U around it
                    (the reference keeps the first mesh on equal t: wherever both are hit, the lower index is named) and a wide
                    shell K around all three.  For n > 64: K, L and I below 64 and U at 64 (n = 65) or beyond — U is a member in
                    the tail of a container below 64, the container in the tail of a member below 64, the upper half of a pair
                    that straddles 63 | 64, and an outer layer with transparent texels in the tail
          V J       for n >= 70: a shell V in the tail whose inner box J lies below 64 and in no other box
          F63 F64   for n >= 64 (n >= 66): plain boxes at index exactly 63 (64) beside the cluster, nothing between them and the
                    camera (for n = 65 mesh 64 is U, seen where K's and L's texels are transparent)
posed   the meshes of MeshBuilder.buildScene(synthetic_skin(kind, seed), pose) with free pose angles (0.005 degree entries, below
        the 0.01 degree gate, included) at random positions among k boxes, n = POSED_COUNTS[(seed // 3) % 6]; for n > 64 two rotated
        parts, one of them an outer layer, lie at an index >= 64 (n = 65 has ONE tail mesh: the rotated outer layer).  n = 64 is
        kViewLds at capacity: culling off, bundle decisions on
texels  two to eight meshes and a texel pool of exactly TEXEL_TOTALS[(seed // 3) % 6] texels: one large, partly transparent texture
        on an outer layer, small ones and a filler; the texture that holds the LAST texels of the pool lies on a shell in front
        of the camera and between light and ground, so that the last staged alpha word and the first unstaged one are read: the
        pool's last texel is opaque and the one before it transparent, and for 65 537 texels — ONE texel beyond the staged words —
        that texture is a grid of four to six texels, so the texel covers a sixth of every face or more (check_block asks every
        case of 65 536, 65 537 and 65 552 texels for such hits by itself)

(seed // 3: the sweep's seed k is a case of group k % 3, so a group's cases are 3 seeds apart — block_seeds.)  Lights as in
fuzz_cases.make_bundle_case: far, near a box, inside the bounds, on a face plane; radii 0 ... 25.  Frames at most 72 x 56.  Every
fourth case of a group gives the beauty render a general-variant config: 114 ... 160 shadow samples, AO with 114 ... 140 samples, or
9 / 12 / 17 / 20 bounces (17 and 20 exceed kMaxStack); pass_config(cfg) is the clamped config of the passes, which refuse those.

The expected scene view of a case is batch_fuzz_cases.expected_view(batch_fuzz_cases.flat_header(scene)).  No device is used here."""
from __future__ import annotations

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import batch_fuzz_cases as B
import fuzz_cases
import pass_fuzz_cases as PF

f32 = np.float32
GROUPS = ("count", "posed", "texels")
COUNTS = (48, 62, 63, 64, 65, 66, 70, 96, 128, 129, 130, 200)
POSED_COUNTS = (40, 63, 64, 65, 80, 140)
TEXEL_TOTALS = (None, 65536, 65537, 65552, -90000, 65537)  # None: 65 520 ... 65 535; -90000: about 90 000
CENTRE = np.asarray([0.0, 16.0, 0.0])
LDS_TEXEL_BUDGET = 60000  # the pool of a count / posed scene of at most 64 meshes stays below 65 536: its view is the count's
FACES = ("back", "front", "left", "right", "top", "bottom")


# ---- boxes -----------------------------------------------------------------------------------------------------------
class _Pool:
    """Counts the texels of the textures met so far (a texture object shared by faces or meshes is pooled once)."""

    def __init__(self, budget=None):
        self.seen, self.texels, self.budget = set(), 0, budget

    def new_texels(self, mesh) -> int:
        fresh = {id(t): t for t in mesh.tri_texture if t is not None and id(t) not in self.seen}
        return sum(t.width * t.height for t in fresh.values() if t.width > 0 and t.height > 0 and len(t.pixels))

    def add(self, mesh):
        self.texels += self.new_texels(mesh)
        self.seen.update(id(t) for t in mesh.tri_texture if t is not None)
        return mesh


def _grid(g, w, h, density) -> abi.Texture:
    px = g.random((w * h, 4)).astype(f32)
    px[:, 3] = (g.random(w * h) < density).astype(f32)
    return abi.Texture(w, h, px)


def _box(g, pool, centre, size, offset, outer):
    """fuzz_cases._box; where its textures would take the pool beyond its budget, the same box under one 2 x 2 texture."""
    import scenes

    m = fuzz_cases._box(g, centre, size, offset, outer)
    if pool.budget is not None and pool.texels + pool.new_texels(m) > pool.budget:
        m = scenes.build_box(_grid(g, 2, 2, 0.5 if outer else 1.0), centre, size, offset)
    return pool.add(m)


def _shell(g, pool, centre, size, offset, density, w=8, h=8):
    """An outer layer whose six faces have texel grids of their own, transparent with probability 1 - density."""
    import scenes

    return pool.add(scenes.build_box({k: _grid(g, w, h, density) for k in FACES}, centre, size, offset))


def _random_boxes(g, pool, count, lo, hi, sizes, floor_y=None) -> list:
    """`count` meshes with the ingredients of fuzz_cases._box_scene, centres in [lo, hi]."""
    meshes, placed = [], []
    if floor_y is not None and count > 4 and g.random() < 0.3:  # a floor under everything
        meshes.append(_box(g, pool, (0.0, floor_y, 0.0), (70.0, 1.0, 70.0), 0.0, False))
    while len(meshes) < count:
        c, size = g.uniform(lo, hi), g.uniform(sizes[0], sizes[1], 3)
        if placed:
            pc, ps, po = placed[g.integers(0, len(placed))]
            r = g.random()
            if r < 0.15:  # nested in a previous box
                size = ps * g.uniform(0.3, 0.8, 3)
                c = pc + (ps - size) * g.uniform(-0.5, 0.5, 3)
            elif r < 0.3:  # touching / overlapping it
                c = pc + g.uniform(-1, 1, 3) * ps
            elif r < 0.4:  # identical to it (its inner box)
                c, size = pc, ps
        if g.random() < 0.08:
            size = size.copy()
            size[g.integers(0, 3)] = 0.0  # a flat box
        placed.append((c, size, 0.0))
        meshes.append(_box(g, pool, c, size, 0.0, False))
        if len(meshes) < count and g.random() < 0.6:  # its outer layer, from a hair's breadth to a wide shell
            offset = float([1e-3, 2e-3, 0.02, 0.25, 0.5, 2.0][g.integers(0, 6)])
            meshes.append(_box(g, pool, c, size, offset, True))
            if len(meshes) < count and g.random() < 0.1:  # and that outer layer once more: an identical pair of shells
                meshes.append(_box(g, pool, c, size, offset, True))
    return meshes


def _place(order: list, fixed: dict) -> list:
    """The meshes `order` with those of `fixed` (index -> mesh) swapped into their places."""
    rest = [m for m in order if all(m is not f for f in fixed.values())]
    out, k = [], 0
    for i in range(len(order)):
        if i in fixed:
            out.append(fixed[i])
        else:
            out.append(rest[k])
            k += 1
    assert k == len(rest) and len(out) == len(order)
    return out


def _light(g, sc, centre):
    """The lights of fuzz_cases.make_bundle_case: far, near a box, inside the bounds, on the plane of some face."""
    r = g.random()
    if r < 0.35:
        lp = centre + g.normal(size=3) * g.uniform(15, 80)
    elif r < 0.7:
        lp = centre + g.uniform(-10, 10, 3) * np.asarray([1.0, 1.6, 1.0])
    elif r < 0.85:
        lp = centre + g.uniform(-3, 3, 3)
    else:
        tri = sc.meshes[g.integers(0, len(sc.meshes))].triangles
        lp = np.asarray(tri[g.integers(0, len(tri))][:3], np.float64) + np.asarray([g.uniform(-40, 40), 0.0, g.uniform(-40, 40)])
    sc.light_position = tuple(float(x) for x in lp)
    sc.light_radius = float([0.0, 1e-3, 0.05, 0.5, 3.0, 3.0, 9.0, 25.0][g.integers(0, 8)])
    sc.light_color = (1.0, 1.0, 1.0, 1.0)


def _camera_basis(direction):
    """(right, up) of a camera at centre + t * direction that looks at the centre, up = +y (camera.cpp:10-16)."""
    fwd = -direction / np.linalg.norm(direction)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    return right, np.cross(right, fwd)


def _general(seed: int) -> bool:
    """Every fourth case of a group, one place on with every block of 12: each mesh count meets a general-variant config."""
    k = seed // 3
    return (k + k // 12) % 4 == 3


def _frame(g, general: bool):
    if general:  # the oracle's time: 160 shadow rays, or 140 AO rays, per hit
        return int(g.integers(24, 49)), int(g.integers(24, 37))
    return int(g.integers(24, 73)), int(g.integers(24, 57))


def _config(g, w, h, general: bool) -> abi.Config:
    """make_bundle_case's ranges; general: one of the three reasons for the general kernel variants."""
    kw = dict(width=w, height=h, maxBounces=int([0, 1, 2, 4][g.integers(0, 4)]), samplesPerPixel=int([1, 2, 4][g.integers(0, 3)]),
              tileSize=int([8, 16, 32, 32][g.integers(0, 4)]), shadowSamples=int([2, 3, 4, 8, 8, 8, 16, 32][g.integers(0, 8)]),
              aoSamples=int([1, 2, 5, 8, 16, 32, 64, 113][g.integers(0, 8)]), aoRadius=float(f32(g.uniform(0.5, 8.0))))
    if g.random() < 0.1:
        kw.update(aoEnabled=True, aoSamples=int([2, 8][g.integers(0, 2)]))
    if general:
        kw.update(samplesPerPixel=1, maxBounces=min(kw["maxBounces"], 2))
        which = int(g.integers(0, 3))
        if which == 0:
            kw["shadowSamples"] = int(g.integers(114, 161))
        elif which == 1:
            kw.update(aoEnabled=True, aoSamples=int(g.integers(114, 141)))
        else:
            kw.update(maxBounces=int([9, 12, 17, 20][g.integers(0, 4)]), shadowSamples=int([2, 4, 8][g.integers(0, 3)]))
    return abi.Config(**kw)


def pass_config(cfg) -> abi.Config:
    """The config of the scene-only passes and the light layers for a case: the beauty config's frame, tile and shadow settings,
    clamped to what the passes accept (at most 113 shadow and AO samples, 1 ... 8 bounces)."""
    return abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, softShadows=cfg.softShadows, shadowSamples=min(int(cfg.shadowSamples), 113),
                      maxBounces=min(max(1, int(cfg.maxBounces)), 8), aoSamples=min(int(cfg.aoSamples), 113), aoRadius=cfg.aoRadius)


def is_general(cfg) -> bool:
    return not B.expected_envelope(cfg)


def _ground(g, sd) -> float:
    lo, hi = PF.y_range(sd)
    return float(f32(lo + [0.0, 0.0, -0.02, -0.3, 0.1][g.integers(0, 5)] * (hi - lo)))


# ---- group count -----------------------------------------------------------------------------------------------------
def _count_case(seed: int):
    g = np.random.default_rng(seed ^ 0xB16C0000)
    n = COUNTS[(seed // 3) % len(COUNTS)]
    general = _general(seed)
    w, h = _frame(g, general)
    ang, elev, dist = g.uniform(0, 2 * np.pi), g.uniform(0.05, 0.75), g.uniform(44, 60)
    direction = np.asarray([np.cos(elev) * np.sin(ang), np.sin(elev), np.cos(elev) * np.cos(ang)])
    right, up = _camera_basis(direction)
    fov = 60.0
    front = CENTRE + 24.0 * direction  # in front of the volume, whose boxes reach 20.4 from the centre at most
    pool = _Pool(LDS_TEXEL_BUDGET if n <= 64 else None)
    # the cluster, the boxes at 63 and 64, the shell in the tail with its inner box
    s = g.uniform(2.5, 4.0, 3)
    I = _box(g, pool, front, s, 0.0, False)
    L = _shell(g, pool, front, s, 0.4, 0.5)
    U = _shell(g, pool, front, s, 0.4, 0.9)
    K = _shell(g, pool, front, s, 1.5, 0.4)
    side = (dist - 24.0) * np.tan(np.radians(fov / 2)) * 0.55 * (right if w >= h else up)
    F63 = _box(g, pool, front - side + g.uniform(-0.5, 0.5, 3), g.uniform(1.5, 3.0, 3), 0.0, False) if n >= 64 else None
    F64 = _box(g, pool, front + side + g.uniform(-0.5, 0.5, 3), g.uniform(1.5, 3.0, 3), 0.0, False) if n >= 66 else None
    V = J = None
    if n >= 70:
        c, sv = g.uniform([-9, 4, -6], [9, 28, 6]), g.uniform(2.0, 5.0, 3)
        J = _box(g, pool, c, sv * 0.7, 0.0, False)
        V = _shell(g, pool, c, sv, 0.3, 0.4)
    special = [m for m in (I, L, U, K, F63, F64, V, J) if m is not None]
    fill = _random_boxes(g, pool, n - len(special), [-9, 4, -6], [9, 28, 6], (0.5, 5.0), floor_y=-3.0)
    order = [(special + fill)[i] for i in g.permutation(n)]
    # the places: below 64 any free index below min(n, 63); in the tail any from 65 (66 with V) to min(n, 80)
    low = [int(i) for i in g.permutation(min(n, 63))]
    fixed = {}
    if n > 64:
        tail = [int(i) for i in 65 + g.permutation(min(n, 80) - 65)] if n > 65 else []
        fixed[64 if n == 65 else tail.pop()] = U
        if V is not None:
            fixed[tail.pop()] = V
    else:
        fixed[low.pop()] = U
    for m in (L, K, I, J):
        if m is not None:
            fixed[low.pop()] = m
    if F63 is not None:
        fixed[63] = F63
    if F64 is not None:
        fixed[64] = F64
    meshes = _place(order, fixed)
    index = {name: next(i for i, x in enumerate(meshes) if x is m) for name, m in
             (("I", I), ("L", L), ("U", U), ("K", K), ("F63", F63), ("F64", F64), ("V", V), ("J", J)) if m is not None}
    import scenes

    sc = scenes.simple_scene(meshes, fov=fov)
    _light(g, sc, CENTRE)
    sc.camera_position = tuple(float(x) for x in CENTRE + dist * direction)
    sc.camera_target = tuple(float(x) for x in CENTRE + g.uniform(-1, 1, 3))
    sc.camera_up = (0.0, 1.0, 0.0)
    sd = M.SceneDesc(sc)
    cfg = _config(g, w, h, general)
    ground = _ground(g, sd)
    kw = {k: getattr(cfg, k) for k in ("width", "height", "maxBounces", "samplesPerPixel", "tileSize", "shadowSamples", "aoEnabled", "aoSamples")}
    what = (f"big count seed {seed}: {n} boxes SPECIALS {index} camera {np.round(sc.camera_position, 3).tolist()} light {np.round(sc.light_position, 3).tolist()} "
            f"r {sc.light_radius} plane {ground!r} {kw}")
    return sd, cfg, ground, what, {"n": n, "index": index}


# ---- group posed -----------------------------------------------------------------------------------------------------
def _figure(g):
    """The meshes of a posed figure: at least three rotated parts, an outer layer among them."""
    while True:
        kind = ["S64", "S64", "S64", "S32"][g.integers(0, 4)]
        skin = M.synthetic_skin(kind, seed=int(g.integers(1, 1 << 30)))
        pose = np.zeros(12, f32)
        for k in range(12):
            r = g.random()
            if r < 0.45:
                pose[k] = g.uniform(-180, 180)
            elif r < 0.75:
                pose[k] = g.uniform(-40, 40)
            elif r < 0.85:
                pose[k] = 0.005 * g.choice([-1.0, 1.0])  # below the 0.01 degree gate
        fig = abi.scene_from_numpy(M.MeshBuilder.buildScene(skin, pose).to_numpy())
        rotated = [m for m in fig.meshes if m.hasRotation and (abs(m.rotX) > 0.01 or abs(m.rotZ) > 0.01)]
        if len(rotated) >= 3 and any(m.isOuterLayer for m in rotated) and any(not m.isOuterLayer for m in rotated):
            return kind, pose, fig


def _posed_case(seed: int):
    g = np.random.default_rng(seed ^ 0xB16D0000)
    n = POSED_COUNTS[(seed // 3) % len(POSED_COUNTS)]
    general = _general(seed)
    w, h = _frame(g, general)
    kind, pose, fig = _figure(g)
    pool = _Pool(LDS_TEXEL_BUDGET if n <= 64 else None)
    for m in fig.meshes:
        pool.add(m)
    boxes = _random_boxes(g, pool, n - len(fig.meshes), [-14, 1, -10], [14, 33, 10], (0.5, 3.5))
    order = [(fig.meshes + boxes)[i] for i in g.permutation(n)]
    fixed = {}
    if n > 64:
        rotated = [m for m in fig.meshes if m.hasRotation and (abs(m.rotX) > 0.01 or abs(m.rotZ) > 0.01)]
        outer = [m for m in rotated if m.isOuterLayer]
        inner = [m for m in rotated if not m.isOuterLayer]
        tail = [int(i) for i in 64 + g.permutation(min(n, 90) - 64)]
        fixed[tail.pop()] = outer[g.integers(0, len(outer))]
        if n > 65:
            fixed[tail.pop()] = inner[g.integers(0, len(inner))]
    meshes = _place(order, fixed)
    fig.meshes = meshes
    sc = fig
    _light(g, sc, CENTRE)
    ang, elev, dist = g.uniform(0, 2 * np.pi), g.uniform(-0.1, 0.7), g.uniform(38, 58)
    direction = np.asarray([np.cos(elev) * np.sin(ang), np.sin(elev), np.cos(elev) * np.cos(ang)])
    sc.camera_position = tuple(float(x) for x in CENTRE + dist * direction)
    sc.camera_target = tuple(float(x) for x in CENTRE + g.uniform(-2, 2, 3))
    sc.camera_up = (0.0, 1.0, 0.0)
    sc.camera_fov = 60.0
    sd = M.SceneDesc(sc)
    cfg = _config(g, w, h, general)
    ground = _ground(g, sd)
    where = [i for i, m in enumerate(meshes) if m.hasRotation]
    kw = {k: getattr(cfg, k) for k in ("width", "height", "maxBounces", "samplesPerPixel", "tileSize", "shadowSamples", "aoEnabled", "aoSamples")}
    what = (f"big posed seed {seed}: {n} meshes, {kind} pose {np.round(pose, 3).tolist()} parts with a rotation at {where} camera "
            f"{np.round(sc.camera_position, 3).tolist()} light {np.round(sc.light_position, 3).tolist()} r {sc.light_radius} plane {ground!r} {kw}")
    return sd, cfg, ground, what, {"n": n}


# ---- group texels ----------------------------------------------------------------------------------------------------
def _texels_case(seed: int):
    import scenes

    g = np.random.default_rng(seed ^ 0xB16E0000)
    total = TEXEL_TOTALS[(seed // 3) % len(TEXEL_TOTALS)]
    if total is None:
        total = int(g.integers(65520, 65536))
    elif total < 0:
        total = int(g.integers(88000, 92001))
    general = _general(seed)
    w, h = _frame(g, general)
    pool = _Pool(20000)  # (the budget of the small boxes: the large texture takes the rest)
    n = int(g.integers(2, 9))
    # the shell whose texture holds the last texels of the pool, and the box in it: in front of the camera, above the ground
    lw, lh = [(8, 8), (8, 4), (4, 8), (6, 6), (16, 2), (5, 7)][g.integers(0, 6)]
    if total == 65537:  # ONE texel lies beyond the staged words, texel 65 536: on a grid this small it covers a sixth of every face or more
        lw, lh = [(2, 2), (3, 2), (2, 3)][g.integers(0, 3)]
    last_tex = _grid(g, lw, lh, 0.5)
    last_tex.pixels[-1, 3], last_tex.pixels[-2, 3] = 1.0, 0.0  # the pool's last texel is hit, the one before it is seen through
    lc, ls = np.asarray([g.uniform(-1, 1), g.uniform(7, 10), g.uniform(5, 7)]), g.uniform(4.0, 6.0, 3)
    meshes = [pool.add(scenes.build_box({k: _grid(g, 4, 4, 1.0) for k in FACES}, lc, ls))] if n >= 3 else []
    # one large, partly transparent texture on an outer layer, beside and behind
    bc, bs = np.asarray([g.choice([-9.0, 9.0]), g.uniform(8, 14), g.uniform(-6, -2)]), g.uniform(5.0, 9.0, 3)
    if n >= 4:
        meshes.append(pool.add(scenes.build_box({k: _grid(g, 3, 3, 1.0) for k in FACES}, bc, bs)))
    small = []  # further boxes under small textures
    for _ in range(max(0, n - 4)):
        c = np.asarray([g.uniform(-12, 12), g.uniform(3, 24), g.uniform(-8, 2)])
        offset = float([0.0, 0.0, 0.25][g.integers(0, 3)])
        small.append(_box(g, pool, c, g.uniform(1.0, 4.0, 3), offset, offset > 0))
    pool.budget = None
    room = total - pool.texels - lw * lh
    bw = int(g.integers(200, 251))
    bh = (room - int(g.integers(1, 2000))) // bw
    big = _grid(g, bw, bh, float([0.3, 0.6, 0.9][g.integers(0, 3)]))
    filler = _grid(g, 1, room - bw * bh, 0.7)  # what remains, as one column
    assert bh > 100 and filler.height >= 1
    faces = {k: big for k in FACES}
    faces["bottom"] = filler
    shell = pool.add(scenes.build_box(faces, bc, bs, 0.5))
    meshes = meshes + small
    meshes = [meshes[i] for i in g.permutation(len(meshes))]
    meshes.insert(int(g.integers(0, len(meshes) + 1)), shell)
    meshes.append(pool.add(scenes.build_box(last_tex, lc, ls, float([0.25, 0.5, 1.0][g.integers(0, 3)]))))  # the last new texture
    if len(meshes) < 8 and g.random() < 0.3:  # a mesh behind it that brings no new texture
        meshes.append(scenes.build_box({k: (big if i % 2 else None) for i, k in enumerate(FACES)}, (g.uniform(-4, 4), g.uniform(14, 20), g.uniform(-8, -3)), g.uniform(2.0, 4.0, 3), 0.25))
    assert pool.texels == total and 2 <= len(meshes) <= 8
    last = next(i for i, m in enumerate(meshes) if m.tri_texture[0] is last_tex)
    sc = scenes.simple_scene(meshes, fov=float(g.uniform(35, 60)))
    # the light above and behind the shell, the camera in front of and above it: the shell's shadow lies between them
    sc.light_position = (float(lc[0] + g.uniform(-6, 6)), float(g.uniform(24, 45)), float(lc[2] + g.uniform(-12, 2)))
    sc.light_radius = float([0.0, 0.05, 0.5, 3.0, 3.0, 9.0][g.integers(0, 6)])
    sc.light_color = (1.0, 1.0, 1.0, 1.0)
    ang, elev, dist = g.uniform(-0.7, 0.7), g.uniform(0.15, 0.7), g.uniform(14, 24)
    sc.camera_position = tuple(float(x) for x in lc + dist * np.asarray([np.cos(elev) * np.sin(ang), np.sin(elev), np.cos(elev) * np.cos(ang)]))
    sc.camera_target = tuple(float(x) for x in lc + g.uniform(-1, 1, 3) - np.asarray([0.0, 2.0, 0.0]))
    sc.camera_up = (0.0, 1.0, 0.0)
    sd = M.SceneDesc(sc)
    cfg = _config(g, w, h, general)
    lo, hi = PF.y_range(sd)
    ground = float(f32(lo + [0.0, 0.0, -0.02, -0.1][g.integers(0, 4)] * (hi - lo)))
    kw = {k: getattr(cfg, k) for k in ("width", "height", "maxBounces", "samplesPerPixel", "tileSize", "shadowSamples", "aoEnabled", "aoSamples")}
    what = (f"big texels seed {seed}: {len(meshes)} meshes, {total} texels ({bw}x{bh} on a shell, a filler of {filler.height}, the last {lw}x{lh} on mesh {last}) "
            f"camera {np.round(sc.camera_position, 3).tolist()} light {np.round(sc.light_position, 3).tolist()} r {sc.light_radius} plane {ground!r} {kw}")
    return sd, cfg, ground, what, {"total": total, "last_mesh": last, "last_texels": lw * lh}


_MAKERS = {"count": _count_case, "posed": _posed_case, "texels": _texels_case}


def make_big_case_info(seed: int, group: str):
    """make_big_case and what the generator put where: {"n", "index"} / {"n"} / {"total", "last_mesh", "last_texels"}."""
    sd, cfg, ground, what, info = _MAKERS[group](seed)
    hdr = B.flat_header(sd)
    if group == "texels":  # shared textures are pooled once: the header is the count that holds
        assert hdr["n_texels"] == info["total"], (what, hdr["n_texels"])
    else:
        assert hdr["n_meshes"] == info["n"], what
    return sd, cfg, ground, what, info


def make_big_case(seed: int, group: str):
    return make_big_case_info(seed, group)[:4]


def nominal(seed: int, group: str):
    """The mesh count (count, posed) or the entry of TEXEL_TOTALS (texels) of a seed, which follows from the seed alone."""
    table = {"count": COUNTS, "posed": POSED_COUNTS, "texels": TEXEL_TOTALS}[group]
    return table[(seed // 3) % len(table)]


def seed_with(group: str, first: int, wanted) -> int:
    """The first seed of the block from `first` whose case has `wanted` meshes (texels), without building a case."""
    return next(seed for seed in block_seeds(group, first) if nominal(seed, group) == wanted)


def sweep_case(seed: int):
    """The sweep's case of a seed: the three groups in turn."""
    return make_big_case(seed, GROUPS[seed % 3])


def scene_centre(sd) -> np.ndarray:
    v = np.concatenate([np.asarray(m["triangles"], np.float64).reshape(-1, 3) for m in sd.to_numpy()["meshes"] if len(m["triangles"])])
    return np.median(v, axis=0)


def case_rays(sd, seed: int, n: int = 1500) -> np.ndarray:
    """scenes.random_rays aimed at the scene."""
    import scenes

    c = scene_centre(sd)
    return scenes.random_rays(n, seed=seed ^ 0x4A75, target=tuple(float(x) for x in c), spread=12.0, dist=(20.0, 60.0))


# ---- the oracle's planes of a case, and what they hold ------------------------------------------------------------------
def pass_expectation(oracle, case) -> dict:
    """{"surfaces", "ground", "reflection", "light"} of a case under pass_config: layers_checker.expected_surfaces,
    ground_checker.expected_ground, reflection_checker.expected_reflection, light_checker.expected_light."""
    import ground_checker as G
    import layers_checker as L
    import light_checker as LC
    import reflection_checker as R

    sd, cfg, ground, _ = case[:4]
    pc = pass_config(cfg)
    out = {"surfaces": L.expected_surfaces(oracle, sd, pc.width, pc.height), "ground": G.expected_ground(oracle, sd, pc, ground),
           "reflection": R.expected_reflection(oracle, sd, pc, ground), "light": LC.expected_light(oracle, sd, pc)}
    LC.assert_miss_constants(out["light"])
    R.assert_miss_constants(out["reflection"])
    for e in out.values():
        for a in e.values():
            a.setflags(write=False)
    return out


def beauty_expectation(oracle, case, i: int, seed: int) -> dict:
    """{"frame" the oracle's render, "transparent" the transparent checker's frame for every third case (else None), "rays",
    "hits" oracle.intersect of case_rays}."""
    sd, cfg = case[0], case[1]
    frame = oracle.render(sd.ptr, cfg)
    clear = B.transparent_checker_lib().render(sd.ptr, cfg, "transparent", threads=4)[0] if i % 3 == 2 else None
    rays = case_rays(sd, seed)
    out = {"frame": frame, "transparent": clear, "rays": rays, "hits": oracle.intersect(sd.ptr, rays)}
    for a in out.values():
        if a is not None:
            a.setflags(write=False)
    return out


CENSUS = ("tail hits", "tail hits on rotated meshes", "tail hits on outer layers", "pixels of mesh 63", "pixels of mesh 64", "pixels of the straddling pair",
          "dark ground", "penumbra ground", "penumbra hits", "partly occluded hits", "reflected pixels", "hits in the last staged alpha word",
          "hits beyond alpha word 4096")
# the census numbers a group must hold in every block (the others are recorded all the same)
REQUIRED = {"count": (0, 2, 3, 4, 5, 6, 7, 8, 9, 10), "posed": (0, 1, 2, 3, 4, 6, 7, 8, 9, 10), "texels": (6, 7, 8, 9, 10, 11, 12)}


def pair_pixels(oracle, sd, cfg, surf, lower: int, upper: int) -> int:
    """Pixels where both meshes of the identical pair are hit at the scene's own t; the scene's hit must name the lower index."""
    import layers_checker as L
    import scenes

    rays = L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height)
    a, b = oracle.intersect_mesh(sd.ptr, lower, rays), oracle.intersect_mesh(sd.ptr, upper, rays)
    depth, mesh = surf["depth"].reshape(-1), surf["mesh"].reshape(-1)
    both = (a["hit"] != 0) & (b["hit"] != 0) & (scenes.bits(a["t"]) == scenes.bits(b["t"])) & (scenes.bits(a["t"]) == scenes.bits(depth))
    named = mesh[both]
    assert (named <= lower).all(), f"equal t on meshes {lower} and {upper}: the oracle names {sorted(set(named.tolist()))}"
    return int((named == lower).sum())


def last_word_hits(sd, hdr, surf, info) -> tuple:
    """(hits whose texel lies in the last alpha word, hits whose texel lies beyond word 4096), on the mesh whose texture holds the
    last texels of the pool: its texels' colours all differ, so the albedo names the texel."""
    m = info["last_mesh"]
    base, tw, th = int(hdr["tex_off"][m][0]), int(hdr["tex_w"][m][0]), int(hdr["tex_h"][m][0])
    assert base + tw * th == hdr["n_texels"] and tw * th == info["last_texels"], "the shell's texture is not the pool's last"
    t = sd.to_numpy()["meshes"][m]["tri_texture"][0]
    px = np.ascontiguousarray(sd.to_numpy()["textures"][int(t)]["pixels"], f32)
    where = {px[i].tobytes(): base + i for i in range(tw * th)}
    assert len(where) == tw * th
    last = beyond = 0
    for albedo in surf["albedo"][surf["mesh"] == m]:
        k = where.get(np.ascontiguousarray(albedo, f32).tobytes())
        if k is not None:
            last += k // 16 == hdr["alpha_words"] - 1
            beyond += k // 16 >= B.K_ALPHA_LDS_WORDS_MAX
    return int(last), int(beyond)


def census(oracle, case, group, exp) -> np.ndarray:
    """The numbers of CENSUS of one case, from the oracle's planes `exp` (pass_expectation)."""
    import ground_checker as G
    import light_checker as LC
    import reflection_checker as R

    sd, cfg, _, _, info = case
    hdr = B.flat_header(sd)
    surf = exp["surfaces"]
    hit, mesh = surf["hit"], surf["mesh"]
    tail = hit & (mesh >= 64)
    flags = hdr["flags"]
    out = np.zeros(len(CENSUS), np.int64)
    out[0] = tail.sum()
    out[1] = (tail & ((flags[np.maximum(mesh, 0)] & B.MESH_ROTATED) != 0)).sum()
    out[2] = (tail & ((flags[np.maximum(mesh, 0)] & B.MESH_OUTER) != 0)).sum()
    out[3], out[4] = (mesh == 63).sum(), (mesh == 64).sum()
    if group == "count":
        lower, upper = sorted((info["index"]["L"], info["index"]["U"]))
        out[5] = pair_pixels(oracle, sd, pass_config(cfg), surf, lower, upper)
    out[6:8] = G.counts(exp["ground"])[1:]
    lc = LC.counts(exp["light"])
    out[8], out[9] = lc[2], lc[3]
    out[10] = R.counts(exp["reflection"])[1]
    if group == "texels":
        last, beyond = last_word_hits(sd, hdr, surf, info)
        if B.expected_view(hdr) == "hbm":
            out[12] = beyond
        else:
            out[11] = last
    return out


# ---- the fixed blocks of 12 cases of the suite -----------------------------------------------------------------------
BLOCK_SIZE = 12


def block_seeds(group: str, first: int) -> list:
    """The 12 seeds of a block: 3 apart (the sweep gives seed k to group k % 3), every count of the group among them."""
    assert first % 3 == 0
    return [first + 3 * i + GROUPS.index(group) for i in range(BLOCK_SIZE)]


def block_cases(group: str, first: int) -> list:
    return [make_big_case_info(seed, group) for seed in block_seeds(group, first)]


# What the ORACLE holds over a block, measured on the CPU, in the order of CENSUS.  exact: asserted as it stands (the first block
# of each group); otherwise every required number must reach half of what is written here.  A frame of constants, or a scene that
# avoids its own edge, passes neither.
BLOCKS = {
    ("count", 36000): dict(exact=True, census=(552, 0, 245, 89, 82, 123, 5386, 4764, 1382, 875, 3375, 0, 0)),
    ("count", 36036): dict(exact=False, census=(1226, 0, 283, 120, 111, 159, 5043, 2536, 218, 836, 2579, 0, 0)),
    ("count", 36072): dict(exact=False, census=(1087, 0, 326, 73, 79, 121, 2427, 3021, 706, 748, 1457, 0, 0)),
    ("posed", 36000): dict(exact=True, census=(470, 246, 298, 14, 34, 0, 4699, 2463, 172, 1068, 1187, 0, 0)),
    ("posed", 36036): dict(exact=False, census=(671, 448, 354, 31, 111, 0, 2292, 4451, 572, 1493, 743, 0, 0)),
    ("posed", 36072): dict(exact=False, census=(517, 329, 346, 27, 61, 0, 5507, 4237, 344, 1166, 866, 0, 0)),
    ("texels", 36000): dict(exact=True, census=(0, 0, 0, 0, 0, 0, 3342, 894, 443, 1415, 4226, 487, 910)),
    ("texels", 36036): dict(exact=False, census=(0, 0, 0, 0, 0, 0, 3173, 5757, 2015, 2033, 4343, 356, 1279)),
    ("texels", 36072): dict(exact=False, census=(0, 0, 0, 0, 0, 0, 3217, 2346, 443, 2057, 4744, 131, 1182)),
}
BLOCK_IDS = [f"{g}-{s}" for g, s in BLOCKS]
_CACHE = {}


def block_pass_expectations(oracle, group, first) -> list:
    """The block's pass expectations, computed once per session and never modified."""
    key = ("pass", group, first)
    if key not in _CACHE:
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(4) as pool:  # (the oracle's calls release the GIL; the planes do not depend on the threads)
            _CACHE[key] = list(pool.map(lambda c: pass_expectation(oracle, c), block_cases(group, first)))
    return _CACHE[key]


def block_case_census(oracle, group, first) -> np.ndarray:
    """The census of each case of the block: (12, len(CENSUS))."""
    key = ("census", group, first)
    if key not in _CACHE:
        exps = block_pass_expectations(oracle, group, first)
        _CACHE[key] = np.asarray([census(oracle, c, group, e) for c, e in zip(block_cases(group, first), exps)])
    return _CACHE[key]


def block_census(oracle, group, first) -> np.ndarray:
    return block_case_census(oracle, group, first).sum(axis=0)


def check_block(oracle, group, first) -> list:
    """The block's pass expectations after the floor of its census: exactly BLOCKS' numbers for a group's first block, half of
    them elsewhere, and every required number positive."""
    spec = BLOCKS[(group, first)]
    total = block_census(oracle, group, first)
    print(f"big {group} {first} census:", dict(zip(CENSUS, total.tolist())))
    req = REQUIRED[group]
    if group == "texels":  # every case AT the limit by itself: 65 537 texels have ONE texel beyond the staged words, and it is hit
        for seed, per in zip(block_seeds(group, first), block_case_census(oracle, group, first)):
            if nominal(seed, group) in (65536, 65537, 65552):
                assert per[11] + per[12] >= 5, f"big texels seed {seed}: {per[11]} hits in the last staged alpha word, {per[12]} beyond word 4096"
    assert all(total[k] > 0 for k in req), f"big {group} {first}: the oracle holds no {[CENSUS[k] for k in req if total[k] <= 0]}"
    if spec["exact"]:
        assert tuple(total.tolist()) == tuple(spec["census"]), f"big {group} {first}: the oracle holds {total.tolist()}, not {spec['census']}: the generator differs"
    else:
        assert all(2 * total[k] >= spec["census"][k] for k in req), f"big {group} {first}: the oracle holds {total.tolist()}, less than half of {spec['census']}"
    return block_pass_expectations(oracle, group, first)


def worker_sweep_expectation(args) -> tuple:
    """For a worker process that never uses the device: (pass expectation, beauty expectation, census) of sweep case (seed, k)."""
    import oraclelib

    seed, k = args
    orc = oraclelib.Oracle()
    group = GROUPS[seed % 3]
    case = make_big_case_info(seed, group)
    pe = pass_expectation(orc, case)
    return pe, beauty_expectation(orc, case, k, seed), census(orc, case, group, pe)
