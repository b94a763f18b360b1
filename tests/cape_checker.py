"""What a cape must build, hold and show, from the host alone — a helper, not a test.

The cape is restated here in numpy float32, apart from the library's tables: the 64x32 image unwrapped as the box
{ox, oy, w, h, d} = {0, 0, 10, 16, 1}; the mesh {10, 16, 1} at {0, 16, -2.5}, hinged at {0, 24, -2} by rot_x = angle; the box
turned half a turn about y, so the face slots (0 back -z, 1 front +z, 2 left +x, 3 right -x, 4 top, 5 bottom) take the unwrap's
rectangles crosswise, top and bottom read turned half a turn; the eight corners and twelve triangles in the builder's order.
The rotation's sine and cosine are the project's own (mcrt_sinf / mcrt_cosf): the flattener stores them per rotated mesh, and
``trig`` reads them from the blob of a one-mesh scene made here.
The expected blob of a repainted caped handle: ``buildScene`` of OPAQUE copies of skin and cape (nothing is dropped), the
textures overwritten through the tables with ``u8 / 255.0f``, flattened on the host."""
from __future__ import annotations

import functools

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import skin_paint_checker as S
import slim_checker as SL

f32 = np.float32
CAPE_BOX = (0, 0, 10, 16, 1)
# face slot -> (x, y, w, h) in the cape image, and whether it is read turned half a turn
SLOT_RECTS = [((1, 1, 10, 16), False), ((12, 1, 10, 16), False), ((11, 1, 1, 16), False), ((0, 1, 1, 16), False),
              ((1, 0, 10, 1), True), ((11, 0, 10, 1), True)]
UNWRAP_FACE = (1, 0, 3, 2, 4, 5)  # the slot's rectangle as a face of SL.face_rect(CAPE_BOX, .)
N_TEXELS = 372
POSITION, SIZE, PIVOT = (0.0, 16.0, -2.5), (10.0, 16.0, 1.0), (0.0, 24.0, -2.0)
ANGLES = (0.0, 0.005, 10.0, 45.0, 90.0)
# corner index = x + 2 * y + 4 * z; quads in face-slot order, two triangles (0, 1, 2), (0, 2, 3) each
QUADS = ((2, 3, 1, 0), (7, 6, 4, 5), (3, 7, 5, 1), (6, 2, 0, 4), (6, 7, 3, 2), (0, 1, 5, 4))
KINDS = {"S64": (64, "classic", 12), "S64S": (64, "slim", 12), "S32": (32, "classic", 7)}  # kind -> height, model, skin meshes


def texel_pixel(face, tx, ty):
    (x, y, w, h), turned = SLOT_RECTS[face]
    return (x + (w - 1 - tx if turned else tx), y + (h - 1 - ty if turned else ty))


@functools.lru_cache(maxsize=None)
def pool_rows():
    """Per texel of the cape mesh, in pool order: (face, tx, ty, cape pixel index y * 64 + x), a (372, 4) int32 array."""
    rows = []
    for face, ((x, y, w, h), turned) in enumerate(SLOT_RECTS):
        for ty in range(h):
            for tx in range(w):
                px, py = texel_pixel(face, tx, ty)
                rows.append((face, tx, ty, py * 64 + px))
    out = np.array(rows, np.int32)
    out.setflags(write=False)
    return out


def face_texels(cape_rgba8, face) -> np.ndarray:
    """(w * h, 4) float32: the texture of a face slot, u8 / 255.0f."""
    texel = np.asarray(cape_rgba8, np.uint8).astype(f32) / f32(255.0)
    (x, y, w, h), turned = SLOT_RECTS[face]
    r = texel[y:y + h, x:x + w]
    return (r[::-1, ::-1] if turned else r).reshape(-1, 4).copy()


def corners() -> np.ndarray:
    hw, hh, hd = f32(SIZE[0]) / f32(2), f32(SIZE[1]) / f32(2), f32(SIZE[2]) / f32(2)
    p = np.array(POSITION, f32)
    lo, hi = p - np.array([hw, hh, hd], f32), p + np.array([hw, hh, hd], f32)
    return np.array([[(hi if i & 1 else lo)[0], (hi if i & 2 else lo)[1], (hi if i & 4 else lo)[2]] for i in range(8)], f32)


def local_triangles() -> np.ndarray:
    """(36, 3) float32: the unposed box's twelve triangles."""
    c = corners()
    return np.array([c[q[k]] for q in QUADS for tri in ((0, 1, 2), (0, 2, 3)) for k in tri], f32)


@functools.lru_cache(maxsize=None)
def trig(angle):
    """(cos, sin) of `angle` degrees as the project's mcrt_cosf / mcrt_sinf give them: what the flattener stores as the forward
    x rotation of a mesh turned by that angle."""
    tex = {k: abi.Texture(1, 1, np.ones((1, 4), f32)) for k in ("back", "front", "left", "right", "top", "bottom")}
    import scenes

    mesh = scenes.build_box(tex, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    mesh.hasRotation, mesh.rotX, mesh.rotZ, mesh.pivot = True, float(angle), 0.0, (0.0, 0.0, 0.0)
    mesh.localTriangles = np.array(mesh.triangles, f32)
    blob = M.flatten(scenes.simple_scene([mesh]))
    fm = np.frombuffer(blob[192:192 + 192], f32)
    return f32(fm[13]), f32(fm[14])


def world_triangles(angle) -> np.ndarray:
    """rotate_about in float32, operation by operation: p - pivot; ny = y c - z s, nz = y s + z c; + pivot."""
    v = local_triangles()
    if not abs(f32(angle)) > f32(0.01):
        return v
    c, s = trig(float(angle))
    pv = np.array(PIVOT, f32)
    p = v - pv
    ny = p[:, 1] * c - p[:, 2] * s
    nz = p[:, 1] * s + p[:, 2] * c
    return np.stack([p[:, 0] + pv[0], ny + pv[1], nz + pv[2]], axis=1).astype(f32)


@functools.lru_cache(maxsize=None)
def cape(name) -> np.ndarray:
    """The cape images of the suite, read-only: name -> (32, 64, 4) uint8."""
    if name == "synthetic":
        a = M.synthetic_cape().copy()
    elif name == "all_bytes":  # every byte value in the colour channels inside the unwrap's corner, alphas 1..254
        y, x = np.mgrid[0:32, 0:64]
        i = 22 * y + x
        a = np.stack([i & 255, (7 * i + 13) & 255, 255 - (i & 255), 1 + i % 254], axis=-1).astype(np.uint8)
    elif name == "one_hole":  # alpha 0 in exactly one texel: (5, 7), on the outward face
        a = M.synthetic_cape().copy()
        a[7, 5, 3] = 0
    elif name == "transparent":
        a = np.zeros((32, 64, 4), np.uint8)
    elif name == "marker":  # pixel value = pixel index
        y, x = np.mgrid[0:32, 0:64]
        i = 64 * y + x
        a = np.stack([i & 255, i >> 8, np.full_like(i, 7), np.full_like(i, 255)], axis=-1).astype(np.uint8)
    else:
        raise KeyError(name)
    a.setflags(write=False)
    return a


def skin(kind) -> np.ndarray:
    return SL.skin("synthetic") if kind == "S64S" else S.skin("synthetic_" + kind)


def full_table_scene(kind, skin_rgba8, cape_rgba8, pose, angle, look=None):
    """The description a repainted caped handle stands for: every part and the cape present, their texels through the tables."""
    height, model, n_skin = KINDS[kind]
    base = (SL.full_table_scene(skin_rgba8, pose, None, model) if height == 64 else S.full_table_scene(skin_rgba8, pose)).to_numpy()
    opaque = np.full((32, 64, 4), 255, np.uint8)
    white = np.full((height, 64, 4), 255, np.uint8)
    d = M.MeshBuilder.buildScene(white, pose, model=model, cape=opaque, cape_angle=angle).to_numpy()
    assert len(d["meshes"]) == n_skin + 1 == len(base["meshes"]) + 1 and len(d["textures"]) == 6 * (n_skin + 1)
    for t in range(6 * n_skin):
        d["textures"][t]["pixels"][:] = base["textures"][t]["pixels"]
    for face in range(6):
        t = int(d["meshes"][n_skin]["tri_texture"][2 * face])
        assert t == 6 * n_skin + face
        d["textures"][t]["pixels"][:] = face_texels(cape_rgba8, face)
    if look is not None:
        for k in S.LOOK_FIELDS:
            d[k] = np.asarray(look[k], f32) if isinstance(look[k], tuple) else f32(look[k])
    return M.SceneDesc(abi.scene_from_numpy(d))


_BLOBS, _FRAMES = {}, {}


def _key(kind, skin_rgba8, cape_rgba8, pose, angle, look):
    return (kind, None if cape_rgba8 is None else np.asarray(cape_rgba8, np.uint8).tobytes(), float(angle)) + S._key(skin_rgba8, pose, look)


def expected_blob(kind, skin_rgba8, cape_rgba8, pose, angle, look=None) -> bytes:
    k = _key(kind, skin_rgba8, cape_rgba8, pose, angle, look)
    if k not in _BLOBS:
        _BLOBS[k] = M.flatten(full_table_scene(kind, skin_rgba8, cape_rgba8, pose, angle, look))
    return _BLOBS[k]


def reference_scene(kind, skin_rgba8, cape_rgba8, pose, angle, look=None):
    """``buildScene(skin, pose, model, cape, angle)`` with the look: the oracle's scene (transparent parts and cape dropped)."""
    sd = M.MeshBuilder.buildScene(np.ascontiguousarray(skin_rgba8), pose, model=KINDS[kind][1], cape=cape_rgba8, cape_angle=angle)
    return S.apply_look(sd, look)


@functools.lru_cache(maxsize=None)
def behind(yaw=180.0) -> dict:
    """A look from behind (yaw 180) or three-quarter behind (150), as the dict form of skin_paint_checker: the builder's look
    with the camera on ``orbit_look``'s orbit at distance 50 (the default camera cannot see a cape)."""
    d = M.orbit_look(yaw, 0.0, 50.0).desc
    out = {}
    for k in S.LOOK_FIELDS:
        v = getattr(d, k)
        out[k] = tuple(float(x) for x in v) if hasattr(v, "__len__") else float(v)
    return out


def oracle_frame(oracle, kind, skin_rgba8, cape_rgba8, pose, angle, cfg: abi.Config, look=None) -> np.ndarray:
    """The CPU oracle's frame of that scene; computed once per argument set, read-only.  `look`: a dict (or None)."""
    k = _key(kind, skin_rgba8, cape_rgba8, pose, angle, look) + (bytes(cfg.to_c()),)
    if k not in _FRAMES:
        frame = oracle.render(reference_scene(kind, skin_rgba8, cape_rgba8, pose, angle, look).ptr, cfg)
        frame.setflags(write=False)
        _FRAMES[k] = frame
    return _FRAMES[k]


def cape_pixels(oracle, sd, width, height) -> int:
    """How many pixels of the oracle's pixel-centre id layer name the LAST mesh of `sd` — the cape, where it has one."""
    import layers_checker

    mesh = layers_checker.expected_surfaces(oracle, sd, width, height)["mesh"]
    return int((mesh == sd.desc.n_meshes - 1).sum())


def header(blob: bytes) -> dict:
    return SL.header(blob)
