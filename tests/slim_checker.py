"""What the slim ("Alex") player model must build, hold and show, from the host alone — a helper, not a test.

The slim tables are restated here, apart from the library's: per mesh of the full table (12 meshes: {head, body, right arm,
left arm, right leg, left leg} x {inner, outer}) the unwrap box {ox, oy, w, h, d} and from it the rectangle of each face slot
(0 back, 1 front, 2 left, 3 right, 4 top, 5 bottom).  Slim differs from classic in the four arm boxes alone: w = 3.
The expected blob of a repainted slim handle: ``buildScene(model="slim")`` of an OPAQUE copy of the skin (no outer part is
dropped), its 72 textures overwritten texel by texel through these tables with ``skin / 255.0f``, the look put in, flattened on
the host.  The expected frame: the CPU oracle's render of ``buildScene(skin, pose, model="slim")`` with the same look."""
from __future__ import annotations

import functools

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import skin_paint_checker as S

f32 = np.float32
CLASSIC_BOXES = [(0, 0, 8, 8, 8), (32, 0, 8, 8, 8), (16, 16, 8, 12, 4), (16, 32, 8, 12, 4), (40, 16, 4, 12, 4), (40, 32, 4, 12, 4),
                 (32, 48, 4, 12, 4), (48, 48, 4, 12, 4), (0, 16, 4, 12, 4), (0, 32, 4, 12, 4), (16, 48, 4, 12, 4), (0, 48, 4, 12, 4)]
SLIM_BOXES = list(CLASSIC_BOXES)
SLIM_BOXES[4:8] = [(40, 16, 3, 12, 4), (40, 32, 3, 12, 4), (32, 48, 3, 12, 4), (48, 48, 3, 12, 4)]
ARM_MESHES = (4, 5, 6, 7)  # right arm, its outer layer, left arm, its outer layer
N_TEXELS = {"classic": 3264, "slim": 3136}
# the pixels the detection rule looks at, (x, y, w, h): columns of the inner arms' unwraps that a slim figure never reads
DETECTION_RECTS = ((50, 16, 2, 4), (54, 20, 2, 12), (42, 48, 2, 4), (46, 52, 2, 12))
KIND = {"classic": "S64", "slim": "S64S"}


def boxes(model):
    return SLIM_BOXES if model == "slim" else CLASSIC_BOXES


def face_rect(box, face):
    """(x, y, w, h) of a face slot of an unwrap box."""
    ox, oy, w, h, d = box
    return [(ox + 2 * d + w, oy + d, w, h), (ox + d, oy + d, w, h), (ox, oy + d, d, h), (ox + d + w, oy + d, d, h),
            (ox + d, oy, w, d), (ox + d + w, oy, w, d)][face]


@functools.lru_cache(maxsize=None)
def pool_rows(model):
    """Per pool texel, in pool order: (mesh, face, tx, ty, skin pixel index y * 64 + x), an (n, 5) int32 array."""
    rows = []
    for mesh, box in enumerate(boxes(model)):
        for face in range(6):
            x, y, w, h = face_rect(box, face)
            rows += [(mesh, face, tx, ty, (y + ty) * 64 + x + tx) for ty in range(h) for tx in range(w)]
    out = np.array(rows, np.int32)
    out.setflags(write=False)
    return out


def detection_pixels():
    return [(x, y) for rx, ry, w, h in DETECTION_RECTS for y in range(ry, ry + h) for x in range(rx, rx + w)]


@functools.lru_cache(maxsize=None)
def skin(name) -> np.ndarray:
    """The slim skins of the suite, read-only: name -> (64, 64, 4) uint8."""
    if name == "synthetic":
        a = M.synthetic_skin("S64S").copy()
    elif name == "all_bytes":  # every byte value in the colour channels, alphas 1..254 (the detection pixels too: the model is given)
        a = S.skin("all_bytes").copy()
    elif name == "overlays_cleared":  # every overlay cleared: the builder drops all six outer parts
        a = M.synthetic_skin("S64S").copy()
        head, rest = S._overlay("S64")
        a[head | rest, 3] = 0
    elif name == "all_opaque":
        a = M.synthetic_skin("S64S").copy()
        a[..., 3] = 255
    elif name == "arm_hole":  # one alpha-0 texel at (45, 22), the right arm's front face: MESH_OPAQUE leaves that inner mesh alone
        a = M.synthetic_skin("S64S").copy()
        a[22, 45, 3] = 0
    elif name == "marker":  # pixel value = pixel index, alpha 255 but where that would be 0: (r, g) = index, b = 7
        y, x = np.mgrid[0:64, 0:64]
        i = 64 * y + x
        a = np.stack([i & 255, i >> 8, np.full_like(i, 7), np.full_like(i, 255)], axis=-1).astype(np.uint8)
    else:
        raise KeyError(name)
    a.setflags(write=False)
    return a


def full_table_scene(skin_rgba8, pose, look=None, model="slim"):
    """The description a repainted handle of `model` stands for: every part present, the skin's texels through the tables here."""
    opaque = np.array(skin_rgba8, np.uint8)
    opaque[..., 3] = 255
    d = M.MeshBuilder.buildScene(opaque, pose, model=model).to_numpy()
    assert len(d["meshes"]) == 12 and len(d["textures"]) == 72
    texel = np.asarray(skin_rgba8, np.uint8).astype(f32) / f32(255.0)  # u8 / 255.0f
    for m, mesh in enumerate(d["meshes"]):
        for face in range(6):
            t = int(mesh["tri_texture"][2 * face])
            assert t == 6 * m + face
            tex = d["textures"][t]
            x, y, w, h = face_rect(boxes(model)[m], face)
            assert (tex["width"], tex["height"]) == (w, h), (m, face)
            tex["pixels"][:] = texel[y:y + h, x:x + w].reshape(-1, 4)
    if look is not None:
        for k in S.LOOK_FIELDS:
            d[k] = np.asarray(look[k], f32) if isinstance(look[k], tuple) else f32(look[k])
    return M.SceneDesc(abi.scene_from_numpy(d))


_BLOBS, _FRAMES = {}, {}


def expected_blob(skin_rgba8, pose, look=None, model="slim") -> bytes:
    k = S._key(skin_rgba8, pose, look) + (model,)
    if k not in _BLOBS:
        _BLOBS[k] = M.flatten(full_table_scene(skin_rgba8, pose, look, model))
    return _BLOBS[k]


def reference_scene(skin_rgba8, pose, look=None, model="slim"):
    """``buildScene(skin, pose, model=...)`` with the look: the oracle's scene (fully transparent outer parts dropped)."""
    return S.apply_look(M.MeshBuilder.buildScene(np.ascontiguousarray(skin_rgba8), pose, model=model), look)


def oracle_frame(oracle, skin_rgba8, pose, cfg: abi.Config, look=None, model="slim") -> np.ndarray:
    """The CPU oracle's frame of that scene; computed once per (skin, pose, look, model, config), read-only."""
    k = S._key(skin_rgba8, pose, look) + (model, bytes(cfg.to_c()))
    if k not in _FRAMES:
        frame = oracle.render(reference_scene(skin_rgba8, pose, look, model).ptr, cfg)
        frame.setflags(write=False)
        _FRAMES[k] = frame
    return _FRAMES[k]


def header(blob: bytes) -> dict:
    hdr = np.frombuffer(blob[:192], np.uint32)
    return {"n_meshes": int(hdr[1]), "n_texels": int(hdr[2]), "mesh_offset": int(hdr[32]), "texel_offset": int(hdr[33]),
            "blob_bytes": int(hdr[34]), "alpha_offset": int(hdr[35]), "alpha_words": int(hdr[36])}
