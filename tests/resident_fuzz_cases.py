"""Seeded walks over the states of REPAINTABLE resident scenes (mcrt_scene_create_skin, mcrt_scene_set_skin*, mcrt_scene_set_view*,
DESIGN §13, §16, §17) — generator and model, no device; a helper, not a test.

make_skin(g, kind)   an RGBA8 skin of random bytes whose alpha plane is drawn from four modes, with whole parts cleared or made
                     opaque, faces cleared or made opaque, and one alpha-0 texel at the first or last pool texel of a mesh
make_view(g)         (pose | None, look | None): builtin or free angles, some at 0, some either side of rotatePoint's 0.01 degree
                     gate; an orbit look 8 ... 200 units out with its own fov, light and background colour
make_script(seed)    2 to 4 handles and their operations with every argument: create / close (the pooled shell changes hands in
                     between), repaints, views, background modes, renders (some repeated until the launch graph replays), the
                     passes, blob checkpoints, and — even seeds — a stretch of more than kTableSlots batch calls without a host
                     wait
Model                applies the operations to plain Python state per handle and names what every checkpoint must show
Expectations         the values: blobs from skin_paint_checker.expected_blob, frames from the CPU oracle's render of
                     reference_scene(skin, pose, look) (the transparent checker's in transparent mode), passes from the pass
                     checkers on full_table_scene(skin, pose, look); cached by state

Every expectation comes from the CPU oracle and the host flattener; nothing here loads the device."""
from __future__ import annotations

import hashlib
import math
import os
import re

import numpy as np

import bake_checker as BC
import ground_checker as G
import layers_checker as L
import light_checker as LC
import minecraftskin_raytracer_amd as M
import reflection_checker as R
import skin_paint_checker as S
from minecraftskin_raytracer_amd import abi

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_ROTATED, MESH_OPAQUE = 2, 32  # flat_scene.h
SKIN_SENTINEL = 0xA5
N_MESHES = {"S64": 12, "S32": 7, "slim": 12}
BLOCK_SIZE = 6

CONFIGS = {
    "default": abi.Config(width=48, height=32, tileSize=16),  # the reference's defaults: 3 bounces, 1 spp, soft shadows
    "hard": abi.Config(width=48, height=32, tileSize=8, softShadows=False),
    "ao": abi.Config(width=64, height=64, tileSize=32, aoEnabled=True),
    "spp2": abi.Config(width=40, height=24, tileSize=16, samplesPerPixel=2),  # no multiple of the tile
    "dof": abi.Config(width=48, height=32, tileSize=32, dofEnabled=True, aperture=0.5),  # focusDistance 0: |target - position|
    "flat": abi.Config(width=40, height=24, tileSize=8, gradientBg=False),  # the look's own background colour
}
CONFIG_NAMES = tuple(CONFIGS)
PASSES = ("layers", "ground", "reflection", "light", "bake", "pick")


def _source(name):
    with open(os.path.join(ROOT, "minecraftskin_raytracer_amd", "csrc", name), encoding="utf-8") as f:
        return f.read()


def record_at() -> int:
    """The sighting at which a handle records its launch graph (render_enqueue.cpp)."""
    return int(re.search(r"constexpr int kRecordAt = (\d+);", _source("render_enqueue.cpp")).group(1))


def table_slots() -> int:
    """The table uploads a device keeps in flight (device_stores.cpp)."""
    return int(re.search(r"constexpr int kTableSlots = (\d+);", _source("device_stores.cpp")).group(1))


# ---- the skin's layout: which skin pixels a mesh and a face are cut from, through skin_texel -------------------------------------
_LAYOUT = {}


def layout(kind) -> dict:
    """{"pool": (n,) skin pixel index y * 64 + x per pool texel, "mesh", "face": (n,) per pool texel} of the full table of `kind`:
    "S64", "S32", or "slim" — the 64 x 64 skin on the slim model, from slim_checker's restated tables."""
    if kind == "slim" and kind not in _LAYOUT:
        import slim_checker

        rows = slim_checker.pool_rows("slim")
        assert len(rows) == slim_checker.N_TEXELS["slim"]
        _LAYOUT[kind] = {"pool": rows[:, 4].astype(np.int64), "mesh": rows[:, 0].copy(), "face": rows[:, 1].copy()}
    if kind not in _LAYOUT:
        h = 64 if kind == "S64" else 32
        table = M.texel_table(S.full_table_scene(np.full((h, 64, 4), 255, np.uint8), np.zeros(12, f32)))
        assert (table[:, 0] >= 0).all() and len(table) == (3264 if kind == "S64" else 2016)
        pool = np.empty(len(table), np.int64)
        for t, (m, face, tx, ty) in enumerate(table):
            x, y = M.skin_texel(kind, int(m), int(face), int(tx), int(ty))
            pool[t] = 64 * y + x
        assert np.array_equal(pool, M.skin_pool_map(kind))
        _LAYOUT[kind] = {"pool": pool, "mesh": table[:, 0].copy(), "face": table[:, 1].copy()}
    return _LAYOUT[kind]


def make_skin(g, kind, drop=None) -> np.ndarray:
    """drop: how many outer parts are cleared whole (default: drawn).  kind "slim": a 64 x 64 skin cut by the slim model's layout."""
    h = 32 if kind == "S32" else 64
    lay = layout(kind)
    a = g.integers(0, 256, (h, 64, 4), dtype=np.uint8)
    mode = int(g.integers(4))
    if mode == 0:  # density
        alpha = np.where(g.random((h, 64)) < g.choice([0.02, 0.3, 0.7, 0.98]), 255, 0)
    elif mode == 1:  # the classes
        alpha = g.choice(np.array([0, 1, 127, 254, 255]), (h, 64), p=[0.1, 0.15, 0.15, 0.15, 0.45])
    elif mode == 2:  # rectangles of zeros
        alpha = np.full((h, 64), 255)
        for _ in range(int(g.integers(1, 6))):
            x, y, w, hh = int(g.integers(64)), int(g.integers(h)), int(g.integers(1, 20)), int(g.integers(1, 12))
            alpha[y:y + hh, x:x + w] = 0
    else:
        alpha = g.integers(0, 256, (h, 64))
    flat = alpha.reshape(-1).astype(np.uint8)
    n_meshes = N_MESHES[kind]
    outer = [m for m in range(n_meshes) if m % 2 == 1] if kind != "S32" else [1]
    n_drop = (int(g.integers(len(outer) + 1)) if g.random() < 0.8 else 0) if drop is None else min(int(drop), len(outer))
    dropped = set(g.choice(outer, n_drop, replace=False).tolist())
    for m in range(n_meshes):
        of_mesh = lay["mesh"] == m
        if m in dropped:  # all six faces cleared: the reference drops the part
            flat[lay["pool"][of_mesh]] = 0
            continue
        r = g.random()
        if r < 0.4:  # the whole part opaque
            flat[lay["pool"][of_mesh]] = g.choice(np.array([1, 254, 255], np.uint8))
        elif r < 0.7:  # some faces cleared or made opaque
            for face in range(6):
                q = g.random()
                if q < 0.25:
                    flat[lay["pool"][of_mesh & (lay["face"] == face)]] = 0
                elif q < 0.6:
                    flat[lay["pool"][of_mesh & (lay["face"] == face)]] = 255
        if g.random() < 0.35:  # exactly one alpha-0 texel, at the mesh boundary inside a wave
            idx = np.flatnonzero(of_mesh)
            flat[lay["pool"][idx]] = np.maximum(flat[lay["pool"][idx]], 1)
            flat[lay["pool"][idx[0] if g.random() < 0.5 else idx[-1]]] = 0
    if kind == "S32" and g.random() < 0.5:  # the half wave that ends the pool
        last = lay["pool"][-32:]
        flat[last] = g.choice(np.array([0, 255], np.uint8), 32)
        i, j = (int(v) for v in g.choice(32, 2, replace=False))  # both classes, whatever was drawn
        flat[last[i]], flat[last[j]] = 0, 255
    a[..., 3] = flat.reshape(h, 64)
    # the dropped parts stay dropped whatever the later steps wrote (a mirrored limb of a legacy skin shares its pixels)
    for m in dropped:
        a.reshape(-1, 4)[lay["pool"][lay["mesh"] == m], 3] = 0
    a.setflags(write=False)
    return a


def _orbit(yaw_deg, pitch_deg, distance, target):
    yaw, pitch = math.radians(yaw_deg), math.radians(pitch_deg)
    return (float(target[0] + distance * math.cos(pitch) * math.sin(yaw)), float(target[1] + distance * math.sin(pitch)),
            float(target[2] + distance * math.cos(pitch) * math.cos(yaw)))


def make_look(g, distance=None, centred=False) -> dict:
    dist = float(math.exp(g.uniform(math.log(8.0), math.log(200.0)))) if distance is None else float(distance)
    target = (0.0, 18.0, 0.0)
    if not centred:
        r = g.random()
        if r < 0.1:  # the figure leaves the frame
            target = (float(g.choice([-1, 1]) * dist * 2.0), 18.0, 0.0)
        elif r < 0.5:
            target = (float(g.uniform(-4, 4)), float(g.uniform(4, 30)), float(g.uniform(-3, 3)))
    pitch = float(g.uniform(-25, 25)) if centred else float(g.uniform(-80, 80))
    fov = float(g.uniform(50, 80)) if centred else float(g.uniform(10, 120))
    radius = 0.0 if g.random() < 0.2 else float(g.uniform(0.1, 6.0))
    return {"light_position": (float(g.uniform(-40, 40)), float(g.uniform(5, 60)), float(g.uniform(-40, 40))),
            "light_color": (1.0, float(g.uniform(0.7, 1.0)), float(g.uniform(0.7, 1.0)), 1.0), "light_intensity": float(g.uniform(0.5, 1.2)),
            "light_radius": radius, "camera_position": _orbit(float(g.uniform(-180, 180)), pitch, dist, target), "camera_target": target,
            "camera_up": (0.0, 1.0, 0.0), "camera_fov": fov,
            "background_color": (float(g.uniform(0, 1)), float(g.uniform(0, 1)), float(g.uniform(0, 1)), 1.0)}


def make_pose(g):
    r = g.random()
    if r < 0.3:
        return M.getBuiltinPoses()[int(g.integers(7))].astype(f32)
    if r < 0.45:
        return np.zeros(12, f32)  # `posed` becomes false
    pose = (g.uniform(-180.0, 180.0, 12) * (g.random(12) < 0.6)).astype(f32)
    tiny = g.random(12) < 0.15
    pose[tiny] = g.uniform(-0.02, 0.02, 12).astype(f32)[tiny]  # either side of the gate
    if g.random() < 0.08:
        pose[:] = g.uniform(-0.009, 0.009, 12).astype(f32)  # every angle below the gate: an un-posed figure
    return pose


def make_view(g):
    r = g.random()
    pose = None if r < 0.25 else make_pose(g)
    look = None if (g.random() < 0.25 and pose is not None) or g.random() < 0.1 else make_look(g)
    return pose, look


# ---- scripts ---------------------------------------------------------------------------------------------------------------------
class _Gen:
    """The little the generator has to know of the handles: which slots are open, their kinds, and on which streams mutations
    are still unordered against a pass (the header leaves that ordering to the caller)."""

    def __init__(self, g, n):
        self.g, self.ops = g, []
        self.kind = [None] * n
        self.dirty = [set() for _ in range(n)]
        self.bakes = 0

    def open(self, kind=None):
        return [s for s, k in enumerate(self.kind) if k is not None and (kind is None or k == kind)]

    def emit(self, op):
        self.ops.append(op)
        return op

    def synced(self):
        for d in self.dirty:
            d.clear()

    def create(self, slot, between=None):
        g = self.g
        kind = "S64" if g.random() < 0.65 else "S32"
        pose = None if g.random() < 0.3 else make_pose(g)
        look = None if g.random() < 0.4 else make_look(g)
        self.kind[slot] = kind
        self.dirty[slot].clear()
        self.emit({"op": "create", "slot": slot, "kind": kind, "pose": pose, "look": look, "between": between})

    def close(self, slot):
        self.kind[slot] = None
        self.emit({"op": "close", "slot": slot})

    def subset(self, kind=None, least=1):
        slots = self.open(kind)
        n = int(self.g.integers(least, len(slots) + 1)) if len(slots) >= least else 0
        return [int(s) for s in self.g.permutation(slots)[:n]]

    def set_skin(self, slot=None, form=None, stream=None, skin=None):
        g = self.g
        form = form or ("host", "device", "batch")[int(g.integers(3))]
        stream = int(g.integers(2)) if stream is None else stream
        if form == "batch":
            kinds = [k for k in ("S64", "S32") if self.open(k)]
            kind = kinds[int(g.integers(len(kinds)))] if slot is None else self.kind[slot]
            slots = self.subset(kind)
            if slot is not None and slot not in slots:
                slots.append(slot)
            skins = [make_skin(g, kind) if skin is None or s != slot else skin for s in slots]
            op = {"op": "set_skin", "form": "batch", "slots": slots, "skins": skins, "offset": 0, "gap": int(g.choice([0, 4, 64, 100])), "stream": stream}
        else:
            slot = int(g.choice(self.open())) if slot is None else slot
            op = {"op": "set_skin", "form": form, "slots": [slot], "skins": [make_skin(g, self.kind[slot]) if skin is None else skin],
                  "offset": int(g.choice([0, 4, 8, 12])) if form == "device" else 0, "gap": 0, "stream": stream}
        for s in op["slots"]:
            if form != "host":
                self.dirty[s].add(stream)
        return self.emit(op)

    def set_view(self, slot=None, form=None, stream=None, view=None):
        g = self.g
        form = form or ("host", "device", "batch")[int(g.integers(3))]
        stream = int(g.integers(2)) if stream is None else stream
        if form == "batch":
            kinds = [k for k in ("S64", "S32") if self.open(k)]
            kind = kinds[int(g.integers(len(kinds)))] if slot is None else self.kind[slot]
            slots = self.subset(kind)
            if slot is not None and slot not in slots:
                slots.append(slot)
            views = [make_view(g) if view is None or s != slot else view for s in slots]
            poses = [v[0] for v in views]
            if any(p is None for p in poses):  # a batch has a pose for every handle or for none
                if view is not None and view[0] is not None or g.random() < 0.5:
                    poses = [make_pose(g) if p is None else p for p in poses]
                else:
                    poses = None
            looks = [v[1] for v in views]
            if all(k is None for k in looks) and g.random() < 0.5:
                looks = None
            if poses is None and (looks is None or all(k is None for k in looks)):
                looks = [make_look(g) for _ in slots]
            op = {"op": "set_view", "form": "batch", "slots": slots, "poses": poses, "looks": looks, "stream": stream}
        else:
            slot = int(g.choice(self.open())) if slot is None else slot
            pose, look = make_view(g) if view is None else view
            op = {"op": "set_view", "form": form, "slots": [slot], "poses": [pose], "looks": [look], "stream": stream}
        for s in op["slots"]:
            if form != "host":
                self.dirty[s].add(stream)
        return self.emit(op)

    def render(self, slots=None, cfg=None, repeat=1, buffer=None, stream=None, wait=None, outputs=None):
        g = self.g
        batch = slots is None and g.random() < 0.35
        if slots is None:
            slots = self.subset() if batch else [int(g.choice(self.open()))]
        wait = (repeat > 1 or buffer is not None or g.random() < 0.6) if wait is None else wait
        op = {"op": "render", "slots": slots, "batch": batch or len(slots) > 1, "cfg": cfg or CONFIG_NAMES[int(g.integers(len(CONFIG_NAMES)))],
              "outputs": outputs or ("f32", "f32", "u8", "both")[int(g.integers(4))], "repeat": repeat, "buffer": buffer,
              "stream": int(g.integers(2)) if stream is None else stream, "lead": int(g.integers(3)), "gap": int(g.choice([0, 7, 100])), "wait": wait}
        if wait:
            self.synced()
        return self.emit(op)

    def do_pass(self, which=None, slots=None, stream=None, wait=True):
        g = self.g
        if which is None:
            which = PASSES[int(g.choice(len(PASSES), p=[0.22, 0.2, 0.2, 0.2, 0.06, 0.12]))]
        if which == "bake" and self.bakes >= 2:
            which = "layers"
        batch = slots is None and which != "pick" and g.random() < 0.35
        if slots is None:
            slots = self.subset() if batch else [int(g.choice(self.open()))]
        if which == "bake":
            slots = slots[:2 - self.bakes]
            self.bakes += len(slots)
        need = set().union(*[self.dirty[s] for s in slots])
        sync = len(need) > 1 or (stream is not None and bool(need - {stream})) or (which == "pick" and bool(need))
        if stream is None:
            stream = next(iter(need)) if len(need) == 1 else int(g.integers(2))
        if not sync and g.random() < 0.3:
            sync = True
        if sync:
            self.synced()
        op = {"op": "pass", "which": which, "slots": slots, "batch": batch or len(slots) > 1, "cfg": CONFIG_NAMES[int(g.integers(len(CONFIG_NAMES)))],
              "ground": float(g.uniform(-1.0, 0.5)), "grid": 1 if g.random() < 0.8 else 2, "stream": stream, "sync": sync, "wait": wait}
        if wait:
            self.synced()
        return self.emit(op)

    def stretch(self):
        """More than kTableSlots batch calls with no host wait in between: the mutations and the passes on one stream, the
        renders on either (the handles' events order them)."""
        g = self.g
        self.emit({"op": "sync"})
        self.synced()
        stream = int(g.integers(2))
        kinds = [k for k in ("S64", "S32") if len(self.open(k)) >= 1]
        calls = table_slots() + 2 + int(g.integers(3))
        for k in range(calls):
            kind = kinds[int(g.integers(len(kinds)))]
            r = k % 4 if k < 4 else int(g.integers(4))
            if r == 0:
                slots = self.subset(kind)
                self.emit({"op": "set_skin", "form": "batch", "slots": slots, "skins": [make_skin(g, kind) for _ in slots], "offset": 0,
                           "gap": int(g.choice([0, 4, 64])), "stream": stream})
            elif r == 1:
                slots = self.subset(kind)
                self.emit({"op": "set_view", "form": "batch", "slots": slots, "poses": [make_pose(g) for _ in slots] if g.random() < 0.7 else None,
                           "looks": [make_look(g) if g.random() < 0.8 else None for _ in slots], "stream": stream})
                if self.ops[-1]["poses"] is None and all(k is None for k in self.ops[-1]["looks"]):
                    self.ops[-1]["looks"][0] = make_look(g)
            elif r == 2:
                self.render(slots=self.subset(), cfg=("default", "spp2")[int(g.integers(2))], wait=False)
                self.ops[-1]["batch"] = True
            else:
                self.do_pass(which=("layers", "ground", "reflection", "light")[int(g.integers(4))], slots=self.subset(), stream=stream, wait=False)
                self.ops[-1]["batch"], self.ops[-1]["sync"] = True, False
        self.emit({"op": "sync"})
        self.synced()


def _near(g):
    return make_look(g, distance=float(g.uniform(8.0, 10.0)), centred=True)


def _far(g):
    return make_look(g, distance=float(g.uniform(170.0, 200.0)), centred=True)


def make_script(seed: int) -> dict:
    """{"seed", "handles", "ops"}: 18 to 40 operations, every create, close and host wait counted, and for even seeds a stretch of
    kTableSlots + 2 ... 4 batch calls between two host waits on top: 18 to 55 in all, more than the 20 to 30 first planned (what a
    block must hold is forced in, below, and the random steps come on top).  The seed's place in its block of six settles what a block must not miss: seed % 3 the kind of change under
    the replayed graph (the footprint, `posed`, the skin), seed % 7 the parts the replay handle's skin drops, seed % 6 a shell that
    changes hands through a plain scene (0) or the other kind (3), a bake (2) and a pick (4)."""
    g = np.random.default_rng([0x5EED, int(seed)])
    n = int(g.integers(2, 5))
    gen = _Gen(g, n)
    for s in range(n):
        gen.create(s)
    for s in range(n):
        if g.random() < 0.8:
            gen.set_skin(slot=s)
    # the replayed graph: one handle, one config, one buffer; record_at() + 1 renders at an unchanged state, a change, the same
    # render, the change back, the same render
    h = int(g.integers(n))
    cfg = ("default", "hard", "ao", "spp2")[int(g.integers(4))]
    key = f"replay-{h}-{cfg}"
    outputs = ("f32", "both")[int(g.integers(2))]
    variant = seed % 3
    gen.set_skin(slot=h, skin=make_skin(g, gen.kind[h], drop=seed % 7))  # the blocks reach every count of dropped parts
    if variant == 0:  # the footprint: near, far, near
        there, back = (None, _far(g)), (None, _near(g))
        gen.set_view(slot=h, form=("host", "device")[int(g.integers(2))], view=(make_pose(g), _near(g)))
        if seed % 2:
            there, back = (None, _near(g)), (None, _far(g))
            gen.ops[-1]["looks"] = [_far(g)]
    elif variant == 1:  # `posed`: true, false, true
        there, back = (np.zeros(12, f32), None), (M.getBuiltinPoses()[1 + int(g.integers(6))].astype(f32), None)
        gen.set_view(slot=h, form="device", view=(M.getBuiltinPoses()[6].astype(f32), make_look(g, distance=float(g.uniform(25, 45)), centred=True)))
    else:  # the skin: other opaque bits under the same view
        there = back = None
        gen.set_view(slot=h, form="batch", view=(make_pose(g), make_look(g, distance=float(g.uniform(20, 40)), centred=True)))
    gen.render(slots=[h], cfg=cfg, repeat=record_at() + 1, buffer=key, outputs=outputs)
    for view in (there, back):
        if view is None:
            gen.set_skin(slot=h)
        else:
            gen.set_view(slot=h, form=("host", "device", "batch")[int(g.integers(3))], view=view)
        gen.render(slots=[h], cfg=cfg, buffer=key, outputs=outputs)
    if variant == 2:  # a view change over the bits the skin has set, and a repaint over the view's: either order
        gen.set_view(slot=h)
        gen.emit({"op": "blob", "slot": h})
        gen.set_skin(slot=h)
        gen.emit({"op": "blob", "slot": h})
    gen.synced()
    stretch_at = int(g.integers(2, 4)) if seed % 2 == 0 else -1
    budget = int(g.integers(4, 9))
    for step in range(budget):
        if step == 1 and seed % 6 in (0, 3):  # the pooled shell changes hands
            slot = int(g.choice(gen.open()))
            gen.close(slot)
            gen.create(slot, between="plain" if seed % 6 == 0 else "other")
            gen.set_skin(slot=slot)
            gen.render(slots=[slot], wait=True)
            continue
        if step == 1 and seed % 6 in (2, 4):
            gen.do_pass(which="bake" if seed % 6 == 2 else "pick")
            if seed % 6 == 2:
                gen.ops[-1]["grid"] = 1
            continue
        if step == stretch_at:
            gen.stretch()
            continue
        r = g.random()
        if r < 0.10 and len(gen.open()) > 1:  # the pooled shell changes hands
            slot = int(g.choice(gen.open()))
            gen.close(slot)
            gen.create(slot, between=(None, "plain", "other")[int(g.integers(3))])
            gen.set_skin(slot=slot)
        elif r < 0.22:
            gen.set_skin()
        elif r < 0.36:
            gen.set_view()
        elif r < 0.42:
            gen.emit({"op": "set_background", "slot": int(g.choice(gen.open())), "mode": ("reference", "transparent")[int(g.integers(2))]})
        elif r < 0.66:
            gen.render()
        elif r < 0.94:
            gen.do_pass()
        else:
            gen.emit({"op": "blob", "slot": int(g.choice(gen.open()))})
    gen.emit({"op": "sync"})
    for s in gen.open():
        gen.emit({"op": "blob", "slot": s})
    for s in gen.open():
        gen.close(s)
    return {"seed": int(seed), "handles": n, "ops": gen.ops}


def _canon(v):
    if isinstance(v, np.ndarray):
        return (v.dtype.str, v.shape, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest())
    if isinstance(v, dict):
        return tuple((k, _canon(x)) for k, x in sorted(v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_canon(x) for x in v)
    return v


def script_digest(script) -> str:
    """Every argument of every operation, as one hash."""
    return hashlib.sha256(repr(_canon(script)).encode()).hexdigest()


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _white(kind):
    a = np.full((64 if kind == "S64" else 32, 64, 4), 255, np.uint8)
    a.setflags(write=False)
    return a


class State:
    """What a handle stands for."""

    def __init__(self, kind, pose, look):
        self.kind, self.skin = kind, _white(kind)
        self.pose = np.zeros(12, f32) if pose is None else np.asarray(pose, f32)
        self.look = look
        self.pose0, self.look0 = self.pose, self.look  # what the handle was created with
        self.background = "reference"
        self.stale_opaque = False  # (defect 1)
        self.history = ""  # the mutations so far: s = repaint, v = view

    def snapshot(self):
        return {"kind": self.kind, "skin": self.skin, "pose": self.pose, "look": self.look, "background": self.background,
                "stale_opaque": self.stale_opaque, "history": self.history[-2:]}


DEFECTS = {1: "MESH_OPAQUE is taken from the view's table instead of kept", 2: "a NULL pose falls back to the creation pose",
           3: "a NULL look falls back to the builder's default", 4: "a batch applies entry i to the i-th handle in sorted order",
           5: "the repaint leaves the last half wave of an S32 pool unwritten"}


class Model:
    """Applies a script's operations; apply(op) returns the checkpoints the operation makes: dicts {"what", "slot", "state", ...}.
    defect: 0, or one of DEFECTS — a deliberately wrong model, for the sensitivity checks."""

    def __init__(self, defect=0):
        self.defect = defect
        self.slots = {}

    def apply(self, op) -> list:
        kind = op["op"]
        if kind == "create":
            self.slots[op["slot"]] = State(op["kind"], op["pose"], op["look"])
        elif kind == "close":
            del self.slots[op["slot"]]
        elif kind == "set_background":
            self.slots[op["slot"]].background = op["mode"]
        elif kind == "set_skin":
            order = sorted(op["slots"]) if self.defect == 4 and op["form"] == "batch" else op["slots"]
            for slot, skin in zip(order, op["skins"]):
                st = self.slots[slot]
                if self.defect == 5 and st.kind == "S32":
                    keep = layout("S32")["pool"][-32:]
                    skin = np.array(skin)
                    skin.reshape(-1, 4)[keep] = st.skin.reshape(-1, 4)[keep]
                    skin.setflags(write=False)
                st.skin, st.stale_opaque = skin, False
                st.history += "s"
        elif kind == "set_view":
            order = sorted(op["slots"]) if self.defect == 4 and op["form"] == "batch" else op["slots"]
            for i, slot in enumerate(order):
                st = self.slots[slot]
                pose = None if op["poses"] is None else op["poses"][i]
                look = None if op["looks"] is None else op["looks"][i]
                st.pose = np.asarray(pose, f32) if pose is not None else (st.pose0 if self.defect == 2 else st.pose)
                st.look = look if look is not None else (None if self.defect == 3 else st.look)
                st.stale_opaque = self.defect == 1
                st.history += "v"
        elif kind == "render":
            return [{"what": "frame", "slot": s, "state": self.slots[s].snapshot(), "cfg": op["cfg"], "repeat": op["repeat"]} for s in op["slots"]]
        elif kind == "pass":
            return [{"what": op["which"], "slot": s, "state": self.slots[s].snapshot(), "cfg": op["cfg"], "ground": op["ground"], "grid": op["grid"]}
                    for s in op["slots"]]
        elif kind == "blob":
            return [{"what": "blob", "slot": op["slot"], "state": self.slots[op["slot"]].snapshot()}]
        return []


def checkpoints(script, defect=0) -> list:
    """[(operation index, checkpoint)] of the whole script."""
    model, out = Model(defect), []
    for i, op in enumerate(script["ops"]):
        out += [(i, c) for c in model.apply(op)]
    return out


def pick_pixels(cfg):
    ys, xs = np.mgrid[1:cfg.height:3, 0:cfg.width:5]
    return np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.int32)


# ---- the values ------------------------------------------------------------------------------------------------------------------
_CHECKER = []


def _transparent_checker():
    import batch_fuzz_cases

    return batch_fuzz_cases.transparent_checker_lib()


def blob_of(state) -> bytes:
    blob = S.expected_blob(state["skin"], state["pose"], state["look"])
    if state["stale_opaque"]:  # (defect 1) the white figure's bits
        white = S.expected_blob(_white(state["kind"]), state["pose"], state["look"])
        b = bytearray(blob)
        hdr = np.frombuffer(blob[:192], np.uint32)
        for m in range(int(hdr[1])):
            at = int(hdr[32]) + 192 * m + 68
            b[at:at + 4] = white[at:at + 4]
        blob = bytes(b)
    return blob


def mesh_flags(blob) -> np.ndarray:
    return np.frombuffer(S.blob_parts(blob)["mesh flags"], np.uint32)


class Expectations:
    """The values of checkpoints, computed once per state."""

    def __init__(self, oracle, threads=1):
        self.oracle, self.threads = oracle, threads
        self.cache = {}

    def _once(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    @staticmethod
    def key(state):
        return S._key(state["skin"], state["pose"], state["look"])

    def full(self, state):
        return S.full_table_scene(state["skin"], state["pose"], state["look"])

    def frame(self, state, cfg_name):
        """(frame, figure pixels: those with a sample whose primary ray hits the figure, meshes of the reference-shaped scene)"""
        cfg = CONFIGS[cfg_name]

        def make():
            import dataclasses

            sd = S.reference_scene(state["skin"], state["pose"], state["look"])
            frame, hits = _transparent_checker().render(sd.ptr, cfg, "transparent", threads=self.threads)
            if state["background"] != "transparent":
                frame = self.oracle.render(sd.ptr, dataclasses.replace(cfg, threadCount=self.threads))
            frame.setflags(write=False)
            return frame, int((hits > 0).sum()), int(sd.desc.n_meshes)

        return self._once(("frame", self.key(state), cfg_name, state["background"]), make)

    def full_table_frame(self, state, cfg_name):
        """The oracle's frame of the full-table scene: the dropped-part identity says it is frame()'s."""
        import dataclasses

        cfg, sd = CONFIGS[cfg_name], self.full(state)
        if state["background"] == "transparent":
            return _transparent_checker().render(sd.ptr, cfg, "transparent", threads=self.threads)[0]
        return self.oracle.render(sd.ptr, dataclasses.replace(cfg, threadCount=self.threads))

    def surfaces(self, state, cfg_name):
        cfg = CONFIGS[cfg_name]
        return self._once(("surfaces", self.key(state), cfg.width, cfg.height), lambda: L.expected_surfaces(self.oracle, self.full(state), cfg.width, cfg.height))

    def value(self, c):
        """The expectation of one checkpoint."""
        what, state = c["what"], c["state"]
        if what == "blob":
            return blob_of(state)
        if what == "frame":
            return self.frame(state, c["cfg"])
        if what in ("layers", "pick"):
            return self.surfaces(state, c["cfg"])
        cfg = CONFIGS[c["cfg"]]
        if what == "ground":
            return self._once(("ground", self.key(state), c["cfg"], c["ground"]), lambda: G.expected_ground(self.oracle, self.full(state), cfg, c["ground"]))
        if what == "reflection":
            return self._once(("reflection", self.key(state), c["cfg"], c["ground"]), lambda: R.expected_reflection(self.oracle, self.full(state), cfg, c["ground"]))
        if what == "light":
            return self._once(("light", self.key(state), c["cfg"]), lambda: LC.expected_light(self.oracle, self.full(state), cfg))
        if what == "bake":
            return self._once(("bake", self.key(state), c["cfg"], c["grid"]), lambda: BC.expected_bake(self.oracle, self.full(state), cfg, c["grid"]))
        raise KeyError(what)

    def of_script(self, script) -> list:
        """[(operation index, checkpoint, value)]"""
        return [(i, c, self.value(c)) for i, c in checkpoints(script)]


_WORKER = []


def worker_script_expectation(seed: int) -> list:
    """Expectations.of_script(make_script(seed)) on one thread and with a cache of its own: for a pool of processes that never
    touch the device."""
    import oraclelib

    if not _WORKER:
        _WORKER.append(oraclelib.Oracle())
    return Expectations(_WORKER[0], threads=1).of_script(make_script(seed))


# ---- the census --------------------------------------------------------------------------------------------------------------------
def posed(state) -> bool:
    return bool((mesh_flags(blob_of(state)) & MESH_ROTATED).any())


def census(scripts, expectations) -> dict:
    """What the oracle sees in the scripts — expectations: per script the list of Expectations.of_script."""
    ops, counts, figure = {}, {"S64": {}, "S32": {}}, []
    opaque_set, opaque_clear = [0] * 12, [0] * 12
    to_posed = to_plain = 0
    order = {"sv": 0, "vs": 0}
    zoom = {"in": 0, "out": 0, "in_replayed": 0, "out_replayed": 0}
    there_and_back = tail_mixed = renders = empty = 0
    for script, exp in zip(scripts, expectations):
        for op in script["ops"]:
            name = op["op"] + ("-" + op["form"] if "form" in op else "-" + op["which"] if "which" in op else "")
            if op["op"] in ("render", "pass"):
                name += "-batch" if op["batch"] else ""
            ops[name] = ops.get(name, 0) + 1
            if op["op"] == "set_skin":
                for skin in op["skins"]:
                    if skin.shape[0] == 32:
                        a = skin.reshape(-1, 4)[layout("S32")["pool"][-32:], 3]
                        tail_mixed += int((a == 0).any() and (a != 0).any())
        # the course of `posed` and of the footprint, per handle
        model, was, run = Model(), {}, {}
        last_frame, sighted = {}, {}
        values = {}
        for i, c, v in exp:
            values.setdefault(i, []).append((c, v))
        for i, op in enumerate(script["ops"]):
            model.apply(op)
            if op["op"] == "create":
                for d in (was, run, last_frame):
                    d.pop(op["slot"], None)
            if op["op"] in ("create", "set_view"):
                for s in ([op["slot"]] if op["op"] == "create" else op["slots"]):
                    now = posed(model.slots[s].snapshot())
                    if s in was and was[s] != now:
                        to_posed += int(now)
                        to_plain += int(not now)
                        run[s] = (run.get(s, "T" if was[s] else "F") + ("T" if now else "F"))[-3:]
                        there_and_back += int(run[s] == "TFT")
                    was[s] = now
            for c, v in values.get(i, []):
                state = c["state"]
                if c["what"] in ("frame", "blob"):
                    flags = mesh_flags(blob_of(state))
                    for m, f in enumerate(flags):
                        opaque_set[m] += int(bool(f & MESH_OPAQUE))
                        opaque_clear[m] += int(not f & MESH_OPAQUE)
                    white = mesh_flags(S.expected_blob(_white(state["kind"]), state["pose"], state["look"]))
                    if state["history"] in order and ((flags ^ white) & MESH_OPAQUE).any():
                        order[state["history"]] += 1
                if c["what"] == "frame":
                    frame, pixels, n_ref = v
                    cfg = CONFIGS[c["cfg"]]
                    px = cfg.width * cfg.height
                    counts[state["kind"]][n_ref] = counts[state["kind"]].get(n_ref, 0) + 1
                    figure.append(pixels)
                    renders += 1
                    empty += int(pixels == 0)
                    key = (c["slot"], c["cfg"], op["buffer"])
                    before = sighted.get(key, 0) if op["buffer"] else 0
                    prev = last_frame.get(c["slot"])
                    if prev is not None:
                        grew = prev < 0.1 and pixels / px > 0.5
                        shrank = prev > 0.5 and pixels / px < 0.1
                        zoom["in"] += int(grew)
                        zoom["out"] += int(shrank)
                        zoom["in_replayed"] += int(grew and before > record_at())
                        zoom["out_replayed"] += int(shrank and before > record_at())
                    last_frame[c["slot"]] = pixels / px
                    if op["buffer"]:
                        sighted[key] = before + op["repeat"]
    return {"ops": dict(sorted(ops.items())), "mesh_counts": {k: dict(sorted(v.items())) for k, v in counts.items()},
            "opaque_set": opaque_set, "opaque_clear": opaque_clear, "figure_pixels": figure, "to_posed": to_posed, "to_plain": to_plain,
            "posed_there_and_back": there_and_back, "opaque_differs_after": order, "zoom": zoom, "s32_tail_mixed": tail_mixed,
            "renders": renders, "empty_frames": empty}


def add_census(total: dict, c: dict) -> dict:
    """Adds a census to a running total (the figure pixels as their sum and the frames they fill by tenths)."""
    for k, v in c.items():
        if k == "figure_pixels":
            total["figure_pixels"] = total.get("figure_pixels", 0) + sum(v)
        elif isinstance(v, dict):
            add_census(total.setdefault(k, {}), v)
        elif isinstance(v, list):
            total[k] = [a + b for a, b in zip(total.get(k, [0] * len(v)), v)]
        else:
            total[k] = total.get(k, 0) + v
    return total


def block_scripts(first) -> list:
    return [make_script(first + k) for k in range(BLOCK_SIZE)]


_BLOCKS = {}


def block_expectations(oracle, first):
    """(scripts, their expectations, census) of a block, computed once per process."""
    if first not in _BLOCKS:
        scripts = block_scripts(first)
        e = Expectations(oracle, threads=2)
        exps = [e.of_script(s) for s in scripts]
        _BLOCKS[first] = (scripts, exps, census(scripts, exps))
    return _BLOCKS[first]


# first seed of a block -> the census the CPU oracle gives (tests/test_resident_fuzz_cases.py pins and explains it)
BLOCKS = {0: {'ops': {'blob': 19,
             'close': 21,
             'create': 21,
             'pass-bake': 1,
             'pass-ground': 3,
             'pass-ground-batch': 6,
             'pass-layers': 2,
             'pass-layers-batch': 2,
             'pass-pick': 1,
             'pass-reflection': 1,
             'pass-reflection-batch': 1,
             'render': 24,
             'render-batch': 12,
             'set_background': 2,
             'set_skin-batch': 18,
             'set_skin-device': 13,
             'set_skin-host': 12,
             'set_view-batch': 14,
             'set_view-device': 6,
             'set_view-host': 5,
             'sync': 12},
     'mesh_counts': {'S64': {6: 3, 7: 2, 10: 1, 11: 6, 12: 8}, 'S32': {6: 20, 7: 7}},
     'opaque_set': [28, 11, 28, 32, 26, 9, 22, 4, 14, 8, 4, 12],
     'opaque_clear': [38, 55, 38, 34, 40, 57, 44, 26, 16, 22, 26, 18],
     'figure_pixels': [828, 8, 610, 404, 337, 0, 47, 625, 0, 861, 248, 234, 183, 1044, 396, 183, 234, 601, 392, 114, 126, 136, 114, 419, 516, 870,
                       670, 4, 1536, 12, 26, 48, 141, 152, 163, 163, 163, 0, 163, 0, 254, 111, 0, 405, 504, 487, 202],
     'to_posed': 9,
     'to_plain': 5,
     'posed_there_and_back': 4,
     'opaque_differs_after': {'sv': 13, 'vs': 13},
     'zoom': {'in': 3, 'out': 2, 'in_replayed': 2, 'out_replayed': 2},
     's32_tail_mixed': 11,
     'renders': 47,
     'empty_frames': 5},
 6: {'ops': {'blob': 25,
             'close': 23,
             'create': 23,
             'pass-bake': 1,
             'pass-ground': 2,
             'pass-ground-batch': 4,
             'pass-layers': 1,
             'pass-layers-batch': 4,
             'pass-light-batch': 3,
             'pass-pick': 3,
             'pass-reflection-batch': 3,
             'render': 26,
             'render-batch': 8,
             'set_background': 4,
             'set_skin-batch': 17,
             'set_skin-device': 14,
             'set_skin-host': 15,
             'set_view-batch': 13,
             'set_view-device': 8,
             'set_view-host': 2,
             'sync': 12},
     'mesh_counts': {'S64': {6: 8, 7: 2, 8: 4, 9: 2, 10: 1, 11: 2, 12: 10}, 'S32': {6: 12, 7: 4}},
     'opaque_set': [28, 17, 24, 24, 32, 20, 17, 15, 21, 8, 10, 5],
     'opaque_clear': [42, 53, 46, 46, 38, 50, 53, 29, 23, 36, 34, 39],
     'figure_pixels': [845, 5, 657, 92, 22, 59, 795, 705, 3, 344, 848, 57, 1744, 1620, 1656, 415, 415, 151, 672, 442, 617, 68, 0, 0, 9, 0, 13, 3953,
                       27, 100, 6, 49, 34, 56, 44, 476, 44, 152, 44, 10, 194, 133, 236, 1536, 4096],
     'to_posed': 9,
     'to_plain': 5,
     'posed_there_and_back': 5,
     'opaque_differs_after': {'sv': 18, 'vs': 10},
     'zoom': {'in': 3, 'out': 3, 'in_replayed': 2, 'out_replayed': 2},
     's32_tail_mixed': 14,
     'renders': 45,
     'empty_frames': 3}}

def census_digest(script, exp) -> str:
    """The census of one script alone, as a short hash."""
    return hashlib.sha256(repr(census([script], [exp])).encode()).hexdigest()[:16]


_SCRIPTS = {}


def script_expectation(oracle, seed):
    """(script, its expectations, the digest of its census) of one script of a block, computed once per process."""
    if seed not in _SCRIPTS:
        script = make_script(seed)
        exp = Expectations(oracle, threads=2).of_script(script)
        _SCRIPTS[seed] = (script, exp, census_digest(script, exp))
    return _SCRIPTS[seed]


# seed of a block's script -> the digest of the census the CPU oracle gives for it alone: what a GPU test of one script asserts
SCRIPTS = {0: '180f5e246d33059f', 1: 'adf7055f21f9b3c2', 2: 'c442c53338cddc43', 3: '12370e4d9cb180f5', 4: 'e72f47ea0b34f364', 5: '1b678b40511402e3', 6: 'b14b45a9b8c3cf01', 7: '9039c1a3b09d406a', 8: 'be6ced561c724677', 9: '458832873b0498a3', 10: '3fa6a6d0c6a5a107', 11: 'd92aedb206875b5b'}
