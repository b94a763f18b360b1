"""Loaders for the TEST-ONLY libraries: the CPU oracle (oracle/libmcrt_oracle.so) and, when it has
been built in the dev container, the compiled reference (oracle/_ref/libmcref.so)."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

from minecraftskin_raytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "libmcrt_oracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcref.so")


def build_oracle() -> None:
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)


class CpuLib:
    """Common wrapper for the oracle (prefix mcrt_oracle_) and the reference (prefix mcref_)."""

    def __init__(self, path: str, prefix: str):
        self.lib = C.CDLL(path)
        self.prefix = prefix
        abi.declare_common(self.lib, prefix)
        fn = getattr(self.lib, prefix + "render")
        fn.restype = C.c_int
        fn.argtypes = [C.POINTER(abi.McrtSceneDesc), C.POINTER(abi.McrtConfig), abi.c_float_p, abi.PROGRESS_FN, C.c_void_p]

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def render(self, desc_ptr, cfg: abi.Config, progress=None) -> np.ndarray:
        c = cfg.to_c()
        out = np.zeros((max(cfg.height, 0), max(cfg.width, 0), 4), np.float32)
        cb = abi.PROGRESS_FN(progress) if progress else C.cast(None, abi.PROGRESS_FN)
        buf = out if out.size else np.zeros(4, np.float32)
        self._f("render")(desc_ptr, C.byref(c), abi.fptr(buf), cb, None)
        return out

    def render_rows(self, desc_ptr, cfg: abi.Config, row_first: int, row_step: int, frame: np.ndarray) -> int:
        """Tile rows row_first, row_first + row_step, ... into `frame` (H, W, 4) on the library's thread pool; returns
        the number of tiles rendered."""
        c = cfg.to_c()
        f = self._f("render_rows")
        f.restype = C.c_int
        f.argtypes = [C.POINTER(abi.McrtSceneDesc), C.POINTER(abi.McrtConfig), C.c_int, C.c_int, abi.c_float_p]
        return int(f(desc_ptr, C.byref(c), row_first, row_step, abi.fptr(frame)))

    def render_tile(self, desc_ptr, cfg: abi.Config, tile, frame: np.ndarray) -> None:
        c = cfg.to_c()
        t = abi.McrtTile(*tile)
        self._f("render_tile")(desc_ptr, C.byref(c), C.byref(t), abi.fptr(frame))

    def generate_tiles(self, w, h, ts):
        n = self._f("generate_tiles")(w, h, ts, None, 0)
        arr = (abi.McrtTile * max(n, 1))()
        self._f("generate_tiles")(w, h, ts, arr, n)
        return [(arr[i].x, arr[i].y, arr[i].width, arr[i].height) for i in range(n)]

    def intersect(self, desc_ptr, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), abi.HIT_DTYPE)
        self._f("intersect")(desc_ptr, abi.fptr(rays), len(rays), out.ctypes.data)
        return out

    def intersect_mesh(self, desc_ptr, mesh_index: int, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), abi.HIT_DTYPE)
        self._f("intersect_mesh")(desc_ptr, mesh_index, abi.fptr(rays), len(rays), out.ctypes.data)
        return out

    def trace(self, desc_ptr, cfg, rays: np.ndarray, depth: int, max_bounces: int) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), 4), np.float32)
        c = cfg.to_c() if cfg is not None else None
        self._f("trace")(desc_ptr, C.byref(c) if c is not None else None, abi.fptr(rays), len(rays), depth, max_bounces, abi.fptr(out))
        return out

    def shade(self, desc_ptr, hit_rec, view_dir, params=None, shadow_factor=-1.0) -> np.ndarray:
        h = abi.McrtHit()
        h.hit = int(hit_rec["hit"])
        h.t = float(hit_rec["t"])
        for k in range(3):
            h.point[k] = float(hit_rec["point"][k])
            h.normal[k] = float(hit_rec["normal"][k])
        for k in range(4):
            h.texture_color[k] = float(hit_rec["texture_color"][k])
        h.is_outer_layer = int(hit_rec["is_outer_layer"])
        v = np.asarray(view_dir, np.float32)
        p = np.asarray(params, np.float32) if params is not None else None
        out = np.zeros(4, np.float32)
        self._f("shade")(desc_ptr, C.byref(h), abi.fptr(v), abi.fptr(p) if p is not None else None, C.c_float(shadow_factor), abi.fptr(out))
        return out

    def in_shadow(self, desc_ptr, point, normal, light_pos) -> bool:
        a, b, c = (np.asarray(x, np.float32) for x in (point, normal, light_pos))
        return bool(self._f("in_shadow")(desc_ptr, abi.fptr(a), abi.fptr(b), abi.fptr(c)))

    def soft_shadow(self, desc_ptr, point, normal, samples: int, seed: int) -> float:
        a, b = (np.asarray(x, np.float32) for x in (point, normal))
        return float(self._f("soft_shadow")(desc_ptr, abi.fptr(a), abi.fptr(b), samples, seed & 0xFFFFFFFF))

    def ao(self, desc_ptr, point, normal, samples: int, radius: float, seed: int) -> float:
        a, b = (np.asarray(x, np.float32) for x in (point, normal))
        return float(self._f("ao")(desc_ptr, abi.fptr(a), abi.fptr(b), samples, C.c_float(radius), seed & 0xFFFFFFFF))

    def soft_shadow_many(self, desc_ptr, points, normals, samples: int, seeds) -> np.ndarray:
        """soft_shadow at every row of points / normals (n, 3) with its own seed: (n,) float32."""
        return np.array([self.soft_shadow(desc_ptr, p, n, samples, int(s)) for p, n, s in zip(points, normals, seeds)], np.float32)

    def ao_many(self, desc_ptr, points, normals, samples: int, radius: float, seeds) -> np.ndarray:
        return np.array([self.ao(desc_ptr, p, n, samples, radius, int(s)) for p, n, s in zip(points, normals, seeds)], np.float32)

    def background(self, desc_ptr, cfg, u: float, v: float) -> np.ndarray:
        out = np.zeros(4, np.float32)
        c = cfg.to_c() if cfg is not None else None
        self._f("background")(desc_ptr, C.byref(c) if c is not None else None, C.c_float(u), C.c_float(v), abi.fptr(out))
        return out

    def camera_ray(self, desc_ptr, u: float, v: float, aspect: float) -> np.ndarray:
        out = np.zeros(6, np.float32)
        self._f("camera_ray")(desc_ptr, C.c_float(u), C.c_float(v), C.c_float(aspect), abi.fptr(out))
        return out

    def seed_cast(self, f: float) -> int:
        return int(self._f("seed_cast")(C.c_float(f)))

    def quantize(self, rgba: np.ndarray) -> np.ndarray:
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 4)
        out = np.zeros((len(rgba), 4), np.uint8)
        self._f("quantize")(abi.fptr(rgba), out.ctypes.data_as(C.POINTER(C.c_uint8)), len(rgba))
        return out


class Oracle(CpuLib):
    def __init__(self):
        if not os.path.exists(ORACLE_SO):
            build_oracle()
        super().__init__(ORACLE_SO, "mcrt_oracle_")

    def mt_uniform(self, seed: int, n: int, std: bool = False) -> np.ndarray:
        out = np.zeros(n, np.float32)
        self._f("mt_uniform_std" if std else "mt_uniform")(seed & 0xFFFFFFFF, n, abi.fptr(out))
        return out


class Reference(CpuLib):
    """The compiled reference; only available where oracle/_ref/libmcref.so exists."""

    def __init__(self):
        super().__init__(REF_SO, "mcref_")

    @staticmethod
    def available() -> bool:
        return os.path.exists(REF_SO)

    def build_skin_scene(self, skin_rgba8: np.ndarray, pose=None) -> dict:
        skin = np.ascontiguousarray(skin_rgba8, np.uint8)
        h, w = skin.shape[:2]
        p = np.asarray(pose if pose is not None else [0.0] * 12, np.float32)
        out = C.POINTER(abi.McrtSceneDesc)()
        rc = self._f("build_skin_scene")(skin.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, abi.fptr(p), C.byref(out))
        if rc != 0:
            raise RuntimeError(f"mcref_build_skin_scene failed: {rc}")
        d = abi.desc_to_numpy(out.contents)
        self._f("scene_desc_free")(out)
        return d

    def build_default_scene(self, pose=None) -> dict:
        p = np.asarray(pose if pose is not None else [0.0] * 12, np.float32)
        out = C.POINTER(abi.McrtSceneDesc)()
        self._f("build_default_scene")(abi.fptr(p), C.byref(out))
        d = abi.desc_to_numpy(out.contents)
        self._f("scene_desc_free")(out)
        return d

    def write_png(self, path: str, image: np.ndarray) -> bool:
        """ImageWriter::writePNG of the reference (quantise + stbi_write_png)."""
        img = np.ascontiguousarray(image, np.float32)
        f = self._f("write_png")
        f.argtypes = [C.c_char_p, abi.c_float_p, C.c_int, C.c_int]
        return bool(f(os.fsencode(path), abi.fptr(img), img.shape[1], img.shape[0]))

    def load_png(self, path: str, max_pixels: int = 1 << 24):
        """Image::load of the reference (stb decoder, /255.0f) → (H, W, 4) float32 or None."""
        buf = np.zeros(max_pixels * 4, np.float32)
        w, h = C.c_int(), C.c_int()
        f = self._f("load_png")
        f.argtypes = [C.c_char_p, abi.c_float_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if not f(os.fsencode(path), abi.fptr(buf), max_pixels, C.byref(w), C.byref(h)):
            return None
        return buf[: w.value * h.value * 4].reshape(h.value, w.value, 4).copy()

    def builtin_pose(self, index: int) -> np.ndarray:
        out = np.zeros(12, np.float32)
        if self._f("builtin_pose")(index, abi.fptr(out)) != 0:
            raise IndexError(index)
        return out


# ---- the compiled reference's answers, stored: the oracle-vs-reference tests where oracle/_ref cannot be built ----
REF_OUTPUTS = os.path.join(ROOT, "tests", "golden", "reference_outputs.npz")
_REPLAYED = ("builtin_pose", "build_skin_scene", "build_default_scene", "render", "intersect", "seed_cast", "soft_shadow_many", "ao_many")


STORED_IN_FULL_BYTES = 256  # larger answers (and structured ones) are stored as digests (RecordedArray)


def _canonical_floats(a) -> np.ndarray:
    """The bits scenes.assert_bit_equal compares: float32, with every NaN alike (NaN payloads may differ)."""
    f = np.array(a, np.float32, order="C")
    f[np.isnan(f)] = np.float32("nan")
    return f


def digest(a, kind: str) -> str:
    """SHA-256 of what one comparison of the tests looks at: "bytes" = the raw bytes (scene data), "floats" = the
    canonical float32 bits (renders), "hits" = hit flags, then t / point / normal / texture_color / outer flag of the
    rows that hit (what scenes.assert_hits_equal compares)."""
    h = hashlib.sha256()
    if kind == "bytes":
        h.update(np.ascontiguousarray(a).tobytes())
    elif kind == "floats":
        h.update(_canonical_floats(a).tobytes())
    elif kind == "hits":
        m = a["hit"] != 0
        h.update(np.ascontiguousarray(a["hit"]).tobytes())
        for f in ("t", "point", "normal", "texture_color"):
            h.update(_canonical_floats(a[f][m]).tobytes())
        h.update(np.ascontiguousarray(a["is_outer_layer"][m]).tobytes())
    else:
        raise ValueError(kind)
    return h.hexdigest()


class RecordedArray:
    """A large reference answer as stored: its shape, dtype and the digest of what its comparison looks at.
    matches(a, kind) holds exactly when that comparison between `a` and the answer itself would pass."""

    def __init__(self, shape, dtype: str, kind: str, sha256: str):
        self.shape, self.dtype, self.kind, self.sha256 = tuple(shape), dtype, kind, sha256

    def matches(self, a, kind: str) -> bool:
        if kind != self.kind:
            raise ValueError(f"a {self.kind} digest was recorded for this answer, not a {kind} one")
        if kind == "bytes":
            return digest(a, kind) == self.sha256
        a = np.asarray(a)
        if kind == "hits" and str(a.dtype) != self.dtype:
            return False
        return a.shape == self.shape and digest(a, kind) == self.sha256


# which comparison each method's answers meet in the tests (scenes.assert_bit_equal / assert_hits_equal / same_bytes)
_DIGEST_KIND = {"render": "floats", "intersect": "hits", "soft_shadow_many": "floats", "ao_many": "floats"}


def _to_spec(value, blob: bytearray, kind: str):
    """A reference return value as JSON-able structure: small numpy leaves are packed into `blob`, larger ones are
    stored as a RecordedArray digest of `kind`."""
    if isinstance(value, np.ndarray) and (value.nbytes > STORED_IN_FULL_BYTES or value.dtype.fields):
        return {"recorded": {"shape": list(value.shape), "dtype": str(value.dtype), "kind": kind, "sha256": digest(value, kind)}}
    if isinstance(value, (np.ndarray, np.generic)):
        arr = np.ascontiguousarray(value)
        spec = {"array" if isinstance(value, np.ndarray) else "scalar": [len(blob), arr.dtype.str, list(arr.shape)]}
        blob += arr.tobytes()
        return spec
    if isinstance(value, dict):
        return {"dict": {k: _to_spec(v, blob, kind) for k, v in value.items()}}
    if isinstance(value, (list, tuple)):
        return {"list": [_to_spec(v, blob, kind) for v in value]}
    if value is None or isinstance(value, (bool, int, float)):
        return {"value": value}
    raise TypeError(f"cannot store a {type(value).__name__}")


def _from_spec(spec, blob: np.ndarray):
    if "recorded" in spec:
        return RecordedArray(**spec["recorded"])
    for key in ("array", "scalar"):
        if key in spec:
            off, dtype, shape = spec[key]
            arr = np.frombuffer(blob, np.dtype(dtype), count=int(np.prod(shape, dtype=np.int64)), offset=off).reshape(shape).copy()
            return arr if key == "array" else arr[()]
    if "dict" in spec:
        return {k: _from_spec(v, blob) for k, v in spec["dict"].items()}
    if "list" in spec:
        return [_from_spec(v, blob) for v in spec["list"]]
    return spec["value"]


class RecordingReference:
    """The live reference, logging every answer of one test (conftest writes the log to REF_OUTPUTS)."""

    def __init__(self, live: Reference, log: list):
        self._live, self._log = live, log

    def __getattr__(self, name):
        if name not in _REPLAYED:
            raise AttributeError(f"{name} is not recorded (add it to oraclelib._REPLAYED)")
        fn = getattr(self._live, name)

        def call(*args, **kw):
            out = fn(*args, **kw)
            self._log.append((name, out))
            return out
        return call


def write_reference_outputs(logs: dict, path: str = REF_OUTPUTS) -> None:
    blob, index = bytearray(), {}
    for test, calls in sorted(logs.items()):
        index[test] = [[name, _to_spec(out, blob, _DIGEST_KIND.get(name, "bytes"))] for name, out in calls]
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index, separators=(",", ":")).encode(), np.uint8),
                        blob=np.frombuffer(bytes(blob), np.uint8))


class ReplayReference:
    """Answers one test's reference calls, in order, from REF_OUTPUTS (recorded from the compiled reference by
    running the same test with MCRT_RECORD_REFERENCE=1 where oracle/_ref is built)."""

    _store = None

    def __init__(self, test: str):
        if ReplayReference._store is None:
            z = np.load(REF_OUTPUTS)
            ReplayReference._store = (json.loads(z["index"].tobytes()), z["blob"])
        index, self._blob = ReplayReference._store
        if test not in index:
            raise KeyError(f"{os.path.relpath(REF_OUTPUTS, ROOT)} holds no reference answers for {test}: record them again")
        self._calls, self._test, self._n = index[test], test, 0

    def __getattr__(self, name):
        if name not in _REPLAYED:
            raise AttributeError(name)

        def call(*args, **kw):
            assert self._n < len(self._calls), f"{self._test}: more reference calls than were recorded"
            recorded, spec = self._calls[self._n]
            assert recorded == name, f"{self._test}: call {self._n} is {name}, recorded {recorded}: record the answers again"
            self._n += 1
            return _from_spec(spec, self._blob)
        return call
