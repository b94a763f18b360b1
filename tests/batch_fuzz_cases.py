"""Seeded random BATCHES for the HIP-vs-oracle parity sweep of the batched entries (tools/gpu_fuzz.py, modes batch and
pass-batch) and its fixed-seed run (tests/test_gpu_batch_fuzz.py, tests/test_batch_fuzz_cases.py).  The batched kernels run the
single-frame bodies; what a batch adds — per-frame rows of a device table, one kernel variant and one dynamic LDS size for all
frames, launch shapes taken from frame 0, per-frame output pointers and plane heights, the envelope and its fall-back — is met
only by frames that differ the way real batches do.  Every draw comes from a generator of its own: the seeds of fuzz_cases.py
and pass_fuzz_cases.py keep their meaning.

make_beauty_batch   one config (the config half of fuzz_cases.make_case) for 1 ... 16 frames whose scenes are the scene halves
                    of make_case, make_bundle_case and make_wide_case (2 : 1 : 1), one batch in eight with the 70-box scene
                    whose tables are read from HBM; one background mode per batch; outputs with a lead and a stride gap
make_pass_batch     16 cases of a group of pass_fuzz_cases.py under ONE config, each at its own plane height, one handle
                    listed twice at two heights
make_mixed_pass_batch  four cases each of bundle, wide, long-shadow and far-plane: coordinate magnitudes many orders apart
SPECIALS            fixed batches at configs the draws do not reach (the background kernel, four stream waves per tile, many
                    draws per sample, a batch of one, 300 frames in two launch sequences)

No device is used here."""
from __future__ import annotations

import atexit
import shutil
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

import fuzz_cases
import pass_fuzz_cases as PF

f32 = np.float32
SIZES = (1, 2, 3, 5, 8, 16)
K_MT_SHORT_MAX = 227    # launch_shapes.h: kMtShortMax
K_FLAT_MAX_BOUNCES = 8  # launch_shapes.h: kFlatMaxBounces
K_BATCH_MAX_FRAMES = 256  # kernels.h: kBatchMaxFrames


# ---- what a config means for the batched path, from the config alone -------------------------------------------------
def expected_envelope(cfg) -> bool:
    """Whether frames of `cfg` are inside the batched kernels' envelope: render_plan.cpp's needs_general_variant, negated."""
    soft = bool(cfg.softShadows) and cfg.shadowSamples > 1
    general = (cfg.maxBounces > K_FLAT_MAX_BOUNCES or (soft and 2 * cfg.shadowSamples > K_MT_SHORT_MAX)
               or (bool(cfg.aoEnabled) and (cfg.aoSamples <= 0 or 2 * cfg.aoSamples > K_MT_SHORT_MAX)))
    return not general


K_FACE_LDS_ENTRIES_MAX = 384  # kernels.h: kFaceLdsEntriesMax — six face entries per mesh: 64 meshes
K_ALPHA_LDS_WORDS_MAX = 4096  # kernels.h: kAlphaLdsWordsMax — 16 texels per word: 65 536 texels
MESH_OUTER, MESH_ROTATED = 1, 2  # flat_scene.h


def flat_header(scene) -> dict:
    """What render_plan.cpp's lds_fit is given, and the first-pass groups, read from the flattened blob (flat_scene.h) and never
    asked of the code under test: n_meshes, n_texels, alpha_words, posed (any mesh with MESH_ROTATED), roots (bit i: mesh
    i < 64 is a group root), and per mesh flags, group (64-bit word), lo, hi (3 floats each) and tex_off / tex_w / tex_h (6 ints)."""
    blob = M.flatten(scene)
    hdr = np.frombuffer(blob[:192], np.uint32)
    n, mesh_off = int(hdr[1]), int(hdr[32])
    mesh = np.frombuffer(blob[mesh_off:mesh_off + 192 * n], np.uint32).reshape(n, 48)
    flags = mesh[:, 17].copy()
    return {"n_meshes": n, "n_texels": int(hdr[2]), "alpha_words": int(hdr[36]), "posed": bool((flags & MESH_ROTATED).any()),
            "roots": int(hdr[37]) | (int(hdr[38]) << 32), "flags": flags,
            "group": [int(lo) | (int(hi) << 32) for lo, hi in zip(mesh[:, 44], mesh[:, 45])],
            "lo": mesh[:, 0:3].copy().view(f32), "hi": mesh[:, 3:6].copy().view(f32),
            "tex_off": mesh[:, 18:24].copy().view(np.int32), "tex_w": mesh[:, 24:30].copy().view(np.int32), "tex_h": mesh[:, 30:36].copy().view(np.int32)}


def expected_view(header: dict) -> str:
    """The scene view the kernels of a frame ALONE are compiled against — render_plan.cpp's lds_fit, restated: the tables go to LDS
    only if six face entries per mesh and the alpha words both fit; then the un-posed variants serve a scene without a rotated
    mesh.  "hbm" (kViewHbm), "lds" (kViewLds) or "lds-unposed" (kViewLdsUnposed).  A batch takes the weakest view of its frames."""
    fits = header["alpha_words"] <= K_ALPHA_LDS_WORDS_MAX and header["n_meshes"] * 6 <= K_FACE_LDS_ENTRIES_MAX
    return "hbm" if not fits else ("lds" if header["posed"] else "lds-unposed")


def expected_batch_info(cfg, n: int) -> dict:
    """last_batch_info() of a batch of n frames of one background mode."""
    if expected_envelope(cfg):
        return {"batched_frames": n, "launch_sequences": (n + K_BATCH_MAX_FRAMES - 1) // K_BATCH_MAX_FRAMES}
    return {"batched_frames": 0, "launch_sequences": n}


def draws_per_pixel(cfg) -> int:
    """samplesPerPixel x draws per sample (render_enqueue.cpp: draws_per_sample).  Above 24 no draw plate exists and, in
    reference mode, the background tiles' streams go through HBM too: the tile seeds are read."""
    spp = max(1, cfg.samplesPerPixel)
    return spp * ((2 if spp > 1 else 0) + (2 if cfg.dofEnabled and f32(cfg.aperture) > f32(1e-6) else 0))


# ---- beauty batches --------------------------------------------------------------------------------------------------
SCENE_KINDS = (("case", fuzz_cases.make_case), ("case", fuzz_cases.make_case), ("bundle", fuzz_cases.make_bundle_case),
               ("wide", fuzz_cases.make_wide_case))


def _scene(kind: int, seed: int):
    return SCENE_KINDS[kind][1](seed)[0]


def hbm_scene():
    import scenes

    return M.SceneDesc(scenes.many_boxes())


def make_beauty_batch(seed: int):
    """(scene descriptions, Config, background, layout, what); layout = {"gap", "lead" (pixels), "outputs" ("both" / "f32" /
    "u8")}: frame i starts lead + i * (width * height + gap) pixels into each output's allocation."""
    g = np.random.default_rng(seed ^ 0xBA7C0000)
    cfg_seed = int(g.integers(0, 1 << 30))
    cfg = fuzz_cases.make_case(cfg_seed)[1]  # drawn once per batch; the scene of that case is dropped
    n = int(SIZES[g.integers(0, len(SIZES))])
    hbm_at = int(g.integers(0, n)) if g.random() < 0.125 else -1
    sds, names = [], []
    for i in range(n):
        kind, s = int(g.integers(0, len(SCENE_KINDS))), int(g.integers(0, 1 << 30))
        if i == hbm_at:
            sds.append(hbm_scene())
            names.append("boxes70")
        else:
            sds.append(_scene(kind, s))
            names.append(f"{SCENE_KINDS[kind][0]} {s}")
    background = "transparent" if g.random() < 0.25 else "reference"
    layout = dict(gap=int([0, 0, 1, 100][g.integers(0, 4)]), lead=int([0, 0, 1, 2][g.integers(0, 4)]),
                  outputs=["both", "f32", "u8"][g.integers(0, 3)])
    kw = {k: getattr(cfg, k) for k in ("width", "height", "maxBounces", "samplesPerPixel", "tileSize")}
    what = f"batch seed {seed}: {n} frames [{'; '.join(names)}] config of seed {cfg_seed} {kw} {background} {layout}"
    return sds, cfg, background, layout, what


def _mixed_scenes(n: int, first: int, hbm_at: int = -1) -> list:
    """n scenes of the three generators in turn, from seeds first, first + 1, ..."""
    return [hbm_scene() if i == hbm_at else _scene((1, 2, 3)[i % 3], first + i) for i in range(n)]


def _special(name: str):
    plain = dict(gap=1, lead=1, outputs="both")
    grad = dict(gradientBg=True, gradientScale=0.7)
    if name in ("bg-kernel-33", "bg-kernel-40", "bg-kernel-transparent"):  # spp >= kSlabMinSpp: background_batch_kernel
        spp = 40 if name == "bg-kernel-40" else 33
        cfg = abi.Config(width=24, height=20, tileSize=8, samplesPerPixel=spp, maxBounces=2, shadowSamples=4, **grad)
        return _mixed_scenes(3, 81000), cfg, "transparent" if name.endswith("transparent") else "reference", plain
    if name in ("four-waves", "four-waves-transparent"):  # 32 x 32 x 40 x 2 draws = 132 twists >= 128: four stream waves per tile
        cfg = abi.Config(width=40, height=36, tileSize=32, samplesPerPixel=40, maxBounces=1, shadowSamples=2, **grad)
        return _mixed_scenes(3, 81100), cfg, "transparent" if name.endswith("transparent") else "reference", plain
    if name == "dof-13":  # four draws per sample, 52 per pixel, a tile of 50 clipped to 50 x 50 and 10 x 6
        cfg = abi.Config(width=60, height=56, tileSize=50, samplesPerPixel=13, maxBounces=2, dofEnabled=True, aperture=0.3, focusDistance=45.0)
        return _mixed_scenes(4, 81200, hbm_at=2), cfg, "reference", plain
    if name == "alone":  # a batch without company
        cfg = abi.Config(width=33, height=21, tileSize=16, samplesPerPixel=3, maxBounces=3, aoEnabled=True, aoSamples=5)
        return _mixed_scenes(1, 81300), cfg, "reference", dict(gap=100, lead=2, outputs="both")
    if name == "three-hundred":  # two launch sequences; per-frame grids at kBatchMinGrid in the first
        cfg = abi.Config(width=24, height=17, tileSize=8, samplesPerPixel=2, maxBounces=1)
        return _mixed_scenes(300, 82000, hbm_at=77), cfg, "reference", dict(gap=0, lead=0, outputs="f32")
    raise KeyError(name)


def make_far_camera_dof_batch():
    """The smallest batch that failed in the sweep tools/gpu_fuzz.py 100000 1000 batch (seed 100411, frame 9), as a batch of one: nine
    boxes scaled by 1e6, the camera 5.7e7 from the origin, under a config with depth of field (aperture 0.05, focus distance 10),
    3 spp and 1 x 1 tiles.  One ulp of the camera's coordinates is 4, so the thin-lens ray's origin and focus point
    (tile_renderer.cpp:42-69) are rounded by about the focus distance and its direction is far off the pinhole's."""
    sd = fuzz_cases.make_wide_case(1070025941)[0]
    cfg = fuzz_cases.make_case(238833773)[1]
    return [sd], cfg, "reference", dict(gap=0, lead=0, outputs="f32"), "regression far camera with depth of field: wide 1070025941 under the config of seed 238833773"


SPECIALS = ("bg-kernel-33", "bg-kernel-40", "four-waves", "bg-kernel-transparent", "four-waves-transparent", "dof-13", "alone",
            "three-hundred")


def make_special_batch(name: str):
    sds, cfg, background, layout = _special(name)
    return sds, cfg, background, layout, f"special batch {name}: {len(sds)} frames {cfg.width}x{cfg.height} tile {cfg.tileSize} spp {cfg.samplesPerPixel} {background}"


# ---- the oracle's frames ---------------------------------------------------------------------------------------------
_CHECKER = []


def transparent_checker_lib():
    """tests/transparent_checker.py's Checker, built once per process into a temporary directory."""
    import transparent_checker

    if not _CHECKER:
        d = tempfile.mkdtemp(prefix="batch_fuzz_checker_")
        atexit.register(shutil.rmtree, d, True)
        _CHECKER.append(transparent_checker.Checker(transparent_checker.build(d)))
    return _CHECKER[0]


def expected_frames(oracle, sds, cfg, background, with_hits=True, threads=None) -> list:
    """Per frame (frame (H, W, 4) float32, pixels with a sample whose primary ray hits a mesh): oracle.render, or in
    transparent mode the transparent checker's frame; the hit counts are the checker's in both modes (-1 without with_hits,
    which spares reference mode the checker's render).  threads: CPU threads per render (default: the machine's); the frames
    do not depend on it."""
    import dataclasses

    import transparent_checker

    # 300 small frames, or frames of one or two tiles (a tile is one thread's work): one thread per frame, the frames side by side
    tiles = -(-cfg.width // cfg.tileSize) * -(-cfg.height // cfg.tileSize)
    many = threads is None and len(sds) > 1 and (len(sds) > 16 or tiles < 4)
    n_threads = 1 if many else (transparent_checker.threads() if threads is None else int(threads))
    ocfg = cfg if threads is None and not many else dataclasses.replace(cfg, threadCount=n_threads)

    def one(sd):
        frame, hits = None, None
        if with_hits or background == "transparent":
            frame, hits = transparent_checker_lib().render(sd.ptr, cfg, "transparent", threads=n_threads)
        if background != "transparent":
            frame = oracle.render(sd.ptr, ocfg)
        frame.setflags(write=False)
        return frame, int((hits > 0).sum()) if with_hits else -1

    if many:
        with ThreadPoolExecutor(transparent_checker.threads()) as pool:  # (ctypes releases the GIL during a render)
            return list(pool.map(one, sds))
    return [one(sd) for sd in sds]


_CACHE = {}


def beauty_expectation(oracle, key, with_hits=True) -> tuple:
    """(case, expected frames) of a beauty batch seed or a special batch's name, computed once per process."""
    if (key, True) in _CACHE:
        return _CACHE[(key, True)]
    if (key, with_hits) not in _CACHE:
        case = make_special_batch(key) if isinstance(key, str) else make_beauty_batch(key)
        _CACHE[(key, with_hits)] = (case, expected_frames(oracle, case[0], case[1], case[2], with_hits))
    return _CACHE[(key, with_hits)]


def distinct_frames(exp) -> tuple:
    """(frames without a hit, frames WITH a hit that equal another frame of the batch as bytes)"""
    seen, same, empty = set(), 0, 0
    for frame, hits in exp:
        if hits == 0:
            empty += 1
            continue
        b = frame.tobytes()
        same += b in seen
        seen.add(b)
    return empty, same


# ---- pass batches ----------------------------------------------------------------------------------------------------
PASS_GROUPS = ("bundle", "wide", "long-shadow", "far-plane")


def _shared_pass_config(g):
    bcfg = fuzz_cases.make_bundle_case(int(g.integers(0, 1 << 30)))[1]  # tile, shadows and bounces as make_pass_case draws them
    return abi.Config(width=int(g.integers(17, 57)), height=int(g.integers(13, 41)), tileSize=bcfg.tileSize, softShadows=bcfg.softShadows,
                      shadowSamples=bcfg.shadowSamples, maxBounces=1 + bcfg.maxBounces % 3)


def _pass_batch(cases, g, what):
    cfg = _shared_pass_config(g)
    sds, heights = [c[0] for c in cases], [c[2] for c in cases]
    k = int(g.integers(0, len(cases)))
    lo, hi = PF.y_range(sds[k])
    second = float(f32(lo + float(g.uniform(-0.3, 0.5)) * (hi - lo)))
    if second == heights[k]:
        second = float(f32(lo - 0.25 * (hi - lo)))
    what = (f"{what}: {cfg.width}x{cfg.height} tile {cfg.tileSize} S {cfg.shadowSamples} bounces {cfg.maxBounces}; frame {k} again at "
            f"{second!r}")
    return sds, cfg, heights, (k, second), what


def make_pass_batch(group: str, first: int):
    """(scene descriptions, shared Config, plane heights, (index, second height), what): the 16 cases of
    pass_fuzz_cases.block_cases(group, first), each with its own scene and plane; the ground and reflection batches list
    handle `index` once more, at the second height."""
    g = np.random.default_rng((first * 4 + PASS_GROUPS.index(group)) ^ 0x9A55BA7C)
    return _pass_batch(PF.block_cases(group, first), g, f"pass batch {group} {first}")


def make_mixed_pass_batch(first: int):
    """Four cases each of bundle, wide, long-shadow and far-plane, from seed `first` of each group, interleaved."""
    per = [PF.block_cases(grp, first, 4) for grp in PASS_GROUPS]
    cases = [per[j][i] for i in range(4) for j in range(4)]
    return _pass_batch(cases, np.random.default_rng(first ^ 0x3A55BA7C), f"pass batch mixed {first}")


def make_pass_batch_of(key):
    group, first = key
    return make_mixed_pass_batch(first) if group == "mixed" else make_pass_batch(group, first)


def frames_of_pass_batch(batch) -> list:
    """(handle index, height) per frame of the ground and reflection batches: the 16, then the one listed twice."""
    sds, _, heights, (k, second), _ = batch
    return [(i, heights[i]) for i in range(len(sds))] + [(k, second)]


def pass_expectation(oracle, key) -> tuple:
    """(batch, ground expectations, reflection expectations per frame of frames_of_pass_batch, surfaces per scene), once per
    process and never modified."""
    import ground_checker as G
    import layers_checker as L
    import reflection_checker as R

    ck = ("pass",) + tuple(key)
    if ck not in _CACHE:
        batch = make_pass_batch_of(key)
        sds, cfg = batch[0], batch[1]
        ground = [G.expected_ground(oracle, sds[i], cfg, h) for i, h in frames_of_pass_batch(batch)]
        reflection = [R.expected_reflection(oracle, sds[i], cfg, h) for i, h in frames_of_pass_batch(batch)]
        surfaces = [L.expected_surfaces(oracle, sd, cfg.width, cfg.height) for sd in sds]
        for e in ground + reflection + surfaces:
            for a in e.values():
                a.setflags(write=False)
        _CACHE[ck] = (batch, ground, reflection, surfaces)
    return _CACHE[ck]


def pass_totals(ground, reflection, surfaces) -> tuple:
    """(dark, penumbra, reflected, layer-hit) pixels of a pass batch's expectations."""
    import ground_checker as G

    gc = np.sum([G.counts(e) for e in ground], axis=0)
    return int(gc[1]), int(gc[2]), int(sum(int(e["hit"].sum()) for e in reflection)), int(sum(int(e["hit"].sum()) for e in surfaces))


# ---- expectations made ahead of the device by worker processes (the long sweeps) --------------------------------------
_WORKER = {}


def _worker_oracle():
    import oraclelib

    if "oracle" not in _WORKER:
        _WORKER["oracle"] = oraclelib.Oracle()
    return _WORKER["oracle"]


def worker_beauty_frames(seed: int) -> list:
    """expected_frames of make_beauty_batch(seed), on two threads: for a pool of processes that never touch the device."""
    case = make_beauty_batch(seed)
    return expected_frames(_worker_oracle(), case[0], case[1], case[2], with_hits=True, threads=2)


def worker_pass_expectation(key) -> tuple:
    """(ground, reflection, surfaces) of pass_expectation(key), likewise."""
    out = pass_expectation(_worker_oracle(), tuple(key))[1:]
    _CACHE.clear()
    return out


# ---- the fixed blocks of the suite -----------------------------------------------------------------------------------
# The ORACLE's totals, measured on the CPU and asserted exactly by tests/test_batch_fuzz_cases.py: per block of four beauty
# batches the hit pixels of its frames, per special batch the same, per pass batch (dark, penumbra, reflected, layer hits).
BLOCK_SIZE = 4
# first seed of a block -> hit pixels of its four batches.  The blocks are chosen, not consecutive: over them the oracle alone
# satisfies every condition of tests/test_batch_fuzz_cases.py (a quarter of the batches with more than 24 draws per pixel, which
# one config in six has; no batch whose only hit lies in one frame), and no batch takes the CPU more than a few seconds.
BEAUTY_BLOCKS = {
    31008: 11604,
    31012: 6485,
    31060: 3979,
    31076: 3915,
    31092: 36290,
    31096: 9354,
    31164: 26504,
    31168: 54277,
    31172: 2897,
    31176: 14675,
    31180: 23143,
    31196: 10824,
}
# name -> (hit pixels, frames without a hit, frames with a hit that equal another frame of the batch: at 24 x 17 two of 300 do)
SPECIAL_TOTALS = {
    "bg-kernel-33": (484, 0, 0),
    "bg-kernel-40": (485, 0, 0),
    "four-waves": (1945, 0, 0),
    "bg-kernel-transparent": (484, 0, 0),
    "four-waves-transparent": (1945, 0, 0),
    "dof-13": (3262, 0, 0),
    "alone": (60, 0, 0),
    "three-hundred": (25456, 1, 2),
}
# (group, first) -> (dark, penumbra, reflected, layer-hit) pixels; each holds at least 100 dark, penumbra and reflected pixels
PASS_BATCHES = {
    ("bundle", 7100): (3145, 857, 1820, 4806),
    ("wide", 9116): (4242, 2599, 812, 3072),
    ("long-shadow", 12212): (5264, 1665, 205, 3805),
    ("far-plane", 15116): (886, 1179, 124, 23),
    ("mixed", 7200): (1344, 1374, 388, 1990),
    ("mixed", 7232): (3283, 1203, 701, 2548),
}
PASS_IDS = [f"{g}-{s}" for g, s in PASS_BATCHES]


def block_seeds(first: int) -> range:
    return range(first, first + BLOCK_SIZE)


def all_beauty_seeds() -> list:
    return [s for first in BEAUTY_BLOCKS for s in block_seeds(first)]


def host_form_seeds() -> list:
    """The third of the drawn batches that also runs through TileRenderer.renderBatch."""
    return [s for s in all_beauty_seeds() if s % 3 == 0]
