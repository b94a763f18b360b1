"""The test-side checker of MCRT_BACKGROUND_TRANSPARENT (tests/cpp/transparent_oracle.cpp): compiled with g++ into a
temporary directory by a session fixture of the tests that use it, with the oracle's flags (oracle/Makefile)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from minecraftskin_raytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "transparent_oracle.cpp")
# oracle/Makefile's CXXFLAGS and include path, plus hidden visibility: only render_tiles is exported
FLAGS = ["-std=c++17", "-O3", "-DNDEBUG", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden"]


def build(out_dir: str) -> str:
    so = os.path.join(out_dir, "libtransparent_oracle.so")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, *FLAGS, "-I", os.path.join(ROOT, "include"), "-shared", "-o", so, SOURCE, "-lpthread", "-lm"])
    return so


class Checker:
    def __init__(self, so_path: str):
        self.lib = C.CDLL(so_path)
        f = self.lib.render_tiles
        f.restype = C.c_int
        f.argtypes = [C.POINTER(abi.McrtSceneDesc), C.POINTER(abi.McrtConfig), C.c_int, C.POINTER(abi.McrtTile), C.c_int,
                      abi.c_float_p, C.POINTER(C.c_int32)]

    def render(self, desc_ptr, cfg: abi.Config, background: str = "transparent", tiles=None, threads: int = 1):
        """(frame (H, W, 4) float32, hit counts (H, W) int32) of the given tiles (default: every tile of the frame);
        pixels outside them are NaN in the frame and -1 in the counts.  `threads` > 1 spreads the tiles over a pool."""
        mode = abi.background_mode(background)
        h, w = cfg.height, cfg.width
        frame = np.full((h, w, 4), np.nan, np.float32)
        hits = np.full((h, w), -1, np.int32)
        if tiles is None:
            ts = cfg.tileSize
            tiles = [(x, y, min(ts, w - x), min(ts, h - y)) for y in range(0, h, ts) for x in range(0, w, ts)]
        c = cfg.to_c()

        def run(chunk):
            arr = (abi.McrtTile * max(len(chunk), 1))(*[abi.McrtTile(*t) for t in chunk])
            rc = self.lib.render_tiles(desc_ptr, C.byref(c), mode, arr, len(chunk), abi.fptr(frame), hits.ctypes.data_as(C.POINTER(C.c_int32)))
            assert rc == 0, rc

        if threads <= 1:
            run(list(tiles))
        else:
            tiles = list(tiles)
            chunks = [tiles[i::4 * threads] for i in range(min(4 * threads, len(tiles)))]  # (a frame of 1 x 1 tiles has thousands)
            with ThreadPoolExecutor(threads) as pool:  # ctypes releases the GIL during the call; tiles are disjoint
                list(pool.map(run, chunks))
        return frame, hits


def threads() -> int:
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))
