"""Deterministic synthetic skins (the reference ships no skin PNG and there is no network).

Definition from SURVEY.md §8(d): 64x64 (S64) or 64x32 (S32) RGBA8 from the LCG
``s = s*1664525 + 1013904223 (mod 2^32)``, seed 12345, row-major; per texel r, g, b = ``s >> 24``
after one step each.  Alpha is 255 on inner-layer areas; on the outer-layer areas of the 64x64
layout (y<16 & x>=32, 32<=y<48, y>=48 & (x<16 | x>=48)) alpha = 255 if ``(s >> 28) < 6`` after a
fourth step, else 0 (~37 % opaque) -> 12 meshes.  For the legacy 64x32 layout only the head
overlay (y<16 & x>=32) is an outer area -> 7 meshes.

S64S is a skin for the slim player model (arms 3 texels wide): the S64 image with alpha 0 on the 128 pixels of the four arm
unwraps that a slim figure never reads — per arm box at origin (ox, oy) the pixels (ox+10..ox+11, oy..oy+3) behind the
narrower top and bottom faces and (ox+14..ox+15, oy+4..oy+15) behind the narrower front and back.  The 64 of the two inner
arm boxes are the pixels the usual slim detection looks at.
"""
from __future__ import annotations

import numpy as np


SLIM_ARM_ORIGINS = ((40, 16), (32, 48), (40, 32), (48, 48))  # right arm, left arm, their outer layers


def slim_unused_mask() -> np.ndarray:
    """(64, 64) bool: the pixels of the classic arm unwraps that the slim unwraps leave unread."""
    mask = np.zeros((64, 64), bool)
    for ox, oy in SLIM_ARM_ORIGINS:
        mask[oy:oy + 4, ox + 10:ox + 12] = True
        mask[oy + 4:oy + 16, ox + 14:ox + 16] = True
    return mask


def synthetic_cape(seed: int = 54321) -> np.ndarray:
    """A deterministic cape image, (32, 64, 4) uint8: r, g, b from the skins' LCG, one step each, row-major over the whole
    image, alpha 255 everywhere — so every one of the 372 texels of the cape's unwrap is opaque and all differ."""
    img = np.zeros((32, 64, 4), dtype=np.uint8)
    s = seed & 0xFFFFFFFF
    for y in range(32):
        for x in range(64):
            rgb = []
            for _ in range(3):
                s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
                rgb.append(s >> 24)
            img[y, x] = (rgb[0], rgb[1], rgb[2], 255)
    return img


def synthetic_skin(kind: str = "S64", seed: int = 12345) -> np.ndarray:
    """Returns (H, 64, 4) uint8."""
    if kind == "S64S":
        img = synthetic_skin("S64", seed)
        img[slim_unused_mask(), 3] = 0
        return img
    if kind not in ("S64", "S32"):
        raise ValueError("kind must be 'S64', 'S32' or 'S64S'")
    h = 64 if kind == "S64" else 32
    img = np.zeros((h, 64, 4), dtype=np.uint8)
    s = seed & 0xFFFFFFFF
    for y in range(h):
        for x in range(64):
            rgb = []
            for _ in range(3):
                s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
                rgb.append(s >> 24)
            if kind == "S64":
                outer = (y < 16 and x >= 32) or (32 <= y < 48) or (y >= 48 and (x < 16 or x >= 48))
            else:
                outer = y < 16 and x >= 32
            a = 255
            if outer:
                s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
                a = 255 if (s >> 28) < 6 else 0
            img[y, x] = (rgb[0], rgb[1], rgb[2], a)
    return img
