"""Expected values of the studio shot (mcrt_render_shot & co) — a helper, not a test.

``compose`` restates the blend of include/mcrt.h ("studio shot") in numpy float32, one rounding per operation, in the order
written there:

    sh    = s * (1 - vis)
    f     = fade > 0 ? clamp(1 - dR / fade, 0, 1) : 1
    ar    = (k * R.a) * f
    keep  = (1 - sh) * (1 - ar)
    fl.c  = pg.c * keep + R.c * ar
    out.c = F.c * F.a + fl.c * (1 - F.a)          out.a = 1

``expected_shot`` takes its four inputs from the CPU oracle alone: F from ``transparent_checker.Checker.render``, vis from
``ground_checker``, R and dR from ``reflection_checker``, the page from ``oracle.background`` at the pixel centres."""
from __future__ import annotations

import functools
import tempfile

import numpy as np

from minecraftskin_raytracer_amd import abi

import ground_checker as G
import layers_checker as L
import reflection_checker as R_
import transparent_checker as T

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
ONE, ZERO = f32(1.0), f32(0.0)
CLASSES = ("opaque figure", "figure edge", "shadow beside the figure", "penumbra beside the figure", "reflection beside the figure")


def _f32(a, what):
    assert isinstance(a, np.ndarray) and a.dtype == f32, f"{what} is {getattr(a, 'dtype', type(a))}, not float32"
    return a


def compose(F, vis, R, dR, page, shot: abi.Shot) -> np.ndarray:
    """F (..., 4), vis (...) or None, R (..., 4) or None, dR (...) or None (only with reflectionFade == 0 or without R),
    page (..., 3) or (3,), all float32 → out (..., 4) float32.  An absent input enters with its miss constant."""
    F = _f32(F, "F")
    shape = F.shape[:-1]
    vis = np.ones(shape, f32) if vis is None else _f32(vis, "vis")
    R = np.zeros(shape + (4,), f32) if R is None else _f32(R, "R")
    s, k, fade = f32(shot.shadowStrength), f32(shot.reflectivity), f32(shot.reflectionFade)
    page = np.broadcast_to(_f32(np.asarray(page, f32), "page"), shape + (3,))
    sh = _f32(s * (ONE - vis), "sh")
    if fade > 0:
        dR = np.full(shape, FLT_MAX, f32) if dR is None else _f32(dR, "dR")
        with np.errstate(over="ignore"):  # FLT_MAX / fade may be inf below fade = 1: 1 - inf = -inf, clamped to 0
            q = _f32(dR / fade, "dR / fade")
        f = _f32(np.minimum(np.maximum(_f32(ONE - q, "1 - q"), ZERO), ONE), "f")
    else:
        f = np.ones(shape, f32)
    ar = _f32(_f32(k * R[..., 3], "k * R.a") * f, "ar")
    keep = _f32(_f32(ONE - sh, "1 - sh") * _f32(ONE - ar, "1 - ar"), "keep")
    under = _f32(ONE - F[..., 3], "1 - F.a")
    out = np.empty(shape + (4,), f32)
    for c in range(3):
        fl = _f32(_f32(page[..., c] * keep, "pg * keep") + _f32(R[..., c] * ar, "R.c * ar"), "fl")
        out[..., c] = _f32(_f32(F[..., c] * F[..., 3], "F.c * F.a") + _f32(fl * under, "fl * (1 - F.a)"), "out")
    out[..., 3] = ONE
    return out


def quantize(rgba: np.ndarray) -> np.ndarray:
    return R_.quantize(rgba)


def page_plane(oracle, sd, cfg, shot: abi.Shot) -> np.ndarray:
    """(H, W, 3) float32: the page colour of every pixel — ``shot.pageColor``, or ``oracle.background`` at the pixel centre."""
    h, w = cfg.height, cfg.width
    if shot.page == "color":
        return np.broadcast_to(np.asarray(shot.pageColor, f32), (h, w, 3)).copy()
    assert shot.page == "reference"
    out = np.empty((h, w, 3), f32)
    for py in range(h):
        v = (f32(py) + f32(0.5)) / f32(h)
        for px in range(w):
            u = (f32(px) + f32(0.5)) / f32(w)
            out[py, px] = oracle.background(sd.ptr, cfg, float(u), float(v))[:3]
    return out


def gradient_plane(cfg) -> np.ndarray:
    """``page_plane`` of the reference page with the gradient on, vectorised (raytracer.cpp:16-34 in numpy float32; numpy's
    float32 sqrt is correctly rounded like the reference's) — for frames too large for a call per pixel.
    tests/test_shot_checker.py holds it against ``page_plane`` bit for bit."""
    assert cfg.gradientBg
    h, w = cfg.height, cfg.width
    u = (np.arange(w, dtype=f32) + f32(0.5)) / f32(w)
    v = (np.arange(h, dtype=f32) + f32(0.5)) / f32(h)
    cx, cy = (u - f32(0.5))[None, :], (v - f32(0.5))[:, None]
    dist = np.sqrt(cx * cx + cy * cy) * f32(2.0) * f32(cfg.gradientScale)
    dist = np.minimum(np.maximum(dist, ZERO), ONE)
    t = _f32(dist * dist, "t")
    out = np.empty((h, w, 3), f32)
    for c in range(3):
        out[..., c] = f32(cfg.bgCenter[c]) * (ONE - t) + f32(cfg.bgEdge[c]) * t
    return out


@functools.lru_cache(maxsize=None)
def transparent_oracle() -> T.Checker:
    """The CPU checker of the transparent frame, compiled once per process into a temporary directory."""
    tmp = tempfile.mkdtemp(prefix="shot_transparent_oracle_")
    return T.Checker(T.build(tmp))


def expected_shot(oracle, sd, cfg, shot: abi.Shot, ground_y, pass_cfg=None, threads=None) -> dict:
    """{"F" (H, W, 4), "vis" (H, W), "R" (H, W, 4), "dR" (H, W), "page" (H, W, 3), "out" (H, W, 4) float32, "rgba8" (H, W, 4)
    uint8} — every input from the CPU oracle, whether or not the shot uses it.  pass_cfg: the config of the two passes where
    cfg's is outside their limits (a shot that skips a pass accepts such a config; it does not read the pass's plane).
    threads: of the transparent checker (default: transparent_checker.threads())."""
    pass_cfg = pass_cfg or cfg
    F, _ = transparent_oracle().render(sd.ptr, cfg, "transparent", threads=threads or T.threads())
    vis = G.expected_ground(oracle, sd, pass_cfg, ground_y)["visibility"]
    refl = R_.expected_reflection(oracle, sd, pass_cfg, ground_y)
    page = page_plane(oracle, sd, cfg, shot)
    out = compose(F, vis, refl["rgba"], refl["distance"], page, shot)
    return {"F": F, "vis": vis, "R": refl["rgba"], "dR": refl["distance"], "page": page, "out": out, "rgba8": quantize(out)}


def classes(exp: dict) -> tuple:
    """Pixels of an expectation by what they show, in the order of CLASSES: F.a == 1; 0 < F.a < 1; vis < 1 beside the figure
    (F.a == 0); 0 < vis < 1 beside it; R.a > 0 beside it."""
    a, vis, ra = exp["F"][..., 3], exp["vis"], exp["R"][..., 3]
    beside = a == 0
    return (int((a == 1).sum()), int(((a > 0) & (a < 1)).sum()), int((beside & (vis < 1)).sum()), int((beside & (vis > 0) & (vis < 1)).sum()),
            int((beside & (ra > 0)).sum()))


def own_planes(mcrt, handles, cfg, heights, pass_cfg=None, stream=None):
    """The transparent frames, ground visibilities and reflection planes of the handles through the library's own calls, as
    numpy arrays (F, vis, R, dR).  pass_cfg: the config of the two passes where cfg's is outside their limits.  Needs the device;
    the handles' background mode is "reference" afterwards."""
    import torch

    stream = torch.cuda.current_stream().cuda_stream if stream is None else stream
    n, h, w = len(handles), cfg.height, cfg.width
    pass_cfg = pass_cfg or cfg
    F = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    vis = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
    R = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    dR = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
    for ds in handles:
        ds.set_background("transparent")
    mcrt.render_batch_device(handles, cfg, F.data_ptr(), 0, stream=stream)
    for ds in handles:
        ds.set_background("reference")
    mcrt.render_ground_batch_device(handles, pass_cfg, heights, visibility_ptr=vis.data_ptr(), stream=stream)
    mcrt.render_reflection_batch_device(handles, pass_cfg, heights, rgba_ptr=R.data_ptr(), distance_ptr=dR.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return F.cpu().numpy(), vis.cpu().numpy(), R.cpu().numpy(), dR.cpu().numpy()


SHOT = abi.Shot(shadowStrength=0.6, reflectivity=0.35, reflectionFade=24.0)  # the shot of the oracle cases


def case_config(name) -> abi.Config:
    """The config of a skin case's shot: 4 samples per pixel, 3 bounces, 8 shadow samples."""
    _, _, _, w, h, tile = L.SKIN_CASES[name]
    return abi.Config(width=w, height=h, tileSize=tile, samplesPerPixel=4, maxBounces=3, softShadows=True, shadowSamples=8)


@functools.lru_cache(maxsize=None)
def skin_expectation(name, ground_y=0.0):
    """(scene description, Config, expectation) of one of layers_checker.SKIN_CASES under SHOT — computed once per session,
    never modified."""
    import oraclelib

    kind, pose, camera, _, _, _ = L.SKIN_CASES[name]
    sd = L.skin_case(kind, pose, camera)
    cfg = case_config(name)
    exp = expected_shot(oraclelib.Oracle(), sd, cfg, SHOT, ground_y)
    for a in exp.values():
        a.setflags(write=False)
    return sd, cfg, exp


def assert_shot_equal(got_f32, got_u8, out: np.ndarray, what=""):
    """Bit for bit against ``out`` (float32) and its quantisation; either ``got`` may be None."""
    import scenes

    if got_f32 is not None:
        scenes.assert_bit_equal(got_f32, out, f"{what} f32")
    if got_u8 is not None:
        want = quantize(out)
        bad = np.argwhere((got_u8 != want).any(axis=-1))
        assert len(bad) == 0, f"{what} rgba8: {len(bad)} pixels differ; first {tuple(bad[0])}: {got_u8[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
