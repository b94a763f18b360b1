"""The shot as a cut-out on the GPU (mcrt_*_ex): the blend kernel alone on synthetic planes, bit for bit against
tests/cutout_checker.py's ``compose_ex``; the bounds; the ``_ex`` entries against the ``_occ`` entries byte for byte where both
apply; whole shots against the CPU oracle alone through the host, batched device and PNG forms; the over-page property on device
output; the shots that skip every pass; stream order behind a repaint and a view change; ``SkinBatch.shots`` with bounds.

So that an empty or figure-only image cannot pass, each oracle case asserts the pixel classes of its expectation
(``cutout_checker.classes``) above ``cutout_checker.FLOORS``; tests/test_cutout_checker.py pins their counts on the CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cutout_checker as X  # noqa: E402
import ground_occlusion_checker as GO  # noqa: E402
import scenes  # noqa: E402
import shot_checker as S  # noqa: E402
import skin_paint_checker as P  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402

gpu_test = pytest.mark.gpu
f32 = np.float32
SENTINEL = -12345.0
BYTE_SENTINEL = 77
BOX_SENTINEL = -777
BOUND = 16 * 2.0 ** -24
TINT = (0.125, 0.7, 0.3)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _scratch(mcrt, cfg, shot, n):
    need = mcrt.shot_scratch_bytes(cfg, shot, n)
    return torch.full((need + 64,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"), need


def _shoot(mcrt, handles, cfg, shot, heights, stride=None, stream=None, bounds=True):
    """render_shot_batch_device into sentinel-filled buffers → (f32 (n, H, W, 4), u8 (n, H, W, 4), boxes (n, 4) or None); checks the
    gaps between the frames, the bytes behind the scratch and the entry behind the boxes."""
    n, px = len(handles), cfg.width * cfg.height
    stride = px if stride is None else stride
    out = torch.full((n * stride * 4,), SENTINEL, dtype=torch.float32, device="cuda")
    out8 = torch.full((n * stride * 4,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    box = torch.full((n + 1, 4), BOX_SENTINEL, dtype=torch.int32, device="cuda")
    scratch, need = _scratch(mcrt, cfg, shot, n)
    mcrt.render_shot_batch_device(handles, cfg, shot, heights, scratch.data_ptr(), need, out.data_ptr(), out8.data_ptr(), stride,
                                  stream if stream is not None else _stream(), box.data_ptr() if bounds else 0)
    torch.cuda.synchronize()
    assert bool((scratch[need:] == BYTE_SENTINEL).all().item()), "written behind the scratch"
    a, b, boxes = out.cpu().numpy().reshape(n, stride * 4), out8.cpu().numpy().reshape(n, stride * 4), box.cpu().numpy()
    assert (a[:, px * 4:] == SENTINEL).all() and (b[:, px * 4:] == BYTE_SENTINEL).all(), "the pixels between two frames were written"
    assert (boxes[n if bounds else 0:] == BOX_SENTINEL).all(), "written behind the boxes"
    return a[:, :px * 4].reshape(n, cfg.height, cfg.width, 4), b[:, :px * 4].reshape(n, cfg.height, cfg.width, 4), boxes[:n] if bounds else None


def _assert_equal(got_f32, got_u8, want, what):
    if got_f32 is not None:
        scenes.assert_bit_equal(got_f32, want, f"{what} f32")
    if got_u8 is not None:
        q = X.quantize(want)
        bad = np.argwhere((got_u8 != q).any(axis=-1))
        assert len(bad) == 0, f"{what} rgba8: {len(bad)} pixels differ; first {tuple(bad[0])}: {got_u8[tuple(bad[0])]} vs {q[tuple(bad[0])]}"


# ---- the kernel alone ---------------------------------------------------------------------------------------------------
def _synthetic(rng, n, h, w):
    F = rng.random((n, h, w, 4), dtype=f32)
    pick = rng.integers(0, 4, (n, h, w))
    F[..., 3] = np.where(pick == 0, f32(0), np.where(pick == 1, f32(1), np.where(pick == 2, f32(1) - f32(2.0 ** -24), F[..., 3])))
    F[F[..., 3] == 0] = 0
    vis = (rng.integers(0, 9, (n, h, w)).astype(f32) / f32(8)).astype(f32)
    R = rng.random((n, h, w, 4), dtype=f32)
    dR = (rng.random((n, h, w), dtype=f32) * f32(40)).astype(f32)
    miss = rng.random((n, h, w)) < 0.4
    R[miss] = 0
    dR[miss] = S.FLT_MAX
    occ = (rng.integers(4, 9, (n, h, w)).astype(f32) / f32(8)).astype(f32)
    return F, vis, R, dR, occ


def _strided(planes, comps, stride, lead=0):
    """(n, H, W[, 4]) → a device buffer with frame i `stride` pixels on behind `lead` elements, sentinels elsewhere."""
    n = planes.shape[0]
    px = planes.shape[1] * planes.shape[2]
    host = np.full(lead + n * stride * comps, SENTINEL, f32)
    host[lead:].reshape(n, stride * comps)[:, :px * comps] = planes.reshape(n, px * comps)
    return _dev(host)


BACKGROUNDS = [(0.125, 0.5, 0.75, 1.0), (0.9, 0.1, 0.3, 1.0), (0.0, 1.0, 0.25, 1.0)]
PAGES = {"transparent": ("transparent", dict()), "color": ("color", dict()), "gradient_0.7": ("reference", dict(gradientScale=0.7)),
         "scene_colour": ("reference", dict(gradientBg=False))}
PAGE_COLOR = (0.93, 0.87, 0.2)


@pytest.fixture(scope="module")
def three_handles(mcrt, gpu):
    sds = []
    for bg in BACKGROUNDS:
        sd = mcrt.MeshBuilder.buildDefaultScene()
        for i in range(4):
            sd.desc.background_color[i] = bg[i]
        sds.append(sd)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    yield sds, handles
    for h in handles:
        h.close()


@gpu_test
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "planes_4_bytes_on"])
@pytest.mark.parametrize("size", [(1, 1), (33, 17), (130, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_kernel_alone_equals_compose_ex(mcrt, gpu, oracle, three_handles, size, lead):
    """Three frames, input stride W * H + 5, output stride W * H + 3, both outputs and each alone; each optional input absent in
    turn; the three pages (the reference page with the gradient and with the scenes' colours); a black and a coloured shadow;
    with the transparent page the boxes.  lead = 1: every plane one element on — the rgba planes and the boxes 4 bytes off a
    16-byte boundary, RGBA8 one byte off a 4-byte boundary."""
    w, h = size
    sds, handles = three_handles
    n, px = 3, w * h
    sin, sout = px + 5, px + 3
    rng = np.random.default_rng(2000 * w + h)
    F, vis, R, dR, occ = _synthetic(rng, n, h, w)
    dF, dvis, dRr, ddR, docc = (_strided(F, 4, sin, lead), _strided(vis, 1, sin, lead), _strided(R, 4, sin, lead), _strided(dR, 1, sin, lead),
                                _strided(occ, 1, sin, lead))
    at = lambda t: t.data_ptr() + lead * t.element_size()  # noqa: E731

    def run(cfg, shot, absent, which="both", cut=False):
        out = torch.full((lead + n * sout * 4,), SENTINEL, dtype=torch.float32, device="cuda")
        out8 = torch.full((lead + n * sout * 4,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        box = torch.full((lead + (n + 1) * 4,), BOX_SENTINEL, dtype=torch.int32, device="cuda")
        mcrt.composite_shot_batch_device(
            handles, cfg, shot, at(dF), 0 if absent == "visibility" else at(dvis), 0 if absent == "reflection" else at(dRr),
            0 if absent == "distance" else at(ddR), at(out) if which != "u8" else 0, at(out8) if which != "f32" else 0, sin, sout, _stream(),
            0 if absent == "occlusion" else at(docc), at(box) if cut else 0)
        torch.cuda.synchronize()
        a, b, c = out.cpu().numpy(), out8.cpu().numpy(), box.cpu().numpy()
        assert (a[:lead] == SENTINEL).all() and (b[:lead] == BYTE_SENTINEL).all() and (c[:lead] == BOX_SENTINEL).all(), "written in front of the planes"
        a, b = a[lead:].reshape(n, sout * 4), b[lead:].reshape(n, sout * 4)
        assert (a[:, px * 4:] == SENTINEL).all() and (b[:, px * 4:] == BYTE_SENTINEL).all(), "the gaps were written"
        assert (c[lead + (n if cut else 0) * 4:] == BOX_SENTINEL).all(), "written behind the boxes"
        if which == "f32":
            assert (b == BYTE_SENTINEL).all()
        if which == "u8":
            assert (a == SENTINEL).all()
        return (a[:, :px * 4].reshape(n, h, w, 4) if which != "u8" else None, b[:, :px * 4].reshape(n, h, w, 4) if which != "f32" else None,
                c[lead:lead + n * 4].reshape(n, 4))

    for page_name, (page_kind, cfg_kw) in PAGES.items():
        cfg = abi.Config(width=w, height=h, **cfg_kw)
        cut = page_kind == "transparent"
        page = None
        if not cut:
            on_page = abi.Shot(page=page_kind, pageColor=PAGE_COLOR)
            pages = [S.page_plane(oracle, sd, cfg, on_page) for sd in (sds if page_name == "scene_colour" else sds[:1])]
            page = np.stack(pages if len(pages) == n else pages * n)
        for colour in ((0.0, 0.0, 0.0), TINT):
            for absent in ("none", "visibility", "reflection", "distance", "occlusion"):
                shot = abi.Shot(page_kind, PAGE_COLOR, 0.6, 0.35, 0.0 if absent == "distance" else 24.0, floorOcclusion=0.5, shadowColor=colour)
                if not shot.needs_ex():
                    continue  # (the entries before: tests/test_gpu_shot.py)
                want = X.compose_ex(F, None if absent == "visibility" else vis, None if absent == "reflection" else R, None if absent == "distance" else dR,
                                    None if absent == "occlusion" else occ, page, shot)
                what = f"{w}x{h} {page_name}, C = {colour}, {absent} absent"
                a, b, boxes = run(cfg, shot, absent, cut=cut)
                _assert_equal(a, b, want, what)
                if cut:
                    assert boxes.tolist() == [X.bounds_of(want[i, ..., 3]).tolist() for i in range(n)], what
            # one output at a time
            shot = abi.Shot(page_kind, PAGE_COLOR, 0.6, 0.35, 24.0, floorOcclusion=0.5, shadowColor=colour)
            if shot.needs_ex():
                want = X.compose_ex(F, vis, R, dR, occ, page, shot)
                _assert_equal(run(cfg, shot, "none", "f32")[0], None, want, f"{w}x{h} {page_name}, f32 alone")
                _assert_equal(None, run(cfg, shot, "none", "u8", cut=cut)[1], want, f"{w}x{h} {page_name}, rgba8 alone")
    # one frame: the record travels as a kernel argument
    cfg = abi.Config(width=w, height=h)
    shot = abi.Shot("transparent", reflectionFade=24.0, shadowColor=TINT)
    out = torch.full((px * 4,), SENTINEL, dtype=torch.float32, device="cuda")
    box = torch.full((2, 4), BOX_SENTINEL, dtype=torch.int32, device="cuda")
    mcrt.composite_shot_batch_device(handles[:1], cfg, shot, at(dF), at(dvis), at(dRr), at(ddR), out.data_ptr(), 0, sin, px, _stream(), 0, box.data_ptr())
    torch.cuda.synchronize()
    want = X.compose_ex(F[0], vis[0], R[0], dR[0], None, None, shot)
    _assert_equal(out.cpu().numpy().reshape(h, w, 4), None, want, f"{w}x{h} one frame")
    assert box.cpu().numpy().tolist() == [X.bounds_of(want[..., 3]).tolist(), [BOX_SENTINEL] * 4]


# ---- the bounds ---------------------------------------------------------------------------------------------------------
def _boxes_of(mcrt, handle, w, h, alpha, which="u8"):
    """The boxes the blend reports for figures that are `alpha` (n, H, W) and nothing else: out = F."""
    n = alpha.shape[0]
    F = np.zeros((n, h, w, 4), f32)
    F[..., 3] = alpha
    F[..., :3] = 0.5 * (alpha[..., None] > 0)
    dF = _dev(F)
    out8 = torch.full((n, h, w, 4), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    box = torch.full((n + 1, 4), BOX_SENTINEL, dtype=torch.int32, device="cuda")
    mcrt.composite_shot_batch_device([handle] * n, abi.Config(width=w, height=h), abi.Shot("transparent"), dF.data_ptr(), out_rgba8_ptr=out8.data_ptr(),
                                     stream=_stream(), bounds_ptr=box.data_ptr())
    torch.cuda.synchronize()
    got = box.cpu().numpy()
    assert (got[n] == BOX_SENTINEL).all(), "written behind the boxes"
    assert np.array_equal(out8.cpu().numpy(), X.quantize(F)), "out = F"
    return got[:n]


@gpu_test
def test_bounds_of_single_pixels_edges_and_empty_frames(mcrt, gpu, three_handles):
    _, handles = three_handles
    w, h = 37, 11
    frames = {"first pixel": [(0, 0)], "last pixel": [(w - 1, h - 1)], "left edge": [(0, 5)], "right edge": [(w - 1, 4)], "top edge": [(20, 0)],
              "bottom edge": [(9, h - 1)], "empty": [], "two corners": [(0, h - 1), (w - 1, 0)], "inside": [(5, 3), (30, 8), (17, 2)]}
    alpha = np.zeros((len(frames), h, w), f32)
    for i, pixels in enumerate(frames.values()):
        for x, y in pixels:
            alpha[i, y, x] = 2.0 ** -30 if (x + y) % 2 else 0.75  # any alpha above 0 counts, whatever it quantises to
    want = [X.bounds_of(a).tolist() for a in alpha]
    assert want[0] == [0, 0, 1, 1] and want[1] == [w - 1, h - 1, w, h] and want[6] == [w, h, 0, 0] and want[7] == [0, 0, w, h]
    # every frame in a launch of its own (the record as a kernel argument), then all in one launch: different boxes side by side
    for i, name in enumerate(frames):
        assert _boxes_of(mcrt, handles[0], w, h, alpha[i:i + 1]).tolist() == [want[i]], name
    assert _boxes_of(mcrt, handles[0], w, h, alpha).tolist() == want
    assert _boxes_of(mcrt, handles[0], w, h, alpha[[7, 6, 8]]).tolist() == [want[7], want[6], want[8]]


@gpu_test
def test_bounds_of_4097_frames(mcrt, gpu, three_handles):
    """4097 frames of 3 x 2: two launches; frame i's content is pixel i % 7 (6: none)."""
    _, handles = three_handles
    n, w, h = 4097, 3, 2
    alpha = np.zeros((n, h * w), f32)
    for i in range(n):
        if i % 7 < 6:
            alpha[i, i % 7] = 1.0
    alpha = alpha.reshape(n, h, w)
    got = _boxes_of(mcrt, handles[0], w, h, alpha)
    want = np.array([X.bounds_of(a) for a in alpha])
    assert want[6].tolist() == [3, 2, 0, 0] and want[4096].tolist() == [1, 0, 2, 1]  # 4096 % 7 == 1
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=1))[:5]


@gpu_test
def test_bounds_behind_the_second_grid_stride_trip(mcrt, gpu, three_handles):
    """2049 x 1024 pixels are 1024 more than 8192 workgroups of 256 lanes visit in one trip: the only content is the last pixel."""
    _, handles = three_handles
    w, h = 2049, 1024
    F = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    F[h - 1, w - 1] = torch.tensor([0.25, 0.5, 0.75, 0.5])
    out8 = torch.full((h, w, 4), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    box = torch.full((2, 4), BOX_SENTINEL, dtype=torch.int32, device="cuda")
    mcrt.composite_shot_batch_device(handles[:1], abi.Config(width=w, height=h), abi.Shot("transparent"), F.data_ptr(), out_rgba8_ptr=out8.data_ptr(),
                                     stream=_stream(), bounds_ptr=box.data_ptr())
    torch.cuda.synchronize()
    assert box.cpu().numpy().tolist() == [[w - 1, h - 1, w, h], [BOX_SENTINEL] * 4]
    assert out8[h - 1, w - 1].tolist() == [64, 128, 191, 128] and int(out8.count_nonzero().item()) == 4


# ---- the _ex entries where the _occ entries apply -----------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("page", ["color", "reference"])
def test_opaque_pages_and_a_black_shadow_equal_the_occ_entries_byte_for_byte(mcrt, gpu, three_handles, page):
    from minecraftskin_raytracer_amd import _lib

    lib = _lib.load()
    _, handles = three_handles
    w, h, n = 33, 17, 3
    px = w * h
    F, vis, R, dR, occ = _synthetic(np.random.default_rng(5), n, h, w)
    F[0, 0, 0] = (-0.0, 0.5, 0.25, 1.0)  # the signs of zero too
    planes = [_dev(a) for a in (F, vis, R, dR, occ)]
    cfg = abi.Config(width=w, height=h, gradientScale=0.7).to_c()
    arr = (C.c_void_p * n)(*[ds._h.value for ds in handles])
    inputs = abi.McrtShotInputs(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), planes[3].data_ptr())
    for o, black in ((0.5, (0.0, 0.0, 0.0)), (0.0, (0.0, 0.0, 0.0)), (0.5, (-0.0, 0.0, -0.0))):
        shot = abi.Shot(page, PAGE_COLOR, 0.6, 0.35, 24.0, floorOcclusion=o, shadowColor=black)
        outs = []
        for ex in (False, True):
            out = torch.full((n, h, w, 4), SENTINEL, dtype=torch.float32, device="cuda")
            out8 = torch.full((n, h, w, 4), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
            if ex:
                s = shot.to_c_ex()
                rc = lib.mcrt_composite_shot_batch_device_ex(arr, n, C.byref(cfg), C.byref(s), C.byref(inputs), planes[4].data_ptr(), px, out.data_ptr(),
                                                             out8.data_ptr(), px, None, _stream())
            else:
                s = shot.to_c()
                rc = lib.mcrt_composite_shot_batch_device_occ(arr, n, C.byref(cfg), C.byref(s), C.byref(inputs), planes[4].data_ptr(), o, px, out.data_ptr(),
                                                              out8.data_ptr(), px, _stream())
            assert rc == 0, lib.mcrt_last_error()
            torch.cuda.synchronize()
            outs.append((out.cpu().numpy(), out8.cpu().numpy()))
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes(), (page, o, black)
        assert (outs[0][0] != SENTINEL).all()


# ---- against the oracle alone -------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("name", list(X.SHOTS))
def test_cutouts_equal_the_oracle(mcrt, gpu, name, tmp_path):
    sd, cfg, shot, exp = X.shot_expectation(name)
    got_classes = X.classes(exp, shot)
    print(name, dict(zip(X.CLASSES, got_classes)), exp["bounds"].tolist())
    assert all(c >= f for c, f in zip(got_classes, X.FLOORS)), got_classes
    want_box = exp["bounds"].tolist()
    # the host form, both outputs, with and without the box
    image, box = mcrt.TileRenderer.renderShot(sd, cfg, shot, 0.0, rgba8=False, bounds=True)
    _assert_equal(image, mcrt.TileRenderer.renderShot(sd, cfg, shot, 0.0), exp["out"], name + " (host form)")
    assert box.dtype == np.int32 and box.tolist() == want_box
    images, boxes = mcrt.TileRenderer.renderShotBatch([sd, sd], cfg, shot, [0.0, 0.0], bounds=True)
    _assert_equal(None, images, np.stack([exp["out"]] * 2), name + " (host form, two frames)")
    assert boxes.tolist() == [want_box] * 2
    # the device forms
    ds = mcrt.DeviceScene(sd)
    try:
        a, b, boxes = _shoot(mcrt, [ds], cfg, shot, [0.0], stride=cfg.width * cfg.height + 7)
        _assert_equal(a[0], b[0], exp["out"], name + " (device form)")
        assert boxes.tolist() == [want_box]
        a, b, _ = _shoot(mcrt, [ds], cfg, shot, [0.0], bounds=False)
        _assert_equal(a[0], b[0], exp["out"], name + " (device form, no boxes)")
        out8 = torch.full((cfg.height, cfg.width, 4), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        box = torch.full((4,), BOX_SENTINEL, dtype=torch.int32, device="cuda")
        scratch, need = _scratch(mcrt, cfg, shot, 1)
        ds.render_shot_device(cfg, shot, 0.0, scratch.data_ptr(), need, 0, out8.data_ptr(), _stream(), box.data_ptr())
        torch.cuda.synchronize()
        _assert_equal(None, out8.cpu().numpy(), exp["out"], name + " (single device form)")
        assert box.cpu().numpy().tolist() == want_box
        ds.check()
    finally:
        ds.close()
    # the files: the whole frame and the box
    whole, cropped = str(tmp_path / "whole.png"), str(tmp_path / "cropped.png")
    assert mcrt.render_shot_png(sd, cfg, whole, shot, 0.0) is True and mcrt.render_shot_png(sd, cfg, cropped, shot, 0.0, crop=True) is True
    assert np.array_equal(GO.read_png(whole), exp["rgba8"])
    x0, y0, x1, y1 = want_box
    assert np.array_equal(GO.read_png(cropped), exp["rgba8"][y0:y1, x0:x1])
    assert (exp["rgba8"][..., 3] < 255).any() and (exp["rgba8"][..., 3] > 0).any()


@gpu_test
def test_png_ex_reports_the_box_and_never_fails_for_an_empty_cutout(mcrt, gpu, tmp_path):
    from minecraftskin_raytracer_amd import _lib

    lib = _lib.load()
    sd, cfg, shot, exp = X.shot_expectation("pose0_33x17_t7")
    c, s = cfg.to_c(), shot.to_c_ex()
    box = np.full(4, BOX_SENTINEL, np.int32)
    for crop in (0, 1):
        path = str(tmp_path / f"crop{crop}.png")
        assert lib.mcrt_render_shot_png_ex(sd.ptr, C.byref(c), C.byref(s), 0.0, os.fsencode(path), crop, box.ctypes.data, 0) == 0, lib.mcrt_last_error()
        assert box.tolist() == exp["bounds"].tolist()
    # nothing in sight: the camera looks away from the figure, and no pass has anything to add
    away = mcrt.MeshBuilder.buildDefaultScene()
    away.desc.camera_target[0], away.desc.camera_target[1], away.desc.camera_target[2] = 0.0, 18.0, 100.0
    small = abi.Config(width=9, height=5, tileSize=4)
    empty = abi.Shot("transparent", shadowStrength=0.0, reflectivity=0.0)
    image, got = mcrt.TileRenderer.renderShot(away, small, empty, 0.0, bounds=True)
    assert (image == 0).all() and got.tolist() == [9, 5, 0, 0]
    path = str(tmp_path / "empty.png")
    c, s = small.to_c(), empty.to_c_ex()
    assert lib.mcrt_render_shot_png_ex(away.ptr, C.byref(c), C.byref(s), 0.0, os.fsencode(path), 1, box.ctypes.data, 0) == 0, lib.mcrt_last_error()
    assert box.tolist() == [9, 5, 0, 0]
    decoded = GO.read_png(path)
    assert decoded.shape == (5, 9, 4) and (decoded == 0).all()  # an empty rectangle: the whole frame


# ---- over any page ------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("page", ["color", "reference"])
def test_the_cutout_over_a_page_is_the_opaque_shot_for_that_page(mcrt, gpu, oracle, page):
    """Device output on both sides: the cut-out composited over the page (in float64) against the opaque shot of the same
    settings — within 16 * 2^-24 in float and one level in RGBA8 (tests/test_cutout_checker.py: the bound's origin)."""
    worst, worst8 = 0.0, 0
    for name in ("pose6_orbit_48x40_t13", "s32_pose1_40x30_t16"):
        sd, cfg, shot, exp = X.shot_expectation(name)
        on_page = X.with_page(shot, page, (0.93, 0.87, 0.2))
        pg = S.page_plane(oracle, sd, cfg, on_page)
        ds = mcrt.DeviceScene(sd)
        try:
            cut = _shoot(mcrt, [ds], cfg, shot, [0.0])[0][0]
            opaque, opaque8, _ = _shoot(mcrt, [ds], cfg, on_page, [0.0], bounds=False)
            ds.check()
        finally:
            ds.close()
        scenes.assert_bit_equal(cut, exp["out"], name)
        assert (opaque[0][..., 3] == 1).all() and (opaque8[0][..., 3] == 255).all()
        composed = X.over(cut, pg)
        diff = float(np.abs(composed - opaque[0][..., :3]).max())
        q = X.quantize(np.concatenate([composed, np.ones(composed.shape[:-1] + (1,))], axis=-1).astype(f32))
        diff8 = int(np.abs(q.astype(int) - opaque8[0].astype(int)).max())
        print(f"{name} over the {page} page: largest difference {diff / 2.0 ** -24:.2f} * 2^-24, {diff8} level(s) in RGBA8")
        worst, worst8 = max(worst, diff), max(worst8, diff8)
    assert worst <= BOUND and worst8 <= 1, (worst / 2.0 ** -24, worst8)


# ---- shots that skip every pass -------------------------------------------------------------------------------------------
@gpu_test
def test_a_cutout_without_floor_is_the_transparent_render(mcrt, gpu):
    """s = k = o = 0: the image is the MCRT_BACKGROUND_TRANSPARENT render's bytes, and the passes' limits — 8 bounces, 113 shadow
    samples, one ambient-occlusion sample — do not apply."""
    sd, cfg, _, exp = X.shot_expectation("pose0_33x17_t7")
    bare = abi.Shot("transparent", shadowStrength=0.0, reflectivity=0.0, floorOcclusion=0.0, shadowColor=TINT)
    heavy = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, samplesPerPixel=2, maxBounces=12, shadowSamples=200, aoSamples=0)
    ds = mcrt.DeviceScene(sd)
    try:
        for c in (cfg, heavy):
            want = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            want8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
            ds.set_background("transparent")
            mcrt.render_batch_device([ds], c, want.data_ptr(), want8.data_ptr(), stream=_stream())
            ds.set_background("reference")
            torch.cuda.synchronize()
            a, b, boxes = _shoot(mcrt, [ds], c, bare, [0.0])
            assert a[0].tobytes() == want.cpu().numpy().tobytes() and b[0].tobytes() == want8.cpu().numpy().tobytes()
            assert boxes.tolist() == [X.bounds_of(a[0][..., 3]).tolist()]
            assert mcrt.shot_scratch_bytes(c, bare, 1) == cfg.width * cfg.height * 16
        scenes.assert_bit_equal(_shoot(mcrt, [ds], cfg, bare, [0.0])[0][0], exp["F"], "the oracle's transparent frame")
        for refused, text in ((abi.Shot("transparent", reflectivity=0.0), "113 shadow samples"), (abi.Shot("transparent", shadowStrength=0.0), "113 shadow samples"),
                              (abi.Shot("transparent", shadowStrength=0.0, reflectivity=0.0, floorOcclusion=0.5), "ao_samples")):
            with pytest.raises(mcrt._lib.McrtError, match=text):
                _shoot(mcrt, [ds], heavy, refused, [0.0])
        deep = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, maxBounces=12)
        with pytest.raises(mcrt._lib.McrtError, match="at most 8 bounces"):
            _shoot(mcrt, [ds], deep, abi.Shot("transparent", shadowStrength=0.0), [0.0])
        ds.check()
    finally:
        ds.close()


# ---- the handle's mode and stream order ---------------------------------------------------------------------------------
@gpu_test
def test_a_cutout_behind_a_repaint_and_a_view_change_on_one_stream(mcrt, gpu):
    cfg = X.case_config("pose6_orbit_48x40_t13")
    shot = X.SHOTS["pose6_orbit_48x40_t13"][6]
    skin, poses = P.skin("inner_hole"), mcrt.getBuiltinPoses()
    want, want_box = mcrt.TileRenderer.renderShot(P.reference_scene(skin, poses[6], P.LOOK), cfg, shot, 0.0, bounds=True)
    stale = mcrt.TileRenderer.renderShot(P.reference_scene(P.skin("synthetic_S64"), poses[0]), cfg, shot, 0.0)
    assert want.tobytes() != stale.tobytes() and (want[..., 3] < 255).any()
    side = torch.cuda.Stream()
    ds = mcrt.DeviceScene.for_skin("S64", poses[0])
    try:
        ds.set_skin(P.skin("synthetic_S64"))

        def frame():
            out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
            torch.cuda.synchronize()
            return out.cpu().numpy()

        before = frame()
        assert (before[..., 3] == 1).all()  # the handle's mode: the reference's background
        assert np.array_equal(_shoot(mcrt, [ds], cfg, shot, [0.0])[1][0], stale)  # the handle has rendered the old skin and view
        scenes.assert_bit_equal(frame(), before, "the frame after the shot: the handle's mode is as it was")
        d_skin = _dev(skin)
        torch.cuda.synchronize()
        ds.set_skin_device(d_skin.data_ptr(), side.cuda_stream)
        ds.set_view_device(poses[6], P.look_desc(P.LOOK), side.cuda_stream)
        _, got, boxes = _shoot(mcrt, [ds], cfg, shot, [0.0], stream=side.cuda_stream)  # no synchronisation in between
        assert np.array_equal(got[0], want) and boxes.tolist() == [want_box.tolist()]
        ds.check()
    finally:
        ds.close()


# ---- the farm -----------------------------------------------------------------------------------------------------------
@gpu_test
def test_skin_batch_shots_with_bounds_equal_render_shot_batch(mcrt, gpu):
    cfg = abi.Config(width=64, height=64, samplesPerPixel=2)
    pose = mcrt.getBuiltinPoses()[3]
    skins = np.stack([P.skin("synthetic_S64"), P.skin("all_transparent"), P.variant(P.skin("inner_hole"), 5)])
    shot = abi.Shot("transparent", reflectionFade=30.0, shadowColor=(0.0, 0.0, 0.25))
    want, want_boxes = mcrt.TileRenderer.renderShotBatch([P.reference_scene(s, pose) for s in skins], cfg, shot, 0.0, bounds=True)
    assert want[0].tobytes() != want[1].tobytes() and (want[..., 3] == 0).any() and (want[..., 3] == 255).any()
    for (x0, y0, x1, y1), image in zip(want_boxes.tolist(), want):  # the boxes hold every pixel whose 8-bit alpha is above 0
        outside = np.ones(image.shape[:2], bool)
        outside[y0:y1, x0:x1] = False
        assert x0 < x1 and y0 < y1 and (image[outside, 3] == 0).all()
    batch = mcrt.SkinBatch(4, "S64", pose)
    try:
        got, boxes = batch.shots(skins, cfg, shot, bounds=True)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert boxes.dtype == np.int32 and np.array_equal(boxes, want_boxes)
        assert np.array_equal(batch.shots(skins, cfg, shot), want)
        floats, boxes = batch.shots(skins[:2], cfg, shot, ground=[0.0, 0.0], rgba8=False, bounds=True)
        assert floats.dtype == np.float32 and np.array_equal(X.quantize(floats), want[:2])
        assert boxes.tolist() == [X.bounds_of(f[..., 3]).tolist() for f in floats] == want_boxes[:2].tolist()
        none, no_boxes = batch.shots(skins[:0], cfg, shot, bounds=True)
        assert none.shape == (0, 64, 64, 4) and no_boxes.shape == (0, 4)
        with pytest.raises(mcrt._lib.McrtError, match="MCRT_PAGE_TRANSPARENT only"):
            batch.shots(skins, cfg, abi.Shot(), bounds=True)
        # the batch's renders keep their mode
        plain = batch.render(skins[:1], cfg, rgba8=True)
        assert np.array_equal(plain, mcrt.TileRenderer.renderBatch([P.reference_scene(skins[0], pose)], cfg, rgba8=True))
    finally:
        batch.close()
