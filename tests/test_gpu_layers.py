"""Geometry layers and picking on the GPU (mcrt_render_layers*, mcrt_scene_pick): depth, normal and albedo bit for bit and
the id fields as exact integers against the CPU oracle (tests/layers_checker.py), for skin scenes of a skin whose texels
all differ and for hand-built box scenes; plane subsets, batches, picks, and a layers pass beside the handle's render.

The skin frames of 3000 pixels and more must show at least 300 hit pixels with inner- and outer-layer hits among them; the
two smaller ones (33x17 at tile 7: 561 pixels in all, and 1x1) are there for their shapes and only have to hit something."""
import ctypes as C

import numpy as np
import pytest
import torch

import layers_checker as L
import scenes
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
PLANES = ("depth", "normal", "albedo", "id")


def _buffers(n, stride, names=PLANES):
    """Device planes for n frames `stride` pixels apart, filled with a sentinel."""
    out = {}
    for k in names:
        dtype, comps = (torch.int32 if k == "id" else torch.float32), abi.LAYER_FORMATS[k][1]
        out[k] = torch.full((n, stride, comps), int(SENTINEL) if k == "id" else SENTINEL, dtype=dtype, device="cuda")
    return out


def _ptrs(buf, names):
    return {f"{k}_ptr": buf[k].data_ptr() for k in names}


def _frames(buf, cfg, names):
    """The frames of the planes `names` as the host forms return them: (n, H, W[, 4])."""
    px = cfg.width * cfg.height
    out = {}
    for k in names:
        a = buf[k].cpu().numpy()[:, :px]
        out[k] = a.reshape(len(a), cfg.height, cfg.width) if k == "depth" else a.reshape(len(a), cfg.height, cfg.width, 4)
    return out


def _device_layers(ds, cfg, names=PLANES, stream=None):
    buf = _buffers(1, cfg.width * cfg.height)
    ds.render_layers_device(cfg, stream=stream if stream is not None else torch.cuda.current_stream().cuda_stream, **_ptrs(buf, names))
    torch.cuda.synchronize()
    return buf, {k: v[0] for k, v in _frames(buf, cfg, names).items()}


def _untouched(t):
    return bool((t == (int(SENTINEL) if t.dtype == torch.int32 else SENTINEL)).all().item())


def test_the_skin_cases_show_every_mesh(mcrt):
    seen = set()
    for name in L.SKIN_CASES:
        kind, exp = L.SKIN_CASES[name][0], L.skin_expectation(name)[2]
        if kind == "S64":
            seen |= set(exp["id"][..., 0][exp["hit"]].tolist())
    assert seen == set(range(12))
    for name in L.FULL_SKIN_CASES:
        exp = L.skin_expectation(name)[2]
        outer = (exp["id"][..., 1] & abi.ID_OUTER) != 0
        assert exp["hit"].sum() >= 300 and (exp["hit"] & outer).any() and (exp["hit"] & ~outer).any(), name


@gpu_test
@pytest.mark.parametrize("name", list(L.SKIN_CASES))
def test_skin_scene_layers_equal_the_oracle(mcrt, gpu, name):
    sd, cfg, exp = L.skin_expectation(name)
    kind = L.SKIN_CASES[name][0]
    outer = (exp["id"][..., 1] & abi.ID_OUTER) != 0
    if name in L.FULL_SKIN_CASES:
        assert exp["hit"].sum() >= 300 and (exp["hit"] & outer).any() and (exp["hit"] & ~outer).any()
    else:
        assert exp["hit"].any()
    got = mcrt.TileRenderer.renderLayers(sd, cfg)
    assert list(got) == list(PLANES)
    L.assert_layers_equal(got, exp, name)
    ds = mcrt.DeviceScene(sd)
    try:
        L.assert_layers_equal(_device_layers(ds, cfg)[1], exp, name + " (device form)")
        ds.check()
    finally:
        ds.close()
    # the id in skin coordinates: the texel the colour names
    ids = got["id"]
    for y, x in np.argwhere(exp["hit"]):
        m, face, tx, ty = (int(v) for v in ids[y, x])
        assert mcrt.skin_texel(kind, m, face, tx, ty) == L.skin_xy_of_color(exp["albedo"][y, x]), (name, x, y)


@gpu_test
@pytest.mark.parametrize("name", L.BOX_CASES)
def test_box_scene_layers_equal_the_oracle(mcrt, gpu, name):
    sd, cfg, exp = L.box_expectation(name)
    ids, hit = exp["id"], exp["hit"]
    back = (ids[..., 1] & abi.ID_BACK) != 0
    if name == "outer_back_face":  # the visible surface of the outer box is its exit face
        assert back.sum() >= 1 and ((ids[..., 1][back] & abi.ID_OUTER) != 0).all() and set((ids[..., 1][back] & 7).tolist()) == {0}
    elif name == "camera_inside":  # leaving the box the camera sits in: every pixel hits, no exit-face flag
        assert hit.all() and not back.any() and len(set((ids[..., 1] & 7).ravel().tolist())) >= 2
    elif name == "null_and_empty":
        bare = hit & (ids[..., 2] == -1)
        assert bare.any() and (ids[..., 3][bare] == -1).all() and (hit & (ids[..., 2] >= 0)).any()
        colours = {tuple(c) for c in exp["albedo"][bare].tolist()}
        assert colours == {(1.0, 0.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0)}  # the reference's magenta and Color()
    elif name == "posed":
        assert hit.sum() >= 100 and back.any() and set(ids[..., 0][hit].tolist()) == {0, 1}
        assert (np.abs(exp["normal"][hit][:, :3]).max(axis=1) < 0.999).any()  # rotated normals
    elif name == "seventy_boxes":
        assert set(ids[..., 0][hit].tolist()) == set(range(70))
    got = mcrt.TileRenderer.renderLayers(sd, cfg)
    L.assert_layers_equal(got, exp, name)


@gpu_test
def test_plane_subsets_leave_the_other_planes_alone(mcrt, gpu):
    sd, cfg, exp = L.skin_expectation("pose3_orbit_70x50")
    ds = mcrt.DeviceScene(sd)
    try:
        subsets = [(a,) for a in PLANES] + [(a, b) for i, a in enumerate(PLANES) for b in PLANES[i + 1:]]
        assert len(subsets) == 10
        for names in subsets:
            buf, got = _device_layers(ds, cfg, names)
            L.assert_layers_equal(got, exp, "+".join(names))
            for k in PLANES:
                if k not in names:
                    assert _untouched(buf[k]), f"{k} was written although only {names} were asked for"
        none, c = abi.McrtLayers(None, None, None, None), cfg.to_c()
        assert mcrt._lib.load().mcrt_render_layers_device(ds._h, C.byref(c), C.byref(none), None) == abi.MCRT_ERR_INVALID
    finally:
        ds.close()


def _pose_sheet(mcrt, n):
    """n views: the built-in poses on an orbit."""
    cams = [(0.0, 0.0, 50.0), (60.0, 15.0, 40.0), (200.0, -20.0, 36.0), (310.0, 45.0, 32.0)]
    return [L.skin_case("S64" if k % 4 else "S32", k % 7, cams[k % len(cams)]) for k in range(n)]


@gpu_test
def test_batch_equals_single_calls_and_keeps_the_gaps(mcrt, gpu):
    cfg = abi.Config(width=64, height=64, tileSize=32)
    sds = _pose_sheet(mcrt, 8)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        stride = px + 100  # not a multiple of four pixels apart from the frame: 16-byte aligned planes all the same
        buf = _buffers(8, stride)
        mcrt.render_layers_batch_device(handles, cfg, frame_stride_pixels=stride, stream=torch.cuda.current_stream().cuda_stream, **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES)
        for k in PLANES:
            assert _untouched(buf[k][:, px:]), f"{k}: the pixels between two frames were written"
        host = mcrt.TileRenderer.renderLayersBatch(sds, cfg)
        hits = 0
        for i, h in enumerate(handles):
            single = _device_layers(h, cfg)[1]
            L.assert_layers_equal({k: v[i] for k, v in batch.items()}, single, f"batch frame {i}")
            L.assert_layers_equal({k: v[i] for k, v in host.items()}, single, f"host batch frame {i}")
            hits += int((single["id"][..., 0] >= 0).sum())
        assert hits >= 8 * 100
        # a stride that leaves the depth planes of odd frames off a 16-byte boundary
        odd = px + 1
        buf = _buffers(3, odd, ("depth", "id"))
        mcrt.render_layers_batch_device(handles[:3], cfg, frame_stride_pixels=odd, stream=torch.cuda.current_stream().cuda_stream, **_ptrs(buf, ("depth", "id")))
        torch.cuda.synchronize()
        got = _frames(buf, cfg, ("depth", "id"))
        for i in range(3):
            L.assert_layers_equal({k: v[i] for k, v in got.items()}, {k: batch[k][i] for k in ("depth", "id")}, f"odd stride, frame {i}")
            assert _untouched(buf["depth"][i, px:]) and _untouched(buf["id"][i, px:])
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_of_unposed_posed_and_hbm_scenes(mcrt, gpu):
    # one launch for three kernel variants' worth of scenes: an un-posed figure and a posed one (tables in LDS) and seventy
    # boxes (tables read from HBM), so the whole batch runs the HBM variant; each frame must be what its own call gives
    cfg = abi.Config(width=70, height=45, tileSize=32)
    sds = [L.skin_case("S64", 0), L.skin_case("S64", 6, (135.0, 20.0, 34.0)), mcrt.SceneDesc(L.box_scene("seventy_boxes")[0])]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        buf = _buffers(3, cfg.width * cfg.height)
        mcrt.render_layers_batch_device(handles, cfg, stream=torch.cuda.current_stream().cuda_stream, **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES)
        for i, h in enumerate(handles):
            single = _device_layers(h, cfg)[1]
            assert (single["id"][..., 0] >= 0).sum() >= 100, f"frame {i} shows too little of its scene"
            L.assert_layers_equal({k: v[i] for k, v in batch.items()}, single, f"mixed batch frame {i}")
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_beyond_the_frames_of_one_launch(mcrt, gpu):
    # one launch takes 4096 frames (blockIdx.y); a handle may be listed any number of times
    n = 4096 + 5
    cfg = abi.Config(width=12, height=8, tileSize=8)
    sds = _pose_sheet(mcrt, 3)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        singles = [_device_layers(h, cfg, ("depth", "id"))[1] for h in handles]
        assert all((s["id"][..., 0] >= 0).any() for s in singles)
        px = cfg.width * cfg.height
        buf = _buffers(n, px, ("depth", "id"))
        mcrt.render_layers_batch_device([handles[i % 3] for i in range(n)], cfg, stream=torch.cuda.current_stream().cuda_stream, **_ptrs(buf, ("depth", "id")))
        torch.cuda.synchronize()
        got = _frames(buf, cfg, ("depth", "id"))
        for k in ("depth", "id"):
            want = np.stack([singles[i % 3][k] for i in range(n)])
            assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), k
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_pick_equals_the_planes_and_the_oracle_point(mcrt, gpu):
    sd, cfg, exp = L.skin_expectation("pose6_orbit_96x64")
    g = np.random.default_rng(7)
    xy = np.stack([g.integers(0, cfg.width, 200), g.integers(0, cfg.height, 200)], axis=1)
    xy = np.concatenate([xy, [[0, 0], [cfg.width - 1, 0], [0, cfg.height - 1], [cfg.width - 1, cfg.height - 1]]]).astype(np.int64)
    assert exp["hit"][xy[:, 1], xy[:, 0]].sum() >= 20
    ds = mcrt.DeviceScene(sd)
    try:
        planes = _device_layers(ds, cfg)[1]
        rec = ds.pick(cfg, xy)
        assert rec.dtype == abi.SURFACE_DTYPE and len(rec) == 204
        at = (xy[:, 1], xy[:, 0])
        ids = np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1)
        assert np.array_equal(ids, planes["id"][at])
        scenes.assert_bit_equal(rec["t"], planes["depth"][at], "pick t")
        scenes.assert_bit_equal(rec["normal"], planes["normal"][at], "pick normal")
        scenes.assert_bit_equal(rec["albedo"], planes["albedo"][at], "pick albedo")
        scenes.assert_bit_equal(rec["point"], exp["point"][at], "pick point")
        one = ds.pick(cfg, xy[37:38])
        assert one.tobytes() == rec[37:38].tobytes()
        assert len(ds.pick(cfg, np.zeros((0, 2), np.int32))) == 0
        with pytest.raises(ValueError):
            ds.pick(cfg, [[cfg.width, 0]])
        ds.check()
    finally:
        ds.close()


@gpu_test
def test_layers_beside_the_beauty_render_of_one_handle(mcrt, gpu):
    sd, lcfg, exp = L.skin_expectation("pose0_default_96x64")
    cfg = abi.Config(width=96, height=64, samplesPerPixel=2)  # the reference's defaults otherwise: 3 bounces, soft shadows
    ds = mcrt.DeviceScene(sd)
    try:
        main, side = torch.cuda.Stream(), torch.cuda.Stream()
        first = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        second = torch.zeros_like(first)
        buf = _buffers(1, cfg.width * cfg.height)
        torch.cuda.synchronize()
        ds.render_device(cfg, first.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.render_layers_device(lcfg, stream=side.cuda_stream, **_ptrs(buf, PLANES))  # no wait for the render: it reads the scene alone
        ds.render_device(cfg, second.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.check()  # waits for all three
        torch.cuda.synchronize()
        scenes.assert_bit_equal(second.cpu().numpy(), first.cpu().numpy(), "beauty after the layers pass")
        assert float(first[..., 3].min().item()) > 0.0  # an opaque frame was rendered
        L.assert_layers_equal({k: v[0] for k, v in _frames(buf, lcfg, PLANES).items()}, exp, "layers beside the render")
    finally:
        ds.close()


@gpu_test
def test_pixels_without_a_mesh_are_empty_in_the_transparent_frame(mcrt, gpu):
    sd, lcfg, exp = L.skin_expectation("pose6_orbit_96x64")
    cfg = abi.Config(width=96, height=64, samplesPerPixel=1, dofEnabled=False)
    frame = mcrt.TileRenderer.render(sd, cfg, background="transparent")
    assert mcrt.TileRenderer.lastErrors() == []
    ids = mcrt.TileRenderer.renderLayers(sd, lcfg, layers=("id",))["id"]
    miss = ids[..., 0] == -1
    assert miss.any() and (~miss).sum() >= 300
    assert not frame[miss].any()
    assert (frame[~miss][:, 3] > 0.0).all()  # and where a mesh is named the figure is there
