"""Skins on resident scenes on the GPU (mcrt_scene_create_skin, mcrt_scene_set_skin*): after a repaint the resident blob is
byte for byte the host's flatten of the full-table scene with that skin's texels, and every frame of the handle is bit for
bit the CPU oracle's frame of ``buildScene(skin, pose)`` — the reference-shaped scene, its fully transparent outer parts
dropped — with the same look (tests/skin_paint_checker.py).  Frames are 96x64 or smaller."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes
import skin_paint_checker as S
import transparent_checker
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib(mcrt):
    from minecraftskin_raytracer_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return transparent_checker.Checker(transparent_checker.build(str(tmp_path_factory.mktemp("transparent_oracle"))))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pose(mcrt, i):
    return mcrt.getBuiltinPoses()[i]


def _device_skin(skin):
    return torch.from_numpy(np.array(skin, np.uint8)).cuda()  # (a copy: the suite's skins are read-only)


def _render(ds, cfg, stream=None):
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream() if stream is None else stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


CONFIGS = {
    "default": abi.Config(width=96, height=64),  # the reference's defaults: 3 bounces, 1 spp, soft shadows, tile 32
    "hard_shadows": abi.Config(width=96, height=64, softShadows=False),
    "ao_64": abi.Config(width=64, height=64, aoEnabled=True),
    "spp2": abi.Config(width=96, height=64, samplesPerPixel=2),
    "small": abi.Config(width=32, height=32),
}


# ---- blob parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose,look", [
    ("synthetic_S64", 0, None), ("synthetic_S32", 0, None), ("head_overlay_only", 6, None), ("all_transparent", 0, None),
    ("all_opaque", 6, None), ("all_bytes", 0, None), ("inner_hole", 6, None), ("synthetic_S64", 6, "look"), ("synthetic_S32", 6, "look"),
])
def test_repainted_blob_equals_the_host_flatten(mcrt, gpu, name, pose, look):
    skin, p, lk = S.skin(name), _pose(mcrt, pose), S.LOOK if look else None
    ds = mcrt.DeviceScene.for_skin(S.kind_of(skin), p, S.look_desc(lk))
    try:
        white = np.full_like(skin, 255)
        S.assert_blob_equal(ds.blob(), S.expected_blob(white, p, lk), f"{name}: before the first repaint")
        d_skin = _device_skin(skin)
        ds.set_skin_device(d_skin.data_ptr(), _stream())
        want = S.expected_blob(skin, p, lk)
        S.assert_blob_equal(ds.blob(), want, f"{name}: device form")
        ds.set_skin(white)  # the host form, there and back
        S.assert_blob_equal(ds.blob(), S.expected_blob(white, p, lk), f"{name}: host form, white")
        ds.set_skin(skin)
        S.assert_blob_equal(ds.blob(), want, f"{name}: host form")
        # an image that is 4-byte but not 16-byte aligned takes the narrow staging loads
        padded = torch.zeros(skin.size + 16, dtype=torch.uint8, device="cuda")
        padded[4:4 + skin.size] = d_skin.reshape(-1)
        ds.set_skin(white)
        ds.set_skin_device(padded.data_ptr() + 4, _stream())
        S.assert_blob_equal(ds.blob(), want, f"{name}: image at a 4-byte boundary")
        ds.check()
    finally:
        ds.close()
    flags = np.frombuffer(S.blob_parts(want)["mesh flags"], np.uint32)
    opaque = [(f & 32) != 0 for f in flags]
    if name == "all_opaque":
        assert all(opaque)
    elif name == "inner_hole":
        assert opaque[0] and not opaque[2] and opaque[4]  # the body's inner mesh alone among the inner ones
    elif name == "all_transparent":
        assert opaque[0::2] == [True] * 6 and opaque[1::2] == [False] * 6
    elif name == "all_bytes":
        assert all(opaque) and len(set(np.frombuffer(S.blob_parts(want)["texel pool"], np.float32).tolist())) == 256


# ---- frame parity against the CPU oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("config,name,pose,look", [
    ("default", "synthetic_S64", 0, None), ("default", "head_overlay_only", 6, None), ("default", "all_transparent", 6, None),
    ("default", "synthetic_S32", 1, None), ("default", "synthetic_S64", 3, "look"), ("hard_shadows", "synthetic_S64", 6, None),
    ("ao_64", "head_overlay_only", 0, None), ("spp2", "all_transparent", 0, None), ("spp2", "synthetic_S64", 6, None),
])
def test_repainted_frames_equal_the_oracle(mcrt, gpu, oracle, config, name, pose, look):
    skin, p, cfg, lk = S.skin(name), _pose(mcrt, pose), CONFIGS[config], S.LOOK if look else None
    n_ref = len(S.reference_scene(skin, p).to_numpy()["meshes"])
    assert n_ref == {"head_overlay_only": 7, "all_transparent": 6, "synthetic_S32": 7}.get(name, 12)  # the reference drops parts
    want = S.oracle_frame(oracle, skin, p, cfg, lk)
    ds = mcrt.DeviceScene.for_skin(S.kind_of(skin), p, S.look_desc(lk))
    try:
        ds.set_skin_device(_device_skin(skin).data_ptr(), _stream())
        scenes.assert_bit_equal(_render(ds, cfg), want, f"{config} {name} pose {pose}")
        ds.check()
    finally:
        ds.close()


@pytest.mark.parametrize("name,pose", [("synthetic_S64", 6), ("all_transparent", 0), ("head_overlay_only", 3)])
def test_repainted_transparent_frames_equal_the_oracle(mcrt, gpu, checker, name, pose):
    skin, p = S.skin(name), _pose(mcrt, pose)
    cfg = abi.Config(width=96, height=64, samplesPerPixel=2)
    want, _ = checker.render(S.reference_scene(skin, p).ptr, cfg, "transparent", threads=transparent_checker.threads())
    ds = mcrt.DeviceScene.for_skin("S64", p)
    try:
        ds.set_background("transparent")
        ds.set_skin(skin)
        got = _render(ds, cfg)
        scenes.assert_bit_equal(got, want, f"transparent {name}")
        assert (got[..., 3] == 0).any() and (got[..., 3] > 0).any()
    finally:
        ds.close()


# ---- repaint sequence and ordering -------------------------------------------------------------------------------------------
def test_repaint_sequence_on_one_handle(mcrt, gpu, oracle):
    p, cfg = _pose(mcrt, 6), CONFIGS["spp2"]  # jittered samples: the background plate and the draw plate come into play
    a, b = S.skin("synthetic_S64"), S.skin("head_overlay_only")
    fa, fb = S.oracle_frame(oracle, a, p, cfg), S.oracle_frame(oracle, b, p, cfg)
    assert fa.tobytes() != fb.tobytes()
    da, db = _device_skin(a), _device_skin(b)
    ds = mcrt.DeviceScene.for_skin("S64", p)
    try:
        ds.set_skin_device(da.data_ptr(), _stream())
        for k in range(3):
            scenes.assert_bit_equal(_render(ds, cfg), fa, f"skin A, render {k}")
        ds.set_skin_device(db.data_ptr(), _stream())
        scenes.assert_bit_equal(_render(ds, cfg), fb, "skin B")
        ds.set_skin_device(da.data_ptr(), _stream())
        scenes.assert_bit_equal(_render(ds, cfg), fa, "skin A again (the recorded launch sequence)")
        scenes.assert_bit_equal(_render(ds, cfg), fa, "skin A, once more")
        ds.check()
    finally:
        ds.close()


def test_a_repaint_on_another_stream_is_ordered_between_two_renders(mcrt, gpu, oracle):
    p, cfg = _pose(mcrt, 0), CONFIGS["default"]
    a, b = S.skin("synthetic_S64"), S.skin("all_transparent")
    fa, fb = S.oracle_frame(oracle, a, p, cfg), S.oracle_frame(oracle, b, p, cfg)
    assert fa.tobytes() != fb.tobytes()
    da, db = _device_skin(a), _device_skin(b)
    first = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    second = torch.zeros_like(first)
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    ds = mcrt.DeviceScene.for_skin("S64", p)
    try:
        ds.set_skin_device(da.data_ptr(), _stream())
        torch.cuda.synchronize()
        ds.render_device(cfg, first.data_ptr(), 0, 1, abi.LAYOUT_FRAME, one.cuda_stream)
        ds.set_skin_device(db.data_ptr(), two.cuda_stream)  # no host wait: the handle's events order it
        ds.render_device(cfg, second.data_ptr(), 0, 1, abi.LAYOUT_FRAME, one.cuda_stream)
        ds.check()
        torch.cuda.synchronize()
        scenes.assert_bit_equal(first.cpu().numpy(), fa, "the render before the repaint")
        scenes.assert_bit_equal(second.cpu().numpy(), fb, "the render behind the repaint")
    finally:
        ds.close()


# ---- batches -------------------------------------------------------------------------------------------------------------
def test_batch_with_a_gap_between_the_images(mcrt, gpu):
    base = S.skin("synthetic_S64")
    skins = [S.variant(base, i + 1) for i in range(4)] + [S.skin("all_transparent")]
    image, stride = 64 * 64 * 4, 64 * 64 * 4 + 64
    host = np.full((5, stride), SENTINEL, np.uint8)
    for i, s in enumerate(skins):
        host[i, :image] = s.reshape(-1)
    d_skins = torch.from_numpy(host).cuda()
    handles = [mcrt.DeviceScene.for_skin("S64", _pose(mcrt, i)) for i in range(5)]
    try:
        mcrt.set_skins_batch_device(handles, d_skins.data_ptr(), stride, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(d_skins.cpu().numpy(), host), "the launch wrote into the image buffer"
        for i, h in enumerate(handles):
            S.assert_blob_equal(h.blob(), S.expected_blob(skins[i], _pose(mcrt, i)), f"handle {i}")
    finally:
        for h in handles:
            h.close()


def test_batch_beyond_one_launch_sequence_of_renders(mcrt, gpu, oracle):
    n, cfg = 300, CONFIGS["small"]  # render_batch_device takes 256 frames per launch sequence
    base = S.skin("synthetic_S64")
    skins = np.stack([S.variant(base, i) for i in range(n)])
    poses = [_pose(mcrt, i % 7) for i in range(n)]
    d_skins = torch.from_numpy(skins).cuda()
    handles = [mcrt.DeviceScene.for_skin("S64", poses[i]) for i in range(n)]
    try:
        mcrt.set_skins_batch_device(handles, d_skins.data_ptr(), stream=_stream())
        for i in (0, n - 1):
            S.assert_blob_equal(handles[i].blob(), S.expected_blob(skins[i], poses[i]), f"handle {i}")
        px = cfg.width * cfg.height
        out = torch.zeros((n, px, 4), dtype=torch.float32, device="cuda")
        mcrt.render_batch_device(handles, cfg, out.data_ptr(), 0, px, _stream())
        torch.cuda.synchronize()
        assert mcrt.last_batch_info() == {"batched_frames": n, "launch_sequences": 2}
        frames = out.cpu().numpy().reshape(n, cfg.height, cfg.width, 4)
        for i in (0, 255, 256, 299):
            scenes.assert_bit_equal(frames[i], S.oracle_frame(oracle, skins[i], poses[i], cfg), f"frame {i}")
    finally:
        for h in handles:
            h.close()


# ---- layers and picks ------------------------------------------------------------------------------------------------------
def test_layers_and_picks_show_the_new_skin(mcrt, gpu):
    cfg = abi.Config(width=96, height=64)
    skins = np.stack([S.skin("all_bytes"), S.skin("head_overlay_only")])
    batch = mcrt.SkinBatch(2, "S64", _pose(mcrt, 3))
    try:
        planes = batch.layers(skins, cfg, layers=("albedo", "id"))
        assert planes["albedo"].shape == (2, 64, 96, 4) and planes["id"].shape == (2, 64, 96, 4)
        for k in range(2):
            texel = skins[k].astype(np.float32) / np.float32(255.0)
            ids, albedo = planes["id"][k], planes["albedo"][k]
            hit = ids[..., 0] >= 0
            assert hit.sum() >= 300
            assert not albedo[~hit].any()
            for y, x in np.argwhere(hit):
                m, face, tx, ty = (int(v) for v in ids[y, x])
                sx, sy = mcrt.skin_texel("S64", m, face, tx, ty)
                assert albedo[y, x].tobytes() == texel[sy, sx].tobytes(), (k, x, y, m, face, tx, ty)
            xy = np.argwhere(hit)[::7, ::-1].astype(np.int32)
            rec = batch.scenes[k].pick(cfg, xy)
            at = (xy[:, 1], xy[:, 0])
            assert np.array_equal(np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1), ids[at])
            scenes.assert_bit_equal(rec["albedo"], albedo[at], f"pick albedo, skin {k}")
        # the cleared overlays of the second skin: of the outer meshes (odd indices) only the head's can be hit
        meshes = planes["id"][1][..., 0]
        meshes = meshes[meshes >= 0]
        assert set(meshes[meshes % 2 == 1].tolist()) <= {1} and (meshes % 2 == 0).any()
    finally:
        batch.close()


# ---- the Python farm class --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgba8", [False, True])
@pytest.mark.parametrize("background", ["reference", "transparent"])
def test_skin_batch_equals_render_batch_of_built_scenes(mcrt, gpu, rgba8, background):
    cfg = abi.Config(width=64, height=48)
    p = _pose(mcrt, 5)
    skins = np.stack([S.skin("synthetic_S64"), S.skin("all_transparent"), S.skin("inner_hole")])
    want = mcrt.TileRenderer.renderBatch([mcrt.MeshBuilder.buildScene(s, p) for s in skins], cfg, rgba8=rgba8, background=background)
    batch = mcrt.SkinBatch(4, "S64", p)
    try:
        got = batch.render(skins, cfg, rgba8=rgba8, background=background)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.tobytes() == want.tobytes()
        again = batch.render(skins[::-1], cfg, rgba8=rgba8, background=background)  # the same handles, other skins
        assert again.tobytes() == want[::-1].tobytes()
        assert batch.render(skins[:0], cfg, rgba8=rgba8).shape == (0, 48, 64, 4)
        # a frame of zero size paints nothing: the handles still show the skins of the last render
        assert batch.render(skins, abi.Config(width=0, height=48), rgba8=rgba8).shape == (3, 48, 0, 4)
        assert batch.layers(skins, abi.Config(width=64, height=48, tileSize=0), layers=("id",))["id"].shape == (3, 48, 64, 4)
        assert batch.scenes[0].blob() == S.expected_blob(skins[2], p)
        with pytest.raises(ValueError):
            batch.render(np.zeros((5, 64, 64, 4), np.uint8), cfg)
    finally:
        batch.close()


# ---- refusals on the device ---------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_blobs_alone(mcrt, gpu, lib):
    p = _pose(mcrt, 0)
    skin = S.skin("synthetic_S64")
    d_skin = _device_skin(np.stack([skin, skin]))
    plain = mcrt.DeviceScene(mcrt.MeshBuilder.buildScene(skin, p))  # not repaintable: mcrt_scene_create's
    a, b = mcrt.DeviceScene.for_skin("S64", p), mcrt.DeviceScene.for_skin("S64", p)
    try:
        before = [h.blob() for h in (plain, a, b)]
        assert before[0] == mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, p))
        ptr = C.c_void_p(d_skin.data_ptr())
        assert lib.mcrt_scene_set_skin_device(plain._h, ptr, None) == abi.MCRT_ERR_INVALID
        assert lib.mcrt_scene_set_skin(plain._h, skin.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.MCRT_ERR_INVALID
        two = (C.c_void_p * 2)(a._h.value, b._h.value)
        assert lib.mcrt_scene_set_skins_batch_device(two, 2, ptr, 64 * 32 * 4, None) == abi.MCRT_ERR_INVALID  # a 64x32 image's size
        twice = (C.c_void_p * 2)(a._h.value, a._h.value)
        assert lib.mcrt_scene_set_skins_batch_device(twice, 2, ptr, 64 * 64 * 4, None) == abi.MCRT_ERR_INVALID
        mixed = (C.c_void_p * 2)(a._h.value, plain._h.value)
        assert lib.mcrt_scene_set_skins_batch_device(mixed, 2, ptr, 64 * 64 * 4, None) == abi.MCRT_ERR_INVALID
        assert [h.blob() for h in (plain, a, b)] == before
    finally:
        for h in (plain, a, b):
            h.close()
