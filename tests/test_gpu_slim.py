"""The slim player model on the GPU: beauty renders of the built figure against the CPU oracle, repaintable slim handles (blob
byte for byte the host's flatten, frames bit for bit the oracle's), classic and slim handles mixed in ONE repaint launch and
in one view launch, every pass on a slim figure, and the farm class with both models (tests/slim_checker.py).  Frames are
64x64 or 128x128, at most 4 samples per pixel and 2 bounces."""
import numpy as np
import pytest
import torch

import bake_checker
import cutout_checker
import ground_checker
import ground_occlusion_checker
import layers_checker
import light_checker
import reflection_checker
import scenes
import shot_checker
import skin_paint_checker as S
import slim_checker as SL
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
IMAGE = 64 * 64 * 4
MESH_OPAQUE = 32
SMALL = abi.Config(width=64, height=64, maxBounces=2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pose(mcrt, i):
    return mcrt.getBuiltinPoses()[i]


def _render(ds, cfg):
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _flags(blob):
    return np.frombuffer(S.blob_parts(blob)["mesh flags"], np.uint32)


# ---- the built figure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", [0, 3], ids=["standing", "waving"])
@pytest.mark.parametrize("config", ["128_1spp", "64_4spp_ao"])
def test_beauty_render_of_the_slim_figure_equals_the_oracle(mcrt, gpu, oracle, pose, config):
    cfg = {"128_1spp": abi.Config(width=128, height=128, maxBounces=2),
           "64_4spp_ao": abi.Config(width=64, height=64, maxBounces=2, samplesPerPixel=4, aoEnabled=True)}[config]
    skin, p = SL.skin("synthetic"), _pose(mcrt, pose)
    if pose == 3:
        assert (float(p[4]), float(p[5])) == (-140.0, -20.0)  # the right arm
    sd = mcrt.MeshBuilder.buildScene(skin, p, model="slim")
    got = mcrt.TileRenderer.render(sd, cfg, device=0)
    assert not mcrt.TileRenderer.lastErrors()
    scenes.assert_bit_equal(got, SL.oracle_frame(oracle, skin, p, cfg), f"slim {config} pose {pose}")
    assert got.tobytes() != mcrt.TileRenderer.render(mcrt.MeshBuilder.buildScene(skin, p), cfg, device=0).tobytes()


# ---- repaintable slim handles ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose,look", [("synthetic", 0, None), ("all_bytes", 3, "look"), ("overlays_cleared", 6, None),
                                            ("all_opaque", 0, "look"), ("arm_hole", 3, None)])
def test_repainted_slim_handle(mcrt, gpu, oracle, name, pose, look):
    skin, p, lk = SL.skin(name), _pose(mcrt, pose), S.LOOK if look else None
    white = np.full_like(skin, 255)
    ds = mcrt.DeviceScene.for_skin("S64S", p, S.look_desc(lk))
    try:
        assert ds.skin_height == 64 and ds.skin_model == "slim" and ds.texels == 3136
        S.assert_blob_equal(ds.blob(), SL.expected_blob(white, p, lk), f"{name}: before the first repaint")
        ds.set_skin(skin)
        want = SL.expected_blob(skin, p, lk)
        S.assert_blob_equal(ds.blob(), want, f"{name}: host form")
        ds.set_skin(white)
        padded = torch.zeros(IMAGE + 16, dtype=torch.uint8, device="cuda")  # 4-byte but not 16-byte aligned: the narrow loads
        padded[4:4 + IMAGE] = torch.from_numpy(np.array(skin).reshape(-1)).cuda()
        ds.set_skin_device(padded.data_ptr() + 4, _stream())
        S.assert_blob_equal(ds.blob(), want, f"{name}: device form, image at a 4-byte boundary")
        frame = _render(ds, SMALL)
        scenes.assert_bit_equal(frame, SL.oracle_frame(oracle, skin, p, SMALL, lk), f"{name}: against the oracle")
        built = mcrt.TileRenderer.render(SL.reference_scene(skin, p, lk), SMALL, device=0)
        scenes.assert_bit_equal(frame, built, f"{name}: against buildScene(model='slim')")
        ds.check()
    finally:
        ds.close()
    opaque = [(f & MESH_OPAQUE) != 0 for f in _flags(want)]
    if name == "arm_hole":  # the right arm's inner mesh, and no other inner one
        assert opaque[0::2] == [True, True, False, True, True, True]
        assert opaque == [(f & MESH_OPAQUE) != 0 for f in _flags(SL.expected_blob(SL.skin("synthetic"), p, lk))][:4] + [False] + opaque[5:]
    elif name == "all_opaque":
        assert all(opaque)
    elif name == "overlays_cleared":
        assert opaque[0::2] == [True] * 6 and opaque[1::2] == [False] * 6


# ---- mixed batches: ONE repaint launch ----------------------------------------------------------------------------------------
def _batch_skin(model, i):
    return S.variant(SL.skin("synthetic") if model == "slim" else S.skin("synthetic_S64"), i + 1)


def _expected(model, skin, pose):
    return SL.expected_blob(skin, pose) if model == "slim" else S.expected_blob(skin, pose)


def _repaint_mixed(mcrt, models, lead, stride):
    """Handles of `models`, skin i at byte lead + i * stride of a device buffer; one set_skins_batch_device; returns the blobs."""
    n = len(models)
    skins = [_batch_skin(m, i) for i, m in enumerate(models)]
    host = np.full(lead + n * stride + 16, 0xA5, np.uint8)
    for i, s in enumerate(skins):
        host[lead + i * stride:lead + i * stride + IMAGE] = s.reshape(-1)
    d_skins = torch.from_numpy(host).cuda()
    assert d_skins.data_ptr() % 16 == 0
    handles = [mcrt.DeviceScene.for_skin(SL.KIND[m], _pose(mcrt, i % 7)) for i, m in enumerate(models)]
    try:
        mcrt.set_skins_batch_device(handles, d_skins.data_ptr() + lead, stride, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(d_skins.cpu().numpy(), host), "the launch wrote into the image buffer"
        blobs = [h.blob() for h in handles]
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()
    return skins, blobs


@pytest.mark.parametrize("lead,stride", [(4, IMAGE + 4), (0, IMAGE + 16)], ids=["scalar_copy_path", "aligned"])
def test_mixed_batch_in_one_launch(mcrt, gpu, lead, stride):
    models = ["classic", "slim", "slim", "classic", "slim"]
    skins, blobs = _repaint_mixed(mcrt, models, lead, stride)
    assert [len(b) for b in blobs] == [len(_expected(m, skins[i], _pose(mcrt, i))) for i, m in enumerate(models)]
    assert len(blobs[1]) == len(blobs[0]) - 128 * 16 - 8 * 4
    for i, m in enumerate(models):
        single = mcrt.DeviceScene.for_skin(SL.KIND[m], _pose(mcrt, i))  # the blob of its own single call
        try:
            single.set_skin(skins[i])
            S.assert_blob_equal(blobs[i], single.blob(), f"handle {i} ({m}) against its own single call")
        finally:
            single.close()
        S.assert_blob_equal(blobs[i], _expected(m, skins[i], _pose(mcrt, i)), f"handle {i} ({m}) against the host's flatten")


@pytest.mark.parametrize("models", [["slim"], ["classic", "slim"] * 16 + ["classic"], ["slim"] * 6, ["classic"] * 6],
                         ids=["one_slim", "33_alternating", "all_slim", "all_classic"])
def test_mixed_batch_edge_sizes(mcrt, gpu, models):
    skins, blobs = _repaint_mixed(mcrt, models, 0, IMAGE)
    for i, m in enumerate(models):
        S.assert_blob_equal(blobs[i], _expected(m, skins[i], _pose(mcrt, i % 7)), f"handle {i} ({m}) of {len(models)}")


# ---- views ---------------------------------------------------------------------------------------------------------------
def test_views_of_a_mixed_batch_in_one_launch(mcrt, gpu):
    models = ["classic", "slim"]
    skins = [S.skin("head_overlay_only"), SL.skin("arm_hole")]
    p0, p1 = _pose(mcrt, 0), _pose(mcrt, 6)
    handles = [mcrt.DeviceScene.for_skin(SL.KIND[m], p0) for m in models]
    fresh = [mcrt.DeviceScene.for_skin(SL.KIND[m], p1, S.look_desc(S.LOOK)) for m in models]
    try:
        for h, f, s in zip(handles, fresh, skins):
            h.set_skin(s)
            f.set_skin(s)
        before = [h.blob() for h in handles]
        mcrt.set_views_batch_device(handles, np.stack([p1, p1]), [S.look_desc(S.LOOK)] * 2, _stream())
        torch.cuda.synchronize()
        for i, m in enumerate(models):
            got = handles[i].blob()
            table = mcrt.skin_view_table(SL.KIND[m], p1, S.look_desc(S.LOOK))
            assert len(table) == 2496 and got[2496:] == before[i][2496:], f"{m}: the view launch wrote behind the prefix"
            assert S.blob_parts(got)["header and meshes but their flags"] == S.blob_parts(table + got[2496:])["header and meshes but their flags"]
            assert np.array_equal(_flags(got) & MESH_OPAQUE, _flags(before[i]) & MESH_OPAQUE) and not (_flags(got) & MESH_OPAQUE).all()
            assert np.array_equal(_flags(got) & ~np.uint32(MESH_OPAQUE), _flags(table + got[2496:]) & ~np.uint32(MESH_OPAQUE))
            want = SL.expected_blob(skins[i], p1, S.LOOK) if m == "slim" else S.expected_blob(skins[i], p1, S.LOOK)
            S.assert_blob_equal(got, want, f"{m}: after the view change")
            scenes.assert_bit_equal(_render(handles[i], SMALL), _render(fresh[i], SMALL), f"{m}: against a fresh handle at that view")
            handles[i].check()
    finally:
        for h in handles + fresh:
            h.close()


# ---- the passes on a slim figure ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slim_figure(mcrt, gpu):
    """A repainted slim handle with the layers checker's skin (every texel its own colour, every outer part kept: 12 meshes in
    the oracle's scene too), its description for the oracle, and a pass config."""
    skin, p = layers_checker.unique_skin("S64"), _pose(mcrt, 3)
    ds = mcrt.DeviceScene.for_skin("S64S", p)
    ds.set_skin(skin)
    sd = SL.reference_scene(skin, p)
    assert sd.desc.n_meshes == 12
    yield ds, sd, skin, abi.Config(width=64, height=64, maxBounces=2)
    ds.close()


def _planes(spec):
    return {k: torch.zeros(shape, dtype=dtype, device="cuda") for k, (shape, dtype) in spec.items()}


def _download(t):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def test_layers_and_pick_on_a_slim_figure(mcrt, slim_figure, oracle):
    ds, sd, skin, cfg = slim_figure
    h, w = cfg.height, cfg.width
    t = _planes({"depth": ((h, w), torch.float32), "normal": ((h, w, 4), torch.float32), "albedo": ((h, w, 4), torch.float32), "id": ((h, w, 4), torch.int32)})
    ds.render_layers_device(cfg, t["depth"].data_ptr(), t["normal"].data_ptr(), t["albedo"].data_ptr(), t["id"].data_ptr(), _stream())
    got = _download(t)
    layers_checker.assert_layers_equal(got, layers_checker.expected_layers(oracle, sd, w, h), "slim layers")
    ids = got["id"]
    arm = np.argwhere(np.isin(ids[..., 0], SL.ARM_MESHES))
    assert len(arm) >= 40
    rec = ds.pick(cfg, arm[:, ::-1].astype(np.int32))
    assert np.array_equal(np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1), ids[arm[:, 0], arm[:, 1]])
    texel = skin.astype(np.float32) / np.float32(255.0)
    for r in rec:
        m, face = int(r["mesh"]), int(r["face"]) & 7
        x, y, fw, fh = SL.face_rect(SL.SLIM_BOXES[m], face)
        sx, sy = mcrt.skin_texel("S64S", m, face, int(r["tx"]), int(r["ty"]))
        assert x <= sx < x + fw and y <= sy < y + fh and fw == (4 if face in (2, 3) else 3)
        assert r["albedo"].tobytes() == texel[sy, sx].tobytes()


def test_ground_shadow_on_a_slim_figure(slim_figure, oracle):
    ds, sd, _, cfg = slim_figure
    h, w = cfg.height, cfg.width
    t = _planes({"visibility": ((h, w), torch.float32), "distance": ((h, w), torch.float32), "matte": ((h, w), torch.uint8)})
    ds.render_ground_device(cfg, 0.0, t["visibility"].data_ptr(), t["distance"].data_ptr(), t["matte"].data_ptr(), _stream())
    exp = ground_checker.expected_ground(oracle, sd, cfg, 0.0)
    ground_checker.assert_ground_equal(_download(t), exp, "slim ground shadow")
    assert (exp["visibility"] < 1).any()


def test_ground_occlusion_on_a_slim_figure(slim_figure, oracle):
    ds, sd, _, cfg = slim_figure
    h, w = cfg.height, cfg.width
    t = _planes({"occlusion": ((h, w), torch.float32), "matte": ((h, w), torch.uint8)})
    ds.render_ground_occlusion_device(cfg, 0.0, occlusion_ptr=t["occlusion"].data_ptr(), matte_ptr=t["matte"].data_ptr(), stream=_stream())
    exp = ground_occlusion_checker.expected_ground_occlusion(oracle, sd, cfg, 0.0)
    ground_occlusion_checker.assert_planes_equal(_download(t), exp, "slim ground occlusion")
    assert (exp["occlusion"] < 1).any()


def test_reflection_on_a_slim_figure(slim_figure, oracle):
    ds, sd, _, cfg = slim_figure
    h, w = cfg.height, cfg.width
    t = _planes({"rgba": ((h, w, 4), torch.float32), "rgba8": ((h, w, 4), torch.uint8), "distance": ((h, w), torch.float32)})
    ds.render_reflection_device(cfg, 0.0, t["rgba"].data_ptr(), t["rgba8"].data_ptr(), t["distance"].data_ptr(), _stream())
    exp = reflection_checker.expected_reflection(oracle, sd, cfg, 0.0)
    reflection_checker.assert_reflection_equal(_download(t), exp, "slim reflection")
    assert exp["hit"].any()


def test_light_layers_on_a_slim_figure(slim_figure, oracle):
    ds, sd, _, cfg = slim_figure
    h, w = cfg.height, cfg.width
    t = _planes({"visibility": ((h, w), torch.float32), "occlusion": ((h, w), torch.float32), "direct": ((h, w, 4), torch.float32)})
    ds.render_light_device(cfg, t["visibility"].data_ptr(), t["occlusion"].data_ptr(), t["direct"].data_ptr(), _stream())
    light_checker.assert_light_equal(_download(t), light_checker.expected_light(oracle, sd, cfg), "slim light layers")


def test_bake_on_a_slim_figure(mcrt, slim_figure, oracle):
    ds, sd, _, cfg = slim_figure
    n = ds.texels
    assert n == 3136
    t = _planes({"position": ((n, 4), torch.float32), "normal": ((n, 4), torch.float32), "visibility": ((n,), torch.float32),
                 "occlusion": ((n,), torch.float32), "direct": ((n, 4), torch.float32)})
    ds.bake_light_device(cfg, 2, t["position"].data_ptr(), t["normal"].data_ptr(), t["visibility"].data_ptr(), t["occlusion"].data_ptr(),
                         t["direct"].data_ptr(), _stream())
    got = _download(t)
    exp = bake_checker.expected_bake(oracle, sd, cfg, grid=2, blob=ds.blob())
    assert np.array_equal(exp["table"], SL.pool_rows("slim")[:, :4])
    bake_checker.assert_bake_equal(got, exp, "slim bake, grid 2")
    # the baked plane in the skin's own layout: the pixels no slim texel is cut from stay at `fill`
    image = mcrt.pool_to_skin("S64S", got["occlusion"], fill=-1.0)
    assert image.shape == (64, 64) and (image[mcrt.skins.slim_unused_mask()] == -1.0).all()
    for x, y in SL.detection_pixels():
        assert image[y, x] == -1.0
    assert (image[20:32, 44:47] >= 0).all()  # the right arm's front face


@pytest.mark.parametrize("page", ["opaque", "cutout"])
def test_studio_shot_of_a_slim_figure(mcrt, gpu, oracle, page):
    skin, p = layers_checker.unique_skin("S64"), _pose(mcrt, 3)
    cfg = abi.Config(width=64, height=64, maxBounces=2)
    sd = SL.reference_scene(skin, p)
    batch = mcrt.SkinBatch(1, "S64", p, slim=True)
    try:
        if page == "opaque":
            exp = shot_checker.expected_shot(oracle, sd, cfg, shot_checker.SHOT, 0.0)
            got = batch.shots(skin[None], cfg, shot_checker.SHOT, ground=0.0, rgba8=False, models=["slim"])
            got8 = batch.shots(skin[None], cfg, shot_checker.SHOT, ground=0.0, models=["slim"])
            shot_checker.assert_shot_equal(got[0], got8[0], exp["out"], "slim studio shot")
        else:
            shot = abi.Shot(page="transparent", reflectionFade=24.0, floorOcclusion=0.5, shadowColor=(0.125, 0.0625, 0.25))
            exp = cutout_checker.expected_shot_ex(oracle, sd, cfg, shot, 0.0)
            got, boxes = batch.shots(skin[None], cfg, shot, ground=0.0, rgba8=False, bounds=True, models=["slim"])
            shot_checker.assert_shot_equal(got[0], None, exp["out"], "slim cut-out")
            assert np.array_equal(boxes[0], exp["bounds"])
    finally:
        batch.close()


# ---- the farm class ----------------------------------------------------------------------------------------------------------
def test_skin_batch_with_both_models(mcrt, gpu):
    cfg = abi.Config(width=64, height=64, maxBounces=2)
    p = _pose(mcrt, 5)
    models = ["classic", "slim", "slim", "classic"]
    skins = np.stack([S.skin("synthetic_S64"), SL.skin("synthetic"), SL.skin("arm_hole"), S.skin("all_transparent")])
    assert [mcrt.skin_model(s) for s in skins] == models
    built = [mcrt.MeshBuilder.buildScene(s, p, model=m) for s, m in zip(skins, models)]
    want = mcrt.TileRenderer.renderBatch(built, cfg)
    classic_want = mcrt.TileRenderer.renderBatch([mcrt.MeshBuilder.buildScene(s, p) for s in skins], cfg)
    assert want[1].tobytes() != classic_want[1].tobytes() and want[0].tobytes() == classic_want[0].tobytes()
    batch, parent = mcrt.SkinBatch(4, "S64", p, slim=True), mcrt.SkinBatch(4, "S64", p)
    try:
        got = batch.render(skins, cfg, models=models)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
        assert batch.render(skins, cfg, models="auto").tobytes() == want.tobytes()
        assert batch.render(skins[::-1], cfg, models=models[::-1]).tobytes() == want[::-1].tobytes()  # the same slots, other models
        none = batch.render(skins, cfg)
        assert none.tobytes() == parent.render(skins, cfg).tobytes() == classic_want.tobytes()
        assert batch.scenes[1].blob() == parent.scenes[1].blob() == S.expected_blob(skins[1], p)
        shot = shot_checker.SHOT
        shots = batch.shots(skins, cfg, shot, ground=0.0, models=models)
        assert shots.tobytes() == mcrt.TileRenderer.renderShotBatch(built, cfg, shot, ground=0.0).tobytes()
        assert batch.shots(skins, cfg, shot, ground=0.0, models="auto").tobytes() == shots.tobytes()
        ids = batch.layers(skins, cfg, layers=("id",), models=models)["id"]
        assert ids.tobytes() != batch.layers(skins, cfg, layers=("id",))["id"].tobytes()
        # another view for both scenes of every slot
        q = _pose(mcrt, 3)
        batch.set_views(q)
        moved = batch.render(skins, cfg, models=models)
        assert moved.tobytes() == mcrt.TileRenderer.renderBatch([mcrt.MeshBuilder.buildScene(s, q, model=m) for s, m in zip(skins, models)], cfg).tobytes()
        with pytest.raises(ValueError):
            batch.render(skins, cfg, models=["slim"])
        with pytest.raises(ValueError):
            parent.render(skins, cfg, models=models)
        with pytest.raises(ValueError):
            mcrt.SkinBatch(1, "S32", slim=True)
    finally:
        batch.close()
        parent.close()
