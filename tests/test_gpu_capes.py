"""Capes on the GPU: beauty renders of built caped figures against the CPU oracle, repaintable caped handles (blob byte for byte
the host's flatten, frames bit for bit the oracle's), the independence of skin and cape repaints, batches, views with a cape
angle, every pass on a caped figure, and the farm class (tests/cape_checker.py).  Frames are 64x64, seen from behind (orbit
yaw 180) or three-quarter behind (150): the default camera cannot see a cape.  Every rendering test first holds the oracle to
at least 64 pixel centres on the cape mesh."""
import numpy as np
import pytest
import torch

import bake_checker
import cape_checker as CK
import cutout_checker
import extra_lights_checker as X
import ground_checker
import ground_occlusion_checker
import layers_checker
import light_checker
import reflection_checker
import scenes
import shot_checker
import skin_paint_checker as S
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
CAPE_BYTES = 64 * 32 * 4
MESH_OPAQUE = 32
SMALL = abi.Config(width=64, height=64, maxBounces=2)
KINDS = ("S64", "S64S", "S32")


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


def _shows_the_cape(oracle, sd, n=64):
    seen = CK.cape_pixels(oracle, sd, 64, 64)
    assert seen >= n, f"only {seen} pixel centres meet the cape: the test would be vacuous"


def _cape_parts(blob):
    """What a cape repaint owns of a caped blob — the last mesh's flags word, the last 372 texels, the last 24 words — and the rest."""
    h = CK.header(blob)
    flag = h["mesh_offset"] + 192 * (h["n_meshes"] - 1) + 68
    texels = h["alpha_offset"] - 372 * 16
    words = h["blob_bytes"] - 24 * 4
    assert h["blob_bytes"] == len(blob)
    cape = blob[flag:flag + 4] + blob[texels:h["alpha_offset"]] + blob[words:]
    rest = blob[:flag] + blob[flag + 4:texels] + blob[h["alpha_offset"]:words]
    return cape, rest


# ---- built scenes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["1spp", "4spp_ao"])
@pytest.mark.parametrize("kind,pose,yaw", [("S64", 0, 180.0), ("S64", 3, 150.0), ("S64S", 3, 180.0), ("S64S", 0, 150.0), ("S32", 0, 150.0), ("S32", 3, 180.0)])
def test_beauty_render_of_a_built_caped_figure_equals_the_oracle(mcrt, gpu, oracle, kind, pose, yaw, config):
    cfg = {"1spp": SMALL, "4spp_ao": abi.Config(width=64, height=64, maxBounces=2, samplesPerPixel=4, aoEnabled=True)}[config]
    skin, cape, p, look = CK.skin(kind), CK.cape("synthetic"), _pose(mcrt, pose), CK.behind(yaw)
    sd = CK.reference_scene(kind, skin, cape, p, 10.0, look)
    _shows_the_cape(oracle, sd)
    got = mcrt.TileRenderer.render(sd, cfg, device=0)
    assert not mcrt.TileRenderer.lastErrors()
    scenes.assert_bit_equal(got, CK.oracle_frame(oracle, kind, skin, cape, p, 10.0, cfg, look), f"{kind} pose {pose} yaw {yaw} {config}")
    capeless = mcrt.TileRenderer.render(CK.reference_scene(kind, skin, None, p, 10.0, look), cfg, device=0)
    assert got.tobytes() != capeless.tobytes()


def test_built_caped_figure_on_a_transparent_background(mcrt, gpu, oracle):
    skin, cape, p, look = CK.skin("S64"), CK.cape("one_hole"), _pose(mcrt, 0), CK.behind(150.0)
    sd = CK.reference_scene("S64", skin, cape, p, 45.0, look)
    _shows_the_cape(oracle, sd)
    got = mcrt.TileRenderer.render(sd, SMALL, device=0, background="transparent")
    solid = CK.oracle_frame(oracle, "S64", skin, cape, p, 45.0, SMALL, look)
    mesh = layers_checker.expected_surfaces(oracle, sd, 64, 64)["mesh"]
    assert np.array_equal(got[..., 3] > 0, mesh >= 0)  # 1 spp: coverage is the pixel-centre hit
    assert got[mesh >= 0].tobytes() == solid[mesh >= 0].tobytes()


# ---- repainted handles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name,pose,yaw,angle", [("S64", "synthetic", 0, 180.0, 10.0), ("S64S", "all_bytes", 3, 150.0, 45.0), ("S32", "one_hole", 0, 150.0, 10.0),
                                                      ("S64", "one_hole", 3, 180.0, 0.005), ("S64S", "synthetic", 0, 180.0, 90.0)])
def test_repainted_caped_handle(mcrt, gpu, oracle, kind, name, pose, yaw, angle):
    height, model, n_skin = CK.KINDS[kind]
    skin, cape, p, look = CK.skin(kind), CK.cape(name), _pose(mcrt, pose), CK.behind(yaw)
    white = np.full_like(skin, 255)
    ds = mcrt.DeviceScene.for_skin(kind, p, S.look_desc(look), cape=True, cape_angle=angle)
    try:
        assert ds.has_cape and ds.texels == {"S64": 3264, "S64S": 3136, "S32": 2016}[kind] + 372
        fresh = ds.blob()
        want_fresh = CK.expected_blob(kind, white, CK.cape("transparent"), p, angle, look)
        S.assert_blob_equal(fresh, want_fresh, "before the first repaint: a white skin and a transparent cape")
        assert not _flags(fresh)[-1] & MESH_OPAQUE and (_flags(fresh)[:-1] & MESH_OPAQUE).all()
        ds.set_skin(skin)
        ds.set_cape(cape)
        want = CK.expected_blob(kind, skin, cape, p, angle, look)
        S.assert_blob_equal(ds.blob(), want, f"{name}: host forms")
        sd = CK.reference_scene(kind, skin, cape, p, angle, look)
        assert sd.desc.n_meshes == n_skin + 1  # every part and the cape have a texel with alpha > 0: the builder keeps them all
        assert want == mcrt.flatten(sd)
        ds.set_cape(None)
        S.assert_blob_equal(ds.blob(), CK.expected_blob(kind, skin, CK.cape("transparent"), p, angle, look), "no cape")
        padded = torch.zeros(CAPE_BYTES + 16, dtype=torch.uint8, device="cuda")  # 4-byte but not 16-byte aligned
        padded[4:4 + CAPE_BYTES] = torch.from_numpy(np.array(cape).reshape(-1)).cuda()
        ds.set_cape_device(padded.data_ptr() + 4, _stream())
        S.assert_blob_equal(ds.blob(), want, f"{name}: device form, image at a 4-byte boundary")
        _shows_the_cape(oracle, sd)
        frame = _render(ds, SMALL)
        scenes.assert_bit_equal(frame, CK.oracle_frame(oracle, kind, skin, cape, p, angle, SMALL, look), f"{name}: against the oracle")
        ds.check()
    finally:
        ds.close()
    opaque = bool(_flags(want)[-1] & MESH_OPAQUE)
    assert opaque == (name != "one_hole")
    if name == "one_hole":  # the predicate word of texel (4, 6) of the outward face differs from the synthetic cape's, and no other
        other = CK.expected_blob(kind, skin, CK.cape("synthetic"), p, angle, look)
        a, b = np.frombuffer(want[-96:], np.uint32), np.frombuffer(other[-96:], np.uint32)
        texel = 6 * 10 + 4
        assert np.flatnonzero(a != b).tolist() == [texel // 16] and (a[texel // 16] >> (2 * (texel % 16))) & 3 == 1


def test_a_transparent_cape_renders_the_capeless_figure(mcrt, gpu, oracle):
    skin, p, look = CK.skin("S64"), _pose(mcrt, 3), CK.behind(150.0)
    caped = mcrt.DeviceScene.for_skin("S64", p, S.look_desc(look), cape=True)
    plain = mcrt.DeviceScene.for_skin("S64", p, S.look_desc(look))
    try:
        for ds in (caped, plain):
            ds.set_skin(skin)
        caped.set_cape(CK.cape("synthetic"))
        shown = _render(caped, SMALL)
        caped.set_cape(CK.cape("transparent"))
        frame = _render(caped, SMALL)
        scenes.assert_bit_equal(frame, _render(plain, SMALL), "transparent cape against the capeless handle")
        scenes.assert_bit_equal(frame, S.oracle_frame(oracle, skin, p, SMALL, look), "transparent cape against the oracle's capeless figure")
        assert shown.tobytes() != frame.tobytes()
    finally:
        caped.close()
        plain.close()


# ---- independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_skin_and_cape_repaints_leave_each_other_alone(mcrt, gpu, kind):
    p = _pose(mcrt, 6)
    skin_a, skin_b = CK.skin(kind), S.variant(CK.skin(kind), 5).copy()
    skin_b[..., 3] = 255  # other MESH_OPAQUE bits than skin_a's
    ds = mcrt.DeviceScene.for_skin(kind, p, cape=True)
    try:
        ds.set_cape(CK.cape("one_hole"))
        ds.set_skin(skin_a)
        first = ds.blob()
        S.assert_blob_equal(first, CK.expected_blob(kind, skin_a, CK.cape("one_hole"), p, 10.0), "cape, then skin")
        ds.set_skin(skin_b)
        second = ds.blob()
        assert _cape_parts(second)[0] == _cape_parts(first)[0] and _cape_parts(second)[1] != _cape_parts(first)[1]
        S.assert_blob_equal(second, CK.expected_blob(kind, skin_b, CK.cape("one_hole"), p, 10.0), "another skin")
        ds.set_cape(CK.cape("all_bytes"))
        third = ds.blob()
        assert _cape_parts(third)[1] == _cape_parts(second)[1] and _cape_parts(third)[0] != _cape_parts(second)[0]
        S.assert_blob_equal(third, CK.expected_blob(kind, skin_b, CK.cape("all_bytes"), p, 10.0), "skin, then another cape")
        ds.check()
    finally:
        ds.close()


# ---- batches ---------------------------------------------------------------------------------------------------------------
def _batch_kinds(n):
    return ["S64", "S64S"] * (n // 2) + ["S64"] * (n % 2) if n > 1 else ["S64S"]


@pytest.mark.parametrize("n,lead,stride", [(1, 0, CAPE_BYTES), (6, 4, CAPE_BYTES + 20), (33, 0, CAPE_BYTES)], ids=["one", "six_padded_stride", "33"])
def test_cape_batches(mcrt, gpu, n, lead, stride):
    """Classic-caped and slim-caped handles mixed in one call; a stride with padding and images at 4-byte boundaries; the
    last frame's cape transparent."""
    kinds = _batch_kinds(n)
    capes = [S.variant(CK.cape(("synthetic", "all_bytes", "one_hole")[i % 3]), i) for i in range(n)]
    capes[-1] = np.array(CK.cape("transparent"))
    host = np.full(lead + n * stride + 16, 0xA5, np.uint8)
    for i, c in enumerate(capes):
        host[lead + i * stride:lead + i * stride + CAPE_BYTES] = c.reshape(-1)
    d_capes = torch.from_numpy(host).cuda()
    handles = [mcrt.DeviceScene.for_skin(k, _pose(mcrt, i % 7), cape=True, cape_angle=10.0 + i) for i, k in enumerate(kinds)]
    try:
        mcrt.set_capes_batch_device(handles, d_capes.data_ptr() + lead, stride, _stream())
        torch.cuda.synchronize()
        assert np.array_equal(d_capes.cpu().numpy(), host), "the launch wrote into the image buffer"
        for i, (h, k) in enumerate(zip(handles, kinds)):
            white = np.full((64, 64, 4), 255, np.uint8)
            S.assert_blob_equal(h.blob(), CK.expected_blob(k, white, capes[i], _pose(mcrt, i % 7), 10.0 + i), f"handle {i} ({k}) of {n}")
            h.check()
        if n == 6:  # one shared cape image through a stride of 0, then no image at all
            mcrt.set_capes_batch_device(handles, d_capes.data_ptr() + lead, 0, _stream())
            torch.cuda.synchronize()
            white = np.full((64, 64, 4), 255, np.uint8)
            for i, (h, k) in enumerate(zip(handles, kinds)):
                S.assert_blob_equal(h.blob(), CK.expected_blob(k, white, capes[0], _pose(mcrt, i % 7), 10.0 + i), f"handle {i}: the shared image")
            mcrt.set_capes_batch_device(handles, 0, CAPE_BYTES, _stream())
            torch.cuda.synchronize()
            for i, (h, k) in enumerate(zip(handles, kinds)):
                S.assert_blob_equal(h.blob(), CK.expected_blob(k, white, CK.cape("transparent"), _pose(mcrt, i % 7), 10.0 + i), f"handle {i}: no image")
    finally:
        for h in handles:
            h.close()


def test_mixed_models_render_in_one_launch_sequence(mcrt, gpu, oracle):
    kinds, p, look = ["S64", "S64S", "S64S", "S64"], _pose(mcrt, 0), CK.behind(150.0)
    capes = [CK.cape("synthetic"), CK.cape("all_bytes"), CK.cape("one_hole"), CK.cape("synthetic")]
    handles = [mcrt.DeviceScene.for_skin(k, p, S.look_desc(look), cape=True) for k in kinds]
    plain = mcrt.DeviceScene.for_skin("S64", p, S.look_desc(look))
    try:
        d_skins = torch.from_numpy(np.stack([CK.skin(k) for k in kinds])).cuda()
        d_capes = torch.from_numpy(np.stack(capes)).cuda()
        mcrt.set_skins_batch_device(handles, d_skins.data_ptr(), stream=_stream())
        mcrt.set_capes_batch_device(handles, d_capes.data_ptr(), stream=_stream())
        out = torch.zeros((4, 64, 64, 4), dtype=torch.float32, device="cuda")
        mcrt.render_batch_device(handles, SMALL, out.data_ptr(), 0, 64 * 64, _stream())
        torch.cuda.synchronize()
        assert mcrt.last_batch_info() == {"batched_frames": 4, "launch_sequences": 1}
        got = out.cpu().numpy()
        for i, k in enumerate(kinds):
            _shows_the_cape(oracle, CK.reference_scene(k, CK.skin(k), capes[i], p, 10.0, look))
            scenes.assert_bit_equal(got[i], CK.oracle_frame(oracle, k, CK.skin(k), capes[i], p, 10.0, SMALL, look), f"frame {i} ({k})")
        for call in (lambda: mcrt.set_skins_batch_device(handles[:1] + [plain], d_skins.data_ptr(), stream=_stream()),
                     lambda: mcrt.set_capes_batch_device([plain], d_capes.data_ptr(), stream=_stream()),
                     lambda: mcrt.set_views_batch_device([plain, handles[0]], stream=_stream())):
            with pytest.raises(mcrt.api.McrtError, match="cape"):
                call()
    finally:
        for h in handles + [plain]:
            h.close()


# ---- views -----------------------------------------------------------------------------------------------------------------
def test_views_with_a_cape_angle(mcrt, gpu, oracle):
    kinds = ["S64", "S64S"]
    p0, p1, look = _pose(mcrt, 0), _pose(mcrt, 3), CK.behind(150.0)
    capes = [CK.cape("one_hole"), CK.cape("synthetic")]
    handles = [mcrt.DeviceScene.for_skin(k, p0, cape=True) for k in kinds]
    try:
        for h, k, c in zip(handles, kinds, capes):
            h.set_skin(CK.skin(k))
            h.set_cape(c)
        before = [h.blob() for h in handles]
        first = _render(handles[0], SMALL)  # twice: the second render may replay a recorded launch graph
        assert first.tobytes() == _render(handles[0], SMALL).tobytes()
        # the single form: pose, look and angle at once
        handles[0].set_view(p1, S.look_desc(look), cape_angle=45.0)
        got = handles[0].blob()
        S.assert_blob_equal(got, CK.expected_blob("S64", CK.skin("S64"), capes[0], p1, 45.0, look), "set_view(cape_angle=45)")
        assert got[2688:] == before[0][2688:]
        assert np.array_equal(_flags(got) & MESH_OPAQUE, _flags(before[0]) & MESH_OPAQUE) and not _flags(got)[-1] & MESH_OPAQUE
        sd = CK.reference_scene("S64", CK.skin("S64"), capes[0], p1, 45.0, look)
        _shows_the_cape(oracle, sd)
        for _ in range(2):  # a replayed launch graph is ordered after the change, and is the new view's
            scenes.assert_bit_equal(_render(handles[0], SMALL), CK.oracle_frame(oracle, "S64", CK.skin("S64"), capes[0], p1, 45.0, SMALL, look), "after the view")
        # None keeps the angle: a plain view change on a caped handle
        handles[0].set_view(p0)
        S.assert_blob_equal(handles[0].blob(), CK.expected_blob("S64", CK.skin("S64"), capes[0], p0, 45.0, look), "set_view(pose) keeps the angle")
        # the batch form, one angle per scene, classic and slim mixed
        mcrt.set_views_batch_device(handles, np.stack([p1, p1]), [S.look_desc(look)] * 2, _stream(), cape_angles=[0.005, 90.0])
        torch.cuda.synchronize()
        for h, k, c, a in zip(handles, kinds, capes, (0.005, 90.0)):
            S.assert_blob_equal(h.blob(), CK.expected_blob(k, CK.skin(k), c, p1, a, look), f"{k}: batch view at {a}")
            fresh = mcrt.DeviceScene.for_skin(k, p1, S.look_desc(look), cape=True, cape_angle=a)
            try:
                fresh.set_skin(CK.skin(k))
                fresh.set_cape(c)
                assert fresh.blob() == h.blob()
                scenes.assert_bit_equal(_render(h, SMALL), _render(fresh, SMALL), f"{k}: against a fresh handle at that view")
            finally:
                fresh.close()
            h.check()
    finally:
        for h in handles:
            h.close()


# ---- the passes on a caped figure ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def caped_figure(mcrt, gpu, oracle):
    """A repainted caped handle seen from three-quarter behind, with the layers checker's skin and the marker cape (every texel
    of a mesh its own colour, every part kept: 13 meshes in the oracle's scene too), its description, and a pass config."""
    skin, cape, p, look = layers_checker.unique_skin("S64"), CK.cape("marker"), _pose(mcrt, 3), CK.behind(150.0)
    ds = mcrt.DeviceScene.for_skin("S64", p, S.look_desc(look), cape=True)
    ds.set_skin(skin)
    ds.set_cape(cape)
    sd = CK.reference_scene("S64", skin, cape, p, 10.0, look)
    assert sd.desc.n_meshes == 13 and ds.blob() == mcrt.flatten(sd)
    _shows_the_cape(oracle, sd)
    yield ds, sd, cape, abi.Config(width=64, height=64, maxBounces=2)
    ds.close()


def _planes(spec):
    return {k: torch.zeros(shape, dtype=dtype, device="cuda") for k, (shape, dtype) in spec.items()}


def _download(t):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def test_layers_and_pick_on_a_caped_figure(mcrt, caped_figure, oracle):
    ds, sd, cape, cfg = caped_figure
    h, w = cfg.height, cfg.width
    t = _planes({"depth": ((h, w), torch.float32), "normal": ((h, w, 4), torch.float32), "albedo": ((h, w, 4), torch.float32), "id": ((h, w, 4), torch.int32)})
    ds.render_layers_device(cfg, t["depth"].data_ptr(), t["normal"].data_ptr(), t["albedo"].data_ptr(), t["id"].data_ptr(), _stream())
    got = _download(t)
    layers_checker.assert_layers_equal(got, layers_checker.expected_layers(oracle, sd, w, h), "caped layers")
    ids = got["id"]
    on_cape = np.argwhere(ids[..., 0] == 12)
    assert len(on_cape) >= 64
    rec = ds.pick(cfg, on_cape[:, ::-1].astype(np.int32))
    assert np.array_equal(np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1), ids[on_cape[:, 0], on_cape[:, 1]])
    texel = cape.astype(np.float32) / np.float32(255.0)
    for r in rec:
        assert int(r["mesh"]) == 12
        cx, cy = mcrt.cape_texel(int(r["face"]) & 7, int(r["tx"]), int(r["ty"]))
        assert r["albedo"].tobytes() == texel[cy, cx].tobytes()
    with pytest.raises(ValueError):
        mcrt.skin_texel("S64", 12, 0, 0, 0)


def test_ground_shadow_on_a_caped_figure(caped_figure, oracle):
    ds, sd, _, cfg = caped_figure
    h, w = cfg.height, cfg.width
    t = _planes({"visibility": ((h, w), torch.float32), "distance": ((h, w), torch.float32), "matte": ((h, w), torch.uint8)})
    ds.render_ground_device(cfg, 0.0, t["visibility"].data_ptr(), t["distance"].data_ptr(), t["matte"].data_ptr(), _stream())
    exp = ground_checker.expected_ground(oracle, sd, cfg, 0.0)
    ground_checker.assert_ground_equal(_download(t), exp, "caped ground shadow")
    assert (exp["visibility"] < 1).any()


def test_ground_occlusion_on_a_caped_figure(caped_figure, oracle):
    ds, sd, _, cfg = caped_figure
    h, w = cfg.height, cfg.width
    t = _planes({"occlusion": ((h, w), torch.float32), "matte": ((h, w), torch.uint8)})
    ds.render_ground_occlusion_device(cfg, 0.0, occlusion_ptr=t["occlusion"].data_ptr(), matte_ptr=t["matte"].data_ptr(), stream=_stream())
    exp = ground_occlusion_checker.expected_ground_occlusion(oracle, sd, cfg, 0.0)
    ground_occlusion_checker.assert_planes_equal(_download(t), exp, "caped ground occlusion")
    assert (exp["occlusion"] < 1).any()


def test_reflection_on_a_caped_figure(caped_figure, oracle):
    ds, sd, _, cfg = caped_figure
    h, w = cfg.height, cfg.width
    t = _planes({"rgba": ((h, w, 4), torch.float32), "rgba8": ((h, w, 4), torch.uint8), "distance": ((h, w), torch.float32)})
    ds.render_reflection_device(cfg, 0.0, t["rgba"].data_ptr(), t["rgba8"].data_ptr(), t["distance"].data_ptr(), _stream())
    exp = reflection_checker.expected_reflection(oracle, sd, cfg, 0.0)
    reflection_checker.assert_reflection_equal(_download(t), exp, "caped reflection")
    assert exp["hit"].any()


def test_light_layers_on_a_caped_figure(caped_figure, oracle):
    ds, sd, _, cfg = caped_figure
    h, w = cfg.height, cfg.width
    t = _planes({"visibility": ((h, w), torch.float32), "occlusion": ((h, w), torch.float32), "direct": ((h, w, 4), torch.float32)})
    ds.render_light_device(cfg, t["visibility"].data_ptr(), t["occlusion"].data_ptr(), t["direct"].data_ptr(), _stream())
    light_checker.assert_light_equal(_download(t), light_checker.expected_light(oracle, sd, cfg), "caped light layers")


def test_bake_on_a_caped_figure(mcrt, caped_figure, oracle):
    ds, sd, _, cfg = caped_figure
    n = ds.texels
    assert n == 3264 + 372
    t = _planes({"position": ((n, 4), torch.float32), "normal": ((n, 4), torch.float32), "visibility": ((n,), torch.float32),
                 "occlusion": ((n,), torch.float32), "direct": ((n, 4), torch.float32)})
    ds.bake_light_device(cfg, 1, t["position"].data_ptr(), t["normal"].data_ptr(), t["visibility"].data_ptr(), t["occlusion"].data_ptr(),
                         t["direct"].data_ptr(), _stream())
    got = _download(t)
    exp = bake_checker.expected_bake(oracle, sd, cfg, grid=1, blob=ds.blob())
    assert np.array_equal(exp["table"][-372:, 0], np.full(372, 12)) and np.array_equal(exp["table"][-372:, 1:], CK.pool_rows()[:, :3])
    assert np.array_equal(exp["table"], mcrt.texel_table(sd))
    bake_checker.assert_bake_equal(got, exp, "caped bake")
    image = mcrt.pool_to_cape(got["occlusion"][-372:], fill=-1.0)
    assert image.shape == (32, 64) and (image[1:17, 1:11] >= 0).all() and image[0, 0] == -1.0 and image[20, 5] == -1.0


@pytest.mark.parametrize("page", ["opaque", "cutout"])
def test_studio_shot_of_a_caped_figure(mcrt, gpu, oracle, page):
    skin, cape, p, look = layers_checker.unique_skin("S64"), CK.cape("synthetic"), _pose(mcrt, 3), CK.behind(150.0)
    cfg = abi.Config(width=64, height=64, maxBounces=2)
    sd = CK.reference_scene("S64", skin, cape, p, 10.0, look)
    _shows_the_cape(oracle, sd)
    batch = mcrt.SkinBatch(1, "S64", p, S.look_desc(look), cape=True)
    try:
        if page == "opaque":
            exp = shot_checker.expected_shot(oracle, sd, cfg, shot_checker.SHOT, 0.0)
            got = batch.shots(skin[None], cfg, shot_checker.SHOT, ground=0.0, rgba8=False, capes=[cape])
            got8 = batch.shots(skin[None], cfg, shot_checker.SHOT, ground=0.0, capes=[cape])
            shot_checker.assert_shot_equal(got[0], got8[0], exp["out"], "caped studio shot")
        else:
            shot = abi.Shot(page="transparent", reflectionFade=24.0, floorOcclusion=0.5, shadowColor=(0.125, 0.0625, 0.25))
            exp = cutout_checker.expected_shot_ex(oracle, sd, cfg, shot, 0.0)
            got, boxes = batch.shots(skin[None], cfg, shot, ground=0.0, rgba8=False, bounds=True, capes=[cape])
            shot_checker.assert_shot_equal(got[0], None, exp["out"], "caped cut-out")
            assert np.array_equal(boxes[0], exp["bounds"])
    finally:
        batch.close()


def test_two_extra_lights_on_a_caped_figure(mcrt, gpu, oracle):
    skin, cape, p, look = CK.skin("S64"), CK.cape("synthetic"), _pose(mcrt, 0), CK.behind(150.0)
    sd = CK.reference_scene("S64", skin, cape, p, 10.0, look)
    _shows_the_cape(oracle, sd)
    cfg = X.config(64, 64, 32)
    # the checker's two lights mirrored to the figure's back, where the camera is
    lights = (abi.Light((-30.0, 20.0, -30.0), (0.35, 0.4, 0.5, 1.0), 4.0), abi.Light((25.0, 5.0, -10.0), (0.9, 0.8, 0.6, 1.0), 0.0))
    want, counts = X.expected_frame(oracle, sd, cfg, lights)
    assert counts[1] >= 100  # primary hits whose colour the extra lights changed
    got = mcrt.TileRenderer.render(sd, cfg, lights=lights, device=0)
    scenes.assert_bit_equal(got, want, "two extra lights on a caped figure")
    ds = mcrt.DeviceScene.for_skin("S64", p, S.look_desc(look), cape=True)
    try:
        ds.set_skin(skin)
        ds.set_cape(cape)
        ds.set_extra_lights(lights)
        scenes.assert_bit_equal(_render(ds, cfg), want, "the same on a repainted caped handle")
    finally:
        ds.close()


# ---- the farm class --------------------------------------------------------------------------------------------------------
def test_skin_batch_with_capes(mcrt, gpu):
    cfg = abi.Config(width=64, height=64, maxBounces=2)
    p, look = _pose(mcrt, 5), CK.behind(150.0)
    models = ["classic", "slim", "slim", "classic", "classic", "slim"]
    skins = np.stack([CK.skin("S64S") if m == "slim" else S.variant(CK.skin("S64"), i) for i, m in enumerate(models)])
    capes = [CK.cape("synthetic"), None, CK.cape("one_hole"), None, CK.cape("all_bytes"), CK.cape("transparent")]
    built = [S.apply_look(mcrt.MeshBuilder.buildScene(s, p, model=m, cape=c, cape_angle=10.0), look) for s, m, c in zip(skins, models, capes)]
    assert [b.desc.n_meshes for b in built] == [13, 12, 13, 12, 13, 12]
    want = mcrt.TileRenderer.renderBatch(built, cfg)
    batch = mcrt.SkinBatch(6, "S64", p, S.look_desc(look), slim=True, cape=True)
    capeless = mcrt.SkinBatch(2, "S64", p, S.look_desc(look))
    try:
        got = batch.render(skins, cfg, models=models, capes=capes)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
        assert mcrt.last_batch_info() == {"batched_frames": 6, "launch_sequences": 1}
        bare = [S.apply_look(mcrt.MeshBuilder.buildScene(s, p, model=m), look) for s, m in zip(skins, models)]
        assert batch.render(skins, cfg, models=models).tobytes() == mcrt.TileRenderer.renderBatch(bare, cfg).tobytes()  # capes=None: none at all
        shots = batch.shots(skins, cfg, shot_checker.SHOT, ground=0.0, models=models, capes=capes)
        assert shots.tobytes() == mcrt.TileRenderer.renderShotBatch(built, cfg, shot_checker.SHOT, ground=0.0).tobytes()
        ids = batch.layers(skins, cfg, layers=("id",), models=models, capes=capes)["id"]
        assert ids.tobytes() == mcrt.TileRenderer.renderLayersBatch([_full(mcrt, s, m, c, p, look) for s, m, c in zip(skins, models, capes)], cfg, layers=("id",))["id"].tobytes()
        assert [(ids[i][..., 0] == 12).sum() >= 64 for i in range(6)] == [c is not None and c.any() for c in capes]
        batch.set_views(cape_angles=45.0)
        moved = batch.render(skins, cfg, models=models, capes=capes)
        again = [S.apply_look(mcrt.MeshBuilder.buildScene(s, p, model=m, cape=c, cape_angle=45.0), look) for s, m, c in zip(skins, models, capes)]
        assert moved.tobytes() == mcrt.TileRenderer.renderBatch(again, cfg).tobytes() and moved.tobytes() != got.tobytes()
        with pytest.raises(ValueError, match="this batch holds no capes"):
            capeless.render(skins[:2], cfg, capes=[None, None])
        with pytest.raises(ValueError, match="this batch holds no capes"):
            capeless.set_views(cape_angles=10.0)
        with pytest.raises(ValueError, match="one image"):
            batch.render(skins, cfg, models=models, capes=capes[:2])
    finally:
        batch.close()
        capeless.close()


def _full(mcrt, skin, model, cape, pose, look):
    """The full-table figure of a farm slot — what the resident scene's mesh indices mean: a part the builder would drop keeps
    its index, and the cape is mesh 12 — with the skin's and the cape's own texels."""
    kind = "S64S" if model == "slim" else "S64"
    return CK.full_table_scene(kind, skin, cape if cape is not None else CK.cape("transparent"), pose, 10.0, look)
