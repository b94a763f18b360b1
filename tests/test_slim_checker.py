"""The slim player model on the host: the pool map, the built scene, the view table, the detection rule and — through the CPU
oracle — the geometry, against the tables restated in tests/slim_checker.py."""
import numpy as np
import pytest

import layers_checker
import skin_paint_checker as S
import slim_checker as SL

f32 = np.float32


# ---- the pool map ----------------------------------------------------------------------------------------------------------
def test_slim_pool_map_follows_the_slim_rectangles(mcrt):
    pmap = mcrt.skin_pool_map("S64S")
    rows = SL.pool_rows("slim")
    assert pmap.dtype == np.int32 and len(pmap) == 3136 == len(rows) == SL.N_TEXELS["slim"]
    assert np.array_equal(pmap, rows[:, 4])
    assert np.array_equal(mcrt.skin_pool_map("slim"), pmap)
    for mesh, face, tx, ty, pixel in rows[::7]:
        assert mcrt.skin_texel("S64S", mesh, face, tx, ty) == (pixel % 64, pixel // 64)
    # a bijection onto exactly the pixels of the slim rectangles
    want = set()
    for box in SL.SLIM_BOXES:
        for face in range(6):
            x, y, w, h = SL.face_rect(box, face)
            want |= {(y + j) * 64 + x + i for j in range(h) for i in range(w)}
    assert len(set(pmap.tolist())) == len(pmap) and set(pmap.tolist()) == want
    unread = set(mcrt.skin_pool_map("S64").tolist()) - want
    assert len(unread) == 128 and {y * 64 + x for x, y in SL.detection_pixels()} < unread
    assert np.array_equal(np.flatnonzero(mcrt.skins.slim_unused_mask().reshape(-1)), sorted(unread))


def test_slim_pool_map_equals_classic_off_the_arms(mcrt):
    slim, classic = SL.pool_rows("slim"), SL.pool_rows("classic")
    assert np.array_equal(mcrt.skin_pool_map("S64"), classic[:, 4])
    for mesh in range(12):
        a, b = mcrt.skin_pool_map("S64S")[slim[:, 0] == mesh], mcrt.skin_pool_map("S64")[classic[:, 0] == mesh]
        if mesh in SL.ARM_MESHES:
            assert len(a) == len(b) - 32 and set(a.tolist()) < set(b.tolist())
        else:
            assert np.array_equal(a, b)


def test_slim_pool_map_agrees_with_the_texel_table_of_the_built_figure(mcrt):
    sd = mcrt.MeshBuilder.buildScene(np.full((64, 64, 4), 255, np.uint8), model="slim")
    table = mcrt.texel_table(sd)
    assert np.array_equal(table, SL.pool_rows("slim")[:, :4])


def test_pool_to_skin_leaves_the_unread_pixels_at_fill(mcrt):
    values = np.arange(1, 3137, dtype=np.int32)
    img = mcrt.pool_to_skin("S64S", values, fill=-5)
    assert img.shape == (64, 64)
    for x, y in SL.detection_pixels():
        assert img[y, x] == -5
    assert (img[mcrt.skins.slim_unused_mask()] == -5).all() and (img != -5).sum() == 3136
    with pytest.raises(ValueError):
        mcrt.pool_to_skin("S64S", np.zeros(3264, np.int32))


# ---- the built scene -------------------------------------------------------------------------------------------------------
def test_slim_scene_of_a_marker_skin(mcrt):
    skin = SL.skin("marker")
    slim = mcrt.MeshBuilder.buildScene(skin, model="slim").to_numpy()
    classic = mcrt.MeshBuilder.buildScene(skin).to_numpy()
    assert len(slim["meshes"]) == 12 == len(classic["meshes"]) and len(slim["textures"]) == 72
    texel = skin.astype(f32) / f32(255.0)
    for m in range(12):
        ms, mc = slim["meshes"][m], classic["meshes"][m]
        for face in range(6):
            ts, tc = slim["textures"][6 * m + face], classic["textures"][6 * m + face]
            x, y, w, h = SL.face_rect(SL.SLIM_BOXES[m], face)
            assert (ts["width"], ts["height"]) == (w, h)
            assert np.asarray(ts["pixels"], f32).tobytes() == texel[y:y + h, x:x + w].tobytes(), (m, face)
            if m not in SL.ARM_MESHES:
                assert (ts["width"], ts["height"]) == (tc["width"], tc["height"]) and np.asarray(ts["pixels"]).tobytes() == np.asarray(tc["pixels"]).tobytes()
        v = np.asarray(ms["triangles"], f32).reshape(-1, 3)
        if m in SL.ARM_MESHES:
            assert [slim["textures"][6 * m + f]["width"] for f in range(6)] == [3, 3, 4, 4, 3, 3]
            grow = f32(0.5) if m % 2 else f32(0.0)
            lo, hi = (f32(-7.0) - grow, f32(-4.0) + grow) if m < 6 else (f32(4.0) - grow, f32(7.0) + grow)
            assert (v[:, 0].min(), v[:, 0].max()) == (lo, hi)
            assert (v[:, 1].min(), v[:, 1].max()) == (f32(12.0) - grow, f32(24.0) + grow) and (v[:, 2].min(), v[:, 2].max()) == (f32(-2.0) - grow, f32(2.0) + grow)
        else:
            assert v.tobytes() == np.asarray(mc["triangles"], f32).tobytes()
            assert np.array_equal(ms["tri_texture"], mc["tri_texture"]) and ms["isOuterLayer"] == mc["isOuterLayer"]
    hdr = SL.header(mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, model="slim")))
    assert hdr["n_meshes"] == 12 and hdr["n_texels"] == 3136 and hdr["alpha_words"] == 196 and hdr["texel_offset"] == 2496
    assert hdr["alpha_offset"] == 2496 + 3136 * 16 and hdr["blob_bytes"] == hdr["alpha_offset"] + 196 * 4


def test_a_posed_slim_arm_turns_about_its_own_axis(mcrt):
    pose = mcrt.getBuiltinPoses()[3]  # waving: the right arm at rotX -140, rotZ -20
    d = mcrt.MeshBuilder.buildScene(SL.skin("all_opaque"), pose, model="slim").to_numpy()
    arm = d["meshes"][4]
    assert arm["hasRotation"] and np.asarray(arm["pivot"], f32).tolist() == [-5.5, 24.0, 0.0]
    assert (float(arm["rotX"]), float(arm["rotZ"])) == (-140.0, -20.0)
    local = np.asarray(arm["localTriangles"], f32).reshape(-1, 3)
    assert (local[:, 0].min(), local[:, 0].max()) == (-7.0, -4.0)


def test_a_fully_transparent_slim_outer_part_is_dropped(mcrt):
    d = mcrt.MeshBuilder.buildScene(SL.skin("overlays_cleared"), model="slim").to_numpy()
    assert len(d["meshes"]) == 6 and not any(m["isOuterLayer"] for m in d["meshes"])
    # a skin whose arm overlay is painted in the column a slim unwrap does not read alone: classic keeps the part, slim drops it
    skin = SL.skin("overlays_cleared").copy()
    skin[40, 55] = (9, 9, 9, 255)  # the right arm's outer layer: the back face's fourth column
    assert len(mcrt.MeshBuilder.buildScene(skin).to_numpy()["meshes"]) == 7
    assert len(mcrt.MeshBuilder.buildScene(skin, model="slim").to_numpy()["meshes"]) == 6


def test_build_scene_model_argument(mcrt):
    slim, classic = SL.skin("synthetic"), S.skin("synthetic_S64")
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(slim, model="auto")) == mcrt.flatten(mcrt.MeshBuilder.buildScene(slim, model="slim"))
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(classic, model="auto")) == mcrt.flatten(mcrt.MeshBuilder.buildScene(classic))
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(slim, model="slim")) != mcrt.flatten(mcrt.MeshBuilder.buildScene(slim))
    with pytest.raises(ValueError):
        mcrt.MeshBuilder.buildScene(S.skin("synthetic_S32"), model="slim")
    with pytest.raises(ValueError):
        mcrt.MeshBuilder.buildScene(slim, model="alex")
    for kind in ("S64S", "slim"):
        with pytest.raises(ValueError):
            mcrt.skin_texel(kind, 4, 1, 3, 0)
    with pytest.raises(ValueError):
        mcrt.skin_pool_map("S32S")


# ---- the view table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose,look", [(0, None), (3, "look"), (6, "look")])
def test_slim_view_table_is_the_prefix_of_the_white_figure(mcrt, pose, look):
    p, lk = mcrt.getBuiltinPoses()[pose], S.LOOK if look else None
    table = mcrt.skin_view_table("S64S", p, S.look_desc(lk))
    white = np.full((64, 64, 4), 255, np.uint8)
    blob = SL.expected_blob(white, p, lk)
    assert len(table) == 2496 == SL.header(blob)["texel_offset"]
    assert table == blob[:2496]
    assert table != mcrt.skin_view_table("S64", p, S.look_desc(lk))


# ---- detection -------------------------------------------------------------------------------------------------------------
def test_skin_model_detection(mcrt):
    slim = mcrt.synthetic_skin("S64S")
    assert mcrt.skin_model(slim) == "slim"
    assert mcrt.skin_model(mcrt.synthetic_skin("S64")) == "classic" and mcrt.skin_model(mcrt.synthetic_skin("S32")) == "classic"
    assert len(SL.detection_pixels()) == 64 and (slim[tuple(zip(*[(y, x) for x, y in SL.detection_pixels()]))][:, 3] == 0).all()
    for rx, ry, w, h in SL.DETECTION_RECTS:  # one pixel per rectangle, its far corner
        one = slim.copy()
        one[ry + h - 1, rx + w - 1, 3] = 1
        assert mcrt.skin_model(one) == "classic"
    other = slim.copy()  # pixels the rule does not look at: the outer arms' unread columns
    other[mcrt.skins.slim_unused_mask() & (np.arange(64)[:, None] >= 32) & (np.arange(64)[None, :] >= 48), 3] = 255
    assert mcrt.skin_model(other) == "slim"
    with pytest.raises(ValueError):
        mcrt.skin_model(np.zeros((48, 64, 4), np.uint8))


def test_synthetic_skins(mcrt):
    s64, slim = mcrt.synthetic_skin("S64"), mcrt.synthetic_skin("S64S")
    mask = mcrt.skins.slim_unused_mask()
    assert mask.sum() == 128 and (slim[mask, 3] == 0).all() and (s64[mask, 3] != 0).any()
    assert np.array_equal(slim[..., :3], s64[..., :3]) and np.array_equal(slim[~mask], s64[~mask])
    with pytest.raises(ValueError):
        mcrt.synthetic_skin("S32S")


# ---- the geometry, through the oracle ---------------------------------------------------------------------------------------
def test_oracle_rays_beside_a_slim_arm_miss_it(mcrt, oracle):
    """The standing figure at 128x128, overlays cleared (inner meshes alone: 2 and 3 are the arms).  Pixel-centre rays that pass
    the arms' front plane z = 2 at 7 < |x| < 8, at arm height, hit the classic arm (x to +-8) and miss the slim one (x to +-7)."""
    skin = SL.skin("overlays_cleared")
    seen = {}
    for model in ("classic", "slim"):
        sd = mcrt.MeshBuilder.buildScene(skin, model=model)
        rays = layers_checker.pixel_rays(oracle, sd.ptr, 128, 128).astype(np.float64)
        t = (2.0 - rays[:, 2]) / rays[:, 5]
        x, y = rays[:, 0] + t * rays[:, 3], rays[:, 1] + t * rays[:, 4]
        beside = (np.abs(x) > 7.1) & (np.abs(x) < 7.9) & (y > 12.5) & (y < 23.5)
        on_arm = (np.abs(x) > 4.1) & (np.abs(x) < 6.9) & (y > 12.5) & (y < 23.5)
        assert beside.sum() >= 40 and (x[beside] > 0).any() and (x[beside] < 0).any()
        mesh = layers_checker.expected_surfaces(oracle, sd, 128, 128)["mesh"].reshape(-1)
        seen[model] = mesh[beside]
        assert np.isin(mesh[on_arm], (2, 3)).all()
    assert np.isin(seen["classic"], (2, 3)).all()
    assert (seen["slim"] == -1).all()
