"""Capes on the host: the builder's cape mesh, its maps, the caped view tables and — through the CPU oracle — its orientation,
against the definition restated in tests/cape_checker.py."""
import numpy as np
import pytest

import cape_checker as CK
import skin_paint_checker as S

f32 = np.float32
KINDS = ("S64", "S64S", "S32")


# ---- the maps --------------------------------------------------------------------------------------------------------------
def test_cape_maps_agree_on_all_372_texels(mcrt):
    pmap, rows = mcrt.cape_pool_map(), CK.pool_rows()
    assert pmap.dtype == np.int32 and len(pmap) == 372 == len(rows) == CK.N_TEXELS
    assert np.array_equal(pmap, rows[:, 3])
    for face, tx, ty, pixel in rows:
        assert mcrt.cape_texel(face, tx, ty) == (pixel % 64, pixel // 64) == CK.texel_pixel(face, tx, ty)
    assert len(set(pmap.tolist())) == 372  # every image pixel once at most
    x, y = pmap % 64, pmap // 64
    assert x.max() == 21 and y.max() == 16 and x.min() == 0 and y.min() == 0
    assert 0 not in pmap and 21 not in pmap  # (0, 0) and (21, 0) are unused
    assert set(pmap.tolist()) == {j * 64 + i for j in range(17) for i in range(22)} - {0, 21}
    # the slots' rectangles are the unwrap's faces of the box {0, 0, 10, 16, 1}, taken crosswise
    import slim_checker as SL

    for slot, (rect, turned) in enumerate(CK.SLOT_RECTS):
        assert rect == SL.face_rect(CK.CAPE_BOX, CK.UNWRAP_FACE[slot]) and turned == (slot >= 4)


def test_cape_texel_refusals(mcrt):
    for args in ((6, 0, 0), (-1, 0, 0), (0, 10, 0), (0, 0, 16), (2, 1, 0), (4, 0, 1), (0, -1, 0)):
        with pytest.raises(mcrt.api.McrtError, match="face_slot must be 0..5|texel outside the face's region"):
            mcrt.cape_texel(*args)


def test_pool_to_cape(mcrt):
    img = mcrt.pool_to_cape(np.arange(1, 373, dtype=np.int32), fill=-5)
    assert img.shape == (32, 64) and (img != -5).sum() == 372 and img[0, 0] == -5 and img[0, 21] == -5 and (img[17:] == -5).all() and (img[:, 22:] == -5).all()
    assert img[1, 1] == 1  # the first pool texel: the outward face's (0, 0)
    planes = mcrt.pool_to_cape(np.zeros((372, 3), f32))
    assert planes.shape == (32, 64, 3)
    with pytest.raises(ValueError):
        mcrt.pool_to_cape(np.zeros(371, np.int32))


def test_synthetic_cape(mcrt):
    c = mcrt.synthetic_cape()
    assert c.shape == (32, 64, 4) and c.dtype == np.uint8 and (c[..., 3] == 255).all()
    assert np.array_equal(c, mcrt.synthetic_cape()) and not np.array_equal(c, mcrt.synthetic_cape(seed=1))


# ---- the built scene -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_no_cape_is_todays_call_byte_for_byte(mcrt, kind):
    height, model, _ = CK.KINDS[kind]
    skin, pose = CK.skin(kind), mcrt.getBuiltinPoses()[3]
    today = mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose, model=model))
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=None)) == today
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=None, cape_angle=45.0)) == today
    # a transparent cape is dropped, whatever its colours
    clear = CK.cape("synthetic").copy()
    clear[..., 3] = 0
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=clear)) == today
    # ... but for the pixels the unwrap does not read
    outside = clear.copy()
    outside[0, 0, 3] = outside[0, 21, 3] = outside[20, 5, 3] = outside[3, 22, 3] = 255
    assert mcrt.flatten(mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=outside)) == today


@pytest.mark.parametrize("angle", CK.ANGLES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_cape_is_one_more_mesh_last_and_equals_the_checker(mcrt, kind, angle):
    height, model, n_skin = CK.KINDS[kind]
    skin, cape, pose = CK.skin(kind), CK.cape("marker"), mcrt.getBuiltinPoses()[3]
    plain = mcrt.MeshBuilder.buildScene(skin, pose, model=model).to_numpy()
    d = mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=cape, cape_angle=angle).to_numpy()
    n = len(plain["meshes"])
    assert len(d["meshes"]) == n + 1 and len(d["textures"]) == len(plain["textures"]) + 6
    for a, b in zip(d["meshes"][:n], plain["meshes"]):
        assert np.asarray(a["triangles"], f32).tobytes() == np.asarray(b["triangles"], f32).tobytes() and np.array_equal(a["tri_texture"], b["tri_texture"])
    m = d["meshes"][n]
    assert not m["isOuterLayer"]
    posed = angle > 0.01
    assert bool(m["hasRotation"]) == posed
    assert np.asarray(m["triangles"], f32).reshape(-1, 3).tobytes() == CK.world_triangles(angle).tobytes()
    if posed:
        assert np.asarray(m["localTriangles"], f32).reshape(-1, 3).tobytes() == CK.local_triangles().tobytes()
        assert np.asarray(m["pivot"], f32).tolist() == list(CK.PIVOT) and (f32(m["rotX"]), f32(m["rotZ"])) == (f32(angle), f32(0.0))
    else:
        assert CK.world_triangles(angle).tobytes() == CK.local_triangles().tobytes()
    for face in range(6):
        t = int(m["tri_texture"][2 * face])
        assert t == int(m["tri_texture"][2 * face + 1]) == len(plain["textures"]) + face
        tex = d["textures"][t]
        assert (tex["width"], tex["height"]) == CK.SLOT_RECTS[face][0][2:]
        assert np.asarray(tex["pixels"], f32).tobytes() == CK.face_texels(cape, face).tobytes(), face
    # the texel table of the built figure names the cape's texels as the last mesh's, in the checker's order
    table = mcrt.texel_table(mcrt.MeshBuilder.buildScene(skin, pose, model=model, cape=cape, cape_angle=angle))
    assert np.array_equal(table[-372:, 0], np.full(372, n)) and np.array_equal(table[-372:, 1:], CK.pool_rows()[:, :3])


def test_the_box_and_the_hinge(mcrt):
    v = CK.local_triangles()
    assert (v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max(), v[:, 2].min(), v[:, 2].max()) == (-5.0, 5.0, 8.0, 24.0, -3.0, -2.0)
    w = CK.world_triangles(45.0)
    hem, top = w[np.isclose(v[:, 1], 8.0)], w[np.isclose(v[:, 1], 24.0) & np.isclose(v[:, 2], -2.0)]
    assert (hem[:, 2] < -10.0).all()  # a positive angle moves the hem towards -z, away from the legs
    assert np.array_equal(top, v[np.isclose(v[:, 1], 24.0) & np.isclose(v[:, 2], -2.0)])  # the hinge edge stays
    c, s = CK.trig(90.0)
    assert abs(float(c)) < 1e-6 and float(s) == 1.0


def test_full_table_figures_sizes(mcrt):
    for kind, (prefix, texels) in {"S64": (2688, 3264 + 372), "S64S": (2688, 3136 + 372), "S32": (1728, 2016 + 372)}.items():
        blob = CK.expected_blob(kind, CK.skin(kind), CK.cape("synthetic"), mcrt.getBuiltinPoses()[0], 10.0)
        h = CK.header(blob)
        assert h["texel_offset"] == prefix and h["n_texels"] == texels and h["n_meshes"] == CK.KINDS[kind][2] + 1
        assert (texels - 372) % 16 == 0 and h["alpha_words"] == (texels - 372) // 16 + 24 and prefix // 16 <= 192


# ---- the orientation, through the oracle -----------------------------------------------------------------------------------
def test_seen_from_behind_the_picture_reads_as_painted(mcrt, oracle):
    """Camera on the -z side looking towards +z: the viewer's left is +x.  A ray that meets the unposed cape's outward face just
    inside its +x edge and just under the hinge (below the head overlay's underside at y = 23.5) is texel (0, 0) of that face, cut from image pixel (1, 1); the far corner is
    (9, 15), from pixel (10, 16)."""
    cape = CK.cape("marker")
    sd = mcrt.MeshBuilder.buildScene(S.skin("synthetic_S64"), cape=cape, cape_angle=0.0)
    cape_mesh = sd.desc.n_meshes - 1
    rays = np.array([[4.5, 23.25, -50.0, 0.0, 0.0, 1.0], [-4.5, 8.5, -50.0, 0.0, 0.0, 1.0]], f32)
    hits = oracle.intersect(sd.ptr, rays)
    own = oracle.intersect_mesh(sd.ptr, cape_mesh, rays)
    assert (hits["hit"] != 0).all() and np.array_equal(hits["t"], own["t"]) and np.allclose(hits["point"][:, 2], -3.0)
    assert np.array_equal(hits["normal"], np.array([[0, 0, -1], [0, 0, -1]], f32))
    texel = cape.astype(f32) / f32(255.0)
    assert hits["texture_color"][0].tobytes() == texel[1, 1].tobytes() == CK.face_texels(cape, 0)[0].tobytes()
    assert hits["texture_color"][1].tobytes() == texel[16, 10].tobytes() == CK.face_texels(cape, 0)[15 * 10 + 9].tobytes()
    # and from the front, through a figure without a body in the way, the inner face: its (0, 0) is at the -x edge
    only = mcrt.MeshBuilder.buildScene(S.skin("synthetic_S64"), cape=cape, cape_angle=0.0).to_numpy()
    front = oracle.intersect_mesh(sd.ptr, cape_mesh, np.array([[-4.5, 23.25, 50.0, 0.0, 0.0, -1.0]], f32))
    assert front["hit"][0] and front["texture_color"][0].tobytes() == texel[1, 12].tobytes()
    assert len(only["meshes"]) == cape_mesh + 1


@pytest.mark.parametrize("yaw", [180.0, 150.0])
@pytest.mark.parametrize("kind,pose", [("S64", 0), ("S64S", 3), ("S32", 0)])
def test_the_looks_of_the_gpu_tests_show_the_cape(mcrt, oracle, kind, pose, yaw):
    """The cap against vacuous GPU tests, checked here: at 64x64 at least 64 pixel centres meet the cape."""
    sd = CK.reference_scene(kind, CK.skin(kind), CK.cape("synthetic"), mcrt.getBuiltinPoses()[pose], 10.0, CK.behind(yaw))
    assert CK.cape_pixels(oracle, sd, 64, 64) >= 64


# ---- the view tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pose,look,angle", [(0, None, 10.0), (3, "look", 45.0), (6, "look", 0.005), (1, None, 90.0)])
def test_caped_view_table_is_the_prefix_of_the_white_caped_figure(mcrt, kind, pose, look, angle):
    height, model, _ = CK.KINDS[kind]
    p, lk = mcrt.getBuiltinPoses()[pose], S.LOOK if look else None
    table = mcrt.skin_view_table(kind, p, S.look_desc(lk), cape_angle=angle)
    white, white_cape = np.full((height, 64, 4), 255, np.uint8), np.full((32, 64, 4), 255, np.uint8)
    sd = S.apply_look(mcrt.MeshBuilder.buildScene(white, p, model=model, cape=white_cape, cape_angle=angle), lk)
    blob = mcrt.flatten(sd)
    size = 1728 if kind == "S32" else 2688
    assert len(table) == size == CK.header(blob)["texel_offset"]
    assert table == blob[:size]
    # without cape_angle: today's bytes
    plain = mcrt.skin_view_table(kind, p, S.look_desc(lk))
    assert len(plain) == size - 192 and plain == mcrt.flatten(S.apply_look(mcrt.MeshBuilder.buildScene(white, p, model=model), lk))[:size - 192]


def test_refusals_of_the_python_layer(mcrt):
    skin, cape = S.skin("synthetic_S64"), CK.cape("synthetic")
    for bad in (np.zeros((64, 64, 4), np.uint8), np.zeros((32, 64, 3), np.uint8), np.zeros((34, 128, 4), np.uint8)):
        with pytest.raises(ValueError, match="a cape image is"):
            mcrt.MeshBuilder.buildScene(skin, cape=bad)
    for angle in (-0.5, 90.5, float("nan"), float("inf")):
        with pytest.raises(mcrt.api.McrtError, match="cape_angle must be within 0 .. 90 degrees"):
            mcrt.MeshBuilder.buildScene(skin, cape=cape, cape_angle=angle)
        with pytest.raises(ValueError, match="cape_angle must be within 0 .. 90 degrees"):
            mcrt.skin_view_table("S64", cape_angle=angle)
    with pytest.raises(ValueError):
        mcrt.MeshBuilder.buildScene(S.skin("synthetic_S32"), model="slim", cape=cape)
