"""tests/bake_checker.py against the reference semantics (CPU, no device), for the skin scenes and the small box scenes of the
GPU suite:

- every sub-sample point the checker forms is sent back through the oracle's intersectMesh on its own mesh, from P + N * 0.25
  along -N: the ray must hit, the hit's normal must equal N bit for bit, and — the scenes give every texel of a mesh (the marker
  skin: every pixel) a colour of its own — its texture colour must name the texel the owner table names;
- the library's owner table (mcrt_bake_texel_table) equals the checker's and, for the full-table figures, mcrt_skin_pool_map;
- the exact counts of live, fully dark, penumbra, partly occluded and fully occluded texels of every case of the GPU suite are
  pinned (bake_checker.COUNTS), and every scene case holds texels of each of the first four classes, 30 or more in the penumbra.
  These are conditions on the inputs, measured with the oracle; they are no tolerances."""
import numpy as np
import pytest

import bake_checker as B
import layers_checker as L
import scenes
import skin_paint_checker as SP

f32 = np.float32


def _send_back(oracle, sd, exp, grid, name_texel):
    """name_texel(mesh, hit record) -> (face, tx, ty) the hit's colour names."""
    table, live = exp["table"], exp["live"]
    n_checked = 0
    for m in np.unique(table[live, 0]):
        idx = np.flatnonzero(live & (table[:, 0] == m))
        P = exp["points"][idx].reshape(-1, 3)
        N = np.repeat(exp["normals"][idx], grid * grid, axis=0)
        rays = np.concatenate([(P + N * f32(0.25)).astype(f32), (-N).astype(f32)], axis=1)
        hits = oracle.intersect_mesh(sd.ptr, int(m), rays)
        assert (hits["hit"] != 0).all(), f"mesh {m}: a sample point is not on its mesh"
        scenes.assert_bit_equal(hits["normal"], N, f"mesh {m}: normals")
        assert np.abs(hits["point"] - P).max() < 1e-4 and np.abs(hits["t"] - 0.25).max() < 1e-4
        for k in range(len(rays)):
            want = tuple(int(x) for x in table[idx[k // (grid * grid)], 1:])
            assert name_texel(int(m), hits[k]) == want, f"mesh {m}, texel {want}, sub-sample {k % (grid * grid)}"
        n_checked += len(rays)
    assert n_checked == int(live.sum()) * grid * grid
    return n_checked


@pytest.mark.parametrize("kind,pose,grid", [("S64", 0, 1), ("S64", 0, 4), ("S64", 6, 3), ("S32", 6, 2), ("S32", 1, 1)])
def test_marker_skin_points_name_their_texels(mcrt, oracle, kind, pose, grid):
    sd = mcrt.MeshBuilder.buildScene(B.marker_skin(kind), mcrt.getBuiltinPoses()[pose])
    exp = B.expected_bake(oracle, sd, B.config(), grid, planes=("position", "normal"))  # the geometry alone: no ray terms
    n = 3264 if kind == "S64" else 2016
    table = exp["table"]
    assert len(table) == n and exp["live"].all()  # opaque: every part present, every texel live
    # (mesh, skin pixel) -> the (face, tx, ty) cut from that pixel, by the builder's own tables (mcrt_skin_texel)
    by_pixel = {tuple(int(v) for v in row): mcrt.skin_texel(kind, *(int(v) for v in row)) for row in table}
    by_colour = {}
    for key, xy in by_pixel.items():
        assert (key[0], xy) not in by_colour, "two texels of one mesh are cut from one pixel: the colour cannot name the texel"
        by_colour[(key[0], xy)] = key[1:]
    checked = _send_back(oracle, sd, exp, grid, lambda m, hit: by_colour[(m, L.skin_xy_of_color(hit["texture_color"]))])
    assert checked == n * grid * grid
    # the owner table: the library's, the checker's, and the pool map of the full-table figure
    assert np.array_equal(mcrt.texel_table(sd), table)
    pmap = mcrt.skin_pool_map(kind)
    for i, row in enumerate(table):
        x, y = by_pixel[tuple(int(v) for v in row)]
        assert y * 64 + x == pmap[i], i


@pytest.mark.parametrize("name", ["two_boxes_q1", "two_boxes_q4", "null_and_empty", "posed", "seventy_boxes"])
def test_box_scene_points_name_their_texels(mcrt, oracle, name):
    sd, cfg, grid, exp = B.case_expectation(name)
    by_colour, _ = L._texel_table(sd.to_numpy())
    _send_back(oracle, sd, exp, grid, lambda m, hit: by_colour[(m, np.ascontiguousarray(hit["texture_color"], f32).tobytes())])
    assert np.array_equal(mcrt.texel_table(sd), exp["table"])


@pytest.mark.parametrize("name", list(B.CASES))
def test_case_counts_are_pinned(mcrt, name):
    sd, cfg, grid, exp = B.case_expectation(name)
    B.assert_counts(name, exp)
    B.assert_dead_constants(exp)
    assert np.array_equal(mcrt.texel_table(sd), exp["table"])


@pytest.mark.parametrize("name", list(B.MODE_CASES))
def test_mode_counts_are_pinned(name):
    sd, cfg, grid, exp = B.case_expectation(name)
    c = B.assert_counts(name, exp, classes=False)
    if name in ("soft_shadows_off", "samples_1", "radius_0"):
        assert c[2] == 0  # one ray per point: no penumbra
    if name.endswith("radius_0") and name.startswith("ao_"):
        assert c[3] == 0 and c[4] == 0 and (exp["occlusion"] == 1.0).all()
    # the cases that walk the ray loop's branches hold enough undecided points (penumbra) or traced ones (partly occluded)
    if name in ("samples_2", "samples_64", "samples_65"):
        assert c[2] == (40 if name == "samples_2" else 76)
    if name in ("ao_2", "ao_64", "ao_65"):
        assert c[3] == (12 if name == "ao_2" else 68)


def test_the_repainted_handles_scenes_hold_the_full_table(mcrt):
    for mode in ("head_only", "all_opaque"):
        sd, cfg, grid, exp = B.case_expectation("overlay_" + mode)
        assert len(exp["table"]) == 3264 and (exp["table"][:, 0] >= 0).all()
        alpha = B.overlay_skin(mode)[..., 3].reshape(-1)
        assert np.array_equal(exp["live"], alpha[mcrt.skin_pool_map("S64")] > 0)


def test_the_contact_faces_are_among_the_texels(mcrt):
    """Pose 0: the arm / body faces at x = +-4, the leg / leg faces at x = 0 and the head / torso faces at y = 24 are baked, from
    origins P + N * 1e-3 strictly inside a neighbouring opaque inner box, where every shadow ray is stopped."""
    sd, cfg, grid, exp = B.case_expectation("s64_pose0")
    live, P, N = exp["live"], exp["position"][:, :3], exp["normal"][:, :3]
    _, meshes, _ = B.parse_blob(mcrt.flatten(sd))
    inner = [m for m in range(len(meshes)) if not int(meshes[m]["flags"]) & B.MESH_OUTER]
    O = (P + N * f32(1e-3)).astype(f32)
    buried = np.zeros(len(P), bool)
    for m in inner:
        buried |= live & (exp["table"][:, 0] != m) & ((O > meshes[m]["lo"]) & (O < meshes[m]["hi"])).all(axis=1)
    print("live texels whose shadow origin lies inside another inner box:", int(buried.sum()))
    assert buried.sum() == BURIED
    assert (exp["visibility"][buried] == 0).all()  # (an AO ray is stopped only where the box ends within the radius)
    assert (exp["occlusion"][buried] == 0).sum() >= 100
    for x in (-4.0, 4.0, 0.0):
        assert (buried & (P[:, 0] == x) & (N[:, 0] != 0)).sum() >= 32, x
    assert (buried & (P[:, 1] == 24.0) & (N[:, 1] != 0)).sum() >= 32


@pytest.mark.parametrize("block", list(B.FUZZ_BLOCKS), ids=B.FUZZ_BLOCK_IDS)
def test_the_oracle_holds_the_fuzz_blocks_totals(oracle, block):
    """So that tests/test_gpu_bake_fuzz.py compares planes that hold live, penumbra and occluded texels, not constants."""
    exps = B.block_expectations(oracle, *block)
    assert len(exps) == 8
    for e in exps:
        B.assert_dead_constants(e)
    total = B.block_totals(exps)
    print(block, "texels, live, penumbra, partly occluded:", total)
    assert total == B.FUZZ_BLOCKS[block]
    assert total[1] >= 10000 and total[2] >= 1000 and total[3] >= 4000


BURIED = 694  # measured: the inner contact faces and the overlay faces that lie inside a neighbouring part
