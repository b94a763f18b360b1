"""The generator of tests/big_scene_cases.py alone, on the CPU: it is deterministic; every block holds the mesh counts and texel
totals on both sides of the limits of the scene tables, under the scene views render_plan.cpp's lds_fit gives them (restated in
batch_fuzz_cases.expected_view, from the flattened header); the structures the generator promises are there, read from the
description and the flattened bounds, flags and first-pass groups; and the ORACLE's planes hold over each block what
big_scene_cases.BLOCKS says — hits on tail meshes, rotated and outer-layer ones among them, on meshes 63 and 64, on the identical
pair (which names the lower index), shadow, penumbra, occlusion, mirror images, and hits whose texel lies in the last staged alpha
word and beyond it — so that tests/test_gpu_big_scene_fuzz.py compares frames that meet these edges, not constants."""
import numpy as np
import pytest

import batch_fuzz_cases as B
import big_scene_cases as BS

MESH_APPLY, MESH_OPAQUE = 4 | 8, 32  # flat_scene.h
BLOCKS_OF = {g: [k for k in BS.BLOCKS if k[0] == g] for g in BS.GROUPS}


def _ids(keys):
    return [f"{g}-{s}" for g, s in keys]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _contains(hdr, k, j) -> bool:
    """flatten.cpp's own test: box k contains box j (float compares on the stored bounds)."""
    return bool((hdr["lo"][k] <= hdr["lo"][j]).all() and (hdr["hi"][k] >= hdr["hi"][j]).all())


@pytest.mark.parametrize("group", BS.GROUPS)
def test_cases_are_deterministic(mcrt, group):
    texts = set()
    for seed in BS.block_seeds(group, 36000)[:6]:
        (sd, cfg, g, what), (sd2, cfg2, g2, what2) = BS.make_big_case(seed, group), BS.make_big_case(seed, group)
        assert what == what2 and g == g2 and np.isfinite(np.float32(g)) and float(np.float32(g)) == g
        assert bytes(cfg.to_c()) == bytes(cfg2.to_c()) and _same(sd.to_numpy(), sd2.to_numpy())
        assert 24 <= cfg.width <= 72 and 24 <= cfg.height <= 56
        assert _same(BS.sweep_case(seed)[0].to_numpy(), sd.to_numpy())  # the sweep's case of that seed
        texts.add(what)
    assert len(texts) == 6


@pytest.mark.parametrize("block", list(BS.BLOCKS), ids=BS.BLOCK_IDS)
def test_every_block_holds_both_sides_of_the_limits_under_the_expected_views(mcrt, block):
    group, first = block
    cases = BS.block_cases(group, first)
    assert len(cases) == 12
    views = {}
    for sd, cfg, ground, what, info in cases:
        hdr = B.flat_header(sd)
        view = B.expected_view(hdr)
        if group == "texels":
            assert 2 <= hdr["n_meshes"] <= 8 and not hdr["posed"] and hdr["n_texels"] == info["total"], what
            assert hdr["alpha_words"] == (info["total"] + 15) // 16
            assert view == ("lds-unposed" if info["total"] <= 65536 else "hbm"), what
            views.setdefault(info["total"], view)
        else:
            assert hdr["n_meshes"] == info["n"] and hdr["posed"] == (group == "posed"), what
            if info["n"] <= 64:  # the count alone decides: the pool stays below 65 536 texels
                assert hdr["alpha_words"] <= B.K_ALPHA_LDS_WORDS_MAX, what
            assert view == ("hbm" if info["n"] > 64 else ("lds" if group == "posed" else "lds-unposed")), what
            views.setdefault(info["n"], view)
    if group == "count":
        assert sorted(views) == sorted(BS.COUNTS)
    elif group == "posed":
        assert sorted(views) == sorted(BS.POSED_COUNTS) and views[64] == "lds"  # at capacity
    else:
        assert {65536, 65537, 65552} <= set(views) and any(65520 <= t <= 65535 for t in views) and any(t > 80000 for t in views)
    assert {63, 64, 65} <= set(views) or group == "texels"
    # every fourth case: a general-variant config for the beauty render, a clamped one for the passes
    general = [c for c in cases if BS.is_general(c[1])]
    assert len(general) == 3
    for sd, cfg, ground, what, info in cases:
        pc = BS.pass_config(cfg)
        assert not BS.is_general(pc) and pc.shadowSamples <= 113 and pc.aoSamples <= 113 and 1 <= pc.maxBounces <= 8
        assert (pc.width, pc.height, pc.tileSize) == (cfg.width, cfg.height, cfg.tileSize)


def test_the_general_configs_have_all_three_reasons(mcrt):
    shadow = ao = bounces = deep = 0
    for group, first in BS.BLOCKS:
        for seed in BS.block_seeds(group, first):
            cfg = BS.make_big_case(seed, group)[1]
            if BS.is_general(cfg):
                shadow += 114 <= cfg.shadowSamples <= 160
                ao += bool(cfg.aoEnabled) and 114 <= cfg.aoSamples <= 140
                bounces += cfg.maxBounces in (9, 12, 17, 20)
                deep += cfg.maxBounces in (17, 20)  # beyond kMaxStack
    assert shadow >= 3 and ao >= 3 and bounces >= 3 and deep >= 1 and shadow + ao + bounces == 27


@pytest.mark.parametrize("block", BLOCKS_OF["count"], ids=_ids(BLOCKS_OF["count"]))
def test_count_scenes_hold_their_structures(mcrt, block):
    lone_roots = 0
    for sd, cfg, ground, what, info in BS.block_cases(*block):
        hdr, n, at = B.flat_header(sd), info["n"], info["index"]
        I, L, U, K = at["I"], at["L"], at["U"], at["K"]
        scene = sd.to_numpy()
        assert not any(m["hasRotation"] for m in scene["meshes"])
        # the identical pair, its container and its member
        assert hdr["lo"][L].tobytes() == hdr["lo"][U].tobytes() and hdr["hi"][L].tobytes() == hdr["hi"][U].tobytes(), what
        assert _contains(hdr, K, U) and _contains(hdr, K, L) and _contains(hdr, U, I) and not _contains(hdr, U, K), what
        for m in (L, U, K):
            assert hdr["flags"][m] & B.MESH_OUTER and not hdr["flags"][m] & MESH_OPAQUE, what  # outer layers with transparent texels
        assert max(I, L, K) < min(n, 63)
        if n > 64:
            assert U >= 64 and (U == 64) == (n == 65), what  # a member in the tail, a container in the tail, the pair astride 63 | 64
        # the first-pass groups know the first 64 meshes only: K is the root of L and I (and of U below 64)
        assert hdr["roots"] >> K & 1 and hdr["group"][K] >> L & 1 and hdr["group"][K] >> I & 1 and not hdr["roots"] >> I & 1, what
        if U < 64:
            assert hdr["group"][K] >> U & 1, what
        assert all(g >> 64 == 0 for g in hdr["group"]) and all(g == 0 for g in hdr["group"][64:])
        if n >= 64:
            assert at["F63"] == 63
        if n >= 66:
            assert at["F64"] == 64
        if n >= 70:  # the member whose only container may lie in the tail
            V, J = at["V"], at["J"]
            assert V >= 64 > J and _contains(hdr, V, J) and hdr["flags"][V] & B.MESH_OUTER and not hdr["flags"][V] & MESH_OPAQUE, what
            others = [k for k in range(64) if k != J and _contains(hdr, k, J) and not (_contains(hdr, J, k) and k > J)]
            assert bool(hdr["roots"] >> J & 1) == (not others), what
            lone_roots += not others
    assert lone_roots >= 2  # members that are roots of their own because their container is beyond the groups


@pytest.mark.parametrize("block", BLOCKS_OF["posed"], ids=_ids(BLOCKS_OF["posed"]))
def test_posed_scenes_hold_rotated_parts_in_the_tail(mcrt, block):
    below_gate = 0
    for sd, cfg, ground, what, info in BS.block_cases(*block):
        hdr, n = B.flat_header(sd), info["n"]
        rotated = [i for i in range(n) if hdr["flags"][i] & B.MESH_ROTATED and hdr["flags"][i] & MESH_APPLY]
        outer = [i for i in rotated if hdr["flags"][i] & B.MESH_OUTER]
        assert len(rotated) >= 3 and outer and len(outer) < len(rotated), what
        assert len([i for i in range(n) if not hdr["flags"][i] & B.MESH_ROTATED]) >= n - 12  # the boxes
        if n > 64:
            assert [i for i in outer if i >= 64], what
            assert len([i for i in rotated if i >= 64]) >= (2 if n > 65 else 1), what
        below_gate += any(m["hasRotation"] and (0 < abs(m["rotX"]) < 0.01 or 0 < abs(m["rotZ"]) < 0.01) for m in sd.to_numpy()["meshes"])
    assert below_gate >= 1  # angles of 0.005 degrees: rotatePoint's gate


@pytest.mark.parametrize("block", BLOCKS_OF["texels"], ids=_ids(BLOCKS_OF["texels"]))
def test_texel_scenes_put_the_last_texels_between_light_and_ground(mcrt, block):
    for sd, cfg, ground, what, info in BS.block_cases(*block):
        hdr, m = B.flat_header(sd), info["last_mesh"]
        scene = sd.to_numpy()
        assert all(hdr["tex_off"][m][f] + hdr["tex_w"][m][f] * hdr["tex_h"][m][f] == hdr["n_texels"] for f in range(6)), what
        assert hdr["flags"][m] & B.MESH_OUTER and not hdr["flags"][m] & MESH_OPAQUE, what
        assert scene["light_position"][1] > hdr["hi"][m][1] and ground <= hdr["lo"][m][1], what
        big = [(i, f) for i in range(hdr["n_meshes"]) for f in range(6) if hdr["tex_w"][i][f] * hdr["tex_h"][i][f] > 40000]
        assert big and all(hdr["flags"][i] & B.MESH_OUTER and not hdr["flags"][i] & MESH_OPAQUE for i, _ in big), what


@pytest.mark.parametrize("block", list(BS.BLOCKS), ids=BS.BLOCK_IDS)
def test_the_oracle_holds_the_blocks_census(oracle, block):
    exps = BS.check_block(oracle, *block)
    assert len(exps) == 12
