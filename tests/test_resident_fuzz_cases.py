"""The CPU twin of tests/test_gpu_resident_fuzz.py: what the oracle sees in the blocks of tests/resident_fuzz_cases.py, pinned, so
that the GPU blocks cannot be hollow — no device here.

Per block of 6 scripts: the same seed gives the same script; the oracle's census is the pinned one (operations by kind and form, the
reference-shaped mesh counts at render checkpoints, per mesh the states with MESH_OPAQUE set and clear, the figure pixels of every
render checkpoint, the `posed` transitions); the conditions that make the block worth running hold for the oracle alone; the
oracle's frame of the reference-shaped scene is its frame of the full-table scene at every render checkpoint (one of them also
against the reference); the view tables are the prefixes of the expected blobs; and each of five deliberately wrong models
differs from the right one at some blob checkpoint of the block — otherwise the block could not catch that defect on the device."""
import numpy as np
import pytest

import resident_fuzz_cases as RF
import scenes
import skin_paint_checker as S

FIRSTS = list(RF.BLOCKS)


@pytest.mark.parametrize("first", FIRSTS)
def test_the_same_seed_gives_the_same_script(first):
    digests = []
    for k in range(RF.BLOCK_SIZE):
        a, b = RF.make_script(first + k), RF.make_script(first + k)
        assert RF.script_digest(a) == RF.script_digest(b)
        assert 2 <= a["handles"] <= 4
        digests.append(RF.script_digest(a))
    assert len(set(digests)) == RF.BLOCK_SIZE


@pytest.mark.parametrize("first", FIRSTS)
def test_the_oracle_holds_the_blocks_census(oracle, first):
    census = RF.block_expectations(oracle, first)[2]
    print(first, census)
    assert census == RF.BLOCKS[first]


def test_the_oracle_holds_every_scripts_census(oracle):
    """What a GPU test of one script asserts before it touches the device."""
    assert list(RF.SCRIPTS) == [first + k for first in FIRSTS for k in range(RF.BLOCK_SIZE)]
    for first in FIRSTS:
        scripts, exps, _ = RF.block_expectations(oracle, first)
        for script, exp in zip(scripts, exps):
            assert RF.census_digest(script, exp) == RF.SCRIPTS[script["seed"]], script["seed"]


@pytest.mark.parametrize("first", FIRSTS)
def test_the_block_is_not_hollow(oracle, first):
    scripts, exps, c = RF.block_expectations(oracle, first)
    # each of the twelve MESH_OPAQUE bits both set and clear; a bit that differs from the view table's across a view change, in
    # each order of repaint and view
    assert all(n > 0 for n in c["opaque_set"]) and all(n > 0 for n in c["opaque_clear"])
    assert c["opaque_differs_after"]["sv"] >= 1 and c["opaque_differs_after"]["vs"] >= 1
    # the footprint grows from under a tenth of the frame to over half between two renders of one handle, and shrinks likewise,
    # each at least once under a replayed graph
    assert c["zoom"]["in"] >= 1 and c["zoom"]["out"] >= 1 and c["zoom"]["in_replayed"] >= 1 and c["zoom"]["out_replayed"] >= 1
    assert c["posed_there_and_back"] >= 1 and c["to_posed"] >= 1 and c["to_plain"] >= 1
    assert c["s32_tail_mixed"] >= 1
    assert 8 * c["empty_frames"] <= c["renders"] and c["renders"] == len(c["figure_pixels"])
    # every form of every operation, the batched passes, and a stretch of more than kTableSlots batch calls without a host wait
    for name in ("set_skin-host", "set_skin-device", "set_skin-batch", "set_view-host", "set_view-device", "set_view-batch", "set_background",
                 "render", "render-batch", "blob", "create", "close"):
        assert c["ops"].get(name, 0) >= 1, name
    assert sum(v for k, v in c["ops"].items() if k.startswith("pass-") and k.endswith("-batch")) >= 1
    longest = 0
    for s in scripts:
        run = 0
        for op in s["ops"]:
            batch_call = (op["op"] in ("set_skin", "set_view") and op["form"] == "batch") or (op["op"] in ("render", "pass") and op["batch"] and not op["wait"])
            run = run + 1 if batch_call and not op.get("sync") else 0
            longest = max(longest, run)
    assert longest > RF.table_slots()
    assert any(op["op"] == "render" and op["repeat"] == RF.record_at() + 1 for s in scripts for op in s["ops"])
    for between in ("plain", "other"):  # the pooled shell changes hands
        assert any(op["op"] == "create" and op["between"] == between for s in scripts for op in s["ops"])
    assert c["ops"].get("pass-pick", 0) >= 1 and c["ops"].get("pass-bake", 0) + c["ops"].get("pass-bake-batch", 0) >= 1


def test_the_whole_set_reaches_every_mesh_count(oracle):
    s64, s32 = set(), set()
    for first in FIRSTS:
        c = RF.block_expectations(oracle, first)[2]
        s64 |= set(c["mesh_counts"]["S64"])
        s32 |= set(c["mesh_counts"]["S32"])
    assert s64 == set(range(6, 13)) and len(s32) >= 2


@pytest.mark.parametrize("first", FIRSTS)
def test_passes_follow_their_mutations(first):
    """The header leaves the order of a pass against a mutation of its handle to the caller: same stream, or a host wait."""
    for script in RF.block_scripts(first):
        dirty = {}
        for op in script["ops"]:
            if op["op"] == "create":
                dirty[op["slot"]] = set()
            if op["op"] == "sync" or op.get("sync"):
                for d in dirty.values():
                    d.clear()
            if op["op"] in ("set_skin", "set_view") and op["form"] != "host":
                for s in op["slots"]:
                    dirty[s].add(op["stream"])
            if op["op"] == "pass":
                for s in op["slots"]:
                    assert dirty[s] <= ({op["stream"]} if op["which"] != "pick" else set()), (script["seed"], op)
            if op["op"] in ("render", "pass", "blob") and op.get("wait", True):
                for d in dirty.values():
                    d.clear()


@pytest.mark.parametrize("first", FIRSTS)
def test_dropped_parts_do_not_change_the_oracles_frame(oracle, reference, first):
    scripts, exps, _ = RF.block_expectations(oracle, first)
    e = RF.Expectations(oracle, threads=2)
    seen, against_reference = set(), None
    for exp in exps:
        for i, c, v in exp:
            if c["what"] != "frame":
                continue
            key = (e.key(c["state"]), c["cfg"], c["state"]["background"])
            if key in seen:
                continue
            seen.add(key)
            scenes.assert_bit_equal(e.full_table_frame(c["state"], c["cfg"]), v[0], f"script op {i}: the full table's frame")
            if against_reference is None and c["state"]["background"] == "reference" and v[2] < RF.N_MESHES[c["state"]["kind"]] and v[1] > 100:
                against_reference = (c, v)
    assert against_reference is not None
    c, v = against_reference
    state = c["state"]
    sd = S.reference_scene(state["skin"], state["pose"], state["look"])
    scenes.assert_bit_equal(v[0], reference.render(sd.ptr, RF.CONFIGS[c["cfg"]]), "the oracle's frame against the reference's")


@pytest.mark.parametrize("first", FIRSTS)
def test_view_tables_are_the_prefixes_of_the_expected_blobs(mcrt, first):
    views = 0
    for script in RF.block_scripts(first):
        model = RF.Model()
        for op in script["ops"]:
            model.apply(op)
            if op["op"] not in ("create", "set_view"):
                continue
            for slot in ([op["slot"]] if op["op"] == "create" else op["slots"]):
                st = model.slots[slot]
                table = mcrt.skin_view_table(st.kind, st.pose, S.look_desc(st.look))
                assert len(table) == (2496 if st.kind == "S64" else 1536)
                assert table == S.expected_blob(RF._white(st.kind), st.pose, st.look)[:len(table)], (script["seed"], op["op"], slot)
                views += 1
    assert views >= 30


@pytest.mark.parametrize("defect", list(RF.DEFECTS), ids=[f"defect{d}" for d in RF.DEFECTS])
@pytest.mark.parametrize("first", FIRSTS)
def test_a_wrong_model_differs_somewhere_in_the_block(first, defect):
    """At BLOB checkpoints: there the device's bytes are compared whole, so no differing texel or flag can hide behind the camera."""
    at_blobs = at_renders = 0
    for script in RF.block_scripts(first):
        right, wrong = RF.checkpoints(script), RF.checkpoints(script, defect)
        assert len(right) == len(wrong)
        for (i, a), (j, b) in zip(right, wrong):
            assert i == j and a["what"] == b["what"]
            if a["what"] in ("blob", "frame") and RF.blob_of(a["state"]) != RF.blob_of(b["state"]):
                at_blobs += a["what"] == "blob"
                at_renders += a["what"] == "frame"
    print(f"block {first}: {RF.DEFECTS[defect]}: the states differ at {at_blobs} blob checkpoints and under {at_renders} render checkpoints")
    assert at_blobs >= 1, RF.DEFECTS[defect]


def test_make_skin_reaches_what_the_fixed_skins_do_not(mcrt):
    g = np.random.default_rng(1)
    counts, boundary, tails = set(), 0, 0
    for k in range(120):
        kind = "S64" if k % 3 else "S32"
        skin = RF.make_skin(g, kind)
        assert skin.shape == (64 if kind == "S64" else 32, 64, 4) and skin.dtype == np.uint8
        lay = RF.layout(kind)
        alpha = skin.reshape(-1, 4)[lay["pool"], 3]
        for m in range(RF.N_MESHES[kind]):
            idx = np.flatnonzero(lay["mesh"] == m)
            zeros = alpha[idx] == 0
            boundary += int(zeros.sum() == 1 and (zeros[0] or zeros[-1]))  # one alpha-0 texel, at the mesh boundary inside a wave
        if kind == "S64":
            sd = S.reference_scene(skin, np.zeros(12, np.float32))
            counts.add(int(sd.desc.n_meshes))
        else:
            tails += int((alpha[-32:] == 0).any() and (alpha[-32:] != 0).any())
    assert counts == set(range(6, 13)) and boundary >= 100 and tails >= 10
