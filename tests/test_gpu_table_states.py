"""The three per-device tables (tests/table_state_cases.py): what they hold, and that every kernel gives the same
bits whichever of them a process runs with.

Contents, in this process: the words of the window seed table and of the table of all seeds (mcrt_probe_seed_words) against
the seeding recurrence itself, at the tables' ends, at the boundaries of the launches that fill them and at random seeds.

Routes: the knobs are read once per process, so each table state runs in a child — this file as a script — which runs the
whole battery (renders with row, engine and hard shadows, with and without AO, the general variants, extra lights; boxes across
and beyond both windows' edges; fuzz cases over the whole seed range; every stand-alone pass and the shot) and records per item
the planes and what the handle holds (mcrt_scene_tables).  The parent holds every mask against the state's row, every plane bit
for bit against state "none", and state "none" against the CPU oracle and the checkers.

A captured first AO render: one more child, default knobs."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

KNOBS = ("MCRT_SEED_TABLE", "MCRT_AO_SEED_TABLE", "MCRT_SAMPLE_TABLE")
PASS_METHODS = {"ground": "render_ground_device", "ground_occlusion": "render_ground_occlusion_device", "light": "render_light_device",
                "reflection": "render_reflection_device", "bake": "bake_light_device"}


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _render(ds, cfg, stream=None):
    from minecraftskin_raytracer_amd import abi

    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream() if stream is None else stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _run_item(M, ds, it) -> dict:
    from minecraftskin_raytracer_amd import abi

    cfg = it.cfg
    if it.kind == "render":
        return {"frame": _render(ds, cfg)}
    if it.kind == "shot":
        import shot_checker as S

        need = M.shot_scratch_bytes(cfg, S.SHOT, 1)
        scratch = torch.zeros((need + 64,), dtype=torch.uint8, device="cuda")
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        out8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
        ds.render_shot_device(cfg, S.SHOT, it.middle[0], scratch.data_ptr(), need, out.data_ptr(), out8.data_ptr(), _stream())
        torch.cuda.synchronize()
        return {"f32": out.cpu().numpy(), "rgba8": out8.cpu().numpy()}
    family = abi.FAMILIES[it.family]
    shape = (ds.texels,) if it.family == "bake" else (cfg.height, cfg.width)
    dtypes = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}
    buf = {k: torch.zeros(shape + ((c,) if c > 1 else ()), dtype=dtypes[d], device="cuda") for k, (d, c) in family.formats.items()}
    getattr(ds, PASS_METHODS[it.family])(cfg, *it.middle, stream=_stream(), **{f"{k}_ptr": v.data_ptr() for k, v in buf.items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in buf.items()}


def _child_state(name, out_path):
    """The opening AO render where the state has one, on a handle that lives to the end (so that trimming the pool between
    groups frees no table); then the battery, a fresh handle per group."""
    import minecraftskin_raytracer_amd as M
    import scenes
    import table_state_cases as T

    state = T.STATES[name]
    planes, record = {}, {"masks": {}, "free_before": int(torch.cuda.mem_get_info()[0])}
    t0 = time.perf_counter()
    anchor = None
    if state.opens_with_ao:
        anchor = M.DeviceScene(scenes.skin_scene("S64", 0))
        planes["opening__frame"] = _render(anchor, T.OPENING)
        record["anchor"] = anchor.tables()
    record["device"] = M.device_tables_info()
    for g in T.battery():
        ds = M.DeviceScene(g.scene())
        if g.lights:
            ds.set_extra_lights(list(g.lights))
        record["masks"][f"{g.key}:created"] = ds.tables()
        for it in g.items:
            for k, a in _run_item(M, ds, it).items():
                planes[f"{g.key}:{it.key}__{k}"] = a
            record["masks"][f"{g.key}:{it.key}"] = ds.tables()
        ds.check()
        ds.close()
        M.trim()  # the pooled shell goes, and what it held with it: the next group's handle starts from nothing
    record["device_after"] = M.device_tables_info()
    if anchor is not None:
        anchor.check()
        anchor.close()
    record["seconds"] = time.perf_counter() - t0
    np.savez(out_path, __record__=np.frombuffer(json.dumps(record).encode(), np.uint8), **planes)


CAPTURE_CFG = dict(width=96, height=64, maxBounces=2, samplesPerPixel=4, aoEnabled=True, aoSamples=8)


def _child_capture(out_path):
    import minecraftskin_raytracer_amd as M
    import scenes
    from minecraftskin_raytracer_amd import abi

    planes, record = {}, {"free_before": int(torch.cuda.mem_get_info()[0])}
    ds = M.DeviceScene(scenes.skin_scene("S64", 6))
    ds.set_lanes(1)
    cfg = M.Config(**CAPTURE_CFG)
    planes["warm"] = _render(ds, M.Config(**dict(CAPTURE_CFG, aoEnabled=False)))  # (a capture allocates no workspace: the handle has rendered before)
    record["warm"] = {"tables": ds.tables(), "device": M.device_tables_info()}
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # the handle's first AO render, inside the caller's capture: it must neither build nor take the table
        ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
    record["captured"] = {"tables": ds.tables(), "device": M.device_tables_info()}
    g.replay()
    torch.cuda.synchronize()
    planes["replayed"] = out.cpu().numpy()
    record["replayed"] = {"tables": ds.tables(), "device": M.device_tables_info()}
    planes["plain"] = _render(ds, cfg)  # outside the capture: builds the table, the handle takes it
    record["plain"] = {"tables": ds.tables(), "device": M.device_tables_info()}
    out.zero_()
    g.replay()  # the old graph, recorded without the table
    torch.cuda.synchronize()
    planes["replayed_again"] = out.cpu().numpy()
    record["replayed_again"] = {"tables": ds.tables(), "device": M.device_tables_info()}
    ds.check()
    del g
    ds.close()
    np.savez(out_path, __record__=np.frombuffer(json.dumps(record).encode(), np.uint8), **planes)


# ---------------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _run_child(tmp, what, env_knobs):
    out = str(tmp / f"{what}.npz")
    e = dict(os.environ)
    for k in KNOBS:
        e.pop(k, None)
    e.update({k: v for k, v in env_knobs.items() if v is not None})
    t0 = time.perf_counter()
    subprocess.run([sys.executable, os.path.abspath(__file__), what, out], env=e, check=True, timeout=300)
    wall = time.perf_counter() - t0
    z = np.load(out)
    record = json.loads(z["__record__"].tobytes())
    record["wall"] = wall
    return {k: z[k] for k in z.files if k != "__record__"}, record


def _state_result(tmp_path_factory, name):
    """A state's child, run once per session (strictly one child at a time: the call returns when it has ended)."""
    import table_state_cases as T

    if name not in _RESULTS:
        _RESULTS[name] = _run_child(tmp_path_factory.mktemp(f"tables_{name}"), name, T.STATES[name].env())
        print(f"state {name}: child {_RESULTS[name][1]['wall']:.1f} s in all, {_RESULTS[name][1]['seconds']:.1f} s in the battery")
    return _RESULTS[name]


def _free_bytes():
    return int(torch.cuda.mem_get_info()[0])


def _skip_without_room(free):
    import table_state_cases as T

    if free < T.FULL_TABLE_ROOM:
        pytest.skip(f"the table of all seeds needs {T.FULL_TABLE_ROOM} bytes free, the device has {free}")


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_against_the_oracle(planes, oracle):
    """State "none" — no table at all: every item against the CPU oracle or its checker."""
    import scenes
    import shot_checker as S
    import table_state_cases as T

    for g in T.battery():
        sd = None
        for it in g.items:
            got = {k.split("__", 1)[1]: v for k, v in planes.items() if k.startswith(f"{g.key}:{it.key}__")}
            what = f"{g.key}:{it.key}"
            assert got, what
            if it.kind == "render" and g.lights:
                esd, cfg, want, _ = it.expect()
                assert cfg == it.cfg, what
                scenes.assert_bit_equal(got["frame"], want, what)
            elif it.kind == "render":
                sd = sd or g.scene()
                scenes.assert_bit_equal(got["frame"], oracle.render(sd.ptr, it.cfg), what)
            elif it.kind == "shot":
                (esd, cfg, exp), _ = it.expect()
                assert cfg == it.cfg, what
                S.assert_shot_equal(got["f32"], got["rgba8"], exp["out"], what)
            else:
                e, assert_equal = it.expect()
                assert e[1] == it.cfg and (len(e) == 3 or e[2] == it.middle[0]), what  # the checker's config (and floor) is the item's
                assert_equal(got, e[-1], what)


@pytest.mark.parametrize("name", ["none", "all", "full-only", "no-full", "no-sample"])
def test_every_route_in_a_table_state(mcrt, oracle, gpu, tmp_path_factory, name):
    """The battery in one table state: the device's figures and every handle's mask as the state's row says, every plane bit for
    bit what the state without any table gives, and that state's planes equal to the CPU oracle and the checkers."""
    import scenes
    import table_state_cases as T

    state = T.STATES[name]
    if state.full:
        _skip_without_room(_free_bytes())
    planes, record = _state_result(tmp_path_factory, name)
    if state.full and record["free_before"] < T.FULL_TABLE_ROOM:
        _skip_without_room(record["free_before"])
    # the device's figures after the opening step, and at the end
    want_device = {"window": {"bytes": T.WINDOW_BYTES if state.window and state.opens_with_ao else 0, "builds": int(state.window and state.opens_with_ao)},
                   "full": {"bytes": T.FULL_BYTES if state.full else 0, "builds": int(state.full)},
                   "sample": {"bytes": T.SAMPLE_BYTES if state.sample and state.opens_with_ao else 0, "builds": int(state.sample and state.opens_with_ao)}}
    assert record["device"] == want_device, (name, record["device"])
    if state.opens_with_ao:
        assert record["anchor"] == {"window": state.window, "full": state.full, "sample": state.sample}
    after = record["device_after"]
    assert after["full"] == want_device["full"], after  # built once, before any pass, and kept
    assert (after["window"]["bytes"] > 0) == (state.window and state.opens_with_ao) and (after["window"]["builds"] > 0) == state.window, after
    assert (after["sample"]["bytes"] > 0) == (state.sample and state.opens_with_ao) and (after["sample"]["builds"] > 0) == state.sample, after
    # what every handle held after every item
    want = T.expected_masks(state)
    got = record["masks"]
    assert sorted(k for k in got if not k.endswith(":created")) == sorted(want)
    fresh = {"window": state.window, "full": False, "sample": False}  # a handle just created holds the window table alone
    wrong = [(k, m) for k, m in got.items() if m != (fresh if k.endswith(":created") else want[k])]
    assert not wrong, f"state {name}: {len(wrong)} handle masks are not the state's; the first: {wrong[:6]}"
    # the planes
    if name == "none":
        _check_against_the_oracle(planes, oracle)
        return
    base, _ = _state_result(tmp_path_factory, "none")
    assert sorted(k for k in planes if not k.startswith("opening")) == sorted(base)
    differ = [k for k, a in base.items() if not _same_bytes(planes[k], a)]
    assert not differ, f"state {name}: {len(differ)} planes differ from the state without tables: {differ[:12]}"
    if state.opens_with_ao:
        scenes.assert_bit_equal(planes["opening__frame"], oracle.render(scenes.skin_scene("S64", 0).ptr, T.OPENING), "the opening AO render")


def test_a_captured_first_ao_render(mcrt, oracle, gpu, tmp_path_factory):
    """Default knobs.  A handle that has rendered once without AO (a capture allocates no workspace); then its first AO render,
    recorded into a caller's graph, builds nothing and takes nothing; its replay
    equals the oracle; a plain AO render then builds the table of all seeds and the handle takes it; the old graph, replayed
    again, gives the same bits."""
    import scenes
    import table_state_cases as T
    from minecraftskin_raytracer_amd import abi

    planes, record = _run_child(tmp_path_factory.mktemp("tables_capture"), "capture", {})
    print(f"capture: child {record['wall']:.1f} s")
    for when in ("warm", "captured", "replayed"):
        assert record[when]["tables"]["full"] is False, when
        assert record[when]["device"]["full"] == {"bytes": 0, "builds": 0}, when
    for when in ("plain", "replayed_again"):
        assert record[when]["tables"]["full"] is True, when
        assert record[when]["device"]["full"] == {"bytes": T.FULL_BYTES, "builds": 1}, when
    ref = oracle.render(scenes.skin_scene("S64", 6).ptr, abi.Config(**CAPTURE_CFG))
    for k in ("replayed", "plain", "replayed_again"):
        scenes.assert_bit_equal(planes[k], ref, k)
    scenes.assert_bit_equal(planes["warm"], oracle.render(scenes.skin_scene("S64", 6).ptr, abi.Config(**dict(CAPTURE_CFG, aoEnabled=False))), "warm")


# ---------------------------------------------------------------------------------------------------------------------
# contents, in this process
# ---------------------------------------------------------------------------------------------------------------------
def test_window_table_words_are_the_recurrence(mcrt, gpu):
    import table_state_cases as T

    seeds = T.window_probe_seeds()
    got = mcrt.probe_seed_words(seeds, "window")
    assert got.dtype == np.uint32 and got.shape == seeds.shape
    bad = np.flatnonzero(got != T.word397(seeds))
    assert len(bad) == 0, f"{len(bad)} words differ; first: seed {seeds[bad[0]]}: {got[bad[0]]:#x}, not {T.word397(seeds[bad[:1]])[0]:#x}"
    info = mcrt.device_tables_info()
    assert info["window"]["bytes"] == T.WINDOW_BYTES and info["window"]["builds"] >= 1
    assert info["sample"] == mcrt.sample_table_info()
    for outside in (T.SEED_HALF, -T.SEED_HALF - 1):
        with pytest.raises(ValueError):
            mcrt.probe_seed_words([outside], "window")


def test_full_table_words_are_the_recurrence(mcrt, gpu):
    """A missing table of all seeds fails the probe — but for a device with less than three times its size free."""
    import table_state_cases as T

    if mcrt.device_tables_info()["full"]["bytes"] == 0:  # (a table that exists needs no room)
        _skip_without_room(_free_bytes())
    seeds = T.full_probe_seeds()
    got = mcrt.probe_seed_words(seeds, "full")
    want = T.word397(seeds)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} words differ; first: seed {seeds[bad[0]]:#x}: {got[bad[0]]:#x}, not {want[bad[0]]:#x}"
    info = mcrt.device_tables_info()
    assert info["full"]["bytes"] == T.FULL_BYTES and info["full"]["builds"] >= 1
    # where both tables serve a seed, their words are equal
    both = seeds[T._in_window(seeds.astype(np.uint32), T.SEED_HALF)]
    signed = np.where(both >= 1 << 31, both - (1 << 32), both)
    assert len(both) >= 6 and np.array_equal(mcrt.probe_seed_words(signed, "window"), mcrt.probe_seed_words(both, "full"))


if __name__ == "__main__":
    if sys.argv[1] == "capture":
        _child_capture(sys.argv[2])
    else:
        _child_state(sys.argv[1], sys.argv[2])
