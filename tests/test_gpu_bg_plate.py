"""Background plates (include/mcrt.h, "Background plates"): the gradient background tiles of a frame configuration are
rendered once per device into a plate and copied from it afterwards.  Every frame here is compared with the CPU oracle
(the transparent one with the test-side checker of that mode), never with the library's own output alone.

The plate knobs are read once per process, so every scenario runs in a child process — this file run as a script — with
the environment it needs: MCRT_BG_PLATE=2 builds a plate at a configuration's first render, the default at its second,
0 never.  A child writes its frames and the plate store's figures (mcrt_bg_plate_info) to an .npz; the parent checks."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

# 13 x 9 tiles of 16 px, the right column and the bottom row clipped; the figure covers the middle, the corners are of one colour
BASE = dict(width=200, height=136, maxBounces=2, samplesPerPixel=4, tileSize=16)
# 7 x 5 tiles of 32 px: tile streams of 14 twists, cut into four parts (both `stream_waves` forms exist)
WIDE = dict(width=200, height=136, maxBounces=2, samplesPerPixel=4, tileSize=32)

# one handle, one key after the other: colour, scale, samples, depth of field, size and tile size each change the key
KEY_SEQUENCE = [
    ("a0", BASE),
    ("colour", dict(BASE, bgCenter=(0.2, 0.7, 0.4, 1.0), bgEdge=(0.9, 0.1, 0.3, 1.0))),
    ("a1", BASE),
    ("scale", dict(BASE, gradientScale=0.6)),
    ("spp2", dict(BASE, samplesPerPixel=2)),
    ("dof", dict(BASE, samplesPerPixel=2, dofEnabled=True, aperture=0.3)),
    ("size", dict(BASE, width=168, height=120)),
    ("tile", dict(BASE, tileSize=24)),
    ("a2", BASE),
]
# more sizes than a device keeps plates for
MANY_SIZES = [(48 + 8 * i, 40 + 4 * i) for i in range(12)]
FUZZ_SEEDS = list(range(3000, 3040))
FUZZ_SECONDS = 60.0


def make_scene(spec):
    """("pose", k): the S64 figure in built-in pose k; ("aside", k): the same seen by a camera moved to the side, so that the
    figure covers other tiles."""
    import scenes

    kind, k = spec
    sd = scenes.skin_scene("S64", k)
    if kind == "aside":
        d = sd.desc
        d.camera_position[0] += 14.0
        d.camera_target[0] += 14.0
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# the child: renders a scenario, saves frames and store figures
# ---------------------------------------------------------------------------------------------------------------------
def _child(scenario, out_path):
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi

    frames, infos = {}, {}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def render(ds, kw, first=0, step=1):
        cfg = M.Config(**kw)
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        ds.render_device(cfg, out.data_ptr(), first, step, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        return out

    if scenario == "repeat":
        ds = M.DeviceScene(make_scene(("pose", 0)))
        for i in range(3):
            frames[f"r{i}"] = render(ds, BASE).cpu().numpy()
            infos[f"r{i}"] = M.bg_plate_info()
        ds.check()
    elif scenario == "two_scenes":
        hs = {"p0": M.DeviceScene(make_scene(("pose", 0))), "p6": M.DeviceScene(make_scene(("pose", 6))),
              "side": M.DeviceScene(make_scene(("aside", 0)))}
        for rnd in range(2):
            for name, ds in hs.items():
                frames[f"{name}_{rnd}"] = render(ds, BASE).cpu().numpy()
        for ds in hs.values():
            ds.check()
        infos["end"] = M.bg_plate_info()
    elif scenario == "keys":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        for label, kw in KEY_SEQUENCE:
            frames[label] = render(ds, kw).cpu().numpy()
            infos[label] = M.bg_plate_info()
        ds.check()
    elif scenario == "variants":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        cfg = M.Config(**WIDE)
        for rnd in range(2):  # (every render call is a sighting: the default mode builds the plate at the first shard call of round 0)
            frames[f"whole_{rnd}"] = render(ds, WIDE).cpu().numpy()
            for world in (2, 3):
                out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
                for r in range(world):  # every rank's cyclic rows into the one frame
                    ds.render_device(cfg, out.data_ptr(), r, world, abi.LAYOUT_FRAME, stream())
                torch.cuda.synchronize()
                frames[f"shards{world}_{rnd}"] = out.cpu().numpy()
            out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            for r in range(3):  # packed rows, scattered by unpack_rows
                rows = ds.owned_pixel_rows(cfg, r, 3)
                packed = torch.zeros((max(rows, 1), cfg.width, 4), dtype=torch.float32, device="cuda")
                ds.render_device(cfg, packed.data_ptr(), r, 3, abi.LAYOUT_PACKED, stream())
                M.unpack_rows_device(cfg, r, 3, packed.data_ptr(), out.data_ptr(), stream())
                torch.cuda.synchronize()
            frames[f"packed_{rnd}"] = out.cpu().numpy()
            f32 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            u8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
            ds.render_device_ex(cfg, f32.data_ptr(), u8.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
            torch.cuda.synchronize()
            frames[f"ex_f32_{rnd}"] = f32.cpu().numpy()
            frames[f"ex_u8_{rnd}"] = u8.cpu().numpy()
            u8only = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
            ds.render_device_ex(cfg, 0, u8only.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
            torch.cuda.synchronize()
            frames[f"only_u8_{rnd}"] = u8only.cpu().numpy()
            for lanes in (1, 2, 3):
                ds.set_lanes(lanes)
                frames[f"lanes{lanes}_{rnd}"] = render(ds, WIDE).cpu().numpy()
            ds.set_lanes(0)
        ds.check()
        infos["end"] = M.bg_plate_info()
    elif scenario == "inflight":
        poses = (0, 2, 4, 6)
        hs = [M.DeviceScene(make_scene(("pose", k))) for k in poses]
        for ds in hs:
            ds.set_lanes(1)
        streams = [torch.cuda.Stream() for _ in hs]
        cfg = M.Config(**BASE)
        rounds = 4
        outs = [[torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda") for _ in hs] for _ in range(rounds)]
        torch.cuda.synchronize()
        for rnd in range(rounds):  # nothing waits between the rounds: four frames in flight, the plate appears among them
            for i, ds in enumerate(hs):
                ds.render_device(cfg, outs[rnd][i].data_ptr(), 0, 1, abi.LAYOUT_FRAME, streams[i].cuda_stream)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            for i, k in enumerate(poses):
                frames[f"p{k}_{rnd}"] = outs[rnd][i].cpu().numpy()
        for ds in hs:
            ds.check()
        infos["end"] = M.bg_plate_info()
    elif scenario == "fuzz":
        from fuzz_cases import make_case

        t0 = time.monotonic()
        done = []
        for seed in FUZZ_SEEDS:
            if time.monotonic() - t0 > FUZZ_SECONDS:
                break
            sd, cfg, what = make_case(seed)
            for k in range(2):
                img = M.TileRenderer.render(sd, cfg)
                assert M.TileRenderer.lastErrors() == [], what
                frames[f"s{seed}_{k}"] = img
            done.append(seed)
        infos["end"] = dict(M.bg_plate_info(), seeds=done)
    elif scenario == "never":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        for rnd in range(2):
            frames[f"flat_{rnd}"] = render(ds, dict(BASE, gradientBg=False)).cpu().numpy()
            frames[f"spp1_{rnd}"] = render(ds, dict(BASE, samplesPerPixel=1)).cpu().numpy()
            frames[f"spp13_{rnd}"] = render(ds, dict(BASE, samplesPerPixel=13)).cpu().numpy()  # the background is not rendered in plan_tiles
            ds.set_background("transparent")
            frames[f"transparent_{rnd}"] = render(ds, BASE).cpu().numpy()
            ds.set_background("reference")
            cfg = M.Config(**BASE)
            tile_frame = np.zeros((cfg.height, cfg.width, 4), np.float32)
            M.TileRenderer.renderTile((16, 0, 16, 16), make_scene(("pose", 6)), cfg, tile_frame)  # a gradient background tile on its own
            assert M.TileRenderer.lastErrors() == []
            frames[f"tile_{rnd}"] = tile_frame
        ds.check()
        infos["end"] = M.bg_plate_info()
    elif scenario == "graph":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        ds.set_lanes(1)
        cfg = M.Config(**BASE)
        frames["direct_0"] = render(ds, BASE).cpu().numpy()  # the key's first render (and the workspace allocation)
        infos["direct_0"] = M.bg_plate_info()
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # the key's second render, inside the caller's capture: it must not build
            ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        infos["captured"] = M.bg_plate_info()
        g.replay()
        torch.cuda.synchronize()
        frames["replay_0"] = out.cpu().numpy()
        out.zero_()
        frames["direct_1"] = render(ds, BASE).cpu().numpy()  # outside the capture: now the plate is built
        infos["direct_1"] = M.bg_plate_info()
        frames["direct_2"] = render(ds, BASE).cpu().numpy()
        g.replay()
        torch.cuda.synchronize()
        frames["replay_1"] = out.cpu().numpy()
        ds.check()
    elif scenario == "memory":
        ds = M.DeviceScene(make_scene(("pose", 0)))
        for rnd in range(2):
            for w, h in MANY_SIZES:
                frames[f"{w}x{h}_{rnd}"] = render(ds, dict(BASE, width=w, height=h)).cpu().numpy()
                infos[f"{w}x{h}_{rnd}"] = M.bg_plate_info()
        ds.check()
        ds.close()
        M.trim()
        infos["trimmed"] = M.bg_plate_info()
    else:
        raise SystemExit(f"unknown scenario {scenario}")
    np.savez(out_path, __infos__=np.frombuffer(json.dumps(infos).encode(), np.uint8), **frames)


def _run(tmp_path, scenario, tag, env=None, plate=None):
    out = str(tmp_path / f"{scenario}_{tag}.npz")
    e = dict(os.environ)
    e.pop("MCRT_BG_PLATE", None)
    if plate is not None:
        e["MCRT_BG_PLATE"] = str(plate)
    e.update(env or {})
    subprocess.run([sys.executable, os.path.abspath(__file__), scenario, out], env=e, check=True, timeout=600)
    z = np.load(out)
    return {k: z[k] for k in z.files if k != "__infos__"}, json.loads(z["__infos__"].tobytes())


class _OracleFrames:
    """oracle frames by (scene spec, config): each rendered once"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, spec, kw):
        from minecraftskin_raytracer_amd import abi

        key = (spec, json.dumps(kw, sort_keys=True))
        if key not in self.cache:
            sd = make_scene(spec)
            self.cache[key] = self.oracle.render(sd.ptr, abi.Config(**kw))
        return self.cache[key]


@pytest.fixture(scope="module")
def ref(oracle):
    return _OracleFrames(oracle)


def _plate_bytes(kw):
    ts = kw["tileSize"]
    return -(-kw["width"] // ts) * -(-kw["height"] // ts) * ts * ts * 16


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plate", [None, 2, 0], ids=["second_sighting", "first_use", "off"])
def test_same_handle_three_times(gpu, ref, tmp_path, plate):
    import scenes

    frames, infos = _run(tmp_path, "repeat", str(plate), plate=plate)
    for i in range(3):
        scenes.assert_bit_equal(frames[f"r{i}"], ref(("pose", 0), BASE), f"render {i}")
    builds = [infos[f"r{i}"]["builds"] for i in range(3)]
    assert builds == {None: [0, 1, 1], 2: [1, 1, 1], 0: [0, 0, 0]}[plate]
    if plate != 0:
        assert infos["r2"]["plates"] == 1 and infos["r2"]["bytes"] == _plate_bytes(BASE)


@pytest.mark.parametrize("plate", [None, 2], ids=["second_sighting", "first_use"])
def test_scenes_that_cover_different_tiles_share_a_plate(gpu, ref, tmp_path, plate):
    import scenes

    frames, infos = _run(tmp_path, "two_scenes", str(plate), plate=plate)
    specs = {"p0": ("pose", 0), "p6": ("pose", 6), "side": ("aside", 0)}
    for name, spec in specs.items():
        for rnd in range(2):
            scenes.assert_bit_equal(frames[f"{name}_{rnd}"], ref(spec, BASE), f"{name} round {rnd}")
    # the scenes do differ in the tiles the figure covers
    assert (ref(("pose", 0), BASE) != ref(("aside", 0), BASE)).any()
    assert infos["end"]["builds"] == 1 and infos["end"]["plates"] == 1


@pytest.mark.parametrize("plate", [None, 2], ids=["second_sighting", "first_use"])
def test_key_changes_on_one_handle(gpu, ref, tmp_path, plate):
    import scenes

    frames, infos = _run(tmp_path, "keys", str(plate), plate=plate)
    for label, kw in KEY_SEQUENCE:
        scenes.assert_bit_equal(frames[label], ref(("pose", 6), kw), label)
    if plate == 2:  # every change of the key is a plate of its own; a key that comes back finds its plate
        builds = [infos[label]["builds"] for label, _ in KEY_SEQUENCE]
        assert builds == [1, 2, 2, 3, 4, 5, 6, 7, 7]
    else:  # only BASE is rendered twice
        assert infos["a2"]["builds"] == 1


@pytest.mark.parametrize("env", [{}, {"MCRT_STREAM_WAVES": "1"}, {"MCRT_STREAM_WAVES": "4"}, {"MCRT_WORKSPACE_MB": "1"}],
                         ids=["default", "one_wave", "four_waves", "multi_pass"])
@pytest.mark.parametrize("plate", [None, 2], ids=["second_sighting", "first_use"])
def test_output_variants_equal_the_whole_frame(gpu, mcrt, ref, tmp_path, plate, env):
    import scenes

    frames, infos = _run(tmp_path, "variants", f"{plate}_{'_'.join(env.values())}", env=env, plate=plate)
    want = ref(("pose", 6), WIDE)
    want8 = mcrt.quantize_rgba8(want)
    for rnd in range(2):
        for name in ("whole", "shards2", "shards3", "packed", "ex_f32", "lanes1", "lanes2", "lanes3"):
            scenes.assert_bit_equal(frames[f"{name}_{rnd}"], want, f"{name} round {rnd}")
        for name in ("ex_u8", "only_u8"):
            assert np.array_equal(frames[f"{name}_{rnd}"], want8), f"{name} round {rnd}"
    assert infos["end"]["builds"] == 1 and infos["end"]["bytes"] == _plate_bytes(WIDE)  # shards, layouts and lanes share one plate


@pytest.mark.parametrize("plate", [None, 2], ids=["second_sighting", "first_use"])
def test_four_handles_in_flight(gpu, ref, tmp_path, plate):
    import scenes

    frames, infos = _run(tmp_path, "inflight", str(plate), plate=plate)
    for k in (0, 2, 4, 6):
        for rnd in range(4):
            scenes.assert_bit_equal(frames[f"p{k}_{rnd}"], ref(("pose", k), BASE), f"pose {k} round {rnd}")
    assert infos["end"]["builds"] == 1 and infos["end"]["plates"] == 1


def test_plate_on_and_off_agree_on_random_cases(gpu, oracle, tmp_path):
    import scenes
    from fuzz_cases import make_case

    on, info_on = _run(tmp_path, "fuzz", "on")
    off, info_off = _run(tmp_path, "fuzz", "off", plate=0)
    assert info_off["end"]["builds"] == 0
    seeds = sorted(set(info_on["end"]["seeds"]) & set(info_off["end"]["seeds"]))
    assert len(seeds) >= 8, (info_on["end"]["seeds"], info_off["end"]["seeds"])
    eligible = 0
    for seed in info_on["end"]["seeds"]:  # the configurations that take a plate (include/mcrt.h)
        cfg = make_case(seed)[1]
        draws = (2 if cfg.samplesPerPixel > 1 else 0) + (2 if cfg.dofEnabled and cfg.aperture > 1e-6 else 0)
        eligible += bool(cfg.gradientBg and cfg.samplesPerPixel > 1 and cfg.samplesPerPixel * draws <= 24)
    for seed in seeds:
        sd, cfg, what = make_case(seed)
        want = oracle.render(sd.ptr, cfg)
        for k in range(2):
            scenes.assert_bit_equal(on[f"s{seed}_{k}"], want, f"plate on, render {k}: {what}")
            scenes.assert_bit_equal(off[f"s{seed}_{k}"], want, f"plate off, render {k}: {what}")
    # Each case is rendered twice, so the second render of an eligible configuration builds.  `eligible` repeats the rule
    # of plan_workspace (the background is rendered in plan_tiles up to 24 draws per pixel) and leaves out the byte budget
    # and the limit of 8 plates: an upper bound of the builds — the sweep did exercise the plate
    assert eligible >= 1 and 1 <= info_on["end"]["builds"] <= eligible, (eligible, info_on["end"])


def test_ineligible_frames_never_allocate(gpu, mcrt, oracle, ref, tmp_path):
    import scenes
    import transparent_checker
    from minecraftskin_raytracer_amd import abi

    frames, infos = _run(tmp_path, "never", "first_use", plate=2)
    assert infos["end"] == {"plates": 0, "bytes": 0, "builds": 0}
    sd = make_scene(("pose", 6))
    checker = transparent_checker.Checker(transparent_checker.build(str(tmp_path)))
    transparent, _ = checker.render(sd.ptr, abi.Config(**BASE), threads=transparent_checker.threads())
    tile = np.zeros((BASE["height"], BASE["width"], 4), np.float32)
    oracle.render_tile(sd.ptr, abi.Config(**BASE), (16, 0, 16, 16), tile)
    for rnd in range(2):
        scenes.assert_bit_equal(frames[f"flat_{rnd}"], ref(("pose", 6), dict(BASE, gradientBg=False)), "flat colour")
        scenes.assert_bit_equal(frames[f"spp1_{rnd}"], ref(("pose", 6), dict(BASE, samplesPerPixel=1)), "1 spp")
        scenes.assert_bit_equal(frames[f"spp13_{rnd}"], ref(("pose", 6), dict(BASE, samplesPerPixel=13)), "13 spp")
        scenes.assert_bit_equal(frames[f"transparent_{rnd}"], transparent, "transparent")
        scenes.assert_bit_equal(frames[f"tile_{rnd}"], tile, "one tile")


def test_render_inside_a_callers_graph_takes_no_plate(gpu, ref, tmp_path):
    import scenes

    frames, infos = _run(tmp_path, "graph", "default")
    for name in ("direct_0", "replay_0", "direct_1", "direct_2", "replay_1"):
        scenes.assert_bit_equal(frames[name], ref(("pose", 6), BASE), name)
    assert infos["direct_0"]["builds"] == 0
    assert infos["captured"]["builds"] == 0  # the key's second render, but inside the capture
    assert infos["direct_1"]["builds"] == 1


def test_memory_stays_bounded_over_many_sizes(gpu, mcrt, ref, tmp_path):
    import scenes

    header = open(os.path.join(ROOT, "include", "mcrt.h")).read()
    budget = int(header.split("#define MCRT_BG_PLATE_BUDGET_MB")[1].split()[0]) << 20
    frames, infos = _run(tmp_path, "memory", "first_use", plate=2)
    for rnd in range(2):
        for w, h in MANY_SIZES:
            scenes.assert_bit_equal(frames[f"{w}x{h}_{rnd}"], ref(("pose", 0), dict(BASE, width=w, height=h)), f"{w}x{h} round {rnd}")
            info = infos[f"{w}x{h}_{rnd}"]
            assert info["plates"] <= 8 and info["bytes"] <= budget, info
    last = infos["%dx%d_1" % MANY_SIZES[-1]]
    assert last["builds"] > 8 and last["plates"] <= 8  # plates nobody holds made way
    assert infos["trimmed"]["plates"] == 0 and infos["trimmed"]["bytes"] == 0


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
