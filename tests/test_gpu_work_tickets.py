"""Work lists by ticket: in `primary` and `lit` a workgroup's first item is its own index and every later one
is claimed from an atomic counter that, like the other pass counters, is never cleared and runs on from render to render.
What can go wrong is a wrong frame (an item taken twice or never, a counter base that does not follow) or a kernel that
never ends; parity is bit-exact, on the uint32 views of the float frames, against the CPU oracle (the transparent frames
against the test-side checker of that mode).

The knobs (MCRT_WORK_TICKETS, the grid sizes) are read once per process, so every scenario runs in a child process — this
file run as a script — with the environment it needs; the child writes its frames to an .npz and the parent checks.  Grids
of 1, 2 or 3 workgroups make a workgroup claim nearly the whole list; 4096 covers the list, so no ticket is taken.

The base shape is 250 x 180 at 4 spp, 4 bounces and tile 32: 8 x 6 tiles, the right column 26 px and the bottom row 20 px."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

BASE = dict(width=250, height=180, maxBounces=4, samplesPerPixel=4, tileSize=32)
SMALL = dict(width=64, height=48, maxBounces=4, samplesPerPixel=4, tileSize=32)
ROOM = dict(width=64, height=48, maxBounces=8, samplesPerPixel=1, tileSize=16)
# the shard (first, step) of BASE that owns the bottom tile row alone, pixel rows 160 .. 179: the figure ends at row 150, no
# mesh bound reaches the row — a render of it has no unit, `lit`'s list is empty and every tile is background, on the very
# handle (and counters) that renders the figure; a whole frame of that kind is the `away` scene's, on a handle of its own
EMPTY_SHARD = (5, 6)
EMPTY_ROWS = slice(160, 180)
GRID3 = {"MCRT_SHARED_GRIDS": "1", "MCRT_PRIMARY_GRID": "3", "MCRT_LIT_GRID": "3"}
BACKGROUNDS = [("gradient", "reference", BASE), ("flat", "reference", dict(BASE, gradientBg=False)), ("transparent", "transparent", BASE),
               ("spp1", "reference", dict(BASE, samplesPerPixel=1))]
BATCH_POSES = (0, 3, 6)
FLIGHT_POSES = (0, 2, 4, 6)


def make_scene(spec):
    import scenes

    kind, k = spec
    if kind == "room":  # test_gpu_parity.py, test_closed_room_fills_every_chain_to_the_last_level: every chain runs to maxBounces
        import minecraftskin_raytracer_amd as M

        wall = scenes.solid((0.7, 0.75, 0.8, 1.0))
        room = scenes.build_box(wall, (0, 18, 0), (60, 40, 60))
        a = scenes.build_box(scenes.solid((0.9, 0.2, 0.2, 1.0)), (-5, 8, -6), (8, 16, 8))
        b = scenes.build_box(scenes.solid((0.2, 0.8, 0.3, 1.0)), (7, 5, 2), (6, 10, 6))
        return M.SceneDesc(scenes.simple_scene([room, a, b], light=(3, 34, 5), cam_pos=(2, 16, 24), cam_target=(0, 12, 0), radius=2.0))
    sd = scenes.skin_scene("S64", k)
    if kind == "away":  # the camera moved far to the side: nothing but background
        d = sd.desc
        d.camera_position[0] += 500.0
        d.camera_target[0] += 500.0
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# the child: renders a scenario into device buffers, saves the frames
# ---------------------------------------------------------------------------------------------------------------------
def _child(scenario, out_path):
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi

    frames = {}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def buffer(cfg, n=None):
        shape = (cfg.height, cfg.width, 4) if n is None else (n, cfg.height, cfg.width, 4)
        return torch.zeros(shape, dtype=torch.float32, device="cuda")

    def render(ds, kw, first=0, step=1):
        cfg = M.Config(**kw)
        out = buffer(cfg)
        ds.render_device(cfg, out.data_ptr(), first, step, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    if scenario == "figure":  # the first render twists in `plan_tiles`, the second builds the plates, the third reads them
        ds = M.DeviceScene(make_scene(("pose", 6)))
        for k in range(3):
            frames[f"r{k}"] = render(ds, BASE)
        ds.check()
    elif scenario == "sequence":  # ONE handle, one set of counters: empty, empty, figure, empty; then the same inside a caller's graph
        ds = M.DeviceScene(make_scene(("pose", 6)))
        ds.set_lanes(1)
        order = [("empty0", EMPTY_SHARD), ("empty1", EMPTY_SHARD), ("figure", (0, 1)), ("empty2", EMPTY_SHARD)]
        for name, (first, step) in order:
            frames[name] = render(ds, BASE, first, step)
        ds.check()
        cfg = M.Config(**BASE)
        outs = {name: buffer(cfg) for name, _ in order}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for name, (first, step) in order:
                ds.render_device(cfg, outs[name].data_ptr(), first, step, abi.LAYOUT_FRAME, stream())
        for rep in range(3):
            for o in outs.values():
                o.zero_()
            g.replay()
            torch.cuda.synchronize()
            for name, o in outs.items():
                frames[f"replay{rep}_{name}"] = o.cpu().numpy()
        frames["after"] = render(ds, BASE)
        ds.check()
        # the camera turned away: a whole frame without any unit, on a handle of its own (a handle holds one scene) — computed in
        # `plan_tiles`, then with the plates built, then copied; the figure's handle renders between them
        away = M.DeviceScene(make_scene(("away", 6)))
        away.set_lanes(1)
        for k in range(3):
            frames[f"away{k}"] = render(away, BASE)
            frames[f"beside{k}"] = render(ds, BASE)
        away.check()
        ds.check()
    elif scenario == "room":
        ds = M.DeviceScene(make_scene(("room", 0)))
        for k in range(2):
            frames[f"r{k}"] = render(ds, ROOM)
        ds.check()
    elif scenario == "backgrounds":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        for k in range(3):
            for name, mode, kw in BACKGROUNDS:
                ds.set_background(mode)
                cfg = M.Config(**kw)
                out = buffer(cfg)
                out8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
                ds.render_device_ex(cfg, out.data_ptr(), out8.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
                torch.cuda.synchronize()
                frames[f"{name}_{k}"] = out.cpu().numpy()
                frames[f"{name}8_{k}"] = out8.cpu().numpy()
        ds.check()
    elif scenario == "variants":
        ds = M.DeviceScene(make_scene(("pose", 6)))
        cfg = M.Config(**BASE)
        for rnd in range(2):
            frames[f"whole_{rnd}"] = render(ds, BASE)
            out = buffer(cfg)
            for r in range(3):  # packed rows of the shards (0,3), (1,3), (2,3), scattered by unpack_rows
                rows = ds.owned_pixel_rows(cfg, r, 3)
                packed = torch.zeros((max(rows, 1), cfg.width, 4), dtype=torch.float32, device="cuda")
                ds.render_device(cfg, packed.data_ptr(), r, 3, abi.LAYOUT_PACKED, stream())
                M.unpack_rows_device(cfg, r, 3, packed.data_ptr(), out.data_ptr(), stream())
                torch.cuda.synchronize()
            frames[f"packed_{rnd}"] = out.cpu().numpy()
            out = buffer(cfg)
            for r in range(2):  # plain shards into one frame
                ds.render_device(cfg, out.data_ptr(), r, 2, abi.LAYOUT_FRAME, stream())
            torch.cuda.synchronize()
            frames[f"shards_{rnd}"] = out.cpu().numpy()
            ds.set_lanes(3)
            frames[f"lanes3_{rnd}"] = render(ds, BASE)
            ds.set_lanes(0)
        ds.check()
    elif scenario == "inflight":
        hs = [M.DeviceScene(make_scene(("pose", k))) for k in FLIGHT_POSES]
        for ds in hs:
            ds.set_lanes(1)
        streams = [torch.cuda.Stream() for _ in hs]
        cfg = M.Config(**BASE)
        rounds = 3
        outs = [[buffer(cfg) for _ in hs] for _ in range(rounds)]
        torch.cuda.synchronize()
        for rnd in range(rounds):  # nothing waits between the rounds
            for i, ds in enumerate(hs):
                ds.render_device(cfg, outs[rnd][i].data_ptr(), 0, 1, abi.LAYOUT_FRAME, streams[i].cuda_stream)
        torch.cuda.synchronize()
        for rnd in range(rounds):
            for i, k in enumerate(FLIGHT_POSES):
                frames[f"p{k}_{rnd}"] = outs[rnd][i].cpu().numpy()
        for ds in hs:
            ds.check()
    elif scenario == "batch":
        hs = [M.DeviceScene(make_scene(("pose", k))) for k in BATCH_POSES]
        cfg = M.Config(**SMALL)
        for call in range(3):
            out = buffer(cfg, len(hs))
            M.render_batch_device(hs, cfg, out.data_ptr(), 0, None, stream())
            torch.cuda.synchronize()
            for i, k in enumerate(BATCH_POSES):
                frames[f"batch{call}_p{k}"] = out[i].cpu().numpy()
        assert M.last_batch_info() == {"batched_frames": len(hs), "launch_sequences": 1}
        for k, ds in zip(BATCH_POSES, hs):
            frames[f"single_p{k}"] = render(ds, SMALL)
            ds.check()
    else:
        raise SystemExit(f"unknown scenario {scenario}")
    np.savez(out_path, **frames)


def _run(tmp_path, scenario, tag, env):
    out = str(tmp_path / f"{scenario}_{tag}.npz")
    e = dict(os.environ)
    for knob in ("MCRT_WORK_TICKETS", "MCRT_SHARED_GRIDS", "MCRT_PRIMARY_GRID", "MCRT_LIT_GRID", "MCRT_QUEUE_GRID", "MCRT_BG_PLATE", "MCRT_DRAW_PLATE",
                 "MCRT_WORKSPACE_MB"):
        e.pop(knob, None)
    e.update(env)
    subprocess.run([sys.executable, os.path.abspath(__file__), scenario, out], env=e, check=True, timeout=300)
    z = np.load(out)
    return {k: z[k] for k in z.files}


class _OracleFrames:
    """oracle frames by (scene spec, config): each rendered once"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, spec, kw):
        from minecraftskin_raytracer_amd import abi

        key = (spec, json.dumps(kw, sort_keys=True))
        if key not in self.cache:
            self.cache[key] = self.oracle.render(make_scene(spec).ptr, abi.Config(**kw))
        return self.cache[key]


@pytest.fixture(scope="module")
def ref(oracle):
    return _OracleFrames(oracle)


def _grids(n):
    return {"MCRT_SHARED_GRIDS": "1", "MCRT_PRIMARY_GRID": str(n), "MCRT_LIT_GRID": str(n)}


# ---------------------------------------------------------------------------------------------------------------------
def test_many_tickets_per_workgroup(gpu, ref, tmp_path):
    """Three workgroups share the lists; one workgroup claims a whole list and must stop; 4096 take no ticket; the static
    stride.  All the same frame, the oracle's."""
    import scenes

    want = ref(("pose", 6), BASE)
    runs = {"grid3": _grids(3), "grid1": _grids(1), "grid4096": _grids(4096), "static3": dict(_grids(3), MCRT_WORK_TICKETS="0")}
    got = {name: _run(tmp_path, "figure", name, env) for name, env in runs.items()}
    for name, frames in got.items():
        for k in range(3):
            scenes.assert_bit_equal(frames[f"r{k}"], got["grid4096"][f"r{k}"], f"{name} against 4096 workgroups, render {k}")
            scenes.assert_bit_equal(frames[f"r{k}"], want, f"{name}, render {k}")


@pytest.mark.parametrize("env", [GRID3, {"MCRT_SHARED_GRIDS": "1"}], ids=["grid3", "shared_default"])
def test_counters_run_on_across_empty_frames_and_graph_replays(gpu, ref, tmp_path, env):
    """The ticket words are never cleared: a render without any unit (`lit`'s list is empty, `primary` has nothing to claim)
    leaves them where they were, twice; the figure's render moves them; the empty render follows; the same four renders
    recorded into a caller's graph are replayed three times, and a plain render follows those."""
    import scenes

    want = ref(("pose", 6), BASE)
    assert scenes.same_bytes(want[EMPTY_ROWS], ref(("away", 6), BASE)[EMPTY_ROWS])  # the shard's rows do show the background alone
    assert not scenes.same_bytes(want, ref(("away", 6), BASE))
    frames = _run(tmp_path, "sequence", "_".join(env.values()), env)
    for prefix in ("", "replay0_", "replay1_", "replay2_"):
        scenes.assert_bit_equal(frames[f"{prefix}figure"], want, f"{prefix}figure")
        for name in ("empty0", "empty1", "empty2"):
            f = frames[f"{prefix}{name}"]
            scenes.assert_bit_equal(f[EMPTY_ROWS], want[EMPTY_ROWS], f"{prefix}{name}")
            assert not f[:EMPTY_ROWS.start].any(), f"{prefix}{name} wrote rows it does not own"
    scenes.assert_bit_equal(frames["after"], want, "the render after the replays")
    for k in range(3):
        scenes.assert_bit_equal(frames[f"away{k}"], ref(("away", 6), BASE), f"the camera turned away, render {k}")
        scenes.assert_bit_equal(frames[f"beside{k}"], want, f"the figure beside it, render {k}")


def test_chase_and_dense_blocks_under_tickets(gpu, ref, tmp_path):
    """The closed room at 64 x 48, 1 spp, 8 bounces: 12 chase blocks, 12 units and 12 dense blocks in `lit`'s list, every chase
    region filled to its last slot — on two workgroups, by ticket and by stride."""
    import scenes

    want = ref(("room", 0), ROOM)
    for name, env in (("tickets", {"MCRT_LIT_GRID": "2"}), ("static", {"MCRT_LIT_GRID": "2", "MCRT_WORK_TICKETS": "0"})):
        frames = _run(tmp_path, "room", name, env)
        for k in range(2):
            scenes.assert_bit_equal(frames[f"r{k}"], want, f"closed room, {name}, render {k}")


def test_backgrounds_and_both_outputs(gpu, oracle, ref, tmp_path):
    """Gradient (its plate built at the first render), flat, transparent and 1 spp frames, float4 and RGBA8 at once, three
    renders each on one handle: equal by ticket and by stride, and equal to the oracle."""
    import scenes
    import transparent_checker
    from minecraftskin_raytracer_amd import abi

    on = _run(tmp_path, "backgrounds", "tickets", dict(GRID3, MCRT_BG_PLATE="2"))
    off = _run(tmp_path, "backgrounds", "static", dict(GRID3, MCRT_BG_PLATE="2", MCRT_WORK_TICKETS="0"))
    checker = transparent_checker.Checker(transparent_checker.build(str(tmp_path)))
    transparent, _ = checker.render(make_scene(("pose", 6)).ptr, abi.Config(**BASE), threads=transparent_checker.threads())
    for name, mode, kw in BACKGROUNDS:
        want = transparent if mode == "transparent" else ref(("pose", 6), kw)
        want8 = oracle.quantize(want).reshape(want.shape)
        for k in range(3):
            scenes.assert_bit_equal(on[f"{name}_{k}"], off[f"{name}_{k}"], f"{name} render {k}: by ticket and by stride")
            scenes.assert_bit_equal(on[f"{name}_{k}"], want, f"{name} render {k}")
            assert np.array_equal(on[f"{name}8_{k}"], want8), f"{name} render {k}: RGBA8 plane"
            assert np.array_equal(off[f"{name}8_{k}"], want8), f"{name} render {k}: RGBA8 plane, by stride"


@pytest.mark.parametrize("env", [GRID3, dict(GRID3, MCRT_WORKSPACE_MB="1")], ids=["one_pass", "multi_pass"])
def test_shards_packed_rows_lanes_and_passes_equal_the_whole_frame(gpu, ref, tmp_path, env):
    import scenes

    frames = _run(tmp_path, "variants", "_".join(env.values()), env)
    want = ref(("pose", 6), BASE)
    for rnd in range(2):
        for name in ("whole", "packed", "shards", "lanes3"):
            scenes.assert_bit_equal(frames[f"{name}_{rnd}"], want, f"{name} round {rnd}")


def test_four_handles_in_flight_on_four_streams(gpu, ref, tmp_path):
    import scenes

    frames = _run(tmp_path, "inflight", "grid3", GRID3)
    for k in FLIGHT_POSES:
        for rnd in range(3):
            scenes.assert_bit_equal(frames[f"p{k}_{rnd}"], ref(("pose", k), BASE), f"pose {k} round {rnd}")


def test_batch_call_equals_single_renders(gpu, ref, tmp_path):
    """The batched kernels share the bodies: one set of counters per frame, the frame by blockIdx.y."""
    import scenes

    frames = _run(tmp_path, "batch", "grid3", GRID3)
    for k in BATCH_POSES:
        want = ref(("pose", k), SMALL)
        scenes.assert_bit_equal(frames[f"single_p{k}"], want, f"pose {k} alone")
        for call in range(3):
            scenes.assert_bit_equal(frames[f"batch{call}_p{k}"], want, f"pose {k}, batch call {call}")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
