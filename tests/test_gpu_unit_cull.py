"""Units by block (DESIGN.md §4 "Units by block"): `plan_tiles` cuts a touched tile into square blocks instead of pixel ranges,
and `primary`, `resolve` and the draws' addresses follow a unit's pixels through one helper (kernel_common.h: UnitMap).
What can go wrong is a wrong frame: a pixel mapped to another place, another draw or another slot, a clipped block that
reaches over its tile.  Parity is bit-exact, on the uint32 views of the float frames: every frame is compared with the CPU
oracle (the transparent ones with the test-side checker of that mode) and with the same render under MCRT_UNIT_BLOCKS=0.
(The issue's second mechanism, a mesh mask per unit with units left out where nothing can touch them, was measured and
taken out again — DESIGN.md §4 "Measured and rejected: units culled by screen bounds" — so the cases that exist for it, the
one-colour corner tile, the far mesh, the 64 meshes, the camera without bounds, are parity cases here, and the structural
check is on the blocks alone.)

The knobs are read once per process, so every setting runs in a child process — this file run as a script — which renders
ALL cases with the environment it is given and writes its frames to an .npz; the parent checks.  Every case is rendered
three times on its handle: the first render has no plates yet, the second builds them, the third reads them."""
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

KNOBS = ("MCRT_UNIT_BLOCKS", "MCRT_BG_PLATE", "MCRT_DRAW_PLATE", "MCRT_WORK_TICKETS", "MCRT_SHARED_GRIDS", "MCRT_PRIMARY_GRID",
         "MCRT_LIT_GRID", "MCRT_QUEUE_GRID", "MCRT_WORKSPACE_MB", "MCRT_STREAM_WAVES")
OFF = {"MCRT_UNIT_BLOCKS": "0"}
SETTINGS = {
    "default": {},
    "off": OFF,
    "no_bg_plate": {"MCRT_BG_PLATE": "0"},
    "bg_plate_first_use": {"MCRT_BG_PLATE": "2"},
    "no_draw_plate": {"MCRT_DRAW_PLATE": "0"},
    "draw_plate_first_use": {"MCRT_DRAW_PLATE": "2"},
}

# 3 x 2 tiles of 32 px; the figure, seen from the side and enlarged, covers parts of four of them: blocks on, under and beside
# the silhouette
FIG = dict(width=96, height=64, tileSize=32, samplesPerPixel=4, maxBounces=2)
# a last tile column 6 px wide and a last tile row 13 px high: clipped blocks
CLIP = dict(width=70, height=45, tileSize=32, samplesPerPixel=4, maxBounces=2)
DOF = dict(dofEnabled=True, aperture=0.3)
# name -> (scene spec, config, background mode)
CASES = {
    "fig96": (("aside", 0), FIG, "reference"),
    "clip70x45": (("pose", 0), CLIP, "reference"),
    **{f"tile{ts}": (("pose", 6), dict(CLIP, tileSize=ts), "reference") for ts in (8, 16, 20, 24)},
    **{f"spp{n}": (("aside", 0), dict(CLIP, samplesPerPixel=n), "reference") for n in (1, 2, 3, 16)},
    "spp64": (("pose", 0), dict(width=64, height=64, tileSize=32, samplesPerPixel=64, maxBounces=1), "reference"),  # 128 draws per pixel: bg_in_plan off
    "dof": (("aside", 0), dict(CLIP, tileSize=16, **DOF), "reference"),
    "dof_fig96": (("aside", 0), dict(FIG, **DOF), "reference"),
    "flat": (("aside", 0), dict(FIG, gradientBg=False), "reference"),
    "transparent": (("aside", 0), FIG, "transparent"),
    # gradientScale 4: every tile but the middle column's is of one colour — the figure's left half lies in one-colour tiles
    "corner": (("aside", 0), dict(FIG, gradientScale=4.0), "reference"),
    "pose6": (("pose", 6), FIG, "reference"),
    "far_mesh": (("far_mesh", 0), FIG, "reference"),
    "meshes64": (("big64", 0), None, "reference"),  # the case's own config
    "cull_off_camera": (("wide", 0), FIG, "reference"),
}
PACKED = dict(FIG, tileSize=16)  # 4 tile rows: the shards (0, 3), (1, 3) and (2, 3) own rows {0, 3}, {1} and {2}
BATCH_SIZES = {"batch_a": FIG, "batch_b": CLIP}
BATCH_POSES = (0, 6)
FLIGHT_POSES = (0, 2, 4, 6)
RECT = (8, 8, 72, 40)  # a renderTile rectangle larger than a tile


def make_scene(spec):
    import big_scene_cases as BS
    import minecraftskin_raytracer_amd as M
    import scenes

    kind, k = spec
    if kind == "big64":
        return _big64()[0]
    if kind == "far_mesh":  # three boxes in view and one far off to the side, which touches no tile
        boxes = [scenes.build_box(scenes.solid((0.9, 0.3, 0.2, 1.0)), (-6, 14, 0), (6, 12, 6)), scenes.build_box(scenes.solid((0.2, 0.7, 0.9, 1.0)), (5, 22, -3), (5, 5, 5)),
                 scenes.build_box(scenes.solid((0.3, 0.8, 0.3, 1.0)), (4, 9, 4), (4, 6, 4)), scenes.build_box(scenes.solid((0.8, 0.8, 0.1, 1.0)), (400, 18, 0), (6, 6, 6))]
        return M.SceneDesc(scenes.simple_scene(boxes, cam_pos=(0, 18, 50), cam_target=(0, 18, 0)))
    sd = scenes.skin_scene("S64", k)
    d = sd.desc
    if kind == "aside":  # the camera moved to the side and the lens narrowed: the figure straddles the tile columns 0 and 1
        d.camera_position[0] += 14.0
        d.camera_target[0] += 14.0
        d.camera_fov = 45.0
    elif kind == "wide":  # tan(fov / 2) above 1e4: the flattener offers no screen bounds (FlatHeader::cull_ok = 0); the camera sits
        d.camera_fov = 179.99  # just in front of the torso so that the figure still fills part of the frame
        d.camera_position[2] = 2.002
    return sd


def _big64():
    """A 64-mesh scene of big_scene_cases (flat pipeline): the tile masks are all ones: every tile is cut into units."""
    import big_scene_cases as BS

    for seed in range(9, 400):
        if BS.nominal(seed, "count") == 64:
            sd, cfg, _, what = BS.make_big_case(seed, "count")
            if not BS.is_general(cfg):
                return sd, cfg, what
    raise AssertionError("no 64-mesh case")


def case_config(name):
    spec, kw, mode = CASES[name]
    if kw is None:
        import dataclasses

        kw = {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in dataclasses.asdict(_big64()[1]).items()}
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# the child: renders every case under the environment it was started with
# ---------------------------------------------------------------------------------------------------------------------
def _child(out_path):
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi

    frames = {}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def buffer(cfg, n=None, dtype=torch.float32):
        shape = (cfg.height, cfg.width, 4) if n is None else (n, cfg.height, cfg.width, 4)
        return torch.zeros(shape, dtype=dtype, device="cuda")

    def render(ds, kw, first=0, step=1):
        cfg = M.Config(**kw)
        out = buffer(cfg)
        ds.render_device(cfg, out.data_ptr(), first, step, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    for name, (spec, _, mode) in CASES.items():
        kw = case_config(name)
        ds = M.DeviceScene(make_scene(spec))
        ds.set_lanes(1)
        ds.set_background(mode)
        for k in range(3):
            frames[f"{name}_{k}"] = render(ds, kw)
        if name in ("fig96", "meshes64", "cull_off_camera", "far_mesh", "spp64"):
            u = ds.units()
            frames[f"{name}_records"], frames[f"{name}_hits"] = u["records"], u["hits"]
        if name == "fig96":
            frames["fig96_blob"] = np.frombuffer(ds.blob(), np.uint8)
        ds.check()

    # layout and handles, on the figure
    ds = M.DeviceScene(make_scene(("aside", 0)))
    cfg = M.Config(**PACKED)
    for k in range(3):
        out = buffer(cfg)
        for r in range(3):  # packed rows of the shards (0,3), (1,3), (2,3), scattered by unpack_rows
            rows = ds.owned_pixel_rows(cfg, r, 3)
            packed = torch.zeros((max(rows, 1), cfg.width, 4), dtype=torch.float32, device="cuda")
            ds.render_device(cfg, packed.data_ptr(), r, 3, abi.LAYOUT_PACKED, stream())
            M.unpack_rows_device(cfg, r, 3, packed.data_ptr(), out.data_ptr(), stream())
            torch.cuda.synchronize()
        frames[f"packed_{k}"] = out.cpu().numpy()
    cfg = M.Config(**FIG)
    for k in range(3):
        out, out8 = buffer(cfg), buffer(cfg, dtype=torch.uint8)
        ds.render_device_ex(cfg, out.data_ptr(), out8.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        frames[f"both_{k}"], frames[f"both8_{k}"] = out.cpu().numpy(), out8.cpu().numpy()
        out8 = buffer(cfg, dtype=torch.uint8)
        ds.render_device_ex(cfg, 0, out8.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        frames[f"only8_{k}"] = out8.cpu().numpy()
    ds.set_lanes(2)
    for k in range(3):
        frames[f"lanes2_{k}"] = render(ds, FIG)
    ds.set_lanes(0)
    ds.check()

    # the batch entry, two calls of different frame size
    hs = [M.DeviceScene(make_scene(("aside" if p == 0 else "pose", p))) for p in BATCH_POSES]
    for call in range(3):
        for name, kw in BATCH_SIZES.items():
            cfg = M.Config(**kw)
            out = buffer(cfg, len(hs))
            M.render_batch_device(hs, cfg, out.data_ptr(), 0, None, stream())
            torch.cuda.synchronize()
            for i, p in enumerate(BATCH_POSES):
                frames[f"{name}_{call}_p{p}"] = out[i].cpu().numpy()
    for ds in hs:
        ds.check()

    # four handles in flight on four streams, then each alone
    hs = [M.DeviceScene(make_scene(("pose", p))) for p in FLIGHT_POSES]
    for ds in hs:
        ds.set_lanes(1)
    streams = [torch.cuda.Stream() for _ in hs]
    cfg = M.Config(**FIG)
    rounds = 3
    outs = [[buffer(cfg) for _ in hs] for _ in range(rounds)]
    torch.cuda.synchronize()
    for rnd in range(rounds):  # nothing waits between the rounds
        for i, ds in enumerate(hs):
            ds.render_device(cfg, outs[rnd][i].data_ptr(), 0, 1, abi.LAYOUT_FRAME, streams[i].cuda_stream)
    torch.cuda.synchronize()
    for rnd in range(rounds):
        for i, p in enumerate(FLIGHT_POSES):
            frames[f"flight_p{p}_{rnd}"] = outs[rnd][i].cpu().numpy()
    for p, ds in zip(FLIGHT_POSES, hs):
        frames[f"lone_p{p}"] = render(ds, FIG)
        ds.check()

    # a renderTile rectangle (mcrt_render_rect): pixel ranges, whatever the knobs say
    cfg = M.Config(**FIG)
    tile_frame = np.zeros((cfg.height, cfg.width, 4), np.float32)
    M.TileRenderer.renderTile(RECT, make_scene(("aside", 0)), cfg, tile_frame)
    assert M.TileRenderer.lastErrors() == []
    frames["rect"] = tile_frame
    np.savez(out_path, **frames)


_RUNS = {}


def _run(tmp_path_factory, setting):
    """the frames of a setting: its child runs once per session"""
    if setting not in _RUNS:
        out = str(tmp_path_factory.mktemp(f"unit_cull_{setting}") / "frames.npz")
        e = dict(os.environ)
        for knob in KNOBS:
            e.pop(knob, None)
        e.update(SETTINGS[setting])
        subprocess.run([sys.executable, os.path.abspath(__file__), out], env=e, check=True, timeout=600)
        z = np.load(out)
        _RUNS[setting] = {k: z[k] for k in z.files}
    return _RUNS[setting]


class _Expected:
    """what every frame must be, each computed once: the oracle's render, or the transparent checker's"""

    def __init__(self, oracle, tmp):
        self.oracle, self.tmp, self.cache, self.checker = oracle, tmp, {}, None

    def __call__(self, spec, kw, mode="reference"):
        from minecraftskin_raytracer_amd import abi

        key = (spec, json.dumps(kw, sort_keys=True), mode)
        if key not in self.cache:
            sd = make_scene(spec)
            if mode == "transparent":
                import transparent_checker

                if self.checker is None:
                    self.checker = transparent_checker.Checker(transparent_checker.build(self.tmp))
                self.cache[key] = self.checker.render(sd.ptr, abi.Config(**kw), threads=transparent_checker.threads())[0]
            else:
                self.cache[key] = self.oracle.render(sd.ptr, abi.Config(**kw))
        return self.cache[key]


@pytest.fixture(scope="module")
def want(oracle, tmp_path_factory):
    return _Expected(oracle, str(tmp_path_factory.mktemp("unit_cull_checker")))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_oracle_and_the_knob_off_render(gpu, want, tmp_path_factory, name, setting):
    import scenes

    spec, _, mode = CASES[name]
    expected = want(spec, case_config(name), mode)
    got, off = _run(tmp_path_factory, setting), _run(tmp_path_factory, "off")
    for k in range(3):
        scenes.assert_bit_equal(got[f"{name}_{k}"], off[f"{name}_{k}"], f"{name} render {k}, {setting}: against MCRT_UNIT_BLOCKS=0")
        scenes.assert_bit_equal(got[f"{name}_{k}"], expected, f"{name} render {k}, {setting}")


@pytest.mark.parametrize("setting", ["default", "no_bg_plate", "bg_plate_first_use"])
def test_layouts_outputs_lanes_batches_and_handles_in_flight(gpu, oracle, want, tmp_path_factory, setting):
    import scenes

    got, off = _run(tmp_path_factory, setting), _run(tmp_path_factory, "off")
    fig = want(("aside", 0), FIG)
    fig8 = oracle.quantize(fig).reshape(fig.shape)
    for k in range(3):
        scenes.assert_bit_equal(got[f"packed_{k}"], want(("aside", 0), PACKED), f"packed rows of three shards, render {k}")
        scenes.assert_bit_equal(got[f"both_{k}"], fig, f"float4 beside RGBA8, render {k}")
        assert np.array_equal(got[f"both8_{k}"], fig8), f"RGBA8 beside float4, render {k}"
        assert np.array_equal(got[f"only8_{k}"], fig8), f"RGBA8 alone, render {k}"
        scenes.assert_bit_equal(got[f"lanes2_{k}"], fig, f"two lanes, render {k}")
    for call in range(3):
        for name, kw in BATCH_SIZES.items():
            for p in BATCH_POSES:
                scenes.assert_bit_equal(got[f"{name}_{call}_p{p}"], want(("aside" if p == 0 else "pose", p), kw), f"{name} call {call} pose {p}")
    for p in FLIGHT_POSES:
        scenes.assert_bit_equal(got[f"lone_p{p}"], want(("pose", p), FIG), f"pose {p} alone")
        for rnd in range(3):
            scenes.assert_bit_equal(got[f"flight_p{p}_{rnd}"], got[f"lone_p{p}"], f"pose {p} in flight, round {rnd}")
    for key in got:
        if not key.endswith(("_records", "_hits", "_blob")):
            assert np.array_equal(got[key].view(np.uint8), off[key].view(np.uint8)), f"{key}, {setting}: against MCRT_UNIT_BLOCKS=0"


def test_render_rect_keeps_its_pixel_ranges(gpu, oracle, tmp_path_factory):
    import scenes
    from minecraftskin_raytracer_amd import abi

    tile = np.zeros((FIG["height"], FIG["width"], 4), np.float32)
    oracle.render_tile(make_scene(("aside", 0)).ptr, abi.Config(**FIG), RECT, tile)
    x, y, w, h = RECT
    assert (tile[y:y + h, x:x + w, :3] != tile[y, x, :3]).any()  # the rectangle does show the figure
    for setting in ("default", "off"):
        scenes.assert_bit_equal(_run(tmp_path_factory, setting)["rect"], tile, f"renderTile rectangle, {setting}")


# ---- the structure of the plan -------------------------------------------------------------------------------------------
F = np.float32


def _touches(screen, x, y, w, h, W, H):
    """mesh_touches_tile (kernel_common.h) without a lens pad, in the kernel's float operations"""
    u0, v0, u1, v1 = (F(v) for v in screen)
    if u0 > u1:
        return True
    W, H = F(W), F(H)
    aspect = W / H
    tu0 = (F(2) * (F(x) - F(2)) / W - F(1)) * aspect - F(1e-3) * aspect - F(1e-3)
    tu1 = (F(2) * (F(x + w) + F(2)) / W - F(1)) * aspect + F(1e-3) * aspect + F(1e-3)
    tv1 = F(1) - F(2) * (F(y) - F(2)) / H + F(2e-3)
    tv0 = F(1) - F(2) * (F(y + h) + F(2)) / H - F(2e-3)
    return not (u1 < tu0 or u0 > tu1 or v1 < tv0 or v0 > tv1)


def _host_blocks(blob, kw, block):
    """{(tile, x, y, w, h)} of every block of every touched tile, from the blob's FlatMesh::screen bounds"""
    hdr = np.frombuffer(blob[:192].tobytes(), np.uint32)
    n, mesh_offset = int(hdr[1]), int(hdr[32])
    assert hdr[3] == 1 and n < 64  # cull_ok
    screens = [np.frombuffer(blob[mesh_offset + 192 * i + 144:mesh_offset + 192 * i + 160].tobytes(), np.float32) for i in range(n)]
    W, H, T = kw["width"], kw["height"], kw["tileSize"]
    out = set()
    tiles_x = -(-W // T)
    for ty in range(-(-H // T)):
        for tx in range(tiles_x):
            x, y = tx * T, ty * T
            w, h = min(T, W - x), min(T, H - y)
            if any(_touches(s, x, y, w, h, W, H) for s in screens):
                out |= {(ty * tiles_x + tx, bx, by, min(block, w - bx), min(block, h - by)) for by in range(0, h, block) for bx in range(0, w, block)}
    return out


def _units(run, name):
    """the queued units of a case: blocks as {(tile, x, y, w, h): hits}, pixel ranges as {(tile, first, end): hits}"""
    blocks, ranges = {}, {}
    for r, hcount in zip(run[f"{name}_records"], run[f"{name}_hits"]):
        if r[0] >> 31:
            blocks[(int(r[0] & 0x7fffffff), int(r[1] & 0xffff), int(r[1] >> 16), int(r[2] & 0xffff), int(r[2] >> 16))] = int(hcount)
        else:
            ranges[(int(r[0]), int(r[1]), int(r[2]))] = int(hcount)
    return blocks, ranges


def test_queued_units_are_the_blocks_of_the_touched_tiles(gpu, tmp_path_factory):
    """The 96 x 64 case: the queued units are exactly the 8 x 8 blocks of the tiles that the bounds of at least one mesh touch —
    the host forms them from FlatMesh::screen with the kernel's arithmetic —, no two share a slot range, and they hold the
    primary hits that the pixel ranges of the knob-off render hold, tile by tile.  Blocks with and without hits both occur."""
    on, off = _run(tmp_path_factory, "default"), _run(tmp_path_factory, "off")
    blocks, ranges = _units(on, "fig96")
    assert not ranges and len(blocks) == len(on["fig96_records"])
    assert set(blocks) == _host_blocks(on["fig96_blob"], FIG, 8)
    spans = sorted((int(r[3]), int(r[3]) + 64 * FIG["samplesPerPixel"]) for r in on["fig96_records"])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    off_blocks, off_ranges = _units(off, "fig96")
    assert not off_blocks and {k[0] for k in off_ranges} == {k[0] for k in blocks}
    for tile in {k[0] for k in blocks}:
        assert sum(h for k, h in blocks.items() if k[0] == tile) == sum(h for k, h in off_ranges.items() if k[0] == tile), tile
    assert any(h == 0 for h in blocks.values()) and any(h > 0 for h in blocks.values())


def test_block_grids_of_other_shapes(gpu, tmp_path_factory):
    """64 meshes and a camera without screen bounds: every tile is touched and cut.  A mesh far off-screen touches no tile.  At
    64 spp (and at 16) no grid of at most 16 blocks gives one chunk per block: the tile keeps its 16 pixel ranges."""
    on = _run(tmp_path_factory, "default")
    for name in ("meshes64", "cull_off_camera"):
        kw = case_config(name)
        tiles = -(-kw["width"] // kw["tileSize"]) * -(-kw["height"] // kw["tileSize"])
        blocks, ranges = _units(on, name)
        assert not ranges and {k[0] for k in blocks} == set(range(tiles)), name
    blocks, _ = _units(on, "far_mesh")
    assert 0 < len({k[0] for k in blocks}) < 6 and sum(blocks.values()) > 0
    blocks, ranges = _units(on, "spp64")
    assert not blocks and len(ranges) == 16 * len({k[0] for k in ranges}) > 0


if __name__ == "__main__":
    _child(sys.argv[1])
