"""The sample table (include/mcrt.h, "Sample table"): a device keeps, by shadow seed, what a hit's light-disk
samples are before the light enters — {cos, sin, sqrt} of the seed's draws — and `lit` reads a traced hit's row instead of
running the engine.  Frames must not depend on it: bit for bit the same with the table on, off and half-applicable (seeds
outside the window, more than 8 samples, hard shadows), and equal to the CPU oracle's.

MCRT_SAMPLE_TABLE is read once per process, so the frame and lifecycle scenarios run in a child process — this file run as
a script — with the environment they need: 2 builds the table at a device's first soft-shadow render, the default at its
second, 0 never.  A child writes its frames and the store's figures (mcrt_sample_table_info) to an .npz; the parent checks."""
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

HALF = 1 << 22  # the window: seeds -2^22 .. 2^22 - 1
BASE = dict(width=96, height=64, maxBounces=2, samplesPerPixel=4)
# the calls of one sequence on one handle: rows serve 8 and 4 samples; 9 samples and hard shadows fall back within it
SEQUENCE = [("s8", dict(shadowSamples=8)), ("s4", dict(shadowSamples=4)), ("s9", dict(shadowSamples=9)), ("hard", dict(softShadows=False)),
            ("s8_again", dict(shadowSamples=8))]
POSES = (0, 6)
# boxes of test_seed_table_window_and_recurrence_agree, re-aimed: the shadow seed is about 67890 * y, the window's edge at
# |y| = 2^22 / 67890 = 61.8.  Inside; across the upper edge; beyond it; inside at the wrapped (negative) end; across the lower
# edge; beyond it.
EDGE_HEIGHTS = [0.0, 60.0, 100.0, -40.0, -62.0, -100.0]


def edge_scene(height):
    import minecraftskin_raytracer_amd as M
    import scenes

    tex = scenes.solid((0.8, 0.6, 0.4, 1.0))
    meshes = [scenes.build_box(tex, (0.0, height, 0.0), (8.0, 12.0, 4.0)), scenes.build_box(tex, (7.0, height + 2.0, 1.0), (3.0, 10.0, 3.0))]
    return M.SceneDesc(scenes.simple_scene(meshes, light=(5.0, height + 30.0, 30.0), cam_pos=(0.0, height + 2.0, 40.0), cam_target=(0.0, height, 0.0)))


EDGE_CFG = dict(width=120, height=90, maxBounces=3, samplesPerPixel=2)


# ---------------------------------------------------------------------------------------------------------------------
# the child: renders a scenario, saves frames and the store's figures
# ---------------------------------------------------------------------------------------------------------------------
def _child(scenario, out_path):
    import torch

    import minecraftskin_raytracer_amd as M
    import scenes
    from minecraftskin_raytracer_amd import abi

    frames, infos = {}, {}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def render(ds, kw):
        cfg = M.Config(**kw)
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        torch.cuda.synchronize()
        return out.cpu().numpy()

    if scenario == "frames":
        for pose in POSES:
            ds = M.DeviceScene(scenes.skin_scene("S64", pose))
            for label, kw in SEQUENCE:
                frames[f"p{pose}_{label}"] = render(ds, dict(BASE, **kw))
                infos[f"p{pose}_{label}"] = M.sample_table_info()
            ds.check()
    elif scenario == "edges":
        for h in EDGE_HEIGHTS:
            ds = M.DeviceScene(edge_scene(h))
            frames[f"y{h}"] = render(ds, EDGE_CFG)
            ds.check()
            infos[f"y{h}"] = M.sample_table_info()
    elif scenario == "lifecycle":
        ds = M.DeviceScene(scenes.skin_scene("S64", 6))
        ds.set_lanes(1)
        cfg = M.Config(**BASE)
        infos["start"] = M.sample_table_info()
        frames["hard_0"] = render(ds, dict(BASE, softShadows=False))  # no soft shadows: not a sighting
        infos["hard_0"] = M.sample_table_info()
        frames["first"] = render(ds, BASE)  # the device's first soft-shadow render
        infos["first"] = M.sample_table_info()
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):  # the second, inside the caller's capture: it must not build
            ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        infos["captured"] = M.sample_table_info()
        g.replay()
        torch.cuda.synchronize()
        frames["replayed"] = out.cpu().numpy()
        infos["replayed"] = M.sample_table_info()
        frames["second"] = render(ds, BASE)  # outside the capture: now the table is built
        infos["second"] = M.sample_table_info()
        frames["third"] = render(ds, BASE)
        infos["third"] = M.sample_table_info()
        out2 = torch.zeros_like(out)
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2):  # a capture with the table built: the render takes none
            ds.render_device(cfg, out2.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
        g2.replay()
        torch.cuda.synchronize()
        frames["replayed_built"] = out2.cpu().numpy()
        ds.check()
        M.trim()  # a handle is left: the table stays
        infos["trim_held"] = M.sample_table_info()
        del g, g2
        ds.close()
        M.trim()
        infos["trimmed"] = M.sample_table_info()
        ds = M.DeviceScene(scenes.skin_scene("S64", 6))
        frames["after_trim_0"] = render(ds, BASE)
        infos["after_trim_0"] = M.sample_table_info()
        frames["after_trim_1"] = render(ds, BASE)
        infos["after_trim_1"] = M.sample_table_info()
        ds.check()
    else:
        raise SystemExit(f"unknown scenario {scenario}")
    np.savez(out_path, __infos__=np.frombuffer(json.dumps(infos).encode(), np.uint8), **frames)


def _run(tmp_path, scenario, knob):
    out = str(tmp_path / f"{scenario}_{knob}.npz")
    e = dict(os.environ)
    e.pop("MCRT_SAMPLE_TABLE", None)
    if knob is not None:
        e["MCRT_SAMPLE_TABLE"] = str(knob)
    subprocess.run([sys.executable, os.path.abspath(__file__), scenario, out], env=e, check=True, timeout=600)
    z = np.load(out)
    return {k: z[k] for k in z.files if k != "__infos__"}, json.loads(z["__infos__"].tobytes())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
def test_rows_are_the_draws_through_sincos_and_sqrt(mcrt, gpu):
    """Rows of the built table against rows formed from the probes that exist: the 16 draws of mcrt_probe_mt_uniform, the fused
    sincos of mcrt_probe_detmath (ops 3 and 4) on float32(2 pi) * d0, numpy's float32 sqrt (rt::sqrt_pos equals IEEE sqrtf:
    test_gpu_parity checks that) — at the window's ends, around zero and at 256 random seeds."""
    rng = np.random.default_rng(20240611)
    seeds = np.concatenate([np.array([-HALF, -HALF + 1, -1, 0, 1, HALF - 1], np.int64), rng.integers(-HALF, HALF, 256)]).astype(np.int32)
    rows = mcrt.probe_sample_rows(seeds)
    assert rows.shape == (len(seeds), 8, 4)
    draws = mcrt.probe_mt_uniform(seeds.astype(np.uint32), 16)
    d0, d1 = draws[:, 0::2], draws[:, 1::2]
    angle = (np.float32(2.0) * np.float32(np.pi) * d0).astype(np.float32)  # rt_core.h: kTwoPi * d0
    sn = mcrt.probe_detmath(3, angle.ravel()).reshape(angle.shape)
    cs = mcrt.probe_detmath(4, angle.ravel()).reshape(angle.shape)
    want = np.stack([cs, sn, np.sqrt(d1, dtype=np.float32), np.zeros_like(cs)], axis=-1)
    assert np.array_equal(_bits(rows), _bits(want))
    info = mcrt.sample_table_info()
    assert info["bytes"] == (1 << 23) * 128 and info["builds"] >= 1
    for bad in (HALF, -HALF - 1):
        with pytest.raises(Exception):
            mcrt.probe_sample_rows([bad])


def test_frames_do_not_depend_on_the_table(mcrt, oracle, gpu, tmp_path):
    """Poses 0 and 6, 96 x 64, 4 spp, 2 bounces; 8 and 4 samples from the rows, 9 samples and hard shadows by the engine within
    the same call sequence: the table built at the first render (knob 2) against no table (knob 0), and the oracle.  That hits
    of these scenes are traced at all — a decided bundle reads no sample — shows in the light pass's visibility plane (which
    takes no table): pixels whose primary hit sees a part of the disk, neither none of it nor all."""
    import scenes
    from minecraftskin_raytracer_amd import abi

    on, info_on = _run(tmp_path, "frames", 2)
    off, info_off = _run(tmp_path, "frames", 0)
    assert sorted(on) == sorted(off) and len(on) == len(POSES) * len(SEQUENCE)
    for k in on:
        assert np.array_equal(_bits(on[k]), _bits(off[k])), k
    assert all(v["builds"] == 0 and v["bytes"] == 0 for v in info_off.values())
    assert all(v["builds"] == 1 and v["bytes"] == (1 << 23) * 128 for v in info_on.values())
    for pose in POSES:
        sd = scenes.skin_scene("S64", pose)
        for label, kw in SEQUENCE[:4]:
            cfg = abi.Config(**dict(BASE, **kw))
            scenes.assert_bit_equal(on[f"p{pose}_{label}"], oracle.render(sd.ptr, cfg), f"pose {pose} {label}")
        assert np.array_equal(_bits(on[f"p{pose}_s8"]), _bits(on[f"p{pose}_s8_again"]))
        vis = mcrt.TileRenderer.renderLight(sd, abi.Config(**dict(BASE, shadowSamples=8)), planes=("visibility",))["visibility"]
        penumbra = int(((vis > 0.0) & (vis < 1.0)).sum())
        print(f"pose {pose}: {penumbra} penumbra pixels of {vis.size}")
        assert penumbra > 0


def test_window_edges(mcrt, oracle, gpu, tmp_path):
    """Boxes whose hits have seeds inside the window, across each of its ends, beyond them and at the wrapped negative end:
    rows and engine mix within one frame, and every frame equals the oracle's."""
    from minecraftskin_raytracer_amd import abi

    got, infos = _run(tmp_path, "edges", 2)
    assert all(v["builds"] == 1 for v in infos.values())
    cfg = abi.Config(**EDGE_CFG)
    for h in EDGE_HEIGHTS:
        scenes_frame = got[f"y{h}"]
        ref = oracle.render(edge_scene(h).ptr, cfg)
        assert np.array_equal(_bits(scenes_frame), _bits(ref)), f"boxes at y = {h}"


def test_default_scene_with_the_table_equals_the_oracle(mcrt, oracle, gpu):
    """The one-shot entry with the table built (the rows test, or any two soft-shadow renders before, built it; the probe
    builds it otherwise): a small frame of the default scene, bit for bit the oracle's."""
    import scenes
    from minecraftskin_raytracer_amd import abi

    mcrt.probe_sample_rows([0])
    assert mcrt.sample_table_info()["bytes"] > 0
    sd = scenes.skin_scene("S64", 0)
    cfg = abi.Config(width=96, height=54, maxBounces=4, samplesPerPixel=4)
    img = mcrt.TileRenderer.render(sd, cfg)
    assert mcrt.TileRenderer.lastErrors() == []
    scenes.assert_bit_equal(img, oracle.render(sd.ptr, cfg), "default scene, table built")


def test_lifecycle(mcrt, oracle, gpu, tmp_path):
    """Default knob.  A hard-shadow render is no sighting; the device's first soft-shadow render builds nothing; the second,
    recorded into a caller's graph, builds nothing either; the next one outside builds; trim with a handle left keeps the
    table, trim with none frees it, and the renders after it — first without, then with a rebuilt table — give the same bits."""
    import scenes
    from minecraftskin_raytracer_amd import abi

    frames, infos = _run(tmp_path, "lifecycle", None)
    size = (1 << 23) * 128
    for when in ("start", "hard_0", "first", "captured", "replayed"):
        assert infos[when] == {"bytes": 0, "builds": 0}, when
    for when in ("second", "third", "trim_held"):
        assert infos[when] == {"bytes": size, "builds": 1}, when
    assert infos["trimmed"] == {"bytes": 0, "builds": 1}
    assert infos["after_trim_0"] == {"bytes": 0, "builds": 1}
    assert infos["after_trim_1"] == {"bytes": size, "builds": 2}
    sd = scenes.skin_scene("S64", 6)
    ref = oracle.render(sd.ptr, abi.Config(**BASE))
    for k in ("first", "replayed", "second", "third", "replayed_built", "after_trim_0", "after_trim_1"):
        assert np.array_equal(_bits(frames[k]), _bits(ref)), k
    scenes.assert_bit_equal(frames["hard_0"], oracle.render(sd.ptr, abi.Config(**dict(BASE, softShadows=False))), "hard shadows")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
