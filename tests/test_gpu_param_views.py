"""Parameters by phase ("Scalar registers"): `primary`, `lit`, `resolve` and `ao` no longer hold their
RenderParams from the kernel's entry; every phase of their item loops reads what it needs through a reference made where the
phase begins (kernel_common.h, phase_params).  What can go wrong is a phase that reads a field from the wrong place — a
single-frame entry whose parameters are not where kernarg_params() looks, a batch entry that looks at another frame's — or
a value that an earlier version kept across the loop and a phase now forms differently.  So: one small frame per way a phase
reads its parameters, each rendered twice on one handle (the counters run on), bit for bit against the CPU oracle on the
uint32 views of the float frames (the transparent frame against the test-side checker of that mode).

The launch knobs are read once per process, so the scenarios run in a child process — this file run as a script — once per
environment: the defaults, MCRT_SHARED_GRIDS=1, and grids of five workgroups, where every workgroup claims most of its items
by ticket and passes each phase's reload many times.  The child writes its frames to an .npz and the parent checks.

Frames are 96 x 64 and 90 x 62 (a clipped right column and bottom row) at tile 32."""
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

FRAME = dict(width=96, height=64, tileSize=32, maxBounces=4, samplesPerPixel=4)
ODD = dict(FRAME, width=90, height=62)
# name: (scene, config, how it is rendered)
SCENARIOS = {
    "spp1_bounces0": (("skin", 0), dict(FRAME, samplesPerPixel=1, maxBounces=0), "plain"),
    "spp4_bounces1": (("skin", 0), dict(FRAME, maxBounces=1), "plain"),
    "spp4_bounces4_posed": (("skin", 6), FRAME, "plain"),
    "depth_of_field": (("skin", 6), dict(ODD, dofEnabled=True, aperture=0.5), "plain"),
    "point_light": (("boxes", 0.0), FRAME, "plain"),
    "hard_shadows": (("skin", 6), dict(FRAME, softShadows=False), "plain"),
    "unposed_boxes": (("boxes", 3.0), ODD, "plain"),
    "ambient_occlusion": (("skin", 6), dict(FRAME, aoEnabled=True), "plain"),
    "hbm_view": (("many", 70), ODD, "plain"),
    "packed_shard2": (("skin", 6), ODD, "packed"),
    "rgba8": (("skin", 6), FRAME, "rgba8"),
    "transparent": (("skin", 6), FRAME, "transparent"),
    "batch3": (("batch", (0, 3, 6)), FRAME, "batch"),
}
ENVS = {
    "defaults": {},
    "shared_grids": {"MCRT_SHARED_GRIDS": "1"},
    "grid5": {"MCRT_PRIMARY_GRID": "5", "MCRT_LIT_GRID": "5"},
}
RENDERS = 2  # in a row on one handle


def make_scene(spec):
    import scenes

    import minecraftskin_raytracer_amd as M

    kind, k = spec
    if kind == "skin":
        return scenes.skin_scene("S64", k)
    if kind == "many":
        return M.SceneDesc(scenes.many_boxes(k))
    # three axis-aligned boxes above a slab, the light of radius k (0: a point light)
    slab = scenes.build_box(scenes.solid((0.7, 0.75, 0.8, 1.0)), (0, 4, 0), (40, 2, 40))
    a = scenes.build_box(scenes.solid((0.9, 0.2, 0.2, 1.0)), (-5, 13, -2), (8, 16, 8))
    b = scenes.build_box(scenes.solid((0.2, 0.8, 0.3, 1.0)), (6, 10, 3), (6, 10, 6))
    c = scenes.build_box(scenes.solid((0.2, 0.3, 0.9, 1.0)), (1, 24, 0), (4, 4, 4))
    return M.SceneDesc(scenes.simple_scene([slab, a, b, c], light=(12, 40, 25), radius=k))


# ---------------------------------------------------------------------------------------------------------------------
# the child: every scenario, RENDERS times on its handle
# ---------------------------------------------------------------------------------------------------------------------
def _child(out_path):
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi

    frames = {}

    def stream():
        return torch.cuda.current_stream().cuda_stream

    for name, (spec, kw, how) in SCENARIOS.items():
        cfg = M.Config(**kw)
        if how == "batch":
            hs = [M.DeviceScene(make_scene(("skin", k))) for k in spec[1]]
            for r in range(RENDERS):
                out = torch.zeros((len(hs), cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
                M.render_batch_device(hs, cfg, out.data_ptr(), 0, None, stream())
                torch.cuda.synchronize()
                for i, k in enumerate(spec[1]):
                    frames[f"{name}_p{k}_{r}"] = out[i].cpu().numpy()
            assert M.last_batch_info() == {"batched_frames": len(hs), "launch_sequences": 1}
            for ds in hs:
                ds.check()
            continue
        ds = M.DeviceScene(make_scene(spec))
        if how == "transparent":
            ds.set_background("transparent")
        for r in range(RENDERS):
            out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            if how == "packed":  # packed rows of the shards (0, 2) and (1, 2), scattered by unpack_rows
                for first in range(2):
                    rows = ds.owned_pixel_rows(cfg, first, 2)
                    packed = torch.zeros((max(rows, 1), cfg.width, 4), dtype=torch.float32, device="cuda")
                    ds.render_device(cfg, packed.data_ptr(), first, 2, abi.LAYOUT_PACKED, stream())
                    M.unpack_rows_device(cfg, first, 2, packed.data_ptr(), out.data_ptr(), stream())
                    torch.cuda.synchronize()
            elif how == "rgba8":
                out8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda")
                ds.render_device_ex(cfg, out.data_ptr(), out8.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
                torch.cuda.synchronize()
                frames[f"{name}8_{r}"] = out8.cpu().numpy()
            else:
                ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream())
                torch.cuda.synchronize()
            frames[f"{name}_{r}"] = out.cpu().numpy()
        ds.check()
    np.savez(out_path, **frames)


@pytest.fixture(scope="module")
def rendered(gpu, tmp_path_factory):
    """frames of every scenario under environment `env`: one child per environment, run when first asked for"""
    cache = {}

    def get(env_name):
        if env_name not in cache:
            out = str(tmp_path_factory.mktemp("param_views") / f"{env_name}.npz")
            e = dict(os.environ)
            for knob in ("MCRT_WORK_TICKETS", "MCRT_SHARED_GRIDS", "MCRT_PRIMARY_GRID", "MCRT_LIT_GRID", "MCRT_AO_GRID", "MCRT_RESOLVE_GRID", "MCRT_QUEUE_GRID",
                         "MCRT_BG_PLATE", "MCRT_DRAW_PLATE", "MCRT_WORKSPACE_MB"):
                e.pop(knob, None)
            e.update(ENVS[env_name])
            subprocess.run([sys.executable, os.path.abspath(__file__), out], env=e, check=True, timeout=300)
            z = np.load(out)
            cache[env_name] = {k: z[k] for k in z.files}
        return cache[env_name]

    return get


@pytest.fixture(scope="module")
def expected(oracle, tmp_path_factory):
    """the oracle's frame of a scenario (the transparent one: the checker's), each rendered once"""
    cache = {}

    def get(spec, kw, how):
        from minecraftskin_raytracer_amd import abi

        key = (spec, json.dumps(kw, sort_keys=True), how == "transparent")
        if key not in cache:
            if how == "transparent":
                import transparent_checker

                checker = transparent_checker.Checker(transparent_checker.build(str(tmp_path_factory.mktemp("transparent_checker"))))
                cache[key], _ = checker.render(make_scene(spec).ptr, abi.Config(**kw), threads=transparent_checker.threads())
            else:
                cache[key] = oracle.render(make_scene(spec).ptr, abi.Config(**kw))
        return cache[key]

    return get


def _check(name, frames, expected, oracle, env_name):
    import scenes

    spec, kw, how = SCENARIOS[name]
    for r in range(RENDERS):
        if how == "batch":
            for k in spec[1]:
                scenes.assert_bit_equal(frames[f"{name}_p{k}_{r}"], expected(("skin", k), kw, "plain"), f"{env_name}: {name}, pose {k}, call {r}")
            continue
        want = expected(spec, kw, how)
        scenes.assert_bit_equal(frames[f"{name}_{r}"], want, f"{env_name}: {name}, render {r}")
        if how == "rgba8":
            assert np.array_equal(frames[f"{name}8_{r}"], oracle.quantize(want).reshape(want.shape)), f"{env_name}: {name}, render {r}: RGBA8 plane"


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_every_phase_reads_its_parameters(rendered, expected, oracle, name):
    _check(name, rendered("defaults"), expected, oracle, "defaults")


@pytest.mark.parametrize("env_name", ["shared_grids", "grid5"])
def test_phases_reload_under_shared_and_tiny_grids(rendered, expected, oracle, env_name):
    """MCRT_SHARED_GRIDS=1: the grids sized for company.  Five workgroups per kernel: nearly every item is claimed by ticket,
    so a workgroup passes each phase's reload once per item, many times over."""
    frames = rendered(env_name)
    for name in SCENARIOS:
        _check(name, frames, expected, oracle, env_name)


if __name__ == "__main__":
    _child(sys.argv[1])
