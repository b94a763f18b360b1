"""A fixed run of the ground-occlusion fuzz (tests/ground_occlusion_fuzz_cases.py) on the GPU: a few dozen seeds and a few batches,
every plane bit for bit against the CPU oracle alone.  ``run_case`` and ``run_batch`` are what tools/gpu_fuzz.py (mode
ground_occlusion) runs per seed in its long sweeps; they return the mismatches as lines."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ground_occlusion_checker as GO  # noqa: E402
import ground_occlusion_fuzz_cases as F  # noqa: E402

gpu_test = pytest.mark.gpu
SEEDS = range(0, 36)
BATCH_SEEDS = range(0, 6)


def differing(got: dict, exp: dict, what: str) -> list:
    """One line per plane that is not bit for bit the expectation's."""
    out = []
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        ne = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype == np.float32 else (a != b)
        if ne.any():
            y, x = np.argwhere(ne)[0]
            out.append(f"MISMATCH {what}: plane {k}: {int(ne.sum())} pixels differ; first (y, x) = ({y}, {x}): {got[k][y, x]} vs {exp[k][y, x]}")
    return out


def run_case(M, oracle, seed: int) -> tuple:
    """(mismatch lines, reached pixels, pixels with occlusion < 1) of one seed: the host form, and for every third seed the
    device form into planes 4 bytes / 1 byte off their allocation."""
    sd, cfg, ground, what, _ = F.make_case(seed)
    exp = GO.expected_ground_occlusion(oracle, sd, cfg, ground)
    lines = differing(M.TileRenderer.renderGroundOcclusion(sd, cfg, ground), exp, what)
    if seed % 3 == 0:
        px = cfg.width * cfg.height
        occ = torch.full((px + 8,), -7.0, dtype=torch.float32, device="cuda")
        matte = torch.full((px + 8,), 99, dtype=torch.uint8, device="cuda")
        ds = M.DeviceScene(sd)
        try:
            ds.render_ground_occlusion_device(cfg, ground, occlusion_ptr=occ.data_ptr() + 4, matte_ptr=matte.data_ptr() + 1,
                                              stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ds.check()
        finally:
            ds.close()
        got = {"occlusion": occ.cpu().numpy()[1:px + 1].reshape(cfg.height, cfg.width), "matte": matte.cpu().numpy()[1:px + 1].reshape(cfg.height, cfg.width)}
        lines += differing(got, exp, what + " | device form, planes off their alignment")
        if occ[0].item() != -7.0 or not bool((occ[px + 1:] == -7.0).all()) or matte[0].item() != 99 or not bool((matte[px + 1:] == 99).all()):
            lines.append(f"MISMATCH {what}: a pixel outside the frame was written")
    return lines, int(exp["reached"].sum()), int((exp["occlusion"] < 1).sum())


def run_batch(M, oracle, seed: int) -> tuple:
    """(mismatch lines, frames) of one batch seed: scenes and heights mixed under one config, frames a stride apart."""
    sds, cfg, heights, what = F.make_batch(seed)
    exps = [GO.expected_ground_occlusion(oracle, sd, cfg, g) for sd, g in zip(sds, heights)]
    n, px = len(sds), cfg.width * cfg.height
    stride = px + 37
    occ = torch.full((n, stride), -7.0, dtype=torch.float32, device="cuda")
    matte = torch.full((n, stride), 99, dtype=torch.uint8, device="cuda")
    handles = [M.DeviceScene(sd) for sd in sds]
    lines = []
    try:
        M.render_ground_occlusion_batch_device(handles, cfg, heights, occlusion_ptr=occ.data_ptr(), matte_ptr=matte.data_ptr(), frame_stride_pixels=stride,
                                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()
    o, m = occ.cpu().numpy(), matte.cpu().numpy()
    for i in range(n):
        got = {"occlusion": o[i, :px].reshape(cfg.height, cfg.width), "matte": m[i, :px].reshape(cfg.height, cfg.width)}
        lines += differing(got, exps[i], f"{what} | frame {i}")
    if not (o[:, px:] == -7.0).all() or not (m[:, px:] == 99).all():
        lines.append(f"MISMATCH {what}: the pixels between two frames were written")
    return lines, n


@gpu_test
def test_fixed_seeds_equal_the_oracle(mcrt, gpu, oracle):
    bad, reached, occluded = [], 0, 0
    for seed in SEEDS:
        lines, r, o = run_case(mcrt, oracle, seed)
        bad += lines
        reached += r
        occluded += o
    print(f"{len(SEEDS)} seeds: the oracle holds {reached} reached pixels, {occluded} of them with occlusion < 1")
    assert occluded >= 100  # the seeds have something to get wrong
    assert not bad, "\n".join(bad[:20])


@gpu_test
def test_fixed_batches_equal_the_oracle(mcrt, gpu, oracle):
    bad, frames = [], 0
    for seed in BATCH_SEEDS:
        lines, n = run_batch(mcrt, oracle, seed)
        bad += lines
        frames += n
    print(f"{len(BATCH_SEEDS)} batches, {frames} frames")
    assert not bad, "\n".join(bad[:20])
