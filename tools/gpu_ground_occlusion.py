"""Device time of the ground-occlusion pass (mcrt_render_ground_occlusion_device & co) and of the studio shot with its
floor-occlusion term, the ways of a case alternated in one process: events on the issuing stream, warm-ups first, then
repetitions with the order of the ways reversed every other time; median and min-max per way.

  1080p, 4k  both planes of the S64 figure (pose 0) at ground_y = 0 with 8 and with 64 samples, radius 3, next to all three planes
             of the ground-shadow pass of the same frame; with them — in a second child process on the class variant of the
             library (below) — the share of the tiles culled, the pixels traced, and the rays they make (traced pixels x A)
  batch64    64 frames at 256x256 (the built-in poses) in one mcrt_render_ground_occlusion_batch_device call against a loop of 64
             single calls, 8 samples; time per 64 frames
  shots64    SkinBatch.shots of 64 skins at 96x96 with floorOcclusion 0 and 0.5; time per call, host to host

    python tools/gpu_ground_occlusion.py --build-variant      (no GPU needed)
    python tools/gpu_ground_occlusion.py [--cases 1080p,...] [--reps 9] [--warmup 5] [--json out.json] [--timeout 240]
    python tools/gpu_ground_occlusion.py --pictures DIR       the default S64 figure's shot at ground 0 with floorOcclusion 0 and
                                                              0.5 as DIR/shot_without.png, DIR/shot_with.png and both side by side
                                                              (kept as tests/golden/ground_occlusion_shot_*.png)

The pass keeps no counters.  --build-variant compiles variants/ground_occlusion_class.so, the library with
tools/ground_occlusion_class_hooks.h, in which the pass writes each pixel's class into the occlusion plane (0 missed, 1 culled by
tile, 2 without a candidate, 3 traced); the size cases count the codes when that file exists and say so when it does not.

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("1080p", "4k", "batch64", "shots64")
VARIANT = os.path.join(ROOT, "variants", "ground_occlusion_class.so")
SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160)}


def build_variant():
    sys.path.insert(0, ROOT)
    from minecraftskin_raytracer_amd.build import build

    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    build(force=True, out=VARIANT, extra_flags=[f"-I{ROOT}/tools", '-DMCRT_KERNEL_HOOKS="ground_occlusion_class_hooks.h"'])
    print(VARIANT)


def write_png(path, rgba8):
    """(H, W, 4) uint8 → a deflated PNG (colour type 6): the library's writer stores the pixels uncompressed, and these
    pictures are kept in the repository."""
    import struct
    import zlib

    import numpy as np

    h, w = rgba8.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(rgba8, np.uint8).reshape(h, w * 4)], axis=1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 9)) + chunk(b"IEND", b""))


def pictures(directory):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    os.makedirs(directory, exist_ok=True)
    sd = scenes.skin_scene("S64", 0)
    cfg = abi.Config(width=480, height=360, samplesPerPixel=4, maxBounces=2, aoSamples=64, aoRadius=3.0)  # (tests/ground_occlusion_checker.py: golden_shot_config)
    without = M.TileRenderer.renderShot(sd, cfg, abi.Shot(), ground=0.0)
    with_term = M.TileRenderer.renderShot(sd, cfg, abi.Shot(floorOcclusion=0.5), ground=0.0)
    changed = (without != with_term).any(axis=-1)
    write_png(os.path.join(directory, "shot_without.png"), without)
    write_png(os.path.join(directory, "shot_with.png"), with_term)
    write_png(os.path.join(directory, "shot_side_by_side.png"), np.concatenate([without, with_term], axis=1))
    print(f"pictures: {cfg.width}x{cfg.height}, {int(changed.sum())} pixels darker with floorOcclusion 0.5; the largest drop of a channel "
          f"{int((without.astype(int) - with_term.astype(int)).max())} of 255")


def measure(case, reps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    stream = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ways, extra, host_timed = {}, {}, False
    if case in SIZES:
        w, h = SIZES[case]
        sd = scenes.skin_scene("S64", 0)
        hnd = M.DeviceScene(sd)
        occ = torch.zeros((w * h,), dtype=torch.float32, device="cuda")
        matte = torch.zeros((w * h,), dtype=torch.uint8, device="cuda")
        dist = torch.zeros((w * h,), dtype=torch.float32, device="cuda")
        cfgs = {a: abi.Config(width=w, height=h, aoSamples=a, aoRadius=3.0) for a in (8, 64)}
        if os.environ.get("MCRT_LIB") == VARIANT:  # the class variant: count the codes of one pass, no timing
            hnd.render_ground_occlusion_device(cfgs[8], 0.0, occlusion_ptr=occ.data_ptr(), stream=stream.cuda_stream)
            torch.cuda.synchronize()
            code = occ.cpu().numpy().reshape(h, w)
            tile = cfgs[8].tileSize
            tiles = [(code[y:y + tile, x:x + tile]) for y in range(0, h, tile) for x in range(0, w, tile)]
            culled = sum(1 for t in tiles if not ((t == 2) | (t == 3)).any())  # no pixel of the tile got as far as its candidates
            return {"case": case, "tiles": len(tiles), "tiles_culled_or_missed": culled, "share_tiles_culled_or_missed": culled / len(tiles),
                    "reached_pixels": int((code > 0).sum()), "pixels_in_kept_tiles_without_candidate": int((code == 2).sum()), "traced_pixels": int((code == 3).sum()),
                    "share_pixels_traced": float((code == 3).sum()) / (w * h)}
        for a in (8, 64):
            ways[f"occlusion_A{a}"] = (lambda c: lambda: hnd.render_ground_occlusion_device(c, 0.0, occlusion_ptr=occ.data_ptr(), matte_ptr=matte.data_ptr(),
                                                                                             stream=stream.cuda_stream))(cfgs[a])
        gcfg = abi.Config(width=w, height=h)  # soft shadows, 8 samples
        ways["ground_shadow_S8"] = lambda: hnd.render_ground_device(gcfg, 0.0, visibility_ptr=occ.data_ptr(), distance_ptr=dist.data_ptr(), matte_ptr=matte.data_ptr(),
                                                                    stream=stream.cuda_stream)
    elif case == "batch64":
        cfg = abi.Config(width=256, height=256, aoSamples=8, aoRadius=3.0)
        sds = [scenes.skin_scene("S64", k % 7) for k in range(64)]
        hs = [M.DeviceScene(sd) for sd in sds]
        occ = torch.zeros((64, 256 * 256), dtype=torch.float32, device="cuda")
        matte = torch.zeros((64, 256 * 256), dtype=torch.uint8, device="cuda")
        ways["batch_call"] = lambda: M.render_ground_occlusion_batch_device(hs, cfg, 0.0, occlusion_ptr=occ.data_ptr(), matte_ptr=matte.data_ptr(), stream=stream.cuda_stream)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.render_ground_occlusion_device(cfg, 0.0, occlusion_ptr=occ[i].data_ptr(), matte_ptr=matte[i].data_ptr(), stream=stream.cuda_stream)
        ways["loop_of_64"] = loop
    else:  # shots64: host to host, wall clock around the call (it synchronises itself)
        host_timed = True
        cfg = abi.Config(width=96, height=96, samplesPerPixel=4, maxBounces=2, aoSamples=8, aoRadius=3.0)
        skins = np.stack([M.synthetic_skin("S64", seed=k + 1) for k in range(64)])
        batch = M.SkinBatch(64, "S64")
        ways["shots_floor_occlusion_0"] = lambda: batch.shots(skins, cfg, abi.Shot(), ground=0.0)
        ways["shots_floor_occlusion_0.5"] = lambda: batch.shots(skins, cfg, abi.Shot(floorOcclusion=0.5), ground=0.0)
    names = list(ways)
    for _ in range(warmup):
        for n in names:
            ways[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for r in range(reps):
        for n in (names if r % 2 == 0 else names[::-1]):
            if host_timed:
                a = time.perf_counter()
                ways[n]()
                times[n].append((time.perf_counter() - a) * 1e3)
            else:
                t0.record(stream)
                ways[n]()
                t1.record(stream)
                t1.synchronize()
                times[n].append(t0.elapsed_time(t1))
    row = {"case": case, "reps": reps, "warmup": warmup, "clock": "host wall clock around the call" if host_timed else "device events", **extra}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    if "batch_call" in row:
        row["batch_over_loop"] = row["batch_call"]["ms_median"] / row["loop_of_64"]["ms_median"]
    if "ground_shadow_S8" in row:
        row["occlusion_A8_over_ground_shadow"] = row["occlusion_A8"]["ms_median"] / row["ground_shadow_S8"]["ms_median"]
    return row


def child(case, a, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--warmup", str(a.warmup)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, env=env)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"{case}: no result within {a.timeout} s — nothing further is started")
    rows = [ln[7:] for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not rows:
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"{case}: exit status {out.returncode} — nothing further is started")
    return json.loads(rows[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--build-variant", action="store_true", help="compile variants/ground_occlusion_class.so and exit")
    ap.add_argument("--pictures", default="", help="write the two shots of the default figure into this directory and exit")
    a = ap.parse_args()
    if a.build_variant:
        build_variant()
        return
    if a.pictures:
        pictures(a.pictures)
        return
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps, a.warmup)), flush=True)
        return
    results = []
    for case in a.cases.split(","):
        row = child(case, a)
        if case in SIZES:
            if os.path.exists(VARIANT):
                row.update({k: v for k, v in child(case, a, env=dict(os.environ, MCRT_LIB=VARIANT)).items() if k != "case"})
                for s in (8, 64):  # rays per microsecond of the pass: traced pixels x A against the time
                    row[f"rays_A{s}"] = row["traced_pixels"] * s
                    row[f"rays_per_us_A{s}"] = row["traced_pixels"] * s / (row[f"occlusion_A{s}"]["ms_median"] * 1e3)
            else:
                print(f"{case}: {VARIANT} is missing (--build-variant): the tiles culled and the pixels traced are not counted", flush=True)
        results.append(row)
        for k, v in row.items():
            if isinstance(v, dict) and "ms_median" in v:
                print(f"{case:8s} {k:34s} {v['ms_median']:9.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})", flush=True)
            elif k.startswith(("share_", "batch_over_", "occlusion_A8_over", "traced_", "tiles", "rays_", "reached_", "pixels_")):
                print(f"{case:8s} {k:34s} {v:12.4f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
