"""Frames/s of N frames rendered three ways, on the device (hipEvents on the issuing stream), after warm-up, repeated with
the order of the ways alternated:

  batch   mcrt_render_batch_device: N handles, one launch sequence (or a few) on one stream
  loop    mcrt_render_device on the same N handles, one after the other on one stream
  four    four handles in flight on four streams, frame k on handle k % 4 (how bench.py measures `value`)

    python tools/gpu_batch.py [--cases default1,default8,default64,default256,turntable36] [--modes batch,loop,four]
                              [--reps 7] [--json out.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import minecraftskin_raytracer_amd as M  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402
import scenes  # noqa: E402

DEFAULT = dict()  # the reference's default Config: 256x256, 3 bounces, 1 spp, tile 32
TURNTABLE = dict(width=512, height=512, maxBounces=3, samplesPerPixel=4)
CASES = {"default1": (DEFAULT, 1, False), "default8": (DEFAULT, 8, False), "default64": (DEFAULT, 64, False),
         "default256": (DEFAULT, 256, False), "turntable36": (TURNTABLE, 36, True)}


def scene_list(n, turntable):
    out = []
    for k in range(n):
        sd = scenes.skin_scene("S64", k % 7)
        if turntable:  # N cameras around one figure
            a = 2.0 * math.pi * k / n
            d = sd.desc
            d.camera_position[0], d.camera_position[2] = 40.0 * math.sin(a), 40.0 * math.cos(a)
        out.append(sd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--modes", default="batch,loop,four")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    modes = a.modes.split(",")
    results = []
    for case in a.cases.split(","):
        kw, n, turntable = CASES[case]
        cfg = abi.Config(**kw)
        px = cfg.width * cfg.height
        handles = [M.DeviceScene(sd) for sd in scene_list(n, turntable)]
        out = torch.zeros((n, px, 4), dtype=torch.float32, device="cuda")
        ref = torch.zeros_like(out)
        main_stream = torch.cuda.current_stream()
        side = [torch.cuda.Stream() for _ in range(4)]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def run(mode, dst):
            if mode == "batch":
                M.render_batch_device(handles, cfg, dst.data_ptr(), 0, px, main_stream.cuda_stream)
            elif mode == "loop":
                for i, h in enumerate(handles):
                    h.render_device(cfg, dst[i].data_ptr(), 0, 1, abi.LAYOUT_FRAME, main_stream.cuda_stream)
            else:  # four frames in flight: handle k % 4 on stream k % 4
                for s in side:
                    s.wait_stream(main_stream)
                for i in range(n):
                    handles[i % 4].render_device(cfg, dst[i].data_ptr(), 0, 1, abi.LAYOUT_FRAME, side[i % 4].cuda_stream)
                for s in side:
                    main_stream.wait_stream(s)

        run("loop", ref)
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for m in modes:
            for _ in range(a.warmup):
                run(m, out)
            torch.cuda.synchronize()
            if m == "batch":
                info = M.last_batch_info()
            out.zero_()
            run(m, out)
            torch.cuda.synchronize()
            want = ref if m != "four" else ref[torch.arange(n, device="cuda") % min(n, 4)]  # frame k of `four` shows handle k % 4's scene
            if not torch.equal(out, want):
                raise SystemExit(f"{case}: {m} differs from the single renders")
        for r in range(a.reps):
            order = modes if r % 2 == 0 else modes[::-1]
            for m in order:
                t0.record(main_stream)
                run(m, out)
                t1.record(main_stream)
                t1.synchronize()
                times[m].append(t0.elapsed_time(t1))
        row = {"case": case, "n": n, "config": kw, "batch_info": info if "batch" in modes else None}
        for m in modes:
            ms = times[m]
            med = statistics.median(ms)
            row[m] = {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "frames_per_s": n / (med / 1e3)}
        results.append(row)
        line = f"{case:12s} N={n:4d}"
        for m in modes:
            r = row[m]
            line += f"  {m} {r['frames_per_s']:9.0f} f/s ({r['ms_median']:.3f} ms, {r['ms_min']:.3f}-{r['ms_max']:.3f})"
        if "batch" in modes and "loop" in modes:
            line += f"  batch/loop x{row['loop']['ms_median'] / row['batch']['ms_median']:.2f}"
        print(line, flush=True)
        for h in handles:
            h.close()
        del out, ref
        torch.cuda.synchronize()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
