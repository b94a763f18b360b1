"""Device time of reference mode against transparent mode (MCRT_BACKGROUND_TRANSPARENT) on the same workloads, in one
process: events on the issuing stream, warm-ups first, then repetitions with the order of the two modes alternated;
median and min-max per mode.  Each mode renders with handles of its own (each keeps its recorded graphs).

  metric1    1920x1080 / 4 bounces / 4 spp, S64 — one frame alone
  metric4    the same, four frames in flight (four handles on four streams, bench.py's way); time per frame
  gui        the reference GUI's defaults: 1920x1080, 4 bounces, 64 spp, AO 16, depth of field 0.3
  4k         3840x2160 / 8 bounces / 16 spp
  8k         7680x4320 / 8 bounces / 64 spp, S32
  batch64    64 frames of the default 256x256 Config in one mcrt_render_batch_device call; time per call

    python tools/gpu_transparent.py [--cases metric1,metric4,gui,4k,8k,batch64] [--modes reference,transparent] [--reps 9]
                                    [--warmup 3] [--json out.json]
(--modes with one mode: a run of its own for a kernel trace of that mode)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # four frames in flight need more than the runtime's 4 queues (bench.py)
import torch  # noqa: E402

import minecraftskin_raytracer_amd as M  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402
import scenes  # noqa: E402

MODES = ("reference", "transparent")
CASES = {  # name: (Config fields, skin, frames in flight, batch size)
    "metric1": (dict(width=1920, height=1080, maxBounces=4, samplesPerPixel=4), "S64", 1, 0),
    "metric4": (dict(width=1920, height=1080, maxBounces=4, samplesPerPixel=4), "S64", 4, 0),
    "gui": (dict(width=1920, height=1080, maxBounces=4, samplesPerPixel=64, aoEnabled=True, aoSamples=16, dofEnabled=True, aperture=0.3), "S64", 1, 0),
    "4k": (dict(width=3840, height=2160, maxBounces=8, samplesPerPixel=16), "S64", 1, 0),
    "8k": (dict(width=7680, height=4320, maxBounces=8, samplesPerPixel=64), "S32", 1, 0),
    "batch64": (dict(), "S64", 1, 64),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    modes = tuple(a.modes.split(","))
    results = []
    main_stream = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for case in a.cases.split(","):
        kw, skin, fif, batch = CASES[case]
        cfg = abi.Config(**kw)
        px = cfg.width * cfg.height
        n_handles = batch if batch else fif
        handles, outs = {}, {}
        for m in modes:
            handles[m] = [M.DeviceScene(scenes.skin_scene(skin, k % 7 if batch else 0)) for k in range(n_handles)]
            for h in handles[m]:
                h.set_background(m)
                if fif > 1:
                    h.set_lanes(1)  # as bench.py: the frames in flight already fill the chip
            outs[m] = torch.zeros((n_handles, px, 4), dtype=torch.float32, device="cuda")
        side = [torch.cuda.Stream() for _ in range(fif)]
        per_call = 2 * fif if fif > 1 else 1  # frames per timed call

        def run(m):
            hs, out = handles[m], outs[m]
            if batch:
                M.render_batch_device(hs, cfg, out.data_ptr(), 0, px, main_stream.cuda_stream)
            elif fif == 1:
                hs[0].render_device(cfg, out[0].data_ptr(), 0, 1, abi.LAYOUT_FRAME, main_stream.cuda_stream)
            else:
                for s in side:
                    s.wait_stream(main_stream)
                for i in range(per_call):
                    hs[i % fif].render_device(cfg, out[i % fif].data_ptr(), 0, 1, abi.LAYOUT_FRAME, side[i % fif].cuda_stream)
                for s in side:
                    main_stream.wait_stream(s)

        for _ in range(a.warmup):
            for m in modes:
                run(m)
        torch.cuda.synchronize()
        info = {}
        if batch:
            for m in modes:
                run(m)
                torch.cuda.synchronize()
                info[m] = M.last_batch_info()
        transparent_share = float((outs["transparent"][..., 3] == 0).float().mean()) if "transparent" in outs else None  # pixels without a hit
        times = {m: [] for m in modes}
        for r in range(a.reps):
            for m in (modes if r % 2 == 0 else modes[::-1]):
                t0.record(main_stream)
                run(m)
                t1.record(main_stream)
                t1.synchronize()
                times[m].append(t0.elapsed_time(t1))
        row = {"case": case, "config": kw, "skin": skin, "frames_in_flight": fif, "batch": batch, "frames_per_call": batch or per_call,
               "reps": a.reps, "warmup": a.warmup, "batch_info": info or None,
               "transparent_pixel_share": transparent_share}
        for m in modes:
            ms = times[m]
            row[m] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms,
                      "ms_per_frame": statistics.median(ms) / (batch or per_call)}
        if len(modes) == 2:
            row["transparent_over_reference"] = row["transparent"]["ms_median"] / row["reference"]["ms_median"]
        results.append(row)
        line = f"{case:8s}"
        for m in modes:
            r = row[m]
            line += f"  {m} {r['ms_median']:8.3f} ms ({r['ms_min']:.3f}-{r['ms_max']:.3f})"
        if len(modes) == 2:
            line += f"  transparent/reference {row['transparent_over_reference']:.3f}  empty={transparent_share:.2f}"
        print(line, flush=True)
        for m in modes:
            for h in handles[m]:
                h.check()
                h.close()
        del outs
        torch.cuda.synchronize()
        M.trim()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
