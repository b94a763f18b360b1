"""What K extra lights cost on the device: the metric frame (1920x1080, 4 bounces, 4 spp, soft shadows) through

  K0_flat        no extra light, S = 8: the flat pipeline (`lit`)
  K0_general     no extra light, S = 114: the general variants' per-level launch sets, forced by the length of the per-hit stream
                 (note: 114 shadow rays per hit instead of 8 — the row says what the per-level pipeline costs at that S, not at S = 8)
  K0_general_b9  no extra light, S = 8, 9 bounces: the general variants forced by the depth instead (the extra levels hold few records)
  K1, K2, K3     1, 2, 3 extra lights, S = 8: the multi-light stages

the ways alternated in one process: a handle per way, events on the issuing stream (mcrt_time_render_device, 10 renders per
reading), warm-ups first, then repetitions with the order of the ways reversed every other time; median and min-max per way, ms
per frame.  Before the timing every K >= 1 frame is compared with the K = 0 frame: it must differ (the lights are on).

    python tools/gpu_extra_lights.py [--reps 9] [--warmup 3] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    a = ap.parse_args()
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    w, h = 1920, 1080
    sd = scenes.skin_scene("S64", 0)
    lights = [abi.Light((-30.0, 20.0, 30.0), (0.35, 0.4, 0.5, 1.0), 4.0), abi.Light((25.0, 5.0, 10.0), (0.9, 0.8, 0.6, 1.0), 3.0),
              abi.Light((0.0, -10.0, 25.0), (0.3, 0.1, 0.1, 1.0), 10.0)]
    base = dict(width=w, height=h, maxBounces=4, samplesPerPixel=4)
    ways = {"K0_flat": (0, abi.Config(**base)), "K0_general": (0, abi.Config(**base, shadowSamples=114)),
            "K0_general_b9": (0, abi.Config(**{**base, "maxBounces": 9})),
            "K1": (1, abi.Config(**base)), "K2": (2, abi.Config(**base)), "K3": (3, abi.Config(**base))}
    stream = torch.cuda.current_stream().cuda_stream
    handles, frames = {}, {}
    for name, (k, cfg) in ways.items():
        ds = M.DeviceScene(sd)
        ds.set_extra_lights(lights[:k])
        handles[name] = ds
        frames[name] = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        ds.render_device(cfg, frames[name].data_ptr(), stream=stream)
    torch.cuda.synchronize()
    for ds in handles.values():
        ds.check()
    for k in (1, 2, 3):
        assert not torch.equal(frames[f"K{k}"], frames["K0_flat"]), f"K{k}: the frame equals the single-light frame"
    times = {name: [] for name in ways}
    order = list(ways)
    for r in range(a.warmup + a.reps):
        for name in (order if r % 2 == 0 else order[::-1]):
            ms = handles[name].time_render_device(ways[name][1], frames[name].data_ptr(), a.iters, stream=stream)
            if r >= a.warmup:
                times[name].append(ms)
    for ds in handles.values():
        ds.check()
        ds.close()
    out = {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "readings": len(t)} for name, t in times.items()}
    lines = [f"{w}x{h}, 4 bounces (K0_general_b9: 9), 4 spp, pose 0; {a.iters} renders per reading, {a.warmup} warm-ups, {a.reps} readings per way, ms per frame",
             f"{'way':16s} {'median':>8s} {'min':>8s} {'max':>8s}   x K0_flat"]
    for name, o in out.items():
        lines.append(f"{name:16s} {o['median_ms']:8.3f} {o['min_ms']:8.3f} {o['max_ms']:8.3f}   {o['median_ms'] / out['K0_flat']['median_ms']:6.2f}")
    print("\n".join(lines))
    if a.txt:
        open(a.txt, "w").write("\n".join(lines) + "\n")
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
