"""Device time of the geometry layers (mcrt_render_layers_device & co) against what they are measured by, the ways of a
case alternated in one process: events on the issuing stream, warm-ups first, then repetitions with the order of the ways
reversed every other time; median and min-max per way.

  1080p      all four layers at 1920x1080, S64 pose 0, against the cheapest beauty frame of the same scene: 1 spp,
             0 bounces, soft shadows off, transparent background; and depth alone and id alone
  4k         all four layers at 3840x2160 (with the same beauty frame beside them)
  batch64    64 frames at 256x256 (the built-in poses) in one mcrt_render_layers_batch_device call against a loop of 64
             mcrt_render_layers_device calls; time per 64 frames
  pick       one mcrt_scene_pick of a single pixel, host to host (a host clock around the synchronous call)

    python tools/gpu_layers.py [--cases 1080p,4k,batch64,pick] [--reps 9] [--warmup 5] [--json out.json] [--timeout 240]

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
CASES = ("1080p", "4k", "batch64", "pick")


def measure(case, reps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    stream = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def planes(n, px, names):
        return {f"{k}_ptr": torch.zeros((n, px, abi.LAYER_FORMATS[k][1]), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
                for k in names}

    ways, note = {}, {}
    if case in ("1080p", "4k"):
        w, h = (1920, 1080) if case == "1080p" else (3840, 2160)
        sd = scenes.skin_scene("S64", 0)
        layers_h, beauty_h = M.DeviceScene(sd), M.DeviceScene(sd)
        beauty_h.set_background("transparent")
        lcfg = abi.Config(width=w, height=h)
        bcfg = abi.Config(width=w, height=h, samplesPerPixel=1, maxBounces=0, softShadows=False)
        frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        keep = [layers_h, beauty_h, frame]
        ways["beauty_cheapest"] = lambda: beauty_h.render_device(bcfg, frame.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
        for name, names in (("layers_all4", abi.LAYER_NAMES),) + ((("layers_depth", ("depth",)), ("layers_id", ("id",))) if case == "1080p" else ()):
            bufs = planes(1, w * h, names)
            keep.append(bufs)
            ways[name] = (lambda b: lambda: layers_h.render_layers_device(lcfg, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in b.items()}))(bufs)
    elif case == "batch64":
        cfg = abi.Config(width=256, height=256)
        hs = [M.DeviceScene(scenes.skin_scene("S64", k % 7)) for k in range(64)]
        bufs = planes(64, 256 * 256, abi.LAYER_NAMES)
        ptrs = {k: v.data_ptr() for k, v in bufs.items()}
        ways["batch_call"] = lambda: M.render_layers_batch_device(hs, cfg, stream=stream.cuda_stream, **ptrs)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.render_layers_device(cfg, stream=stream.cuda_stream, **{k: v[i].data_ptr() for k, v in bufs.items()})
        ways["loop_of_64"] = loop
    elif case == "pick":
        cfg = abi.Config(width=1920, height=1080)
        hnd = M.DeviceScene(scenes.skin_scene("S64", 0))
        xy = [[960, 400]]
        for _ in range(warmup):
            rec = hnd.pick(cfg, xy)
        ms = []
        for _ in range(max(reps, 1) * 5):
            a = time.perf_counter()
            hnd.pick(cfg, xy)
            ms.append((time.perf_counter() - a) * 1e3)
        return {"case": case, "pick_one_pixel_host_to_host": {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "calls": len(ms)},
                "picked_mesh": int(rec["mesh"][0])}
    else:
        raise SystemExit(f"unknown case {case}")
    names = list(ways)
    for _ in range(warmup):
        for n in names:
            ways[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for r in range(reps):
        for n in (names if r % 2 == 0 else names[::-1]):
            t0.record(stream)
            ways[n]()
            t1.record(stream)
            t1.synchronize()
            times[n].append(t0.elapsed_time(t1))
    row = {"case": case, "reps": reps, "warmup": warmup}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    if "beauty_cheapest" in row:
        row["layers_all4_over_beauty"] = row["layers_all4"]["ms_median"] / row["beauty_cheapest"]["ms_median"]
    if "batch_call" in row:
        row["batch_over_loop"] = row["batch_call"]["ms_median"] / row["loop_of_64"]["ms_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps, a.warmup)), flush=True)
        return
    results = []
    for case in a.cases.split(","):
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                 capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{case}: no result within {a.timeout} s — nothing further is started")
        rows = [ln[7:] for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not rows:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit(f"{case}: exit status {out.returncode} — nothing further is started")
        row = json.loads(rows[-1])
        results.append(row)
        for k, v in row.items():
            if isinstance(v, dict) and "ms_median" in v:
                print(f"{case:8s} {k:28s} {v['ms_median']:9.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})", flush=True)
            elif k.endswith(("_over_beauty", "_over_loop")):
                print(f"{case:8s} {k:28s} {v:9.3f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
