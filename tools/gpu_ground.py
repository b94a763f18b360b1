"""Device time of the ground-shadow pass (mcrt_render_ground_device & co) against what it is measured by, the ways of a case
alternated in one process: events on the issuing stream, warm-ups first, then repetitions with the order of the ways reversed
every other time; median and min-max per way.

  1080p_pose0, 1080p_pose6, 4k_pose0, 4k_pose6
             all three ground planes at the scene's floor, S = 8, S64, against the four-plane layers pass of the same frame
             and against the cheapest beauty frame that computes soft shadows at all (1 spp, 0 bounces, soft shadows with 8
             samples, transparent background); and, in a second child process with MCRT_BUNDLE_DECISIONS=0 (the knob is read
             once per process), the ground pass with every reached pixel's rays traced — what the decisions buy.  With them the
             shares of the reached pixels that are fully lit, dark and in the penumbra, and — in a third child process on the
             class variant of the library (below) — the shares of the reached pixels culled by tile, decided and traced
  variants_pose0, variants_pose6
             the pass at 1920x1080 by tile size (32, 16, 8: the culling's granularity), with the matte alone, and with soft
             shadows off (one ray per pixel, no sample positions)
  batch64    64 frames at 256x256 (the built-in poses) in one mcrt_render_ground_batch_device call against a loop of 64
             mcrt_render_ground_device calls; time per 64 frames

    python tools/gpu_ground.py --build-variant      (no GPU needed)
    python tools/gpu_ground.py [--cases 1080p_pose0,...] [--reps 9] [--warmup 5] [--json out.json] [--timeout 240]

The pass keeps no counters.  --build-variant compiles variants/ground_class.so, the library with tools/ground_class_hooks.h, in
which the pass writes each pixel's class into the visibility plane (0 missed, 1 culled by tile, 2 decided, 3 traced); the
size cases count the codes when that file exists and say so when it does not.

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("1080p_pose0", "1080p_pose6", "4k_pose0", "4k_pose6", "batch64", "variants_pose0", "variants_pose6")
VARIANT = os.path.join(ROOT, "variants", "ground_class.so")


def build_variant():
    sys.path.insert(0, ROOT)
    from minecraftskin_raytracer_amd.build import build

    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    build(force=True, out=VARIANT, extra_flags=[f"-I{ROOT}/tools", '-DMCRT_KERNEL_HOOKS="ground_class_hooks.h"'])
    print(VARIANT)


def measure(case, reps, warmup, ground_only):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    stream = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def ground_planes(n, px):
        return {"visibility_ptr": torch.zeros((n, px), dtype=torch.float32, device="cuda"), "distance_ptr": torch.zeros((n, px), dtype=torch.float32, device="cuda"),
                "matte_ptr": torch.zeros((n, px), dtype=torch.uint8, device="cuda")}

    ways, extra = {}, {}
    if case.startswith("variants_"):
        w, h = 1920, 1080
        sd = scenes.skin_scene("S64", int(case[-1]))
        floor = M.scene_floor(sd)
        pass_h = M.DeviceScene(sd)
        gb = ground_planes(1, w * h)
        ptrs = {k: v.data_ptr() for k, v in gb.items()}
        for tile in (32, 16, 8):
            cfg_t = abi.Config(width=w, height=h, tileSize=tile)
            ways[f"tile{tile}_3planes"] = (lambda c: lambda: pass_h.render_ground_device(c, floor, stream=stream.cuda_stream, **ptrs))(cfg_t)
        cfg32, hard = abi.Config(width=w, height=h), abi.Config(width=w, height=h, softShadows=False)
        ways["tile32_matte_only"] = lambda: pass_h.render_ground_device(cfg32, floor, matte_ptr=ptrs["matte_ptr"], stream=stream.cuda_stream)
        ways["tile32_soft_shadows_off"] = lambda: pass_h.render_ground_device(hard, floor, stream=stream.cuda_stream, **ptrs)
    elif case != "batch64":
        size, pose = case.split("_pose")
        w, h = (1920, 1080) if size == "1080p" else (3840, 2160)
        sd = scenes.skin_scene("S64", int(pose))
        floor = M.scene_floor(sd)
        pass_h, beauty_h = M.DeviceScene(sd), M.DeviceScene(sd)
        beauty_h.set_background("transparent")
        gcfg = abi.Config(width=w, height=h)  # soft shadows, 8 samples
        bcfg = abi.Config(width=w, height=h, samplesPerPixel=1, maxBounces=0)
        gb = ground_planes(1, w * h)
        keep = [pass_h, beauty_h, gb]
        ways["ground"] = lambda: pass_h.render_ground_device(gcfg, floor, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in gb.items()})
        if not ground_only:
            frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            lb = {f"{k}_ptr": torch.zeros((w * h, abi.LAYER_FORMATS[k][1]), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
                  for k in abi.LAYER_NAMES}
            keep += [frame, lb]
            ways["layers_all4"] = lambda: pass_h.render_layers_device(gcfg, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in lb.items()})
            ways["beauty_soft_cheapest"] = lambda: beauty_h.render_device(bcfg, frame.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
        extra["floor"] = floor
        if os.environ.get("MCRT_LIB") == VARIANT:  # the class variant: count the codes of one pass, no timing
            ways["ground"]()
            torch.cuda.synchronize()
            code = gb["visibility_ptr"][0].cpu().numpy()
            n = max(int((code > 0).sum()), 1)
            return {"case": case, "reached_pixels": int((code > 0).sum()), "share_culled_by_tile": float((code == 1).sum()) / n,
                    "share_decided": float((code == 2).sum()) / n, "share_traced": float((code == 3).sum()) / n}
    else:
        cfg = abi.Config(width=256, height=256)
        sds = [scenes.skin_scene("S64", k % 7) for k in range(64)]
        floors = [M.scene_floor(sd) for sd in sds]
        hs = [M.DeviceScene(sd) for sd in sds]
        gb = ground_planes(64, 256 * 256)
        ptrs = {k: v.data_ptr() for k, v in gb.items()}
        ways["batch_call"] = lambda: M.render_ground_batch_device(hs, cfg, floors, stream=stream.cuda_stream, **ptrs)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.render_ground_device(cfg, floors[i], stream=stream.cuda_stream, **{k: v[i].data_ptr() for k, v in gb.items()})
        ways["loop_of_64"] = loop
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
    row = {"case": case, "reps": reps, "warmup": warmup, "bundle_decisions": os.environ.get("MCRT_BUNDLE_DECISIONS", "1"), **extra}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    if case != "batch64" and not case.startswith("variants_"):
        vis = gb["visibility_ptr"][0].cpu().numpy()
        reached = gb["distance_ptr"][0].cpu().numpy() < np.finfo(np.float32).max
        n_reached = max(int(reached.sum()), 1)
        row["reached_pixels"] = int(reached.sum())
        row["share_fully_lit"] = float((reached & (vis == 1)).sum()) / n_reached
        row["share_dark"] = float((reached & (vis == 0)).sum()) / n_reached
        row["share_penumbra"] = float((reached & (vis > 0) & (vis < 1)).sum()) / n_reached
    if "layers_all4" in row:
        row["ground_over_layers"] = row["ground"]["ms_median"] / row["layers_all4"]["ms_median"]
        row["ground_over_beauty"] = row["ground"]["ms_median"] / row["beauty_soft_cheapest"]["ms_median"]
    if "batch_call" in row:
        row["batch_over_loop"] = row["batch_call"]["ms_median"] / row["loop_of_64"]["ms_median"]
    return row


def child(case, a, env=None, ground_only=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--warmup", str(a.warmup)]
    if ground_only:
        cmd.append("--ground-only")
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
    ap.add_argument("--ground-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--build-variant", action="store_true", help="compile variants/ground_class.so and exit")
    a = ap.parse_args()
    if a.build_variant:
        build_variant()
        return
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps, a.warmup, a.ground_only)), flush=True)
        return
    results = []
    for case in a.cases.split(","):
        row = child(case, a)
        if case != "batch64" and not case.startswith("variants_"):
            if os.path.exists(VARIANT):
                classes = child(case, a, env=dict(os.environ, MCRT_LIB=VARIANT), ground_only=True)
                assert classes["reached_pixels"] == row["reached_pixels"]
                row.update({k: v for k, v in classes.items() if k.startswith("share_")})
            else:
                print(f"{case}: {VARIANT} is missing (--build-variant): the shares culled, decided and traced are not counted", flush=True)
            traced = child(case, a, env=dict(os.environ, MCRT_BUNDLE_DECISIONS="0"), ground_only=True)
            row["ground_without_decisions"] = traced["ground"]
            row["decisions_speedup"] = traced["ground"]["ms_median"] / row["ground"]["ms_median"]
        results.append(row)
        for k, v in row.items():
            if isinstance(v, dict) and "ms_median" in v:
                print(f"{case:12s} {k:28s} {v['ms_median']:9.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})", flush=True)
            elif k.startswith(("share_", "ground_over_", "batch_over_", "decisions_")):
                print(f"{case:12s} {k:28s} {v:9.3f}", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
