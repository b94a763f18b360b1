"""Device time of the light layers (mcrt_render_light_device & co) against what they are measured by, the ways of a case
alternated in one process: events on the issuing stream, warm-ups first, then repetitions with the order of the ways reversed
every other time; median and min-max per way.

  1080p_pose0, 1080p_pose6, 4k_pose0, 4k_pose6
             the S64 figure, S = 8, A = 8, radius 3: all three planes, visibility + direct alone (the `shade` kernel), occlusion
             alone (the `occlusion` kernel); beside them, for context, the ground pass at y = 0, the four geometry layers, and the
             transparent 1 spp / 0-bounce beauty frame — the only other way to `direct` — without and with ambient occlusion.
             With them the hits of the frame.  The case first checks the recomposition on the frame: the beauty frame equals
             `direct` on the hits, and the AO frame the recomposed planes
  batch64    64 frames at 256x256 (the built-in poses) in one mcrt_render_light_batch_device call against a loop of 64
             mcrt_render_light_device calls; time per 64 frames.  The case first checks that both ways give the same bytes, and
             FAILS (exit status 1) unless the batch's range lies below the loop's: one launch sequence against 64 is the reason
             the batched form exists

    python tools/gpu_light.py [--cases 1080p_pose0,...] [--reps 9] [--warmup 5] [--json out.json] [--txt out.txt] [--timeout 240]

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("1080p_pose0", "1080p_pose6", "4k_pose0", "4k_pose6", "batch64")
GROUND = 0.0


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

    def light_planes(n, px):
        return {"visibility_ptr": torch.zeros((n, px), dtype=torch.float32, device="cuda"), "occlusion_ptr": torch.zeros((n, px), dtype=torch.float32, device="cuda"),
                "direct_ptr": torch.zeros((n, px, 4), dtype=torch.float32, device="cuda")}

    ways, extra = {}, {}
    if case != "batch64":
        size, pose = case.split("_pose")
        w, h = (1920, 1080) if size == "1080p" else (3840, 2160)
        sd = scenes.skin_scene("S64", int(pose))
        pass_h, beauty_h = M.DeviceScene(sd), M.DeviceScene(sd)
        beauty_h.set_background("transparent")
        lcfg = abi.Config(width=w, height=h)  # soft shadows, 8 samples; AO 8 samples, radius 3
        bcfg = abi.Config(width=w, height=h, samplesPerPixel=1, maxBounces=0)
        acfg = abi.Config(width=w, height=h, samplesPerPixel=1, maxBounces=0, aoEnabled=True)
        lb = light_planes(1, w * h)
        frame, frame_ao = (torch.zeros((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        gb = {"visibility_ptr": torch.zeros(w * h, dtype=torch.float32, device="cuda"), "distance_ptr": torch.zeros(w * h, dtype=torch.float32, device="cuda"),
              "matte_ptr": torch.zeros(w * h, dtype=torch.uint8, device="cuda")}
        yb = {f"{k}_ptr": torch.zeros((w * h, abi.LAYER_FORMATS[k][1]), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
              for k in abi.LAYER_NAMES}

        def light(*names):
            ptrs = {k: v.data_ptr() for k, v in lb.items() if k[:-4] in names}
            return lambda: pass_h.render_light_device(lcfg, stream=stream.cuda_stream, **ptrs)

        ways["light_all3"] = light("visibility", "occlusion", "direct")
        ways["light_visibility_direct"] = light("visibility", "direct")
        ways["light_occlusion"] = light("occlusion")
        ways["ground"] = lambda: pass_h.render_ground_device(lcfg, GROUND, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in gb.items()})
        ways["layers_all4"] = lambda: pass_h.render_layers_device(lcfg, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in yb.items()})
        ways["beauty_transparent_1spp_0b"] = lambda: beauty_h.render_device(bcfg, frame.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
        ways["beauty_transparent_1spp_0b_ao"] = lambda: beauty_h.render_device(acfg, frame_ao.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
        # the recomposition on this frame, before anything is timed
        for n in ("light_all3", "beauty_transparent_1spp_0b", "beauty_transparent_1spp_0b_ao"):
            ways[n]()
        torch.cuda.synchronize()
        direct = lb["direct_ptr"][0].cpu().numpy().reshape(h, w, 4)
        occ = lb["occlusion_ptr"][0].cpu().numpy().reshape(h, w)
        hit = direct[..., 3] > 0
        f32 = np.float32
        k = f32(1.0) - f32(acfg.aoIntensity) * (f32(1.0) - occ)
        rec = direct.copy()
        rec[..., :3] = np.clip(rec[..., :3] * k[..., None], f32(0.0), f32(1.0))
        same = frame.cpu().numpy()[hit].tobytes() == direct[hit].tobytes() and frame_ao.cpu().numpy()[hit].tobytes() == rec[hit].tobytes()
        if not same or hit.sum() < 1000:
            raise SystemExit(f"{case}: the beauty frames are not the recomposed planes (hits: {int(hit.sum())})")
        extra = {"recomposition_same_bytes": bool(same), "hits": int(hit.sum()), "share_of_frame_hit": float(hit.sum()) / hit.size,
                 "partly_occluded_hits": int((occ < 1).sum())}
    else:
        cfg = abi.Config(width=256, height=256)
        sds = [scenes.skin_scene("S64", k % 7) for k in range(64)]
        hs = [M.DeviceScene(sd) for sd in sds]
        lb, lb2 = light_planes(64, 256 * 256), light_planes(64, 256 * 256)
        ptrs = {k: v.data_ptr() for k, v in lb.items()}
        ways["batch_call"] = lambda: M.render_light_batch_device(hs, cfg, stream=stream.cuda_stream, **ptrs)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.render_light_device(cfg, stream=stream.cuda_stream, **{k: v[i].data_ptr() for k, v in lb2.items()})
        ways["loop_of_64"] = loop
        ways["batch_call"]()
        loop()
        torch.cuda.synchronize()
        same = all(lb[k].cpu().numpy().tobytes() == lb2[k].cpu().numpy().tobytes() for k in lb)
        hits = int((lb["direct_ptr"][..., 3] > 0).sum().item())
        if not same or hits < 64 * 1000:
            raise SystemExit(f"batch64: the two ways differ (same bytes: {same}, hits: {hits})")
        extra = {"same_bytes": bool(same), "hits": hits}
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
    row = {"case": case, "reps": reps, "warmup": warmup, **extra}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    for other in ("ground", "layers_all4", "beauty_transparent_1spp_0b", "beauty_transparent_1spp_0b_ao"):
        if other in row:
            row[f"light_all3_over_{other}"] = row["light_all3"]["ms_median"] / row[other]["ms_median"]
    if "batch_call" in row:
        row["batch_over_loop"] = row["batch_call"]["ms_median"] / row["loop_of_64"]["ms_median"]
        row["batch_range_below_loop"] = row["batch_call"]["ms_max"] < row["loop_of_64"]["ms_min"]
    return row


def child(case, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--warmup", str(a.warmup)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
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
    ap.add_argument("--txt", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps, a.warmup)), flush=True)
        return
    results, lines, failed = [], [], False

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for case in a.cases.split(","):
        row = child(case, a)
        results.append(row)
        for k, v in row.items():
            if isinstance(v, dict) and "ms_median" in v:
                say(f"{case:12s} {k:34s} {v['ms_median']:10.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})")
            elif k.startswith(("share_", "light_all3_over_", "batch_over_")):
                say(f"{case:12s} {k:34s} {v:10.3f}")
            elif k in ("hits", "partly_occluded_hits", "same_bytes", "recomposition_same_bytes", "batch_range_below_loop"):
                say(f"{case:12s} {k:34s} {v!s:>10s}")
        if case == "batch64" and not row["batch_range_below_loop"]:
            say("batch64: the ranges overlap — the batch call is NOT clear of the loop of 64 calls")
            failed = True
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    if a.txt:
        os.makedirs(os.path.dirname(os.path.abspath(a.txt)), exist_ok=True)
        with open(a.txt, "w") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
