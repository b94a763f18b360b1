"""Device time of the light bake (mcrt_bake_light_device & co), the ways of a case alternated in one process: events on the
issuing stream, warm-ups first, then repetitions with the order of the ways reversed every other time; median and min-max per way.

  s64_q1, s64_q4
             the S64 figure at pose 0 (3264 pool texels), S = 8, A = 8, radius 3, at grid 1 and 4: all five planes, visibility +
             direct alone (the `bake_shade` kernel), occlusion alone (the `bake_occlusion` kernel), position + normal alone; beside
             them, for context, the light layers of the same scene at 1920x1080 (all three planes).  There is no earlier way to
             the bake's values to compare against.  The case first checks that the planes of the partial calls are the bytes of
             the full call
  batch64    64 repainted ``DeviceScene.for_skin`` handles (64 variants of the synthetic skin), grid 1, all five planes, in one
             mcrt_bake_light_batch_device call against a loop of 64 mcrt_bake_light_device calls; time per 64 bakes.  The case
             first checks that both ways give the same bytes, and FAILS (exit status 1) unless the batch's range lies below the
             loop's: one launch per kernel against 64 is the reason the batched form exists

    python tools/gpu_bake.py [--cases s64_q1,...] [--reps 9] [--warmup 5] [--json out.json] [--txt out.txt] [--timeout 240]

Every case runs in a child process of its own under a time limit; the first case that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("s64_q1", "s64_q4", "batch64")


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
    comps = {k: c for k, (_, c) in abi.BAKE_FORMATS.items()}

    def planes(n, texels):
        return {k: torch.full((n, texels, c), -7.0, dtype=torch.float32, device="cuda") for k, c in comps.items()}

    ways, extra = {}, {}
    cfg = abi.Config()  # soft shadows, 8 samples; AO 8 samples, radius 3
    if case != "batch64":
        grid = int(case[-1])
        sd = scenes.skin_scene("S64", 0)
        h = M.DeviceScene(sd)
        n = h.texels
        full, part = planes(1, n), planes(1, n)

        def bake(buf, *names):
            ptrs = {f"{k}_ptr": buf[k].data_ptr() for k in names}
            return lambda: h.bake_light_device(cfg, grid, stream=stream.cuda_stream, **ptrs)

        ways["bake_all5"] = bake(full, *abi.BAKE_NAMES)
        ways["bake_visibility_direct"] = bake(part, "visibility", "direct")
        ways["bake_occlusion"] = bake(part, "occlusion")
        ways["bake_position_normal"] = bake(part, "position", "normal")
        w, hh = 1920, 1080
        lcfg = abi.Config(width=w, height=hh)
        lb = {"visibility_ptr": torch.zeros(w * hh, dtype=torch.float32, device="cuda"), "occlusion_ptr": torch.zeros(w * hh, dtype=torch.float32, device="cuda"),
              "direct_ptr": torch.zeros((w * hh, 4), dtype=torch.float32, device="cuda")}
        ways["light_all3_1080p"] = lambda: h.render_light_device(lcfg, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in lb.items()})
        for name in ways:
            ways[name]()
        torch.cuda.synchronize()
        same = all(full[k].cpu().numpy().tobytes() == part[k].cpu().numpy().tobytes() for k in comps)
        live = int((full["position"][0, :, 3] == 1).sum().item())
        if not same or live < 2000:
            raise SystemExit(f"{case}: the partial calls differ from the full call (same bytes: {same}, live texels: {live})")
        vis = full["visibility"][0, :, 0].cpu().numpy()
        extra = {"same_bytes": bool(same), "texels": n, "live_texels": live, "points": live * grid * grid,
                 "penumbra_texels": int(((vis > 0) & (vis < 1)).sum()), "light_hits_1080p": int((lb["direct_ptr"][:, 3] > 0).sum().item())}
    else:
        import skin_paint_checker as SP

        base = M.synthetic_skin("S64")
        hs = [M.DeviceScene.for_skin("S64", M.getBuiltinPoses()[0]) for _ in range(64)]
        for i, hnd in enumerate(hs):
            hnd.set_skin(SP.variant(base, i))
        n = hs[0].texels
        a, b = planes(64, n), planes(64, n)
        ptrs = {f"{k}_ptr": v.data_ptr() for k, v in a.items()}
        ways["batch_call"] = lambda: M.bake_light_batch_device(hs, cfg, 1, texel_stride=n, stream=stream.cuda_stream, **ptrs)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.bake_light_device(cfg, 1, stream=stream.cuda_stream, **{f"{k}_ptr": v[i].data_ptr() for k, v in b.items()})
        ways["loop_of_64"] = loop
        ways["batch_call"]()
        loop()
        torch.cuda.synchronize()
        same = all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in comps)
        live = int((a["position"][..., 3] == 1).sum().item())
        distinct = len({a["direct"][i].cpu().numpy().tobytes() for i in range(64)})
        if not same or live < 64 * 2000 or distinct != 64:
            raise SystemExit(f"batch64: the two ways differ (same bytes: {same}, live texels: {live}, distinct frames: {distinct})")
        extra = {"same_bytes": bool(same), "texels": n, "live_texels": live, "distinct_frames": distinct}
    names = list(ways)
    for _ in range(warmup):
        for name in names:
            ways[name]()
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            t0.record(stream)
            ways[name]()
            t1.record(stream)
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    row = {"case": case, "reps": reps, "warmup": warmup, **extra}
    for name in names:
        row[name] = {"ms_median": statistics.median(times[name]), "ms_min": min(times[name]), "ms_max": max(times[name]), "ms_all": times[name]}
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
                say(f"{case:10s} {k:26s} {v['ms_median']:10.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})")
            elif k.startswith("batch_over_"):
                say(f"{case:10s} {k:26s} {v:10.3f}")
            elif k in ("texels", "live_texels", "points", "penumbra_texels", "light_hits_1080p", "distinct_frames", "same_bytes", "batch_range_below_loop"):
                say(f"{case:10s} {k:26s} {v!s:>10s}")
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
