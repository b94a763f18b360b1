"""The studio shot (mcrt_render_shot_batch_device & co) against what a user could do without it, the ways of a
case alternated in one process: warm-ups first, then repetitions with the order of the ways reversed every other time; median
and min-max per way.

  farm64     64 variants of the synthetic skin at the default 256x256 Config, RGBA8, HOST TO HOST (wall clock around the whole
             call, skins in host memory to images in host memory):
               shots       ``SkinBatch.shots``: one upload, one repaint, one shot call, one download of 4 B/px
               baseline_a  what the parent commit offers a user without device code: ``SkinBatch.render(background=
                           "transparent")`` + the host forms ``renderGroundBatch`` and ``renderReflectionBatch`` (scene
                           descriptions built beforehand, outside the clock) + the blend in numpy
               baseline_b  the parent's device forms — repaint, ``render_batch_device`` on handles set to transparent,
                           ``render_ground_batch_device``, ``render_reflection_batch_device`` — + the blend written in torch on
                           the device + one download of 4 B/px
             The case first checks that the three ways give the same bytes, and FAILS (exit status 1) if the shot's median is
             above a baseline's median by more than that baseline's own spread (max - min) in this job.
  kernel     one scene at 1920x1080, device events on the issuing stream:
               three_calls  the parent's three device calls (transparent render, ground, reflection)
               shot         ``render_shot_batch_device``: the same three + the blend
               blend_u8 / blend_both   ``composite_shot_batch_device`` alone on those planes, RGBA8 out / both outputs
               launch_1x1   the same call on a 1x1 frame: one workgroup, one pixel — the cost of a launch
             with the blend's bytes, its achieved bytes/s and the time a float4 copy of those bytes takes at the 6.29 TB/s the
             chip's copy kernel reaches.

    python tools/bench_shot.py [--cases farm64,kernel] [--reps 9] [--warmup 3] [--json out.json] [--txt out.txt] [--timeout 400]

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
CASES = ("farm64", "kernel")
COPY_RATE = 6.29e12  # bytes/s of a float4 copy on the MI355X


def _stats(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms_all": ts}


def measure(case, reps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import shot_checker as S
    import skin_paint_checker as SP

    stream = torch.cuda.current_stream()
    shot = abi.Shot(reflectionFade=30.0)
    ways, extra, timer = {}, {}, "wall"
    if case == "farm64":
        n = 64
        cfg = abi.Config()
        w, h = cfg.width, cfg.height
        pose = M.getBuiltinPoses()[0]
        skins = np.stack([SP.variant(M.synthetic_skin("S64"), i) for i in range(n)])
        descs = [M.MeshBuilder.buildScene(s, pose) for s in skins]
        batch = M.SkinBatch(n, "S64", pose)
        page = S.gradient_plane(cfg)
        results = {}

        def shots():
            results["shots"] = batch.shots(skins, cfg, shot, 0.0)

        def baseline_a():
            F = batch.render(skins, cfg, rgba8=False, background="transparent")
            vis = M.TileRenderer.renderGroundBatch(descs, cfg, 0.0, planes=("visibility",))["visibility"]
            refl = M.TileRenderer.renderReflectionBatch(descs, cfg, 0.0, planes=("rgba", "distance"))
            results["baseline_a"] = S.quantize(S.compose(F, vis, refl["rgba"], refl["distance"], page, shot))

        other = M.SkinBatch(n, "S64", pose)  # baseline B's own handles, set to transparent once
        for s in other.scenes:
            s.set_background("transparent")
        dF = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
        dR = torch.zeros_like(dF)
        dvis = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
        ddist = torch.zeros_like(dvis)
        dpage = torch.from_numpy(page).cuda()
        host8 = torch.zeros((n, h, w, 4), dtype=torch.uint8).pin_memory()
        s_, k_, fade = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in (shot.shadowStrength, shot.reflectivity, shot.reflectionFade))

        def baseline_b():
            other._paint(skins, stream)
            M.render_batch_device(other.scenes, cfg, dF.data_ptr(), 0, stream=stream.cuda_stream)
            M.render_ground_batch_device(other.scenes, cfg, 0.0, visibility_ptr=dvis.data_ptr(), stream=stream.cuda_stream)
            M.render_reflection_batch_device(other.scenes, cfg, 0.0, rgba_ptr=dR.data_ptr(), distance_ptr=ddist.data_ptr(), stream=stream.cuda_stream)
            sh = s_ * (1.0 - dvis)
            f = torch.clamp(1.0 - ddist / fade, 0.0, 1.0)
            ar = (k_ * dR[..., 3]) * f
            keep = (1.0 - sh) * (1.0 - ar)
            a = dF[..., 3:]
            out = dF[..., :3] * a + (dpage * keep[..., None] + dR[..., :3] * ar[..., None]) * (1.0 - a)
            out8 = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
            out8[..., :3] = (torch.clamp(out, 0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
            out8[..., 3] = 255
            host8.copy_(out8, non_blocking=True)
            stream.synchronize()
            results["baseline_b"] = host8.numpy().copy()

        ways = {"shots": shots, "baseline_a": baseline_a, "baseline_b": baseline_b}
        for f in ways.values():
            f()
        same_a = bool(np.array_equal(results["shots"], results["baseline_a"]))
        same_b = bool(np.array_equal(results["shots"], results["baseline_b"]))
        distinct = len({results["shots"][i].tobytes() for i in range(n)})
        if not same_a or distinct != n:
            raise SystemExit(f"farm64: the shot differs from baseline A (same bytes: {same_a}, distinct frames: {distinct})")
        extra = {"frames": n, "same_bytes_a": same_a, "same_bytes_b": same_b, "distinct_frames": distinct}
    else:
        timer = "events"
        w, h = 1920, 1080
        px = w * h
        cfg = abi.Config(width=w, height=h)
        ds = M.DeviceScene(M.MeshBuilder.buildScene(M.synthetic_skin("S64"), M.getBuiltinPoses()[0]))
        own = M.DeviceScene(M.MeshBuilder.buildScene(M.synthetic_skin("S64"), M.getBuiltinPoses()[0]))
        own.set_background("transparent")
        dF = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        dR = torch.zeros_like(dF)
        dvis = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        ddist = torch.zeros_like(dvis)
        out = torch.zeros_like(dF)
        out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        need = M.shot_scratch_bytes(cfg, shot, 1)
        scratch = torch.zeros((need,), dtype=torch.uint8, device="cuda")
        tiny = abi.Config(width=1, height=1)

        def three_calls():
            M.render_batch_device([own], cfg, dF.data_ptr(), 0, stream=stream.cuda_stream)
            own.render_ground_device(cfg, 0.0, visibility_ptr=dvis.data_ptr(), stream=stream.cuda_stream)
            own.render_reflection_device(cfg, 0.0, rgba_ptr=dR.data_ptr(), distance_ptr=ddist.data_ptr(), stream=stream.cuda_stream)

        def blend(c, f32, u8):
            return lambda: M.composite_shot_batch_device([own], c, shot, dF.data_ptr(), dvis.data_ptr(), dR.data_ptr(), ddist.data_ptr(), f32, u8,
                                                         stream=stream.cuda_stream)

        ways = {"three_calls": three_calls,
                "shot": lambda: M.render_shot_batch_device([ds], cfg, shot, 0.0, scratch.data_ptr(), need, 0, out8.data_ptr(), stream=stream.cuda_stream),
                "blend_u8": blend(cfg, 0, out8.data_ptr()), "blend_both": blend(cfg, out.data_ptr(), out8.data_ptr()),
                "launch_1x1": blend(tiny, 0, out8.data_ptr())}
        ways["shot"]()
        torch.cuda.synchronize()
        from_shot = out8.cpu().numpy().copy()
        three_calls()
        ways["blend_u8"]()
        torch.cuda.synchronize()
        same = bool(np.array_equal(from_shot, out8.cpu().numpy()))
        if not same:
            raise SystemExit("kernel: the shot differs from the three calls plus the blend")
        extra = {"same_bytes": same, "pixels": px, "blend_u8_bytes": px * 44, "blend_both_bytes": px * 60}
    names = list(ways)
    for _ in range(warmup):
        for name in names:
            ways[name]()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in names}
    for r in range(reps):
        for name in (names if r % 2 == 0 else names[::-1]):
            if timer == "events":
                t0.record(stream)
                ways[name]()
                t1.record(stream)
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1))
            else:
                torch.cuda.synchronize()
                a = time.perf_counter()
                ways[name]()
                times[name].append((time.perf_counter() - a) * 1e3)
    row = {"case": case, "reps": reps, "warmup": warmup, "timer": timer, **extra}
    for name in names:
        row[name] = _stats(times[name])
    if case == "farm64":
        for b in ("baseline_a", "baseline_b"):
            row[f"shots_over_{b}"] = row["shots"]["ms_median"] / row[b]["ms_median"]
            row[f"not_slower_than_{b}"] = row["shots"]["ms_median"] <= row[b]["ms_median"] + (row[b]["ms_max"] - row[b]["ms_min"])
    else:
        row["blend_cost_ms"] = row["shot"]["ms_median"] - row["three_calls"]["ms_median"]
        for k in ("blend_u8", "blend_both"):
            by = row[f"{k}_bytes"]
            row[f"{k}_tb_per_s"] = by / (row[k]["ms_median"] * 1e-3) / 1e12
            row[f"{k}_copy_rate_ms"] = by / COPY_RATE * 1e3
        bound = 2.0 * (row["blend_u8_copy_rate_ms"] + row["launch_1x1"]["ms_median"])
        row["blend_within_twice_copy_plus_launch"] = row["blend_u8"]["ms_median"] <= bound
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--txt", default="")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per case")
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
                say(f"{case:8s} {k:36s} {v['ms_median']:10.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})")
            elif isinstance(v, float):
                say(f"{case:8s} {k:36s} {v:10.4f}")
            elif k not in ("case", "ms_all"):
                say(f"{case:8s} {k:36s} {v!s:>10s}")
        if case == "farm64" and not (row["not_slower_than_baseline_a"] and row["not_slower_than_baseline_b"]):
            say("farm64: the shot is slower than a baseline beyond that baseline's spread")
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
