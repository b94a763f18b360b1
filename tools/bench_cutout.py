"""The studio shot as a cut-out (mcrt_*_ex) against what the parent commit offers for the same image, the ways of a
case alternated in one process like tools/bench_shot.py: warm-ups first, then repetitions with the order of the ways reversed
every other time; median and min-max per way.

  farm64     64 variants of the synthetic skin at the default 256x256 Config, RGBA8, HOST TO HOST (wall clock around the whole
             call, skins in host memory to images in host memory), transparent page:
               shots         ``SkinBatch.shots(..., Shot(page="transparent"))``
               shots_bounds  the same with ``bounds=True``: the boxes come down with the images
               baseline      the parent's device forms — repaint, ``render_batch_device`` on handles set to transparent,
                             ``render_ground_batch_device``, ``render_reflection_batch_device`` — + the cut-out blend written in
                             torch on the device + one download of 4 B/px
             The case first checks that ``shots`` gives the bytes of tests/cutout_checker.py's ``compose_ex`` on the baseline's
             planes and reports whether the torch blend does too, and FAILS (exit status 1) if a median of the new ways is above
             the baseline's median by more than the baseline's own spread (max - min) in this job.
  kernel     one scene at 1920x1080, device events on the issuing stream, ``composite_shot_batch_device`` alone on the planes of
             the library's own three calls:
               opaque_u8 / opaque_both   the parent's blend (reference page), RGBA8 out / both outputs
               cutout_u8 / cutout_both   the cut-out blend without bounds
               cutout_u8_bounds / cutout_both_bounds   with bounds
               launch_1x1                the cut-out blend on a 1x1 frame: the cost of a launch
             with the blend's bytes and its achieved bytes/s, and what the bounds cost against the opaque blend's own range.

    python tools/bench_cutout.py [--cases farm64,kernel] [--reps 9] [--warmup 3] [--json out.json] [--txt out.txt] [--timeout 400]

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


def _stats(ts):
    return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms_all": ts}


def measure(case, reps, warmup):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import cutout_checker as X
    import skin_paint_checker as SP

    stream = torch.cuda.current_stream()
    shot = abi.Shot("transparent", reflectionFade=30.0)
    ways, extra, timer = {}, {}, "wall"
    if case == "farm64":
        n = 64
        cfg = abi.Config()
        w, h = cfg.width, cfg.height
        pose = M.getBuiltinPoses()[0]
        skins = np.stack([SP.variant(M.synthetic_skin("S64"), i) for i in range(n)])
        batch = M.SkinBatch(n, "S64", pose)
        results = {}

        def shots():
            results["shots"] = batch.shots(skins, cfg, shot, 0.0)

        def shots_bounds():
            results["shots_bounds"], results["boxes"] = batch.shots(skins, cfg, shot, 0.0, bounds=True)

        other = M.SkinBatch(n, "S64", pose)  # the baseline's own handles, set to transparent once
        for s in other.scenes:
            s.set_background("transparent")
        dF = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
        dR = torch.zeros_like(dF)
        dvis = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
        ddist = torch.zeros_like(dvis)
        host8 = torch.zeros((n, h, w, 4), dtype=torch.uint8).pin_memory()
        s_, k_, fade = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in (shot.shadowStrength, shot.reflectivity, shot.reflectionFade))

        def baseline():
            other._paint(skins, stream)
            M.render_batch_device(other.scenes, cfg, dF.data_ptr(), 0, stream=stream.cuda_stream)
            M.render_ground_batch_device(other.scenes, cfg, 0.0, visibility_ptr=dvis.data_ptr(), stream=stream.cuda_stream)
            M.render_reflection_batch_device(other.scenes, cfg, 0.0, rgba_ptr=dR.data_ptr(), distance_ptr=ddist.data_ptr(), stream=stream.cuda_stream)
            sh = s_ * (1.0 - dvis)
            f = torch.clamp(1.0 - ddist / fade, 0.0, 1.0)
            ar = (k_ * dR[..., 3]) * f
            keep = (1.0 - sh) * (1.0 - ar)
            af = 1.0 - keep
            a = dF[..., 3]
            u = 1.0 - a
            A = a + af * u
            num = dF[..., :3] * a[..., None] + (dR[..., :3] * ar[..., None]) * u[..., None]
            out = torch.empty_like(dF)
            out[..., :3] = torch.where((A > 0)[..., None], num / A[..., None], torch.zeros_like(num))
            out[..., 3] = torch.where(A > 0, A, torch.zeros_like(A))
            out = torch.where((af == 0)[..., None], dF, out)
            out8 = (torch.clamp(out, 0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
            host8.copy_(out8, non_blocking=True)
            stream.synchronize()
            results["baseline"] = host8.numpy().copy()

        ways = {"shots": shots, "shots_bounds": shots_bounds, "baseline": baseline}
        for f in ways.values():
            f()
        # and the device's share of the two new ways: the shot call alone on the painted handles, device events, no copy
        need = M.shot_scratch_bytes(cfg, shot, n)
        scratch = torch.zeros((max(need, 16),), dtype=torch.uint8, device="cuda")
        d8 = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        dbox = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        device_ms = {"device_shots": [], "device_shots_bounds": []}
        for r in range(warmup + reps):
            for key, ptr in (("device_shots", 0), ("device_shots_bounds", dbox.data_ptr())):
                e0.record(stream)
                M.render_shot_batch_device(batch.scenes, cfg, shot, 0.0, scratch.data_ptr(), need, 0, d8.data_ptr(), stream=stream.cuda_stream, bounds_ptr=ptr)
                e1.record(stream)
                e1.synchronize()
                if r >= warmup:
                    device_ms[key].append(e0.elapsed_time(e1))
        want = X.compose_ex(dF.cpu().numpy(), dvis.cpu().numpy(), dR.cpu().numpy(), ddist.cpu().numpy(), None, None, shot)
        same = bool(np.array_equal(results["shots"], X.quantize(want))) and bool(np.array_equal(results["shots_bounds"], results["shots"]))
        boxes = bool(np.array_equal(results["boxes"], np.array([X.bounds_of(f[..., 3]) for f in want])))
        distinct = len({results["shots"][i].tobytes() for i in range(n)})
        if not same or not boxes or distinct != n:
            raise SystemExit(f"farm64: the cut-outs differ from compose_ex on the baseline's planes (same bytes: {same}, boxes: {boxes}, distinct: {distinct})")
        extra = {"frames": n, "same_bytes_as_compose_ex": same, "same_boxes": boxes, "torch_blend_same_bytes": bool(np.array_equal(results["shots"], results["baseline"])),
                 "torch_blend_largest_level_difference": int(np.abs(results["shots"].astype(int) - results["baseline"].astype(int)).max()),
                 "distinct_frames": distinct, **{k: _stats(v) for k, v in device_ms.items()}}
    else:
        timer = "events"
        w, h = 1920, 1080
        px = w * h
        cfg = abi.Config(width=w, height=h)
        own = M.DeviceScene(M.MeshBuilder.buildScene(M.synthetic_skin("S64"), M.getBuiltinPoses()[0]))
        own.set_background("transparent")
        dF = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        dR = torch.zeros_like(dF)
        dvis = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        ddist = torch.zeros_like(dvis)
        out = torch.zeros_like(dF)
        out8 = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        box = torch.zeros((4,), dtype=torch.int32, device="cuda")
        tiny = abi.Config(width=1, height=1)
        M.render_batch_device([own], cfg, dF.data_ptr(), 0, stream=stream.cuda_stream)
        own.render_ground_device(cfg, 0.0, visibility_ptr=dvis.data_ptr(), stream=stream.cuda_stream)
        own.render_reflection_device(cfg, 0.0, rgba_ptr=dR.data_ptr(), distance_ptr=ddist.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
        opaque = abi.Shot(reflectionFade=30.0)

        def blend(c, sh, f32, u8, bounds=0):
            return lambda: M.composite_shot_batch_device([own], c, sh, dF.data_ptr(), dvis.data_ptr(), dR.data_ptr(), ddist.data_ptr(), f32, u8,
                                                         stream=stream.cuda_stream, bounds_ptr=bounds)

        ways = {"opaque_u8": blend(cfg, opaque, 0, out8.data_ptr()), "opaque_both": blend(cfg, opaque, out.data_ptr(), out8.data_ptr()),
                "cutout_u8": blend(cfg, shot, 0, out8.data_ptr()), "cutout_both": blend(cfg, shot, out.data_ptr(), out8.data_ptr()),
                "cutout_u8_bounds": blend(cfg, shot, 0, out8.data_ptr(), box.data_ptr()),
                "cutout_both_bounds": blend(cfg, shot, out.data_ptr(), out8.data_ptr(), box.data_ptr()),
                "launch_1x1": blend(tiny, shot, 0, out8.data_ptr())}
        ways["cutout_both_bounds"]()
        torch.cuda.synchronize()
        want = X.compose_ex(dF.cpu().numpy(), dvis.cpu().numpy(), dR.cpu().numpy(), ddist.cpu().numpy(), None, None, shot)
        same = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))) and bool(np.array_equal(out8.cpu().numpy(), X.quantize(want)))
        boxes = box.cpu().numpy().tolist() == X.bounds_of(want[..., 3]).tolist()
        if not same or not boxes:
            raise SystemExit(f"kernel: the cut-out differs from compose_ex (same bytes: {same}, box: {boxes})")
        extra = {"same_bytes_as_compose_ex": same, "same_box": boxes, "box": box.cpu().numpy().tolist(), "pixels": px, "u8_bytes": px * 44, "both_bytes": px * 60}
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
        b = row["baseline"]
        for k in ("shots", "shots_bounds"):
            row[f"{k}_over_baseline"] = row[k]["ms_median"] / b["ms_median"]
            row[f"{k}_not_slower_than_baseline"] = row[k]["ms_median"] <= b["ms_median"] + (b["ms_max"] - b["ms_min"])
    else:
        for k in names[:-1]:
            row[f"{k}_tb_per_s"] = row["both_bytes" if "both" in k else "u8_bytes"] / (row[k]["ms_median"] * 1e-3) / 1e12
        for k in ("u8", "both"):
            spread = row[f"opaque_{k}"]["ms_max"] - row[f"opaque_{k}"]["ms_min"]
            row[f"cutout_{k}_minus_opaque_ms"] = row[f"cutout_{k}"]["ms_median"] - row[f"opaque_{k}"]["ms_median"]
            row[f"bounds_{k}_cost_ms"] = row[f"cutout_{k}_bounds"]["ms_median"] - row[f"cutout_{k}"]["ms_median"]
            row[f"bounds_{k}_within_the_opaque_blends_range"] = row[f"bounds_{k}_cost_ms"] <= spread
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
                say(f"{case:8s} {k:44s} {v['ms_median']:10.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})")
            elif isinstance(v, float):
                say(f"{case:8s} {k:44s} {v:10.4f}")
            elif k not in ("case", "ms_all"):
                say(f"{case:8s} {k:44s} {v!s:>10s}")
        if case == "farm64" and not (row["shots_not_slower_than_baseline"] and row["shots_bounds_not_slower_than_baseline"]):
            say("farm64: the cut-out is slower than the baseline beyond the baseline's spread")
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
