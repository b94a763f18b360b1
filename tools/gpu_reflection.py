"""Device time of the ground-reflection pass (mcrt_render_reflection_device & co) against what it is measured by, the ways of a
case alternated in one process: events on the issuing stream, warm-ups first, then repetitions with the order of the ways
reversed every other time; median and min-max per way.

  1080p_pose0, 1080p_pose6, 4k_pose0, 4k_pose6
             all three reflection planes at y = 0 (the soles), S = 8, 3 bounces, S64, against the ground pass and the four-plane
             layers pass of the same frame and against the transparent 1 spp / 3-bounce beauty frame; and, in a second child
             process with MCRT_REFLECT_CULL=0 (the knob is read once per process), the pass with every mesh tested for every
             tile — what the tile culling buys.  With them the reached pixels and the reflected hits of the frame
  batch64    64 frames at 256x256 (the built-in poses) in one mcrt_render_reflection_batch_device call against a loop of 64
             mcrt_render_reflection_device calls; time per 64 frames
  probe_route
             1920x1080, pose 0, HOST TO HOST (time.perf_counter): the one-shot mcrt_render_reflection (rgba and distance) against
             the only way to these values without the pass — reflection rays formed on the host, mcrt_probe_intersect for the
             rays of the reached pixels, mcrt_probe_trace at depth 1 for the rays that hit.  The rays are formed once, outside the
             timed region (in numpy float32 from the flattened scene's camera: what the kernels read), so the probe route is
             charged for its two calls and the selection of the hit rays only.  The case first checks that both ways give the
             same bytes, and FAILS (exit status 1) unless the ranges are apart: max of the pass below min of the probe route

    python tools/gpu_reflection.py [--cases 1080p_pose0,...] [--reps 9] [--warmup 5] [--json out.json] [--txt out.txt] [--timeout 240]

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
CASES = ("1080p_pose0", "1080p_pose6", "4k_pose0", "4k_pose6", "batch64", "probe_route")
GROUND = 0.0


def host_reflection_rays(M, sd, w, h, ground):
    """(reached (n,) bool, rays (n, 6) float32): the pass's reflection rays, formed in numpy float32 from the flattened scene's
    camera as include/mcrt.h defines them (one rounding per operation)."""
    import numpy as np

    f32 = np.float32
    hdr = np.frombuffer(M.flatten(sd)[:192], f32)
    pos, half_h, fwd, right, up = hdr[12:15], hdr[15], hdr[16:19], hdr[20:23], hdr[24:27]

    def normalize(v):
        with np.errstate(all="ignore"):
            l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            out = v * (f32(1.0) / l)[:, None]
        out[l < f32(1e-8)] = 0
        return out

    ys, xs = np.mgrid[0:h, 0:w]
    u = ((xs.ravel().astype(f32) + f32(0.5)) / f32(w)).astype(f32)
    v = ((ys.ravel().astype(f32) + f32(0.5)) / f32(h)).astype(f32)
    aspect = f32(w) / f32(h)
    half_w = half_h * aspect
    su = (f32(2.0) * u - f32(1.0)) * half_w
    sv = (f32(2.0) * (f32(1.0) - v) - f32(1.0)) * half_h
    d = normalize((fwd[None, :] + right[None, :] * su[:, None]) + up[None, :] * sv[:, None])
    g = f32(ground)
    with np.errstate(all="ignore"):
        t = (g - pos[1]) / d[:, 1]
        reached = (d[:, 1] != 0) & (t > 0) & (t <= np.finfo(f32).max)
        P = np.stack([pos[0] + d[:, 0] * t, np.full(len(t), g, f32), pos[2] + d[:, 2] * t], axis=1)
    N = np.array([[0.0, 1.0, 0.0]], f32)
    D = normalize(d)
    dn = (D[:, 0] * N[0, 0] + D[:, 1] * N[0, 1]) + D[:, 2] * N[0, 2]
    R = normalize(D - N * (f32(2.0) * dn)[:, None])
    rays = np.concatenate([P + N * f32(1e-3), R], axis=1).astype(f32)
    assert d.dtype == f32 and P.dtype == f32 and R.dtype == f32
    return reached, rays


def measure_probe_route(reps, warmup):
    import ctypes as C

    import numpy as np

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    from minecraftskin_raytracer_amd._lib import check, load
    import scenes

    w, h = 1920, 1080
    sd = scenes.skin_scene("S64", 0)
    cfg = abi.Config(width=w, height=h)  # soft shadows, 8 samples, 3 bounces
    reached, rays = host_reflection_rays(M, sd, w, h, GROUND)
    idx = np.flatnonzero(reached)
    rr = np.ascontiguousarray(rays[idx])
    ds = M.DeviceScene(sd)
    flt_max = np.finfo(np.float32).max
    new = {"rgba": np.zeros((h, w, 4), np.float32), "distance": np.zeros((h, w), np.float32)}
    old = {"rgba": np.zeros((w * h, 4), np.float32), "distance": np.zeros(w * h, np.float32)}
    c = cfg.to_c()
    planes = abi.McrtReflection(new["rgba"].ctypes.data, None, new["distance"].ctypes.data)

    def one_shot():
        check(load().mcrt_render_reflection(sd.ptr, C.byref(c), GROUND, C.byref(planes), 0))

    def probes():
        hits = ds.intersect(rr)
        hit = hits["hit"] != 0
        colour = ds.trace(cfg, rr[hit], depth=1)
        old["rgba"][...] = 0
        old["distance"][...] = flt_max
        old["rgba"][idx[hit]] = colour
        old["distance"][idx[hit]] = hits["t"][hit]

    one_shot()
    probes()
    same = all(new[k].tobytes() == old[k].reshape(new[k].shape).tobytes() for k in new)
    hits = int((new["distance"] < flt_max).sum())
    if not same or hits < 1000:
        raise SystemExit(f"probe_route: the two ways differ (same bytes: {same}, reflected hits: {hits})")
    ways = {"one_shot_reflection": one_shot, "probe_intersect_and_trace": probes}
    names = list(ways)
    for _ in range(warmup):
        for n in names:
            ways[n]()
    times = {n: [] for n in names}
    for r in range(reps):
        for n in (names if r % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            ways[n]()
            times[n].append((time.perf_counter() - t0) * 1e3)
    row = {"case": "probe_route", "reps": reps, "warmup": warmup, "same_bytes": same, "reached_pixels": int(reached.sum()), "reflected_hits": hits}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    row["probe_over_one_shot"] = row["probe_intersect_and_trace"]["ms_median"] / row["one_shot_reflection"]["ms_median"]
    row["ranges_apart"] = row["one_shot_reflection"]["ms_max"] < row["probe_intersect_and_trace"]["ms_min"]
    ds.close()
    return row


def measure(case, reps, warmup, pass_only):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if case == "probe_route":
        return measure_probe_route(reps, warmup)
    import numpy as np
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    stream = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def reflection_planes(n, px):
        return {"rgba_ptr": torch.zeros((n, px, 4), dtype=torch.float32, device="cuda"), "rgba8_ptr": torch.zeros((n, px, 4), dtype=torch.uint8, device="cuda"),
                "distance_ptr": torch.zeros((n, px), dtype=torch.float32, device="cuda")}

    ways, extra = {}, {}
    if case != "batch64":
        size, pose = case.split("_pose")
        w, h = (1920, 1080) if size == "1080p" else (3840, 2160)
        sd = scenes.skin_scene("S64", int(pose))
        pass_h, beauty_h = M.DeviceScene(sd), M.DeviceScene(sd)
        beauty_h.set_background("transparent")
        rcfg = abi.Config(width=w, height=h)  # soft shadows, 8 samples, 3 bounces
        bcfg = abi.Config(width=w, height=h, samplesPerPixel=1)
        rb = reflection_planes(1, w * h)
        keep = [pass_h, beauty_h, rb]
        ways["reflection"] = lambda: pass_h.render_reflection_device(rcfg, GROUND, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in rb.items()})
        if not pass_only:
            frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            gb = {"visibility_ptr": torch.zeros(w * h, dtype=torch.float32, device="cuda"), "distance_ptr": torch.zeros(w * h, dtype=torch.float32, device="cuda"),
                  "matte_ptr": torch.zeros(w * h, dtype=torch.uint8, device="cuda")}
            lb = {f"{k}_ptr": torch.zeros((w * h, abi.LAYER_FORMATS[k][1]), dtype=torch.int32 if k == "id" else torch.float32, device="cuda")
                  for k in abi.LAYER_NAMES}
            keep += [frame, gb, lb]
            ways["ground"] = lambda: pass_h.render_ground_device(rcfg, GROUND, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in gb.items()})
            ways["layers_all4"] = lambda: pass_h.render_layers_device(rcfg, stream=stream.cuda_stream, **{k: v.data_ptr() for k, v in lb.items()})
            ways["beauty_transparent_1spp"] = lambda: beauty_h.render_device(bcfg, frame.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
    else:
        cfg = abi.Config(width=256, height=256)
        sds = [scenes.skin_scene("S64", k % 7) for k in range(64)]
        hs = [M.DeviceScene(sd) for sd in sds]
        rb = reflection_planes(64, 256 * 256)
        ptrs = {k: v.data_ptr() for k, v in rb.items()}
        ways["batch_call"] = lambda: M.render_reflection_batch_device(hs, cfg, GROUND, stream=stream.cuda_stream, **ptrs)

        def loop():
            for i, hnd in enumerate(hs):
                hnd.render_reflection_device(cfg, GROUND, stream=stream.cuda_stream, **{k: v[i].data_ptr() for k, v in rb.items()})
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
    row = {"case": case, "reps": reps, "warmup": warmup, "reflect_cull": os.environ.get("MCRT_REFLECT_CULL", "1"), **extra}
    for n in names:
        row[n] = {"ms_median": statistics.median(times[n]), "ms_min": min(times[n]), "ms_max": max(times[n]), "ms_all": times[n]}
    if case != "batch64":
        hit = rb["distance_ptr"][0].cpu().numpy() < np.finfo(np.float32).max
        row["reflected_hits"] = int(hit.sum())
        row["share_of_frame_mirrored"] = float(hit.sum()) / hit.size
    for other in ("ground", "layers_all4", "beauty_transparent_1spp"):
        if other in row:
            row[f"reflection_over_{other}"] = row["reflection"]["ms_median"] / row[other]["ms_median"]
    if "batch_call" in row:
        row["batch_over_loop"] = row["batch_call"]["ms_median"] / row["loop_of_64"]["ms_median"]
    return row


def child(case, a, env=None, pass_only=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--reps", str(a.reps), "--warmup", str(a.warmup)]
    if pass_only:
        cmd.append("--pass-only")
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
    ap.add_argument("--txt", default="")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--pass-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.reps, a.warmup, a.pass_only)), flush=True)
        return
    results, lines, failed = [], [], False

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for case in a.cases.split(","):
        row = child(case, a)
        if case not in ("batch64", "probe_route"):
            uncut = child(case, a, env=dict(os.environ, MCRT_REFLECT_CULL="0"), pass_only=True)
            assert uncut["reflected_hits"] == row["reflected_hits"]
            row["reflection_without_culling"] = uncut["reflection"]
            row["culling_speedup"] = uncut["reflection"]["ms_median"] / row["reflection"]["ms_median"]
        results.append(row)
        for k, v in row.items():
            if isinstance(v, dict) and "ms_median" in v:
                say(f"{case:12s} {k:30s} {v['ms_median']:10.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})")
            elif k.startswith(("share_", "reflection_over_", "batch_over_", "culling_", "probe_over_")):
                say(f"{case:12s} {k:30s} {v:10.3f}")
            elif k in ("reflected_hits", "reached_pixels", "same_bytes", "ranges_apart"):
                say(f"{case:12s} {k:30s} {v!s:>10s}")
        if case == "probe_route" and not row["ranges_apart"]:
            say("probe_route: the ranges overlap — the one-shot pass is NOT clear of the probe route")
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
