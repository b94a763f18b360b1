"""N views of ONE skin — a turntable with a walk cycle: N poses, N orbit cameras — at the default Config (256x256, RGBA8 out),
frames left in device memory, two ways, after warm-up, repeated with the order of the ways alternated in one process:

  create  the only way before views of resident scenes: per view DeviceScene.for_skin(kind, pose_i, look_i) and a repaint
          (set_skin_device), then one render_batch_device of the N handles, a wait, and the handles closed
  view    N resident repaintable handles that hold the skin: one set_views_batch_device, one render_batch_device, a wait
  editor  1920x1080 / 4 spp, one handle: a new handle + repaint + render against set_view_device + render
  device  by device events on the issuing stream: the view call alone (the tables' copy and the kernel, with their enqueueing:
          no kernel trace is taken, so the kernel's own duration is not separated), and the host's flatten of the tables alone

    python tools/gpu_scene_view.py [--n 1,36,64] [--reps 7] [--warmup 3] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import minecraftskin_raytracer_amd as M  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def views_of(n):
    """A turntable with a walk cycle: view i of n."""
    walk = M.getBuiltinPoses()[1]
    poses, looks = [], []
    for i in range(n):
        phase = np.float32(np.cos(2.0 * np.pi * i / max(n, 1)))
        poses.append((walk * phase).astype(np.float32))
        looks.append(M.orbit_look(360.0 * i / max(n, 1), 15.0, 50.0))
    return np.stack(poses), looks


def timed(stream, fn):
    t = time.perf_counter()
    fn()
    stream.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,36,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    cfg = abi.Config()  # 256x256, 3 bounces, 1 spp, soft shadows, tile 32
    skin = np.ascontiguousarray(M.synthetic_skin("S64"))
    d_skin = torch.from_numpy(skin).cuda()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    results = {"batches": []}
    for n in [int(v) for v in a.n.split(",")]:
        poses, looks = views_of(n)
        px = cfg.width * cfg.height
        out = {k: torch.zeros((n, px, 4), dtype=torch.uint8, device="cuda") for k in ("create", "view")}
        d_skins = torch.from_numpy(np.stack([skin] * n)).cuda()
        resident = [M.DeviceScene.for_skin("S64") for _ in range(n)]
        M.set_skins_batch_device(resident, d_skins.data_ptr(), stream=s)

        def way_create():
            handles = []
            for i in range(n):
                h = M.DeviceScene.for_skin("S64", poses[i], looks[i])
                h.set_skin_device(d_skin.data_ptr(), s)
                handles.append(h)
            M.render_batch_device(handles, cfg, 0, out["create"].data_ptr(), px, s)
            stream.synchronize()
            for h in handles:
                h.close()

        def way_view():
            M.set_views_batch_device(resident, poses, looks, s)
            M.render_batch_device(resident, cfg, 0, out["view"].data_ptr(), px, s)

        def unview():  # (not timed) another view between two repetitions, so that `view` never finds its own tables in place
            M.set_views_batch_device(resident, poses[::-1].copy(), looks[::-1], s)
            stream.synchronize()

        ways = {"create": way_create, "view": way_view}
        for _ in range(a.warmup):
            for k in ways:
                unview()
                timed(stream, ways[k])
        if out["create"].cpu().numpy().tobytes() != out["view"].cpu().numpy().tobytes():
            raise SystemExit(f"N={n}: the frames of the viewed handles differ from those of the fresh handles")
        times = {k: [] for k in ways}
        for r in range(a.reps):
            for k in (list(ways) if r % 2 == 0 else list(ways)[::-1]):
                unview()
                times[k].append(timed(stream, ways[k]))

        # the view call alone by device events, and the host's share of it alone
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        call_ms, host_ms, enqueue_ms = [], [], []
        for r in range(a.warmup + a.reps):
            unview()
            t0.record(stream)
            t = time.perf_counter()
            M.set_views_batch_device(resident, poses, looks, s)
            e = (time.perf_counter() - t) * 1e3
            t1.record(stream)
            t1.synchronize()
            t = time.perf_counter()
            for i in range(n):
                M.skin_view_table("S64", poses[i], looks[i])
            h = (time.perf_counter() - t) * 1e3
            if r >= a.warmup:
                call_ms.append(t0.elapsed_time(t1)), enqueue_ms.append(e), host_ms.append(h)
        row = {"n": n, "config": "default 256x256, rgba8", "table_bytes": len(M.skin_view_table("S64")), "blob_bytes": len(resident[0].blob()),
               "wall": {k: summary(v) for k, v in times.items()},
               "view_call": {"device_events": summary(call_ms), "host_call": summary(enqueue_ms), "skin_view_table_alone": summary(host_ms)}}
        c, v = row["wall"]["create"], row["wall"]["view"]
        row["speedup"] = c["ms_median"] / v["ms_median"]
        row["ranges_overlap"] = not (v["ms_max"] < c["ms_min"])
        results["batches"].append(row)
        print(f"N={n:3d}  create {c['ms_median']:.3f} ms ({c['ms_min']:.3f}-{c['ms_max']:.3f})  view {v['ms_median']:.3f} ms ({v['ms_min']:.3f}-{v['ms_max']:.3f})"
              f"  x{row['speedup']:.2f}  {'RANGES OVERLAP' if row['ranges_overlap'] else 'ranges apart'}", flush=True)
        line = "       the view call:"
        for k, x in row["view_call"].items():
            line += f"  {k} {x['ms_median']:.4f} ms ({x['ms_min']:.4f}-{x['ms_max']:.4f})"
        print(line + f"  table {row['table_bytes']} B of a {row['blob_bytes']} B blob", flush=True)
        for h in resident:
            h.close()
        del out, d_skins
        torch.cuda.synchronize()

    # the editor's case: one handle, 1920x1080 / 4 spp, an orbit between two brush strokes
    big = abi.Config(width=1920, height=1080, samplesPerPixel=4)
    frame = {k: torch.zeros((big.height, big.width, 4), dtype=torch.uint8, device="cuda") for k in ("create", "view")}
    poses, looks = views_of(16)
    resident = M.DeviceScene.for_skin("S64")
    resident.set_skin_device(d_skin.data_ptr(), s)
    step = {"create": 0, "view": 0}

    def editor_create():
        i = step["create"] = (step["create"] + 1) % 16
        h = M.DeviceScene.for_skin("S64", poses[i], looks[i])
        h.set_skin_device(d_skin.data_ptr(), s)
        h.render_device_ex(big, 0, frame["create"].data_ptr(), 0, 1, abi.LAYOUT_FRAME, s)
        stream.synchronize()
        h.close()

    def editor_view():
        i = step["view"] = (step["view"] + 1) % 16
        resident.set_view_device(poses[i], looks[i], s)
        resident.render_device_ex(big, 0, frame["view"].data_ptr(), 0, 1, abi.LAYOUT_FRAME, s)

    ways = {"create": editor_create, "view": editor_view}
    for _ in range(a.warmup):
        for k in ways:
            timed(stream, ways[k])
    step["create"] = step["view"] = 0
    timed(stream, editor_create), timed(stream, editor_view)
    if frame["create"].cpu().numpy().tobytes() != frame["view"].cpu().numpy().tobytes():
        raise SystemExit("editor: the frame of the viewed handle differs from that of the fresh handle")
    times = {k: [] for k in ways}
    for r in range(a.reps):
        for k in (list(ways) if r % 2 == 0 else list(ways)[::-1]):
            times[k].append(timed(stream, ways[k]))
    ed = {"config": "1920x1080, 4 spp, rgba8", "wall": {k: summary(v) for k, v in times.items()}}
    c, v = ed["wall"]["create"], ed["wall"]["view"]
    ed["speedup"] = c["ms_median"] / v["ms_median"]
    ed["ranges_overlap"] = not (v["ms_max"] < c["ms_min"])
    results["editor"] = ed
    print(f"editor 1920x1080 / 4 spp: create {c['ms_median']:.3f} ms ({c['ms_min']:.3f}-{c['ms_max']:.3f})  view {v['ms_median']:.3f} ms "
          f"({v['ms_min']:.3f}-{v['ms_max']:.3f})  x{ed['speedup']:.2f}  {'RANGES OVERLAP' if ed['ranges_overlap'] else 'ranges apart'}", flush=True)
    resident.check()
    resident.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    # the condition the feature stands on: for a turntable and for 64 views the resident way beats the creating way by more than
    # the repetitions' spread
    missed = [r["n"] for r in results["batches"] if r["n"] in (36, 64) and r["ranges_overlap"]]
    if missed:
        raise SystemExit(f"CONDITION MISSED at N = {missed}: the min-max ranges of `create` and `view` overlap")


if __name__ == "__main__":
    main()
