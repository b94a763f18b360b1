"""What capes cost.  N distinct skins with N distinct capes (one pose, a look from three-quarter behind, the default Config at
256x256, RGBA8 out), after warm-up, the ways alternated in one process; run it in several processes and take the medians of
the medians.

  host to host
    build      MeshBuilder.buildScene(skin, pose, cape=...) per skin, then TileRenderer.renderBatch
    caped      SkinBatch(N, cape=True).render(skins, capes=capes): two uploads, the skin and the cape repaint launches, one
               batched render, one download
    clear      the same handles with capes=None: transparent capes — against
    capeless   SkinBatch(N).render(skins): the price of the thirteenth mesh
  device events on the issuing stream
    skin       set_skins_batch_device of the N caped handles alone
    cape       set_capes_batch_device alone
    both       the two launches one after the other

    python tools/gpu_capes.py [--n 64] [--reps 9] [--warmup 3] [--json out.json] [--capeless-only]

--capeless-only: `capeless` alone (the farm call that this feature must not slow down), for runs that alternate two builds of
the library through MCRT_LIB.
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


def images_of(base, n):
    out = np.stack([base] * n)
    for i in range(n):  # distinct colours, the alphas kept
        out[i, ..., 0] ^= np.uint8(i & 255)
        out[i, ..., 1] += np.uint8((3 * i) & 255)
    return out


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def alternated(ways, reps):
    times = {k: [] for k in ways}
    for r in range(reps):
        for k in (list(ways) if r % 2 == 0 else list(ways)[::-1]):
            times[k].append(ways[k]())
    return times


def host(fn):
    def timed():
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--capeless-only", action="store_true")
    a = ap.parse_args()
    cfg, n = abi.Config(), a.n
    pose, look = M.getBuiltinPoses()[1], M.orbit_look(150.0, 0.0, 50.0)
    skins = images_of(M.synthetic_skin("S64"), n)
    plain = M.SkinBatch(n, "S64", pose, look)
    row = {"n": n, "config": "default 256x256, rgba8", "library": os.environ.get("MCRT_LIB", "")}
    if a.capeless_only:
        way = host(lambda: plain.render(skins, cfg, rgba8=True))
        for _ in range(a.warmup):
            way()
        row["host_to_host"] = {"capeless": summary([way() for _ in range(a.reps)])}
    else:
        capes = list(images_of(M.synthetic_cape(), n))
        caped = M.SkinBatch(n, "S64", pose, look, cape=True)
        def with_look(sd):
            d, b = sd.desc, look.desc
            for k in ("light_position", "light_color", "camera_position", "camera_target", "camera_up", "background_color"):
                for i in range(len(getattr(d, k))):
                    getattr(d, k)[i] = getattr(b, k)[i]
            for k in ("light_intensity", "light_radius", "camera_fov"):
                setattr(d, k, getattr(b, k))
            return sd

        def built():
            return M.TileRenderer.renderBatch([with_look(M.MeshBuilder.buildScene(s, pose, cape=c)) for s, c in zip(skins, capes)], cfg, rgba8=True)

        if caped.render(skins, cfg, rgba8=True, capes=capes).tobytes() != built().tobytes():
            raise SystemExit("SkinBatch.render with capes differs from renderBatch of the built scenes")
        if caped.render(skins, cfg, rgba8=True).tobytes() != plain.render(skins, cfg, rgba8=True).tobytes():
            raise SystemExit("transparent capes change the frames")
        ways = {"build": host(built), "caped": host(lambda: caped.render(skins, cfg, rgba8=True, capes=capes)),
                "clear": host(lambda: caped.render(skins, cfg, rgba8=True)), "capeless": host(lambda: plain.render(skins, cfg, rgba8=True))}
        for _ in range(a.warmup):
            for w in ways.values():
                w()
        row["host_to_host"] = {k: summary(v) for k, v in alternated(ways, a.reps).items()}
        stream = torch.cuda.current_stream()
        d_skins, d_capes = torch.from_numpy(skins).cuda(), torch.from_numpy(np.stack(capes)).cuda()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def events(fn):
            def timed():
                t0.record(stream)
                fn()
                t1.record(stream)
                t1.synchronize()
                return t0.elapsed_time(t1)
            return timed

        def skin():
            M.set_skins_batch_device(caped.scenes, d_skins.data_ptr(), stream=stream.cuda_stream)

        def cape():
            M.set_capes_batch_device(caped.scenes, d_capes.data_ptr(), stream=stream.cuda_stream)

        dev = {"skin": events(skin), "cape": events(cape), "both": events(lambda: (skin(), cape()))}
        for _ in range(a.warmup + 2):
            for w in dev.values():
                w()
        torch.cuda.synchronize()
        row["repaint_device_events"] = {k: summary(v) for k, v in alternated(dev, a.reps).items()}
        caped.close()
    plain.close()
    for part in ("host_to_host", "repaint_device_events"):
        if part in row:
            print(f"N={n} {part}: " + "  ".join(f"{k} {v['ms_median']:.4f} ms ({v['ms_min']:.4f}-{v['ms_max']:.4f})" for k, v in row[part].items()), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
