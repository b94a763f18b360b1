"""One process = one tree, for alternating two builds in one session: 64 classic skins through SkinBatch.render, host to host
at the default Config (RGBA8 out), and the repaint call of the 64 resident handles alone by device events; 6 warm-ups and 31
repetitions each.  Prints one JSON line with median, min and max.

    python tools/gpu_skin_paint_ab.py <directory that holds the package> <label>
"""
import json, statistics, sys, time
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

assert M.__file__.startswith(sys.argv[1]), M.__file__
n, reps, warm = 64, 31, 6
cfg = abi.Config()
pose = M.getBuiltinPoses()[1]
base = M.synthetic_skin("S64")
skins = np.stack([base] * n)
for i in range(n):
    skins[i, ..., 0] ^= np.uint8(i & 255)
batch = M.SkinBatch(n, "S64", pose)
stream = torch.cuda.current_stream()
for _ in range(warm):
    batch.render(skins, cfg, rgba8=True)
host = []
for _ in range(reps):
    t = time.perf_counter()
    batch.render(skins, cfg, rgba8=True)
    host.append((time.perf_counter() - t) * 1e3)
d_skins = torch.from_numpy(skins).cuda()
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for _ in range(warm + 2):
    M.set_skins_batch_device(batch.scenes, d_skins.data_ptr(), stream=stream.cuda_stream)
torch.cuda.synchronize()
dev = []
for _ in range(reps):
    t0.record(stream)
    M.set_skins_batch_device(batch.scenes, d_skins.data_ptr(), stream=stream.cuda_stream)
    t1.record(stream)
    t1.synchronize()
    dev.append(t0.elapsed_time(t1))
batch.close()
s = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
print(json.dumps({"tree": sys.argv[2], "render_host_ms": s(host), "repaint_event_ms": s(dev)}), flush=True)
