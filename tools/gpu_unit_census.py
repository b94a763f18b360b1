"""Census of the work units `plan_tiles` queues for a named scenario of tools/gpu_case.py (mcrt_probe_units), under whatever
MCRT_UNIT_BLOCKS the environment sets: touched tiles, units, units without a primary hit and the samples in them.  One JSON
line per scenario.

    python tools/gpu_unit_census.py base [4k_b4 ...]
"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import minecraftskin_raytracer_amd as M
import scenes

CASES = {
    "base": dict(width=1920, height=1080, maxBounces=4, samplesPerPixel=4),
    "4k_b4": dict(width=3840, height=2160, maxBounces=4, samplesPerPixel=4),
}
for name in sys.argv[1:]:
    cfg = M.Config(**CASES[name])
    ds = M.DeviceScene(scenes.skin_scene("S64", 0))
    ds.set_lanes(1)
    frame = torch.empty((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    for _ in range(4):  # the plates exist from the second render on
        ds.render_device(cfg, frame.data_ptr())
    torch.cuda.synchronize()
    u = ds.units()
    rec, hits = u["records"], u["hits"].astype(np.int64)
    block = (rec[:, 0] >> 31) == 1
    pixels = np.where(block, (rec[:, 2] & 0xffff).astype(np.int64) * (rec[:, 2] >> 16), rec[:, 2].astype(np.int64) - rec[:, 1])
    spp = max(cfg.samplesPerPixel, 1)
    print(json.dumps({
        "case": name, "knobs": {k: os.environ.get(k) for k in ("MCRT_UNIT_BLOCKS",)},
        "touched_tiles": int(len(np.unique(rec[:, 0] & 0x7fffffff))), "units": int(len(rec)), "units_without_hit": int((hits == 0).sum()),
        "samples_queued": int(pixels.sum() * spp), "samples_in_units_without_hit": int(pixels[hits == 0].sum() * spp),
        "primary_hits": int(hits.sum())}))
    ds.check()
