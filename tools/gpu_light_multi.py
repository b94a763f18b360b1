"""What the per-light light layers and bake cost on the device, against the single-light passes:

  layers   1920 x 1080, S = 8 soft shadows, the default figure (pose 0): visibility and direct
  bake     the 3264-texel repaintable S64 figure with an opaque skin, grid 2: visibility and direct

  old_K0      render_light_device / bake_light_device, no extra light: the single-light kernels (`shade`, `bake_shade`)
  new_K0 no sum  the same planes as old_K0 through the new kernels: visibility[0] and direct[0], no combined plane
  new_K0..K3  render_light_multi_device / bake_light_multi_device on a handle with K extra lights: visibility[k] and direct[k] for
              k = 0 .. K and combined (`shade_lights`, `bake_shade_lights`)
  old_x(K+1)  K + 1 calls of the single-light pass on K + 1 handles whose scene light is light k — the only way to per-light planes
              before (ambient on every light and no sum: the planes are not the same, the work is what is compared).  The handles
              are built beforehand, so this row leaves out the K set_view launches a single handle would need between the calls.

the ways alternated in one process: device events around `iters` calls per reading, warm-ups first, then repetitions with the
order of the ways reversed every other time; median and min-max per way, ms per call.  Before the timing new_K0's visibility[0]
and direct[0] are compared with old_K0's planes (they must be equal) and new_K3's combined with its direct[0] (they must differ).

    python tools/gpu_light_multi.py [--reps 9] [--warmup 3] [--iters 20] [--json out.json] [--txt out.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--txt")
    a = ap.parse_args()
    import torch

    import minecraftskin_raytracer_amd as M
    from minecraftskin_raytracer_amd import abi
    import scenes

    lights = [abi.Light((-30.0, 20.0, 30.0), (0.35, 0.4, 0.5, 1.0), 4.0), abi.Light((25.0, 5.0, 10.0), (0.9, 0.8, 0.6, 1.0), 3.0),
              abi.Light((0.0, -10.0, 25.0), (0.3, 0.1, 0.1, 1.0), 10.0)]
    stream = torch.cuda.current_stream().cuda_stream
    w, h = 1920, 1080
    cfg = abi.Config(width=w, height=h, softShadows=True, shadowSamples=8)
    sd = scenes.skin_scene("S64", 0)

    def relit(k):  # a description of the figure whose own light is extra light k (its position, radius and colour)
        d = scenes.skin_scene("S64", 0)
        if k:
            c = lights[k - 1].to_c()
            for i in range(3):
                d.desc.light_position[i] = c.position[i]
            for i in range(4):
                d.desc.light_color[i] = c.color[i]
            d.desc.light_radius = c.radius
        return d

    f1 = [torch.zeros(w * h, dtype=torch.float32, device="cuda") for _ in range(4)]
    f4 = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda") for _ in range(5)]
    old_f1, old_f4 = torch.zeros(w * h, dtype=torch.float32, device="cuda"), torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    per_light = [M.DeviceScene(relit(k)) for k in range(4)]
    multi = []
    for k in range(4):
        ds = M.DeviceScene(sd)
        ds.set_extra_lights(lights[:k])
        multi.append(ds)

    def layers_new(k, total=True):
        multi[k].render_light_multi_device(cfg, [t.data_ptr() for t in f1[:k + 1]], [t.data_ptr() for t in f4[:k + 1]], 0, f4[4].data_ptr() if total else 0, stream)

    def layers_old(n):
        for k in range(n):
            per_light[k].render_light_device(cfg, visibility_ptr=f1[k].data_ptr(), direct_ptr=f4[k].data_ptr(), stream=stream)

    # ---- the bake: a repaintable S64 handle (3264 texels, every one live under an opaque skin), grid 2
    import layers_checker as L

    skin = L.unique_skin("S64").copy()
    skin[..., 3] = 255
    pose = M.getBuiltinPoses()[0]
    n_tex = 3264
    b1 = [torch.zeros(n_tex, dtype=torch.float32, device="cuda") for _ in range(4)]
    b4 = [torch.zeros(n_tex * 4, dtype=torch.float32, device="cuda") for _ in range(5)]
    bake_multi, bake_single = [], []
    for k in range(4):
        ds = M.DeviceScene.for_skin("S64", pose)
        ds.set_skin(skin)
        ds.set_extra_lights(lights[:k])
        bake_multi.append(ds)
        ds = M.DeviceScene.for_skin("S64", pose, look=relit(k) if k else None)
        ds.set_skin(skin)
        bake_single.append(ds)
    assert bake_multi[0].texels == n_tex
    bcfg = abi.Config(softShadows=True, shadowSamples=8)

    def bake_new(k, total=True):
        bake_multi[k].bake_light_multi_device(bcfg, 2, visibility_ptrs=[t.data_ptr() for t in b1[:k + 1]], direct_ptrs=[t.data_ptr() for t in b4[:k + 1]],
                                              combined_ptr=b4[4].data_ptr() if total else 0, stream=stream)

    def bake_old(n):
        for k in range(n):
            bake_single[k].bake_light_device(bcfg, 2, visibility_ptr=b1[k].data_ptr(), direct_ptr=b4[k].data_ptr(), stream=stream)

    # ---- the results first
    per_light[0].render_light_device(cfg, visibility_ptr=old_f1.data_ptr(), direct_ptr=old_f4.data_ptr(), stream=stream)
    layers_new(0)
    torch.cuda.synchronize()
    assert torch.equal(f1[0].view(torch.int32), old_f1.view(torch.int32)) and torch.equal(f4[0].view(torch.int32), old_f4.view(torch.int32)), "K = 0: the planes differ"
    layers_new(3)
    torch.cuda.synchronize()
    changed = int((f4[4].view(torch.int32) != f4[0].view(torch.int32)).view(-1, 4).any(dim=1).sum().item())
    assert changed > 10000, f"K = 3: combined differs from direct[0] on {changed} pixels only"
    bake_new(3)
    torch.cuda.synchronize()
    bchanged = int((b4[4].view(torch.int32) != b4[0].view(torch.int32)).view(-1, 4).any(dim=1).sum().item())
    assert bchanged > 300, f"bake K = 3: combined differs from direct[0] on {bchanged} texels only"
    for ds in per_light + multi + bake_multi + bake_single:
        ds.check()

    ways = {}
    for fam, new, old in (("layers", layers_new, layers_old), ("bake", bake_new, bake_old)):
        ways[f"{fam} old_K0"] = lambda old=old: old(1)
        ways[f"{fam} new_K0 no sum"] = lambda new=new: new(0, False)
        for k in range(4):
            ways[f"{fam} new_K{k}"] = lambda new=new, k=k: new(k)
        for k in range(1, 4):
            ways[f"{fam} old_x{k + 1}"] = lambda old=old, k=k: old(k + 1)

    def reading(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    names = list(ways)
    for _ in range(a.warmup):
        for n in names:
            reading(ways[n])
    times = {n: [] for n in names}
    for r in range(a.reps):
        for n in (names if r % 2 == 0 else names[::-1]):
            times[n].append(reading(ways[n]))
    rows = {n: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for n, t in times.items()}
    lines = [f"device {torch.cuda.get_device_name(0)}; {a.reps} repetitions of {a.iters} calls per way, {a.warmup} warm-ups, the ways alternated",
             f"layers: {w}x{h}, S = 8; K = 3: combined differs from direct[0] on {changed} pixels",
             f"bake: {n_tex} texels, grid 2, S = 8; K = 3: combined differs from direct[0] on {bchanged} texels",
             f"{'way':<22}{'median ms':>12}{'min':>10}{'max':>10}"]
    lines += [f"{n:<22}{r['median_ms']:>12.4f}{r['min_ms']:>10.4f}{r['max_ms']:>10.4f}" for n, r in rows.items()]
    text = "\n".join(lines)
    print(text)
    if a.txt:
        open(a.txt, "w").write(text + "\n")
    if a.json:
        json.dump(dict(rows=rows, reps=a.reps, iters=a.iters, layers_changed=changed, bake_changed=bchanged), open(a.json, "w"), indent=1)
    for ds in per_light + multi + bake_multi + bake_single:
        ds.close()


if __name__ == "__main__":
    main()
