"""Long randomised parity sweep: HIP path vs the CPU oracle, bit-exact.  usage: gpu_fuzz.py <first_seed> <count> [mode]
The beauty render (TileRenderer.render):
  (none)       fuzz_cases.make_case
  bundle       the cases aimed at the whole-bundle shadow decisions, fuzz_cases.make_bundle_case
  wide         the same scenes scaled by 1e-5 ... 1e6 or moved up to 3e6 away from the origin, fuzz_cases.make_wide_case
The scene-only passes (tests/pass_fuzz_cases.py), every plane of a pass, bit for bit:
  ground       renderGround on make_pass_case: odd seeds wide, every third seed under a light lifted clear above every mesh
  reflection   renderReflection on make_pass_case, odd seeds wide
  layers       renderLayers on make_pass_case, odd seeds wide: depth, normal, albedo, and the texel the id plane names
  long-shadow  renderGround and renderReflection on make_long_shadow_case: ground points 200 ... 30 000 out along a shadow
  far-plane    renderGround and renderReflection on make_far_plane_case: planes 10 ... 10 000 scene heights down
A mismatch prints the case, the plane, the number of differing pixels and the first of them; the exit status is then 1.  After
a HIP error (exit status 2) nothing more is started.  MCRT_BUNDLE_DECISIONS=0 / MCRT_REFLECT_CULL=0 in the environment render
without the whole-bundle decisions / the reflection's tile culling: a mismatch that goes away with one is that shortcut's."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import minecraftskin_raytracer_amd as M
import oraclelib
from fuzz_cases import make_bundle_case, make_case, make_wide_case

first, count = int(sys.argv[1]), int(sys.argv[2])
mode = sys.argv[3] if len(sys.argv) > 3 else ""
PASS_MODES = ("ground", "reflection", "layers", "long-shadow", "far-plane")
if mode not in ("", "bundle", "wide") + PASS_MODES:
    sys.exit(f"unknown mode {mode!r}")


def pass_sweep():
    import ground_checker as G, layers_checker as L, pass_fuzz_cases as PF, reflection_checker as R
    from minecraftskin_raytracer_amd._lib import McrtError

    def differing(got, exp, what):
        """(plane, differing pixels, first (y, x)) of the planes that are not bit for bit the expectation's"""
        out = []
        for k in got:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
            if a.dtype == np.float32:
                ne = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
            else:
                ne = a != b
            if ne.ndim == 3:
                ne = ne.any(axis=-1)
            if ne.any():
                y, x = np.argwhere(ne)[0]
                out.append(f"MISMATCH {what}: plane {k}: {int(ne.sum())} pixels differ; first (y, x) = ({y}, {x}): {got[k][y, x]} vs {exp[k][y, x]}")
        return out

    orc = oraclelib.Oracle()
    bad = pixels = shadowed = hits = 0
    t0 = time.time()
    for seed in range(first, first + count):
        if mode in ("ground", "reflection", "layers"):
            sd, cfg, ground, what = PF.make_pass_case(seed, wide=bool(seed & 1), lift_light=mode == "ground" and seed % 3 == 0)
        else:
            sd, cfg, ground, what = PF.GROUPS[mode](seed)
        lines = []
        try:
            if mode in ("ground", "long-shadow", "far-plane"):
                exp = G.expected_ground(orc, sd, cfg, ground)
                lines += differing(M.TileRenderer.renderGround(sd, cfg, ground), exp, what + " | ground")
                pixels += int(exp["reached"].sum()); shadowed += int((exp["visibility"] < 1).sum())
            if mode in ("reflection", "long-shadow", "far-plane"):
                exp = R.expected_reflection(orc, sd, cfg, ground)
                R.assert_miss_constants(exp)
                lines += differing(M.TileRenderer.renderReflection(sd, cfg, ground), exp, what + " | reflection")
                hits += int(exp["hit"].sum())
            if mode == "layers":
                exp = L.expected_surfaces(orc, sd, cfg.width, cfg.height)
                got = M.TileRenderer.renderLayers(sd, cfg)
                lines += differing({k: got[k] for k in ("depth", "normal", "albedo")}, exp, what + " | layers")
                try:
                    L.assert_ids_name_the_surfaces(got["id"], exp, sd.to_numpy(), what + " | layers")
                except AssertionError as e:
                    lines.append(f"MISMATCH {str(e)[:500]}")
                hits += int(exp["hit"].sum())
        except McrtError as e:
            print(f"HIP ERROR {what}: {e}", flush=True)
            print(f"fuzz {mode}: stopped at seed {seed} after {seed - first} cases, {bad} mismatch(es)")
            sys.exit(2)
        if lines:
            bad += 1
            print("\n".join(lines), flush=True)
        if (seed - first) % 100 == 99:
            print(f"... {seed - first + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz {mode}: {count} cases from seed {first}: {bad} mismatch(es); the oracle holds {pixels} ground pixels, {shadowed} of them "
          f"shadowed, and {hits} hits")
    sys.exit(1 if bad else 0)


if mode in PASS_MODES:
    pass_sweep()
if len(sys.argv) > 3 and sys.argv[3] == "bundle":
    make_case = make_bundle_case
if len(sys.argv) > 3 and sys.argv[3] == "wide":
    make_case = make_wide_case
orc = oraclelib.Oracle()
bad = 0
t0 = time.time()
for seed in range(first, first + count):
    sd, cfg, what = make_case(seed)
    img = M.TileRenderer.render(sd, cfg)
    ref = orc.render(sd.ptr, cfg)
    errs = M.TileRenderer.lastErrors()
    same = np.array_equal(img.view(np.uint32), ref.view(np.uint32)) or (np.isnan(img) == np.isnan(ref)).all() and np.array_equal(np.nan_to_num(img), np.nan_to_num(ref))
    if errs or not same:
        bad += 1
        diff = int((img.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"MISMATCH {what}: errors={errs} differing floats={diff} max abs diff={np.nanmax(np.abs(img - ref))}", flush=True)
    if (seed - first) % 50 == 49:
        print(f"... {seed - first + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
print(f"fuzz: {count} cases from seed {first}: {bad} mismatch(es)")
sys.exit(1 if bad else 0)
