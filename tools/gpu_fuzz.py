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
The light layers (tests/light_checker.py), visibility, occlusion and direct bit for bit:
  light        render_light_device on light_checker.sweep_case(seed): make_pass_case, make_wide_pass_case and make_bundle_case in
               turn, AO settings drawn per case (1 ... 113 samples, a radius of 0.01 ... 10 scene heights); every fourth case into
               planes 1 or 2 floats off their allocation, every other case also twice through the batched kernels; the summary
               records the hits, penumbra hits and partly occluded hits compared
Extra lights (tests/extra_lights_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_extra_lights_fuzz.py):
  lights       render_device_ex on extra_lights_fuzz_cases.sweep_case(seed): make_bundle_case and make_pass_case in turn, frames of at
               most 64 x 64 at 1 spp, 1 ... 3 extra lights inside, below, behind and around the figure, radius 0 ... 25, colours 0 ... 2,
               against tests/extra_lights_checker.py; every other case also through the one-shot form; the summary records the hits,
               the hits the extra lights changed, the hits over 1 before the clamp and the penumbra pairs compared
The light bake (tests/bake_checker.py), position, normal, visibility, occlusion and direct of every pool texel bit for bit:
  bake         bake_light_device on bake_checker.sweep_case(seed): light's cases, grid 1 + seed % 4; every fourth case into planes 1 or
               2 floats off their allocation, every other case also twice through the batched kernels; the summary records the
               texels and the live, dark, penumbra and partly occluded texels compared
The batched entries (tests/batch_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_batch_fuzz.py):
  batch        render_batch_device on make_beauty_batch(seed): 1 ... 16 frames of mixed scenes under one config, fresh and stale
               tile seeds, a lead and a stride gap; every third seed also through TileRenderer.renderBatch
  pass-batch   render_layers / ground / reflection_batch_device on 16 scenes under one config, each at its own plane height: the
               groups bundle, wide, long-shadow and far-plane in turn from seed first + 16 k, every fifth batch four cases of each
For these a mismatch prints the batch, the frame index, the plane, the count and the first pixel.
The limits of the scene tables (tests/big_scene_cases.py; the runs and comparisons are those of tests/test_gpu_big_scene_fuzz.py):
  big          seed k is make_big_case(k, ("count", "posed", "texels")[k % 3]): 48 ... 200 boxes around the 64-mesh limit of the masks,
               culling, decisions and groups; posed figures among 40 ... 140 meshes; texel pools of 65 520 ... 90 000 texels; every
               fourth case of a group under a general-variant config.  Per case the beauty render (host and device form, every third
               transparent), intersect on 1 500 rays, ground, reflection, layers with picks and the light planes; the summary
               records the census of what the oracle's planes held (big_scene_cases.CENSUS); a case whose expectation cannot be
               made (the generator's own assertions) ends the run with exit status 3
Repaintable resident scenes (tests/resident_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_resident_fuzz.py):
  resident     seed k is make_script(k): 2 ... 4 handles of DeviceScene.for_skin walked through repaints, views, background modes,
               renders (some until the launch graph replays), the single and batched passes, picks and blob checkpoints on two
               streams, even seeds with a stretch of more than kTableSlots batch calls without a host wait; every checkpoint
               against the oracle and the host flattener; the summary records the scripts, the checkpoints compared by kind and
               the census of what the oracle saw (resident_fuzz_cases.census)
The studio shot (tests/shot_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_shot_fuzz.py):
  shot         even seeds are make_blend_case(seed): planes of 1 ... 70 x 1 ... 40 pixels and 1 ... 6 frames drawn per pixel from
               classes of values (denormals, the quantiser's boundaries, dR at and beside fade, infinities, values up to 1e18),
               three runs each through composite_shot_batch_device with leads, absent inputs and lone outputs of their own, against
               shot_checker.compose; odd seeds are make_shot_case(seed): 1 ... 4 scenes of random skins and views, two calls through
               the batched, single, host and PNG forms against the CPU oracle alone; the summary records the pixels compared and
               the oracle's totals of shot_checker.classes
The shot as a cut-out (tests/cutout_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_cutout_fuzz.py):
  cutout       even seeds k are make_blend_case(k // 2): the shot mode's planes with vis above 1 and below 0 and an occlusion plane
               from the same classes, o and the shadow colour from classes of their own, the transparent page at five places of
               eight (an opaque page with a black shadow and o > 0 takes the _occ entry), boxes asked for behind a lead, against
               cutout_checker.compose_ex and bounds_of; odd seeds k are make_shot_case(k // 2): 1 ... 4 scenes (S64, S32, slim), two
               calls through the batched, single, host, PNG, cropped PNG and SkinBatch forms with the refusals beside them, against
               the CPU oracle alone; the summary records the pixels compared and the oracle's totals of cutout_checker.classes
The ground-occlusion pass (tests/ground_occlusion_fuzz_cases.py; the runs and comparisons are those of tests/test_gpu_ground_occlusion_fuzz.py):
  ground_occlusion   seed k is make_case(k): skins and 48 ... 80-mesh box scenes, posed and not, scaled by 1e-3 ... 1e3, cameras above,
               below and grazing the plane, planes at, below, inside and above the scene, 1 ... 113 samples, radii from 0 to larger than
               the scene, frames of 1 ... 96 pixels a side; every third seed also through the device form into planes off their
               alignment, every eighth seed also make_batch(k) through the batched kernel; the summary records the reached and the
               occluded pixels the oracle held
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
BATCH_MODES = ("batch", "pass-batch")
if mode not in ("", "bundle", "wide", "light", "lights", "bake", "big", "resident", "shot", "cutout", "ground_occlusion") + PASS_MODES + BATCH_MODES:
    sys.exit(f"unknown mode {mode!r}")


def batch_sweep():
    import batch_fuzz_cases as B, test_gpu_batch_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the oracle's frames are made ahead of the device by worker processes (forked before the device is first used; they never
    # use it), in the order of the batches
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    keys = [("mixed", first + 16 * k) if k % 5 == 4 else (B.PASS_GROUPS[k % 4], first + 16 * k) for k in range(count)]
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(B.worker_beauty_frames, range(first, first + count)) if mode == "batch" else pool.imap(B.worker_pass_expectation, keys)
    bad = frames = total = inside = 0
    previous, what = None, ""
    t0 = time.time()
    for k in range(count):
        lines = []
        try:
            if mode == "batch":
                seed = first + k
                case = B.make_beauty_batch(seed)
                what = case[4]
                exp = next(ahead)
                handles = [M.DeviceScene(sd) for sd in case[0]]
                try:
                    lines += T.run_beauty_batch(M, handles, case, exp, previous, single=seed)
                    for h in handles:
                        h.check()
                finally:
                    for h in handles:
                        h.close()
                if seed % 3 == 0:
                    lines += T.run_host_batch(M, case, exp)
                previous = case[1]
                frames += len(exp); total += sum(h for _, h in exp); inside += B.expected_envelope(case[1])
            else:
                what = f"pass batch {keys[k]}"
                batch = B.make_pass_batch_of(keys[k])
                ground, reflection, surfaces = next(ahead)
                lines += T.run_pass_batch(M, batch, ground, reflection, surfaces)
                frames += len(ground); total += np.asarray(B.pass_totals(ground, reflection, surfaces))
        except McrtError as e:
            print(f"HIP ERROR {what}: {e}", flush=True)
            print(f"fuzz {mode}: stopped at batch {k} of {count} from seed {first}, {bad} mismatching batch(es)")
            pool.terminate()
            sys.exit(2)
        if lines:
            bad += 1
            print("\n".join(lines[:20]), flush=True)
        if k % 50 == 49:
            print(f"... {k + 1} batches, {bad} mismatching, {time.time() - t0:.0f} s", flush=True)
    if mode == "batch":
        print(f"fuzz batch: {count} batches from seed {first}: {bad} mismatching batch(es); {frames} frames, {inside} batches inside the "
              f"batched envelope; the oracle holds {total} hit pixels")
    else:
        d, p, r, l = (int(x) for x in np.atleast_1d(total))
        print(f"fuzz pass-batch: {count} batches from seed {first}: {bad} mismatching batch(es); {frames} ground frames; the oracle holds "
              f"{d} dark, {p} penumbra, {r} reflected and {l} layer-hit pixels")
    pool.terminate()
    sys.exit(1 if bad else 0)


def light_sweep():
    import light_checker as LC, test_gpu_light_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the oracle's planes are made ahead of the device by worker processes (forked before the device is first used; they never
    # use it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(LC.worker_sweep_expectation, range(first, first + count))
    bad = 0
    total = np.zeros(5, np.int64)
    t0 = time.time()
    for k, seed in enumerate(range(first, first + count)):
        case = LC.sweep_case(seed)
        exp = next(ahead)
        LC.assert_miss_constants(exp)
        try:
            lines = T.run_case(M, case, exp, T.lead_of(k), twice=k % 2 == 0)
        except McrtError as e:
            print(f"HIP ERROR {case[2]}: {e}", flush=True)
            print(f"fuzz light: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(2)
        total += np.asarray(LC.counts(exp))
        if lines:
            bad += 1
            print("\n".join("MISMATCH " + l for l in lines[:20]), flush=True)
        if k % 100 == 99:
            print(f"... {k + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz light: {count} cases from seed {first}: {bad} mismatch(es); the oracle holds {int(total[0])} hits, {int(total[1])} of them dark and "
          f"{int(total[2])} in the penumbra, and {int(total[3])} partly occluded hits ({int(total[4])} fully occluded)")
    pool.terminate()
    sys.exit(1 if bad else 0)


def lights_sweep():
    import extra_lights_fuzz_cases as F, test_gpu_extra_lights_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the expected frames are made ahead of the device by worker processes (forked before the device is first used; they never
    # use it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(F.worker_sweep_expectation, range(first, first + count))
    bad = 0
    total = np.zeros(4, np.int64)
    t0 = time.time()
    for k, seed in enumerate(range(first, first + count)):
        case = F.sweep_case(seed)
        want, counts = next(ahead)
        try:
            lines = T.run_case(M, case, want, one_shot=k % 2 == 0)
        except McrtError as e:
            print(f"HIP ERROR {case[3]}: {e}", flush=True)
            print(f"fuzz lights: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(2)
        total += np.asarray(counts)
        if lines:
            bad += 1
            print("\n".join("MISMATCH " + l for l in lines[:20]), flush=True)
        if k % 100 == 99:
            print(f"... {k + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz lights: {count} cases from seed {first}: {bad} mismatch(es); the oracle holds {int(total[0])} hits, {int(total[1])} of them changed by "
          f"the extra lights, {int(total[2])} over 1 before the clamp, and {int(total[3])} penumbra (hit, extra light) pairs")
    pool.terminate()
    sys.exit(1 if bad else 0)


def bake_sweep():
    import bake_checker as BC, test_gpu_bake_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the oracle's planes are made ahead of the device by worker processes (forked before the device is first used; they never
    # use it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(BC.worker_sweep_expectation, range(first, first + count))
    bad = texels = 0
    total = np.zeros(5, np.int64)
    t0 = time.time()
    for k, seed in enumerate(range(first, first + count)):
        sd, cfg, grid, what = BC.sweep_case(seed)
        exp = next(ahead)
        BC.assert_dead_constants(exp)
        try:
            lines = T.run_case(M, (sd, cfg, what), exp, T.lead_of(k), twice=k % 2 == 0, grid=grid)
        except McrtError as e:
            print(f"HIP ERROR {what}: {e}", flush=True)
            print(f"fuzz bake: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(2)
        total += np.asarray(BC.counts(exp))
        texels += len(exp["table"])
        if lines:
            bad += 1
            print("\n".join("MISMATCH " + l for l in lines[:20]), flush=True)
        if k % 100 == 99:
            print(f"... {k + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz bake: {count} cases from seed {first}: {bad} mismatch(es); the oracle holds {texels} texels, {int(total[0])} of them live, "
          f"{int(total[1])} fully dark, {int(total[2])} in the penumbra, {int(total[3])} partly occluded and {int(total[4])} fully occluded")
    pool.terminate()
    sys.exit(1 if bad else 0)


def big_sweep():
    import big_scene_cases as BS, test_gpu_big_scene_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the oracle's frames and planes are made ahead of the device by worker processes (forked before the device is first used;
    # they never use it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(BS.worker_sweep_expectation, [(first + k, k) for k in range(count)])
    bad = 0
    total = np.zeros(len(BS.CENSUS), np.int64)
    views = {}
    t0 = time.time()
    for k, seed in enumerate(range(first, first + count)):
        case = BS.make_big_case_info(seed, BS.GROUPS[seed % 3])
        try:
            pexp, bexp, census = next(ahead)
        except Exception as e:  # a worker's: the generator's own assertions, or the oracle's
            print(f"CASE ERROR {case[3]}: {type(e).__name__}: {e}", flush=True)
            print(f"fuzz big: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(3)
        try:
            lines = T.run_big_case(M, case, pexp, bexp, k, seed)
        except McrtError as e:
            print(f"HIP ERROR {case[3]}: {e}", flush=True)
            print(f"fuzz big: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(2)
        total += census
        view = BS.B.expected_view(BS.B.flat_header(case[0]))
        views[view] = views.get(view, 0) + 1
        if lines:
            bad += 1
            print("\n".join(lines[:20]), flush=True)
        if k % 50 == 49:
            print(f"... {k + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz big: {count} cases from seed {first}: {bad} mismatch(es); views {dict(sorted(views.items()))}; the oracle holds "
          + ", ".join(f"{int(t)} {name}" for name, t in zip(BS.CENSUS, total)))
    pool.terminate()
    sys.exit(1 if bad else 0)


def resident_sweep():
    import resident_fuzz_cases as RF, test_gpu_resident_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    # the expectations are made ahead of the device by worker processes (forked before the device is first used; they never use
    # it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    RF._transparent_checker()  # built once, before the fork
    pool = multiprocessing.get_context("fork").Pool(workers)
    ahead = pool.imap(RF.worker_script_expectation, range(first, first + count))
    orc = oraclelib.Oracle()
    bad, compared, total = 0, {}, {}
    t0 = time.time()
    for k, seed in enumerate(range(first, first + count)):
        script = RF.make_script(seed)
        exp = next(ahead)
        try:
            lines = T.run_script(M, orc, script, exp, compared)
        except (McrtError, RuntimeError) as e:  # the library's, or torch's at a host wait
            print(f"HIP ERROR script {seed}: {e}", flush=True)
            print(f"fuzz resident: stopped at seed {seed} after {k} scripts, {bad} mismatching script(s)")
            pool.terminate()
            sys.exit(2)
        RF.add_census(total, RF.census([script], [exp]))
        if lines:
            bad += 1
            print("\n".join(lines[:20]), flush=True)
        if k % 50 == 49:
            print(f"... {k + 1} scripts, {bad} mismatching, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz resident: {count} scripts from seed {first}: {bad} mismatching script(s); checkpoints compared {dict(sorted(compared.items()))}; "
          f"{time.time() - t0:.0f} s; the oracle's census {total}")
    pool.terminate()
    sys.exit(1 if bad else 0)


def shot_sweep(cutout=False):
    import tempfile
    import shot_checker as S, test_gpu_shot_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    if cutout:  # the same sweep over the cut-out's cases, runs and classes
        import cutout_checker as X, cutout_fuzz_cases as SF, test_gpu_cutout_fuzz as TC
        run_blend, run_shot, class_names = TC.run_cutout_blend_case, TC.run_cutout_shot_case, X.CLASSES
        classes_of = lambda case, exp: X.classes(exp, case["calls"][0]["shot"])  # noqa: E731
    else:
        import shot_fuzz_cases as SF
        run_blend, run_shot, class_names = T.run_blend_case, T.run_shot_case, S.CLASSES
        classes_of = lambda case, exp: S.classes(exp)  # noqa: E731

    # the oracle's planes of the whole shots (the odd seeds) are made ahead of the device by worker processes (forked before the
    # device is first used; they never use it), in the order of the seeds
    import multiprocessing

    workers = max(1, min(14, len(os.sched_getaffinity(0)) - 2, int(os.environ.get("OMP_NUM_THREADS", "16")) - 2))
    S.transparent_oracle()  # built once, before the fork
    pool = multiprocessing.get_context("fork").Pool(workers)
    seeds = range(first, first + count)
    # (a cut-out case's place in its block is its seed modulo 8 or 4, so there seed k stands for case k // 2 of its kind: every
    # place is met; the shot mode keeps its numbering)
    case_seed = (lambda s: s // 2) if cutout else (lambda s: s)  # noqa: E731
    ahead = pool.imap(SF.worker_shot_expectation, [case_seed(s) for s in seeds if s % 2])
    shared = T._coloured_handles(M, [(0.125, 0.5, 0.75, 1.0), (0.9, 0.1, 0.3, 1.0), (0.0, 1.0, 0.25, 1.0)])
    tmp = tempfile.mkdtemp(prefix="fuzz_shot_")
    bad = blends = shots = pixels = frames = 0
    total = np.zeros(len(class_names), np.int64)
    t0 = time.time()
    for k, seed in enumerate(seeds):
        try:
            if seed % 2 == 0:
                case = SF.make_blend_case(case_seed(seed))
                lines = run_blend(M, shared, case)
                blends += 1; pixels += 3 * case["n"] * case["w"] * case["h"]
            else:
                case = SF.make_shot_case(case_seed(seed))
                exps = next(ahead)
                lines = run_shot(M, case, exps, tmp)
                shots += 1; frames += sum(len(per_scene) for per_scene in exps)
                for exp in exps[0]:
                    total += np.asarray(classes_of(case, exp))
        except (McrtError, RuntimeError) as e:  # the library's, or torch's at a host wait
            print(f"HIP ERROR {mode} seed {seed}: {e}", flush=True)
            print(f"fuzz {mode}: stopped at seed {seed} after {k} cases, {bad} mismatch(es)")
            pool.terminate()
            sys.exit(2)
        if lines:
            bad += 1
            print("\n".join(lines[:20]), flush=True)
        if k % 500 == 499:
            print(f"... {k + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    for h in shared:
        h.close()
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    print(f"fuzz {mode}: {count} cases from seed {first}: {bad} mismatch(es); {blends} blend cases with {pixels} pixels blended, {shots} shot cases "
          f"with {frames} frames; {time.time() - t0:.0f} s; the oracle holds " + ", ".join(f"{int(t)} {name}" for name, t in zip(class_names, total)))
    pool.terminate()
    sys.exit(1 if bad else 0)


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


def ground_occlusion_sweep():
    import test_gpu_ground_occlusion_fuzz as T
    from minecraftskin_raytracer_amd._lib import McrtError

    orc = oraclelib.Oracle()
    bad = reached = occluded = batches = frames = 0
    t0 = time.time()
    for seed in range(first, first + count):
        try:
            lines, r, o = T.run_case(M, orc, seed)
            reached += r; occluded += o
            if seed % 8 == 0:
                more, n = T.run_batch(M, orc, seed)
                lines += more; batches += 1; frames += n
        except (McrtError, RuntimeError) as e:  # the library's, or torch's at a host wait
            print(f"HIP ERROR ground_occlusion seed {seed}: {e}", flush=True)
            print(f"fuzz ground_occlusion: stopped at seed {seed} after {seed - first} cases, {bad} mismatch(es)")
            sys.exit(2)
        if lines:
            bad += 1
            print("\n".join(lines[:20]), flush=True)
        if (seed - first) % 100 == 99:
            print(f"... {seed - first + 1} cases, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"fuzz ground_occlusion: {count} cases from seed {first}: {bad} mismatch(es); {batches} batches with {frames} frames; {time.time() - t0:.0f} s; "
          f"the oracle holds {reached} reached pixels, {occluded} of them with occlusion < 1")
    sys.exit(1 if bad else 0)


if mode == "ground_occlusion":
    ground_occlusion_sweep()
if mode in PASS_MODES:
    pass_sweep()
if mode in BATCH_MODES:
    batch_sweep()
if mode == "light":
    light_sweep()
if mode == "lights":
    lights_sweep()
if mode == "bake":
    bake_sweep()
if mode == "big":
    big_sweep()
if mode == "resident":
    resident_sweep()
if mode == "shot":
    shot_sweep()
if mode == "cutout":
    shot_sweep(cutout=True)
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
