"""The ground-occlusion fuzz generator (tests/ground_occlusion_fuzz_cases.py) on the CPU: its cases are reproducible, hit every class
it names within the first 200 seeds, stay inside what the pass accepts, and a few of them agree with what the classes claim."""
import numpy as np

import ground_occlusion_fuzz_cases as F

SEEDS = 200


def test_the_first_seeds_hit_every_class(mcrt):
    seen = {}
    for seed in range(SEEDS):
        sd, cfg, ground, what, classes = F.make_case(seed)
        assert classes <= set(F.CLASSES), classes - set(F.CLASSES)
        assert 1 <= cfg.aoSamples <= 113 and np.isfinite(cfg.aoRadius) and np.isfinite(ground), what
        assert 1 <= cfg.width <= 96 and 1 <= cfg.height <= 96 and 4 <= cfg.tileSize <= 32, what
        n = sd.desc.n_meshes
        assert n <= 12 or 48 <= n <= 80, what
        for c in classes:
            seen[c] = seen.get(c, 0) + 1
    missing = [c for c in F.CLASSES if c not in seen]
    print({c: seen.get(c, 0) for c in F.CLASSES})
    assert not missing, missing


def test_cases_are_reproducible(mcrt):
    for seed in (0, 7, 133):
        a, b = F.make_case(seed), F.make_case(seed)
        assert a[3] == b[3] and a[4] == b[4] and a[2] == b[2]
        assert mcrt.flatten(a[0]) == mcrt.flatten(b[0])


def test_the_classes_describe_the_case(mcrt):
    for seed in range(40):
        sd, cfg, ground, what, classes = F.make_case(seed)
        cam_y = float(sd.desc.camera_position[1])
        if "below the plane" in classes:
            assert cam_y < ground, what
        if "above the plane" in classes:
            assert cam_y > ground, what
        lo = mcrt.scene_floor(sd)
        if "at the floor" in classes:
            assert ground == lo, what
        if "below the scene" in classes:
            assert ground < lo, what
        if "inside the scene" in classes:
            assert ground > lo, what
        if "more than 64 meshes" in classes:
            assert sd.desc.n_meshes > 64, what
        if "radius zero" in classes:
            assert cfg.aoRadius == 0.0, what


def test_batches_share_one_config(mcrt):
    for seed in range(6):
        sds, cfg, heights, what = F.make_batch(seed)
        assert 2 <= len(sds) == len(heights) <= 5 and cfg.width <= 40 and cfg.height <= 30, what
