"""The generators of tests/batch_fuzz_cases.py alone, on the CPU, over exactly the seeds tests/test_gpu_batch_fuzz.py uses: what
that file relies on, so that neither a frame of constants nor two swapped frames can pass it.  The oracle's totals equal the
recorded constants; the frames of a batch differ from each other; almost every frame holds a hit; most batches are inside the
batched envelope and some are not; a quarter read their tile seeds; every pass batch holds shadow, penumbra and mirror images."""
import numpy as np
import pytest

import batch_fuzz_cases as B
import pass_fuzz_cases as PF


def _same_scene(a, b) -> bool:
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_scene(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same_scene(x, y) for x, y in zip(a, b))
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_batches_are_deterministic_and_drawn_as_described(mcrt):
    sizes, modes, gaps, leads, outputs, hbm = set(), set(), set(), set(), set(), 0
    for seed in B.all_beauty_seeds():
        sds, cfg, background, layout, what = B.make_beauty_batch(seed)
        sizes.add(len(sds)), modes.add(background), gaps.add(layout["gap"]), leads.add(layout["lead"]), outputs.add(layout["outputs"])
        hbm += "boxes70" in what
        assert cfg.threadCount == 0 and 9 <= cfg.width < 150 and 9 <= cfg.height < 110
    assert sizes == set(B.SIZES) and modes == {"reference", "transparent"} and outputs == {"both", "f32", "u8"}
    assert gaps == {0, 1, 100} and leads == {0, 1, 2}
    assert hbm >= 3  # about one batch in eight: the 70-box scene, whose tables no LDS view takes
    for seed in B.all_beauty_seeds()[:6]:
        a, b = B.make_beauty_batch(seed), B.make_beauty_batch(seed)
        assert a[2:] == b[2:] and bytes(a[1].to_c()) == bytes(b[1].to_c())
        assert all(_same_scene(x.to_numpy(), y.to_numpy()) for x, y in zip(a[0], b[0]))


def test_the_frames_of_a_batch_differ_the_way_real_batches_do(mcrt):
    """Over the drawn batches: mesh counts from one box to the 70, coordinate magnitudes six orders apart and point lights beside
    wide ones WITHIN single batches."""
    spans, lights, counts = [], [], []
    for seed in B.all_beauty_seeds():
        nps = [sd.to_numpy() for sd in B.make_beauty_batch(seed)[0]]
        mags = [PF.mask_slack(s) for s in nps]
        spans.append(max(mags) / min(mags))
        radii = [float(s["light_radius"]) for s in nps]
        lights.append(min(radii) == 0.0 and max(radii) >= 3.0)
        counts.append((min(len(s["meshes"]) for s in nps), max(len(s["meshes"]) for s in nps)))
    assert sum(s >= 1e3 for s in spans) >= 8 and max(spans) >= 1e6
    assert sum(lights) >= 4
    assert sum(lo <= 2 and hi >= 12 for lo, hi in counts) >= 4 and max(hi for _, hi in counts) == 70


def test_the_envelope_and_the_seed_readers(mcrt):
    cfgs = [B.make_beauty_batch(seed)[1] for seed in B.all_beauty_seeds()]
    inside = sum(B.expected_envelope(c) for c in cfgs)
    print(f"{inside} of {len(cfgs)} drawn batches are inside the envelope")
    assert 5 * inside >= 4 * len(cfgs) and len(cfgs) - inside >= 2
    device_form = cfgs + [B.make_special_batch(name)[1] for name in B.SPECIALS if name != "three-hundred"]
    big = sum(B.draws_per_pixel(c) > 24 for c in device_form)
    print(f"{big} of {len(device_form)} device-form batches draw more than 24 numbers per pixel; {sum(B.draws_per_pixel(c) > 24 for c in cfgs)} of the drawn ones")
    assert 4 * big >= len(device_form) and 4 * sum(B.draws_per_pixel(c) > 24 for c in cfgs) >= len(cfgs)
    # the restated rule at its edges
    from minecraftskin_raytracer_amd import abi
    assert B.expected_envelope(abi.Config(maxBounces=8)) and not B.expected_envelope(abi.Config(maxBounces=9))
    assert B.expected_envelope(abi.Config(shadowSamples=113)) and not B.expected_envelope(abi.Config(shadowSamples=114))
    assert B.expected_envelope(abi.Config(shadowSamples=114, softShadows=False))
    assert B.expected_envelope(abi.Config(aoEnabled=True, aoSamples=113)) and not B.expected_envelope(abi.Config(aoEnabled=True, aoSamples=114))
    assert not B.expected_envelope(abi.Config(aoEnabled=True, aoSamples=0)) and B.expected_envelope(abi.Config(aoSamples=0))
    assert B.expected_batch_info(abi.Config(), 300) == {"batched_frames": 300, "launch_sequences": 2}
    assert B.expected_batch_info(abi.Config(maxBounces=9), 5) == {"batched_frames": 0, "launch_sequences": 5}


@pytest.mark.parametrize("first", list(B.BEAUTY_BLOCKS))
def test_the_oracle_holds_the_blocks_hits_and_its_frames_differ(oracle, first):
    total = 0
    for seed in B.block_seeds(first):
        (sds, cfg, background, layout, what), exp = B.beauty_expectation(oracle, seed)
        empty, same = B.distinct_frames(exp)
        assert same == 0, f"{what}: {same} frames with a hit equal another frame of the batch"
        assert len(sds) < 2 or len(sds) - empty >= 2, f"{what}: fewer than two frames with a hit"
        total += sum(h for _, h in exp)
    assert total == B.BEAUTY_BLOCKS[first], f"block {first}: the oracle holds {total} hit pixels, not {B.BEAUTY_BLOCKS[first]}: the generator differs"


def test_frames_without_a_hit_are_rare(oracle):
    frames = empty = 0
    for seed in B.all_beauty_seeds():  # (computed once per process: the blocks' test above has them)
        exp = B.beauty_expectation(oracle, seed)[1]
        frames += len(exp)
        empty += B.distinct_frames(exp)[0]
    print(f"{empty} of {frames} frames hold no hit")
    assert frames > 200 and 20 * empty <= frames


@pytest.mark.parametrize("name", B.SPECIALS)
def test_the_oracle_holds_the_special_batches_hits(oracle, name):
    (sds, cfg, background, layout, what), exp = B.beauty_expectation(oracle, name)
    empty, same = B.distinct_frames(exp)
    assert (sum(h for _, h in exp), empty, same) == B.SPECIAL_TOTALS[name], what
    assert len(sds) - empty >= min(len(sds), 2)
    assert B.expected_envelope(cfg)


def test_the_special_configs_reach_what_they_are_for(mcrt):
    """The planning rules of render_plan.cpp restated for the special configs: kSlabMinSpp = 33 samples for the background
    kernel where the background's draws are not made in plan_tiles; a tile stream of at least 128 twists of 624 draws."""
    cfg = {name: B.make_special_batch(name)[1] for name in B.SPECIALS}
    for name in ("bg-kernel-33", "bg-kernel-40", "four-waves"):
        assert cfg[name].samplesPerPixel >= 33 and B.draws_per_pixel(cfg[name]) > 24 and cfg[name].gradientBg
    for name in ("four-waves", "four-waves-transparent"):
        c = cfg[name]
        tile_draws = min(c.tileSize, c.width) * min(c.tileSize, c.height) * B.draws_per_pixel(c)
        assert -(-tile_draws // 624) >= 128
    assert B.draws_per_pixel(cfg["dof-13"]) == 52 and cfg["dof-13"].tileSize == 50
    assert len(B.make_special_batch("alone")[0]) == 1
    sds, c, _, _, _ = B.make_special_batch("three-hundred")
    assert len(sds) == 300 and (c.width, c.height, c.tileSize, c.maxBounces, c.samplesPerPixel) == (24, 17, 8, 1, 2)


@pytest.mark.parametrize("key", list(B.PASS_BATCHES), ids=B.PASS_IDS)
def test_the_oracle_holds_the_pass_batches_totals(oracle, key):
    import reflection_checker as R

    batch, ground, reflection, surfaces = B.pass_expectation(oracle, key)
    sds, cfg, heights, (k, second), what = batch
    assert len(sds) == 16 and 17 <= cfg.width < 57 and 13 <= cfg.height < 41 and 1 <= cfg.maxBounces <= 3
    assert second != heights[k] and np.isfinite(np.float32(second))
    for e in reflection:
        R.assert_miss_constants(e)
    totals = B.pass_totals(ground, reflection, surfaces)
    assert totals == B.PASS_BATCHES[key], f"{what}: the oracle holds {totals}, not {B.PASS_BATCHES[key]}: the generator differs"
    assert min(totals[:3]) >= 100
    # the frame listed twice differs at its two heights
    assert ground[k]["distance"].tobytes() != ground[16]["distance"].tobytes()
    if key[0] == "mixed":  # magnitudes many orders apart within one launch
        slack = [PF.mask_slack(sd.to_numpy()) for sd in sds]
        assert max(slack) / min(slack) >= 1e3
