"""Extra lights (include/mcrt.h, "extra lights") on the GPU: every frame bit for bit, as uint32, against the expectation that
tests/extra_lights_checker.py forms from the CPU oracle alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import big_scene_cases as B
import extra_lights_checker as X
import layers_checker as L
import scenes
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
POSE0 = "pose0_default_96x64"
SMALL = "pose0_33x17_t7"
TWO = X.lights_key(X.CASES["fill_left+kicker"])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device(ds, cfg, first=0, step=1, rgba8=False, out=None):
    f32 = out if out is not None else torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    u8 = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.uint8, device="cuda") if rgba8 else None
    ds.render_device_ex(cfg, f32.data_ptr(), u8.data_ptr() if rgba8 else 0, first, step, abi.LAYOUT_FRAME, _stream())
    torch.cuda.synchronize()
    return (f32.cpu().numpy(), u8.cpu().numpy()) if rgba8 else f32.cpu().numpy()


def _render_device(mcrt, sd, cfg, lights, **kw):
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        out = _device(ds, cfg, **kw)
        ds.check()
        return out
    finally:
        ds.close()


def _one_shot(mcrt, sd, cfg, lights, **kw):
    img = mcrt.TileRenderer.render(sd, cfg, lights=lights, **kw)
    assert mcrt.TileRenderer.lastErrors() == []
    return img


# ---- the three pinned cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.CASES))
def test_pinned_cases_equal_the_checker(mcrt, gpu, oracle, name):
    lights = X.CASES[name]
    sd, cfg, want, _ = X.skin_expectation(POSE0, X.lights_key(lights))
    img, img8 = _render_device(mcrt, sd, cfg, lights, rgba8=True)
    scenes.assert_bit_equal(img, want, f"{name}: device form")
    want8 = oracle.quantize(want).reshape(cfg.height, cfg.width, 4)
    assert np.array_equal(img8, want8), f"{name}: RGBA8 plane of the device form"
    scenes.assert_bit_equal(_one_shot(mcrt, sd, cfg, lights), want, f"{name}: one-shot form")
    assert np.array_equal(mcrt.TileRenderer.renderRGBA8(sd, cfg, lights=lights), want8), f"{name}: one-shot RGBA8"
    assert mcrt.TileRenderer.lastErrors() == []


# ---- shadow sampling variants ----------------------------------------------------------------------------------------
# The pinned cases above hold at least 100 changed hits, 30 hits over 1 and 30 penumbra pairs each (tests/test_extra_lights_checker.py).
# The 33 x 17 frame cannot: it has 561 pixels and 40 hits in all (38 ... 40 of them changed, 2 ... 34 over 1, 4 ... 9 penumbra pairs by
# the lights used); it is here for its size — tiles of 7 that no block of 64 lanes divides, two workgroups' worth of pairs at S = 64.
VARIANTS = {
    "hard_ao_1bounce": dict(name=SMALL, lights=TWO, soft=False, bounces=1, ao=True),
    "S5_atomic": dict(name=SMALL, lights=TWO, samples=5),
    "S8": dict(name=SMALL, lights=TWO, samples=8),
    "S64_full_wave": dict(name=SMALL, lights=TWO, samples=64),
    "point_key_disk_fill": dict(name=SMALL, lights=X.lights_key((X.FILL_LEFT,)), key_radius=0.0),
    "disk_key_point_fill": dict(name=SMALL, lights=X.lights_key((X.KICKER,))),
    "spp3_jitter": dict(name="pose5_orbit_64x64_t16", lights=TWO, spp=3),
    "bounces9": dict(name=SMALL, lights=X.lights_key((X.FILL_LEFT,)), bounces=9),  # two reasons for the general variants
    "posed_skin": dict(name="pose6_orbit_96x64", lights=X.lights_key(X.CASES["three"])),
}


@pytest.mark.parametrize("which", list(VARIANTS))
def test_sampling_variants_equal_the_checker(mcrt, gpu, which):
    sd, cfg, want, _ = X.skin_expectation(**VARIANTS[which])
    lights = X.lights_of(VARIANTS[which]["lights"])
    scenes.assert_bit_equal(_render_device(mcrt, sd, cfg, lights), want, f"{which}: device form")
    scenes.assert_bit_equal(_one_shot(mcrt, sd, cfg, lights), want, f"{which}: one-shot form")


def test_black_light_under_spp_dof_and_ao_changes_nothing(mcrt, gpu, oracle):
    # the whole pipeline, lens draws included, where the checker does not go: a light of colour 0 adds exactly +0
    sd = L.skin_case("S64", 6, (135.0, 20.0, 34.0))
    cfg = abi.Config(width=64, height=48, tileSize=16, maxBounces=2, samplesPerPixel=4, dofEnabled=True, aperture=0.4, aoEnabled=True, aoSamples=4)
    black = [abi.Light((-20.0, 25.0, 15.0), (0.0, 0.0, 0.0, 1.0), 5.0)]
    plain = mcrt.TileRenderer.render(sd, cfg)
    assert mcrt.TileRenderer.lastErrors() == []
    lit = _one_shot(mcrt, sd, cfg, black)
    scenes.assert_bit_equal(lit, plain, "black light vs render without lights")
    scenes.assert_bit_equal(lit, oracle.render(sd.ptr, cfg), "black light vs oracle.render")
    scenes.assert_bit_equal(_render_device(mcrt, sd, cfg, black), plain, "black light, device form")


# ---- the three scene views -------------------------------------------------------------------------------------------
def _box_case(mcrt):
    sc, w, h, tile = L.box_scene("outer_back_face")
    return mcrt.SceneDesc(sc), X.config(w, h, tile)


def _many_mesh_case():
    # a posed scene of 140 meshes: the HBM view, at the smallest frame the generator draws (24 x 24)
    sd, _, _, what = B.make_big_case(B.seed_with("posed", 36000, 140), "posed")
    return sd, X.config(24, 24, 8, bounces=1), what


@pytest.mark.parametrize("view", ["boxes_unposed", "many_meshes_hbm"])
def test_scene_views_equal_the_checker(mcrt, gpu, oracle, view):
    if view == "boxes_unposed":
        sd, cfg = _box_case(mcrt)
        lights = (abi.Light((-20.0, 30.0, 25.0), (0.5, 0.5, 0.7, 1.0), 4.0), abi.Light((15.0, 10.0, 20.0), (0.8, 0.6, 0.4, 1.0), 0.0))
    else:
        sd, cfg, _ = _many_mesh_case()
        c = B.scene_centre(sd)
        lights = (abi.Light(tuple(float(v) for v in c + np.array([-30.0, 25.0, 30.0])), (0.6, 0.6, 0.8, 1.0), 4.0),
                  abi.Light(tuple(float(v) for v in c + np.array([20.0, -5.0, 25.0])), (0.7, 0.5, 0.4, 1.0), 0.0))
    want, counts = X.expected_frame(oracle, sd, cfg, lights)
    assert counts[0] >= 50 and counts[1] >= 25, counts
    scenes.assert_bit_equal(_render_device(mcrt, sd, cfg, lights), want, f"{view}: device form")
    scenes.assert_bit_equal(_one_shot(mcrt, sd, cfg, lights), want, f"{view}: one-shot form")


# ---- transparent background ------------------------------------------------------------------------------------------
def test_transparent_background_keeps_the_figure(mcrt, gpu, oracle):
    lights = X.CASES["three"]
    sd, cfg, want, _ = X.skin_expectation(POSE0, X.lights_key(lights))
    hit = (oracle.intersect(sd.ptr, L.pixel_rays(oracle, sd.ptr, cfg.width, cfg.height))["hit"] != 0).reshape(cfg.height, cfg.width)
    img = _one_shot(mcrt, sd, cfg, lights, background="transparent")
    scenes.assert_bit_equal(img[hit], want[hit], "covered pixels of the transparent frame")
    assert (img[~hit] == 0).all()
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        ds.set_background("transparent")
        img = _device(ds, cfg)
        scenes.assert_bit_equal(img[hit], want[hit], "covered pixels, device form")
        assert (img[~hit] == 0).all()
    finally:
        ds.close()


# ---- lifecycle -------------------------------------------------------------------------------------------------------
def _refused(mcrt, call):
    with pytest.raises(mcrt._lib.McrtError) as e:
        call()
    assert e.value.code == abi.MCRT_ERR_INVALID and "extra lights: beauty render only" in str(e.value)


def _light_passes(mcrt, ds, cfg):
    """the passes whose result depends on the light, as callables"""
    n = cfg.width * cfg.height
    f1 = torch.zeros(n, dtype=torch.float32, device="cuda")
    f4 = torch.zeros(n * 4, dtype=torch.float32, device="cuda")
    t4 = torch.zeros(max(ds.texels, 1) * 4, dtype=torch.float32, device="cuda")
    shot = abi.Shot()
    scratch = torch.zeros(mcrt.shot_scratch_bytes(cfg, shot) // 4 + 4, dtype=torch.float32, device="cuda")
    keep = (f1, f4, t4, scratch)
    return keep, {
        "ground": lambda: ds.render_ground_device(cfg, 0.0, visibility_ptr=f1.data_ptr(), stream=_stream()),
        "reflection": lambda: ds.render_reflection_device(cfg, 0.0, rgba_ptr=f4.data_ptr(), stream=_stream()),
        "light": lambda: ds.render_light_device(cfg, direct_ptr=f4.data_ptr(), stream=_stream()),
        "bake": lambda: ds.bake_light_device(cfg, 1, direct_ptr=t4.data_ptr(), stream=_stream()),
        "shot": lambda: ds.render_shot_device(cfg, shot, 0.0, scratch.data_ptr(), scratch.numel() * 4, out_f32_ptr=f4.data_ptr(), stream=_stream()),
        "composite": lambda: mcrt.composite_shot_batch_device([ds], cfg, shot, f4.data_ptr(), out_f32_ptr=f4.data_ptr(), stream=_stream()),
    }


def test_lifecycle_replay_change_and_removal(mcrt, gpu, oracle):
    sd, cfg, want_two, _ = X.skin_expectation(POSE0, TWO)
    _, _, want_bright, _ = X.skin_expectation(POSE0, X.lights_key(X.CASES["bright_front"]))
    _, _, want_none, _ = X.skin_expectation(POSE0)
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(X.CASES["fill_left+kicker"])
        assert [(l.position, l.radius) for l in ds.extra_lights] == [(tuple(l.position), l.radius) for l in X.CASES["fill_left+kicker"]]
        for i in range(6):  # the fourth sighting records the launch graph, the later ones replay it
            scenes.assert_bit_equal(_device(ds, cfg), want_two, f"two lights, render {i}")
        ds.set_extra_lights(X.CASES["bright_front"])  # the recorded graph carries the old lights: not replayed
        for i in range(6):
            scenes.assert_bit_equal(_device(ds, cfg), want_bright, f"changed lights, render {i}")
        keep, passes = _light_passes(mcrt, ds, cfg)
        for name, call in passes.items():
            _refused(mcrt, call)
        ds.set_extra_lights([])
        assert ds.extra_lights == []
        scenes.assert_bit_equal(_device(ds, cfg), want_none, "after set_extra_lights([])")
        scenes.assert_bit_equal(want_none, oracle.render(sd.ptr, cfg), "the checker without lights")
        for name, call in passes.items():
            call()
        torch.cuda.synchronize()
        ds.check()
        del keep
    finally:
        ds.close()


def test_unchanged_passes_run_with_extra_lights(mcrt, gpu):
    sd, cfg, _, _ = X.skin_expectation(POSE0, TWO)
    _, _, layers = L.skin_expectation(POSE0)
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(X.CASES["fill_left+kicker"])
        depth = torch.zeros((cfg.height, cfg.width), dtype=torch.float32, device="cuda")
        occ = torch.zeros((cfg.height, cfg.width), dtype=torch.float32, device="cuda")
        ds.render_layers_device(cfg, depth_ptr=depth.data_ptr(), stream=_stream())
        ds.render_ground_occlusion_device(cfg, 0.0, occlusion_ptr=occ.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        scenes.assert_bit_equal(depth.cpu().numpy(), layers["depth"], "layers depth with extra lights")
        x, y = np.argwhere(layers["hit"])[0][::-1]
        assert ds.pick(cfg, np.array([[x, y]], np.int32))["mesh"][0] == layers["id"][y, x, 0]
    finally:
        ds.close()


def test_lights_survive_set_skin_and_set_view(mcrt, gpu, oracle):
    poses = mcrt.getBuiltinPoses()
    skin = L.unique_skin("S64")
    lights = X.CASES["fill_left+kicker"]
    cfg = X.config(64, 48, 16)
    ds = mcrt.DeviceScene.for_skin("S64", poses[0])
    try:
        ds.set_extra_lights(lights)
        ds.set_skin(skin)
        want, counts = X.expected_frame(oracle, mcrt.MeshBuilder.buildScene(skin, poses[0]), cfg, lights)
        assert counts[1] >= 100, counts
        scenes.assert_bit_equal(_device(ds, cfg), want, "after set_skin")
        ds.set_view(poses[3])
        want, _ = X.expected_frame(oracle, mcrt.MeshBuilder.buildScene(skin, poses[3]), cfg, lights)
        scenes.assert_bit_equal(_device(ds, cfg), want, "after set_view")
        assert len(ds.extra_lights) == 2
    finally:
        ds.close()


# ---- batches and shards ----------------------------------------------------------------------------------------------
def test_batch_of_handles_with_0_to_3_lights(mcrt, gpu):
    sets = [(), (X.BRIGHT_FRONT,), X.CASES["fill_left+kicker"], X.CASES["three"]]
    exps = [X.skin_expectation(POSE0, X.lights_key(s)) for s in sets]
    sd, cfg = exps[0][0], exps[0][1]
    handles = [mcrt.DeviceScene(sd) for _ in sets]
    try:
        for ds, s in zip(handles, sets):
            ds.set_extra_lights(s)
        out = torch.zeros((len(sets), cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        mcrt.render_batch_device(handles, cfg, out_f32_ptr=out.data_ptr(), stream=_stream())
        info = mcrt.last_batch_info()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i, e in enumerate(exps):
            scenes.assert_bit_equal(got[i], e[2], f"frame {i} of the batch ({len(sets[i])} extra lights)")
        assert info == {"batched_frames": 1, "launch_sequences": 4}, info  # the three lit ones went alone
        for ds in handles:
            ds.check()
    finally:
        for ds in handles:
            ds.close()


def test_row_shards_assemble_to_the_frame(mcrt, gpu):
    sd, cfg, want, _ = X.skin_expectation("pose5_orbit_64x64_t16", X.lights_key(X.CASES["three"]))
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(X.CASES["three"])
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        _device(ds, cfg, 0, 2, out=out)
        scenes.assert_bit_equal(_device(ds, cfg, 1, 2, out=out), want, "shards (0, 2) and (1, 2)")
    finally:
        ds.close()


# ---- one large frame -------------------------------------------------------------------------------------------------
BAND = (200, 264)  # 64 pixel rows across the top of the 1080p figure's head (it starts at row 244): about 4 000 hits


def test_1080p_band_with_two_lights(mcrt, gpu, oracle):
    sd = L.skin_case("S64", 0, None)
    cfg = X.config(1920, 1080, 32, bounces=2)
    lights = X.CASES["fill_left+kicker"]
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        img = _device(ds, cfg)
        ds.check()
    finally:
        ds.close()
    want, counts = X.expected_frame(oracle, sd, cfg, lights, rows=BAND)
    assert counts[0] >= 1000 and counts[1] >= 500, counts
    scenes.assert_bit_equal(img[BAND[0]:BAND[1]], want[BAND[0]:BAND[1]], "rows 200 .. 263 of the 1080p frame")
