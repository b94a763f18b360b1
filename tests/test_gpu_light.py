"""The light layers on the GPU (mcrt_render_light*): visibility, occlusion and direct bit for bit (as uint32) against the CPU oracle
(tests/light_checker.py) — the seven skin frames, four lights, the shadow modes, ambient occlusion at four sample counts and four
radii, box scenes, tile sizes, frame shapes and plane alignments, plane subsets, batches, the host form and the wrappers, a pass
beside the handle's renders, the pass without bundle decisions and without the inside fast path, the occlusion plane before and
after the device holds the table of all seeds, a repainted handle, the recomposition of the beauty frame on the device, and a
1920 x 1080 frame.

So that a plane of constants cannot pass, every case asserts first what its expectation holds, as (hits, dark hits, penumbra hits,
hits with occlusion < 1, hits with occlusion 0): at least 30 penumbra hits and 100 partly occluded hits, and besides the oracle's
EXACT counts, so that any change of the expectation is noticed — they are all there is where the frame, the light or the radius
holds fewer (the 33 x 17 frame holds 40 hits, 2 of them in the penumbra)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import layers_checker as L  # noqa: E402
import light_checker as LC  # noqa: E402
import scenes  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
PLANES = LC.PLANES
COMPONENTS = {"visibility": 1, "occlusion": 1, "direct": 4}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, stride, names=PLANES, lead=0):
    """Device planes for n frames `stride` pixels apart, filled with a sentinel; `lead` floats in front of frame 0."""
    return {k: torch.full((lead + n * stride * COMPONENTS[k],), SENTINEL, dtype=torch.float32, device="cuda") for k in names}


def _ptrs(buf, names, lead=0):
    return {f"{k}_ptr": buf[k].data_ptr() + lead * 4 for k in names}


def _frames(buf, cfg, names, n=1, stride=None, lead=0):
    px = cfg.width * cfg.height
    stride = px if stride is None else stride
    out = {}
    for k in names:
        c = COMPONENTS[k]
        a = buf[k].cpu().numpy()[lead:].reshape(n, stride * c)[:, :px * c]
        out[k] = a.reshape((n, cfg.height, cfg.width) + ((c,) if c > 1 else ()))
    return out


def _untouched(t):
    return bool((t == SENTINEL).all().item())


def _device_light(ds, cfg, names=PLANES, stream=None, lead=0):
    buf = _buffers(1, cfg.width * cfg.height, lead=lead)
    ds.render_light_device(cfg, stream=stream if stream is not None else _stream(), **_ptrs(buf, names, lead))
    torch.cuda.synchronize()
    return buf, {k: v[0] for k, v in _frames(buf, cfg, names, lead=lead).items()}


def _check_both_forms(mcrt, sd, cfg, exp, what, names=PLANES):
    """The one-shot host form and the device form of one frame against the expectation."""
    LC.assert_miss_constants(exp)
    got = mcrt.TileRenderer.renderLight(sd, cfg, planes=names)
    assert list(got) == [k for k in PLANES if k in names]
    LC.assert_light_equal(got, exp, what)
    ds = mcrt.DeviceScene(sd)
    try:
        LC.assert_light_equal(_device_light(ds, cfg, names)[1], exp, what + " (device form)")
        ds.check()
    finally:
        ds.close()


def _counts(what, exp, exact, floor=True):
    c = LC.counts(exp)
    print(what, "hits, dark, penumbra, occlusion < 1, occlusion = 0:", c)
    assert c == exact, f"{what}: the oracle holds {c}, not {exact}"
    if floor:
        assert c[2] >= 30 and c[3] >= 100
    return c


SKIN_COUNTS = {  # the oracle's counts at S = 8, A = 8, radius 3; which frames reach the floor of 30 penumbra and 100 occluded hits
    "pose0_default_96x64": ((551, 68, 32, 182, 10), True),
    "pose6_orbit_96x64": ((1079, 1060, 15, 352, 31), False),  # the figure from behind: nearly all of it in its own shadow
    "pose3_orbit_70x50": ((611, 583, 10, 236, 16), False),
    "pose5_orbit_64x64_t16": ((1790, 481, 347, 714, 49), True),
    "s32_pose1_96x64": ((487, 49, 23, 139, 3), False),
    "pose0_33x17_t7": ((40, 5, 2, 11, 1), False),
    "pose0_1x1": ((1, 0, 1, 1, 0), False),
}


@gpu_test
@pytest.mark.parametrize("name", list(L.SKIN_CASES))
def test_skin_frames_equal_the_oracle(mcrt, gpu, name):
    sd, cfg, exp = LC.skin_expectation(name)
    exact, floor = SKIN_COUNTS[name]
    _counts(name, exp, exact, floor)
    _check_both_forms(mcrt, sd, cfg, exp, name)


LIGHTS = {  # on pose 6 (1079 hits, 352 partly occluded): name -> (light position, radius, exact counts, the floor holds)
    "radius_25": (None, 25.0, (1079, 790, 288, 352, 31), True),
    "radius_0": (None, 0.0, (1079, 1075, 0, 352, 31), False),  # the one isInShadow ray at S = 8, with the raw normal
    "below_the_feet": ((10.0, -5.0, 20.0), None, (1079, 727, 82, 352, 31), True),
    "inside_the_head": ((0.0, 28.0, 0.0), None, (1079, 1072, 7, 352, 31), False),
}


@gpu_test
@pytest.mark.parametrize("case", list(LIGHTS))
def test_lights(mcrt, gpu, case):
    light, radius, exact, floor = LIGHTS[case]
    sd, cfg, exp = LC.skin_expectation("pose6_orbit_96x64", light=light, radius=radius)
    _counts(case, exp, exact, floor)
    _check_both_forms(mcrt, sd, cfg, exp, case)


MODES = {  # pose 6 under the light of radius 25: name -> (checker arguments, exact (hits, dark, penumbra))
    "soft_shadows_off": (dict(soft=False), (1079, 1075, 0)),  # shade()'s own test, normalised normal
    "samples_1": (dict(samples=1), (1079, 1075, 0)),
    "samples_3": (dict(samples=3), (1079, 897, 176)),
    "samples_8": (dict(samples=8), (1079, 790, 288)),
    "samples_113": (dict(samples=113), (1079, 697, 382)),
    # the ray loop's other branches: a group smaller than a wave, the whole ballot, the first count past it
    "samples_2": (dict(samples=2), (1079, 931, 123)),
    "samples_64": (dict(samples=64), (1079, 700, 379)),
    "samples_65": (dict(samples=65), (1079, 700, 379)),
}


@gpu_test
@pytest.mark.parametrize("case", list(MODES))
def test_shadow_modes(mcrt, gpu, case):
    kw, exact = MODES[case]
    names = ("visibility", "direct")
    sd, cfg, exp = LC.skin_expectation("pose6_orbit_96x64", radius=25.0, planes=names, **kw)
    c = LC.counts(exp)
    print(case, c)
    assert c[:3] == exact
    if kw.get("samples", 0) > 1:
        assert c[2] >= 30
    _check_both_forms(mcrt, sd, cfg, exp, case, names)


AO_COUNTS = {  # pose 5 (1790 hits): (samples, radius) -> (hits with occlusion < 1, hits with occlusion 0, distinct values of the plane)
    (1, 0.0): (0, 0, 1), (1, 0.5): (22, 22, 2), (1, 3.0): (396, 396, 2), (1, 1000.0): (500, 500, 2),
    (8, 0.0): (0, 0, 1), (8, 0.5): (65, 0, 6), (8, 3.0): (714, 49, 9), (8, 1000.0): (1062, 73, 9),
    (16, 0.0): (0, 0, 1), (16, 0.5): (78, 0, 10), (16, 3.0): (753, 16, 17), (16, 1000.0): (1236, 29, 17),
    (113, 0.0): (0, 0, 1), (113, 0.5): (178, 0, 39), (113, 3.0): (825, 0, 109), (113, 1000.0): (1501, 0, 112),
}


@gpu_test
@pytest.mark.parametrize("samples", [1, 8, 16, 113])
@pytest.mark.parametrize("radius", [0.0, 0.5, 3.0, 1000.0])
def test_ambient_occlusion(mcrt, gpu, samples, radius):
    sd, cfg, exp = LC.skin_expectation("pose5_orbit_64x64_t16", ao_samples=samples, ao_radius=radius)
    c = LC.counts(exp)
    got = (c[3], c[4], len(np.unique(exp["occlusion"])))
    print(samples, radius, c, got)
    assert c[0] == 1790 and got == AO_COUNTS[(samples, radius)]
    if radius >= 3.0:
        assert c[3] >= 100
    if radius == 0.0:
        assert (exp["occlusion"] == 1.0).all()  # no ray can be occluded
    _check_both_forms(mcrt, sd, cfg, exp, f"A {samples} radius {radius}", ("occlusion",))


BOX_COUNTS = {"outer_back_face": (80, 32, 8, 50, 0), "camera_inside": (960, 582, 0, 0, 0), "null_and_empty": (137, 4, 8, 0, 0),
              "posed": (191, 14, 29, 87, 1), "seventy_boxes": (98, 0, 0, 14, 0)}


@gpu_test
@pytest.mark.parametrize("name", L.BOX_CASES)
def test_box_scenes(mcrt, gpu, name):
    sd, cfg, exp = LC.box_expectation(name)
    _counts(name, exp, BOX_COUNTS[name], floor=False)
    _check_both_forms(mcrt, sd, cfg, exp, name)


@gpu_test
@pytest.mark.parametrize("tile", [32, 16, 8, 7])
def test_tile_sizes(mcrt, gpu, tile):
    sd, cfg, exp = LC.skin_expectation("pose0_default_96x64")  # the tile size is the culling's granularity, never a value
    _counts(f"tile {tile}", exp, SKIN_COUNTS["pose0_default_96x64"][0])
    _check_both_forms(mcrt, sd, LC.config(cfg.width, cfg.height, tile), exp, f"tile {tile}")


@gpu_test
@pytest.mark.parametrize("lead", [0, 1, 2])
def test_single_store_paths(mcrt, gpu, lead):
    """Widths that are no multiple of 4 (70 and 33), and planes `lead` floats off their allocation: 4 or 8 bytes off a 16-byte
    boundary, for the frames of width 96 too."""
    for name in ("pose3_orbit_70x50", "pose0_33x17_t7", "pose0_default_96x64"):
        sd, cfg, exp = LC.skin_expectation(name)
        assert LC.counts(exp) == SKIN_COUNTS[name][0]
        ds = mcrt.DeviceScene(sd)
        try:
            buf, got = _device_light(ds, cfg, lead=lead)
            LC.assert_light_equal(got, exp, f"{name}, planes {lead} floats on")
            for k in PLANES:
                assert _untouched(buf[k][:lead]), f"{k}: written in front of the plane"
            ds.check()
        finally:
            ds.close()


@gpu_test
def test_plane_subsets_leave_the_other_planes_alone(mcrt, gpu):
    sd, cfg, exp = LC.skin_expectation("pose5_orbit_64x64_t16")
    _counts("subsets", exp, SKIN_COUNTS["pose5_orbit_64x64_t16"][0])
    ds = mcrt.DeviceScene(sd)
    try:
        subsets = [(a,) for a in PLANES] + [(a, b) for i, a in enumerate(PLANES) for b in PLANES[i + 1:]] + [PLANES]
        assert len(subsets) == 7
        for names in subsets:
            buf, got = _device_light(ds, cfg, names)
            LC.assert_light_equal(got, exp, "+".join(names))
            for k in PLANES:
                if k not in names:
                    assert _untouched(buf[k]), f"{k} was written although only {names} were asked for"
        none, c = abi.McrtLightPlanes(None, None, None), cfg.to_c()
        assert mcrt._lib.load().mcrt_render_light_device(ds._h, C.byref(c), C.byref(none), None) == abi.MCRT_ERR_INVALID
    finally:
        ds.close()


@gpu_test
def test_batch_of_five_scenes_keeps_the_gaps(mcrt, gpu, oracle):
    cfg = LC.config(64, 48, 32)
    cams = [(0.0, 20.0, 50.0), (60.0, 35.0, 40.0), (200.0, 25.0, 36.0), (310.0, 45.0, 32.0), (135.0, 20.0, 34.0)]
    sds = [L.skin_case("S64" if k % 2 else "S32", (k * 3) % 7, cams[k]) for k in range(5)]
    exps = [LC.expected_light(oracle, sd, cfg) for sd in sds]
    total = np.sum([LC.counts(e) for e in exps], axis=0)
    print("five frames: hits, dark, penumbra, occlusion < 1, occlusion = 0:", total)
    assert tuple(int(t) for t in total) == (2515, 1586, 110, 735, 66) and all(LC.counts(e)[0] > 0 for e in exps)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        stride = px + 101  # odd frames start off a 16-byte boundary of visibility and occlusion
        buf = _buffers(5, stride)
        mcrt.render_light_batch_device(handles, cfg, frame_stride_pixels=stride, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES, 5, stride)
        for k in PLANES:
            gaps = buf[k].reshape(5, stride * COMPONENTS[k])[:, px * COMPONENTS[k]:]
            assert _untouched(gaps), f"{k}: the pixels between two frames were written"
        for i in range(5):
            LC.assert_light_equal({k: v[i] for k, v in batch.items()}, exps[i], f"batch frame {i}")
        # a batch equals the same frames rendered singly
        for i, h in enumerate(handles):
            LC.assert_light_equal({k: v[i] for k, v in batch.items()}, _device_light(h, cfg)[1], f"batch frame {i} against its own call")
        # one handle listed twice
        names = ("occlusion", "direct")
        buf = _buffers(2, px, names)
        mcrt.render_light_batch_device([handles[3], handles[3]], cfg, stream=_stream(), **_ptrs(buf, names))
        torch.cuda.synchronize()
        twice = _frames(buf, cfg, names, 2)
        for i in range(2):
            LC.assert_light_equal({k: v[i] for k, v in twice.items()}, exps[3], f"one handle, frame {i}")
        # the host wrapper, frame after frame
        host = mcrt.TileRenderer.renderLightBatch(sds, cfg)
        for i in range(5):
            LC.assert_light_equal({k: v[i] for k, v in host.items()}, exps[i], f"host frame {i}")
        sub = mcrt.TileRenderer.renderLightBatch(sds[:2], cfg, planes=("direct", "visibility"))
        assert list(sub) == ["visibility", "direct"]
        LC.assert_light_equal({k: v[1] for k, v in sub.items()}, exps[1], "host wrapper, two planes")
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_of_unposed_posed_and_hbm_scenes(mcrt, gpu):
    # an un-posed and a posed figure and seventy boxes in one launch (the HBM variant for all three); each frame must be what
    # its own call gives
    cfg = LC.config(70, 45, 32)
    sds = [L.skin_case("S64", 0), L.skin_case("S64", 6, (135.0, 20.0, 34.0)), mcrt.SceneDesc(L.box_scene("seventy_boxes")[0])]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        buf = _buffers(3, cfg.width * cfg.height)
        mcrt.render_light_batch_device(handles, cfg, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES, 3)
        for i, h in enumerate(handles):
            single = _device_light(h, cfg)[1]
            assert (single["direct"][..., 3] > 0).sum() >= 100, f"frame {i} holds too few hits"
            LC.assert_light_equal({k: v[i] for k, v in batch.items()}, single, f"mixed batch frame {i}")
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_beyond_the_frames_of_one_launch(mcrt, gpu, oracle):
    n = 4096 + 1  # one launch takes 4096 frames (blockIdx.y)
    cfg = LC.config(8, 8, 8)
    sds = [L.skin_case("S64", 6, (40.0, 60.0, 22.0)), L.skin_case("S64", 0, (40.0, 60.0, 22.0))]
    exps = [LC.expected_light(oracle, sd, cfg) for sd in sds]
    print("4097 frames of 8 x 8:", [LC.counts(e) for e in exps])
    assert [LC.counts(e) for e in exps] == [(43, 4, 12, 16, 1), (34, 13, 1, 11, 1)]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        buf = _buffers(n, px)
        mcrt.render_light_batch_device([handles[i % 2] for i in range(n)], cfg, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        got = _frames(buf, cfg, PLANES, n)
        for i in (0, 4095, 4096):
            LC.assert_light_equal({k: v[i] for k, v in got.items()}, exps[i % 2], f"frame {i} of {n}")
        for k in PLANES:  # and every other frame is one of the two
            want = np.stack([exps[i % 2][k] for i in range(n)])
            assert np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), k
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_light_pass_between_two_renders_of_one_handle(mcrt, gpu):
    sd, lcfg, exp = LC.skin_expectation("pose0_default_96x64")
    cfg = abi.Config(width=96, height=64, samplesPerPixel=2, aoEnabled=True)  # the reference's defaults otherwise: 3 bounces, soft shadows
    ds = mcrt.DeviceScene(sd)
    try:
        main, side = torch.cuda.Stream(), torch.cuda.Stream()
        first = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        second = torch.zeros_like(first)
        single = torch.zeros_like(first)
        buf = _buffers(1, cfg.width * cfg.height)
        ds.render_device(cfg, single.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.check()
        torch.cuda.synchronize()
        ds.render_device(cfg, first.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.render_light_device(lcfg, stream=side.cuda_stream, **_ptrs(buf, PLANES))  # no wait for the render: it reads the scene alone
        ds.render_device(cfg, second.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.check()  # waits for all three
        torch.cuda.synchronize()
        scenes.assert_bit_equal(first.cpu().numpy(), single.cpu().numpy(), "beauty before the light pass")
        scenes.assert_bit_equal(second.cpu().numpy(), single.cpu().numpy(), "beauty after the light pass")
        assert float(single[..., 3].min().item()) > 0.0  # an opaque frame was rendered
        LC.assert_light_equal({k: v[0] for k, v in _frames(buf, lcfg, PLANES).items()}, exp, "light pass beside the renders")
    finally:
        ds.close()


def _child(argv):
    """A fresh process: the frame of a skin case through the host form, saved as .npz (the development knobs are read once)."""
    import minecraftskin_raytracer_amd as M

    sd, cfg, _ = LC.skin_expectation(argv[0], planes=("visibility", "direct"))
    np.savez(argv[1], **M.TileRenderer.renderLight(sd, cfg))


@gpu_test
@pytest.mark.parametrize("knob", ["MCRT_BUNDLE_DECISIONS", "MCRT_INSIDE_FAST"])
def test_without_a_development_knob_the_planes_are_the_same(mcrt, gpu, tmp_path, knob):
    sd, cfg, exp = LC.skin_expectation("pose5_orbit_64x64_t16")
    _counts(knob, exp, SKIN_COUNTS["pose5_orbit_64x64_t16"][0])
    default = mcrt.TileRenderer.renderLight(sd, cfg)
    out = str(tmp_path / "knob.npz")
    env = dict(os.environ, **{knob: "0"})
    subprocess.run([sys.executable, os.path.abspath(__file__), "pose5_orbit_64x64_t16", out], env=env, check=True, timeout=300)
    z = np.load(out)
    for k in PLANES:
        assert z[k].tobytes() == default[k].tobytes(), f"{knob}=0 changes {k}"
    LC.assert_light_equal({k: z[k] for k in PLANES}, exp, f"{knob}=0")


@gpu_test
def test_occlusion_before_and_after_the_device_holds_the_table_of_all_seeds(mcrt, gpu):
    """The occlusion kernel seeds its engines by the recurrence until an ambient-occlusion RENDER on the device has built the table
    of all seeds; then it reads mt[397] from it.  The same bytes either way (when an earlier test of the session has rendered with
    ambient occlusion, the table exists from the start, and both passes read it)."""
    sd, cfg, exp = LC.skin_expectation("pose5_orbit_64x64_t16")
    _counts("seed table", exp, SKIN_COUNTS["pose5_orbit_64x64_t16"][0])
    ds, other = mcrt.DeviceScene(sd), mcrt.DeviceScene(L.skin_case("S64", 0))
    try:
        before = _device_light(ds, cfg, ("occlusion",))[1]
        LC.assert_light_equal(before, exp, "before the AO render")
        frame = torch.zeros((32, 32, 4), dtype=torch.float32, device="cuda")
        other.render_device(abi.Config(width=32, height=32, aoEnabled=True), frame.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
        other.check()
        after = _device_light(ds, cfg, ("occlusion",))[1]
        assert after["occlusion"].tobytes() == before["occlusion"].tobytes()
        fresh = mcrt.DeviceScene(sd)
        try:
            LC.assert_light_equal(_device_light(fresh, cfg, ("occlusion",))[1], exp, "a handle created after the AO render")
        finally:
            fresh.close()
        ds.check()
    finally:
        ds.close()
        other.close()


@gpu_test
def test_repainted_handle(mcrt, gpu):
    name = "pose6_orbit_96x64"
    sd, cfg, exp = LC.skin_expectation(name, radius=25.0)
    _counts("repainted", exp, LIGHTS["radius_25"][2])
    kind, pose, camera, w, h, tile = L.SKIN_CASES[name]
    ds = mcrt.DeviceScene.for_skin(kind, mcrt.getBuiltinPoses()[pose], look=sd)
    try:
        white = _device_light(ds, cfg)[1]  # white and opaque until the first repaint: the same geometry, other texels
        assert (white["direct"][..., 3] == 1.0).sum() >= exp["hit"].sum()
        assert not np.array_equal(white["direct"], exp["direct"])
        ds.set_skin(L.unique_skin(kind))
        LC.assert_light_equal(_device_light(ds, cfg)[1], exp, "after set_skin")
        ds.check()
    finally:
        ds.close()


@gpu_test
@pytest.mark.parametrize("name,kw", [("pose0_default_96x64", dict()), ("pose6_orbit_96x64", dict(radius=25.0)), ("pose5_orbit_64x64_t16", dict(soft=False))],
                         ids=["pose0", "pose6_radius25", "pose5_hard"])
def test_recomposition_on_the_device(mcrt, gpu, name, kw):
    """include/mcrt.h, "light layers": `direct` equals the handle's transparent frame at 1 spp / 0 bounces on every pixel whose
    id.mesh >= 0, and clamp(direct.rgb * (1 - intensity * (1 - occlusion))) the frame with ambient occlusion — all five planes
    from the device."""
    sd, cfg, exp = LC.skin_expectation(name, **kw)
    c = LC.counts(exp)
    assert c[0] >= 500 and c[3] >= 100
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_background("transparent")
        got = _device_light(ds, cfg)[1]
        LC.assert_light_equal(got, exp, name)
        px = cfg.width * cfg.height
        ids = torch.full((px, 4), -7, dtype=torch.int32, device="cuda")
        ds.render_layers_device(cfg, id_ptr=ids.data_ptr(), stream=_stream())
        frames = {}
        for ao, intensity in ((False, 0.5), (True, 0.5), (True, 0.9)):
            out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
            ds.render_device(LC.beauty_config(cfg, ao, intensity), out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
            ds.check()
            frames[(ao, intensity)] = out.cpu().numpy()
        torch.cuda.synchronize()
        on = ids.cpu().numpy().reshape(cfg.height, cfg.width, 4)[..., 0] >= 0
        assert np.array_equal(on, exp["hit"])
        scenes.assert_bit_equal(frames[(False, 0.5)][on], got["direct"][on], "beauty without AO against direct")
        assert (frames[(False, 0.5)][~on] == 0).all()
        for intensity in (0.5, 0.9):
            scenes.assert_bit_equal(frames[(True, intensity)][on], LC.recompose(got["direct"], got["occlusion"], intensity)[on],
                                    f"beauty with AO {intensity} against the recomposition")
        assert not np.array_equal(frames[(True, 0.5)][on], frames[(False, 0.5)][on])
    finally:
        ds.close()


@gpu_test
def test_full_hd_frame(mcrt, gpu, oracle):
    """1920 x 1080, pose 0, default camera: the miss constants wherever the oracle misses on sampled rows, and 16 tiles bit for
    bit — the 14 tiles that hold the most hits (counted in the pass's own direct plane, which the oracle then has to confirm
    pixel by pixel), one corner tile and one edge tile."""
    w, h, tile = 1920, 1080, 32
    sd = L.skin_case("S64", 0)
    cfg = LC.config(w, h, tile)
    ds = mcrt.DeviceScene(sd)
    try:
        got = _device_light(ds, cfg)[1]
        ds.check()
    finally:
        ds.close()

    def rays_of(xs, ys):
        aspect = np.float32(w) / np.float32(h)
        return np.stack([oracle.camera_ray(sd.ptr, float((np.float32(x) + np.float32(0.5)) / np.float32(w)),
                                           float((np.float32(y) + np.float32(0.5)) / np.float32(h)), float(aspect)) for x, y in zip(xs, ys)])

    hit = got["direct"][..., 3] > 0
    assert ((got["direct"][~hit] == 0).all() and (got["visibility"][~hit] == 1.0).all() and (got["occlusion"][~hit] == 1.0).all())
    rows = list(range(0, h, 90)) + [h - 1]
    n_hit_rows = 0
    for y in rows:  # every pixel of the sampled rows: the pass misses exactly where the oracle does
        oh = oracle.intersect(sd.ptr, rays_of(range(w), [y] * w))["hit"] != 0
        assert np.array_equal(oh, hit[y]), f"row {y}"
        n_hit_rows += int(oh.any())
    assert n_hit_rows >= 5
    per_tile = {(tx, ty): int(hit[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile].sum()) for ty in range(34) for tx in range(60)}
    chosen = sorted(per_tile, key=per_tile.get, reverse=True)[:14] + [(0, 33), (59, 16)]
    assert len(set(chosen)) == 16
    total = np.zeros(5, np.int64)
    for tx, ty in chosen:
        x0, y0 = tx * tile, ty * tile
        tw, th = min(tile, w - x0), min(tile, h - y0)
        ys, xs = np.mgrid[y0:y0 + th, x0:x0 + tw]
        exp = LC.expected_at(oracle, sd, cfg, rays_of(xs.ravel(), ys.ravel()))
        tile_exp = {k: v.reshape((th, tw) + v.shape[1:]) for k, v in exp.items()}
        total += LC.counts(tile_exp)
        LC.assert_light_equal({k: got[k][y0:y0 + th, x0:x0 + tw] for k in PLANES}, tile_exp, f"tile ({tx}, {ty})")
    print("checked tiles: hits, dark, penumbra, occlusion < 1, occlusion = 0:", total, "hits in the frame:", int(hit.sum()))
    assert total[0] >= 10000 and total[2] >= 30 and total[3] >= 100


if __name__ == "__main__":
    _child(sys.argv[1:])
