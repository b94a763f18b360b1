"""The ground-reflection pass on the GPU (mcrt_render_reflection*): rgba and distance bit for bit (as uint32) and rgba8 byte for
byte against the CPU oracle (tests/reflection_checker.py) — skin frames at three heights, planes above the figure, cameras below
and above the plane, lights, shadow modes, bounce counts, box scenes at their own floor, frame shapes, plane subsets, batches, the
host form and the wrappers, a pass beside the handle's renders, the pass without bundle decisions and without tile culling, and a
1920 x 1080 frame.

So that a plane of zeros cannot pass, a case asserts what its expectation holds, as (reached, reflected hits, chains with a
second-level hit, level-1 hits in the penumbra): the full-size skin frames at least 100 hits and 20 second-level hits, the
penumbra case at least 40 penumbra hits.  Where the given frame, camera, light and plane hold fewer, the case asserts the
oracle's EXACT counts instead, so that any change of the expectation is noticed: the 64 x 32 skin at the floor (3072, 107, 0, 2:
no chain of it goes on), 33 x 17 (264, 9, 0, 0), 1 x 1 and the plane no pixel reaches (0, 0, 0, 0), the planes at y = 40 — seen
from below it mirrors the top of the head (3072, 20, 5, 3), seen from above it mirrors nothing (4096, 0, 0, 0) —, the cameras
below (3072, 98, 73, 0) and above (4096, 66, 39, 10) the floor, and the five box scenes."""
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

import ground_checker as G  # noqa: E402
import layers_checker as L  # noqa: E402
import reflection_checker as R  # noqa: E402
import scenes  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
BYTE_SENTINEL = 77
PLANES = R.PLANES
FLT_MAX = R.FLT_MAX
COMPONENTS = {"rgba": 4, "rgba8": 4, "distance": 1}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _buffers(n, stride, names=PLANES, lead=0):
    """Device planes for n frames `stride` pixels apart, filled with a sentinel; `lead` elements in front of frame 0."""
    out = {}
    for k in names:
        count = lead + n * stride * COMPONENTS[k]
        out[k] = (torch.full((count,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda") if k == "rgba8"
                  else torch.full((count,), SENTINEL, dtype=torch.float32, device="cuda"))
    return out


def _ptrs(buf, names, lead=0):
    return {f"{k}_ptr": buf[k].data_ptr() + lead * buf[k].element_size() for k in names}


def _frames(buf, cfg, names, n=1, stride=None, lead=0):
    px = cfg.width * cfg.height
    stride = px if stride is None else stride
    out = {}
    for k in names:
        c = COMPONENTS[k]
        a = buf[k].cpu().numpy()[lead:].reshape(n, stride * c)[:, :px * c]
        out[k] = a.reshape((n, cfg.height, cfg.width) + ((c,) if c > 1 else ()))
    return out


def _sentinel(t):
    return BYTE_SENTINEL if t.dtype == torch.uint8 else SENTINEL


def _untouched(t):
    return bool((t == _sentinel(t)).all().item())


def _device_reflection(ds, cfg, ground, names=PLANES, stream=None, lead=0):
    buf = _buffers(1, cfg.width * cfg.height, lead=lead)
    ds.render_reflection_device(cfg, ground, stream=stream if stream is not None else _stream(), **_ptrs(buf, names, lead))
    torch.cuda.synchronize()
    return buf, {k: v[0] for k, v in _frames(buf, cfg, names, lead=lead).items()}


def _check_both_forms(mcrt, sd, cfg, ground, exp, what):
    """The one-shot host form and the device form of one frame against the expectation."""
    R.assert_miss_constants(exp)
    got = mcrt.TileRenderer.renderReflection(sd, cfg, ground)
    assert list(got) == list(PLANES)
    R.assert_reflection_equal(got, exp, what)
    ds = mcrt.DeviceScene(sd)
    try:
        R.assert_reflection_equal(_device_reflection(ds, cfg, ground)[1], exp, what + " (device form)")
        ds.check()
    finally:
        ds.close()


def _counts(what, exp):
    c = R.counts(exp)
    print(what, "reached, hits, second-level, penumbra:", c)
    return c


FULL = ("pose0_default_96x64", "pose6_orbit_96x64", "pose5_orbit_64x64_t16", "s32_pose1_96x64")
SKIN_FRAMES = [(name, 0.0) for name in L.SKIN_CASES] + [(name, g) for name in FULL for g in (6.0, 12.0)]
# the frames that hold fewer than 100 hits or 20 second-level hits: the oracle's exact counts
EXACT = {("s32_pose1_96x64", 0.0): (3072, 107, 0, 2), ("pose0_33x17_t7", 0.0): (264, 9, 0, 0), ("pose0_1x1", 0.0): (0, 0, 0, 0),
         ("pose3_orbit_70x50", 0.0): (0, 0, 0, 0)}


@gpu_test
@pytest.mark.parametrize("case", SKIN_FRAMES, ids=[f"{n}@{g:g}" for n, g in SKIN_FRAMES])
def test_skin_frames_equal_the_oracle(mcrt, gpu, case):
    name, ground = case
    sd, cfg, exp = R.skin_expectation(name, ground)
    reached, hits, second, pen = _counts(case, exp)
    if case in EXACT:
        assert (reached, hits, second, pen) == EXACT[case]
    else:
        assert hits >= 100 and second >= 20
    if ground > 0:  # a plane through the legs: 136 to 433 hits
        assert 136 <= hits <= 433
    _check_both_forms(mcrt, sd, cfg, ground, exp, f"{name} at {ground}")


PLACEMENTS = {  # name -> (pose, orbit camera or None for the 96 x 64 default frame, w, h, ground, exact counts)
    "plane_above_seen_from_below": (0, None, 96, 64, 40.0, (3072, 20, 5, 3)),
    "plane_above_seen_from_above": (6, (20.0, 80.0, 60.0), 64, 64, 40.0, (4096, 0, 0, 0)),
    "camera_below_the_floor": (0, (30.0, -60.0, 30.0), 64, 48, 0.0, (3072, 98, 73, 0)),
    "camera_above_the_floor": (6, (20.0, 80.0, 60.0), 64, 64, 0.0, (4096, 66, 39, 10)),
}


@gpu_test
@pytest.mark.parametrize("case", list(PLACEMENTS))
def test_plane_and_camera_placement(mcrt, gpu, case):
    pose, camera, w, h, ground, exact = PLACEMENTS[case]
    if camera is None:
        sd, cfg, exp = R.skin_expectation("pose0_default_96x64", ground)
    else:
        sd, cfg, exp = R.orbit_expectation(pose, camera, w, h, ground)
    assert _counts(case, exp) == exact
    if case == "camera_below_the_floor":
        assert float(sd.desc.camera_position[1]) < 0.0
    _check_both_forms(mcrt, sd, cfg, ground, exp, case)


LIGHTS = {  # on pose 6 at the floor (137 hits, 70 second-level): name -> (light position, radius, penumbra hits: least or exact)
    "radius_25": (None, 25.0, 50),          # the penumbra case
    "radius_0": (None, 0.0, 0),             # the one isInShadow ray at S = 8
    "below_the_ground": ((10.0, -5.0, 20.0), None, 7),
    "inside_the_head": ((0.0, 28.0, 0.0), None, 0),
    # the ray loop's other branches under the radius-25 light, where enough level-1 hits are undecided to enter it: a group
    # smaller than a wave, the whole ballot, the first count past it
    "samples_2": (None, 25.0, 16),
    "samples_64": (None, 25.0, 63),
    "samples_65": (None, 25.0, 63),
}


@gpu_test
@pytest.mark.parametrize("case", list(LIGHTS))
def test_lights(mcrt, gpu, case):
    light, radius, pen_exact = LIGHTS[case]
    samples = int(case[8:]) if case.startswith("samples_") else 8
    sd, cfg, exp = R.skin_expectation("pose6_orbit_96x64", 0.0, samples=samples, light=light, radius=radius)
    reached, hits, second, pen = _counts(case, exp)
    assert hits >= 100 and second >= 20 and pen == pen_exact
    if case in ("radius_25", "samples_64", "samples_65"):
        assert pen >= 40
    if case == "samples_2":
        assert pen >= 10
    _check_both_forms(mcrt, sd, cfg, 0.0, exp, case)


MODES = {"soft_shadows_off": dict(soft=False), "samples_1": dict(samples=1), "samples_3": dict(samples=3), "samples_8": dict(samples=8),
         "samples_113": dict(samples=113)}


@gpu_test
@pytest.mark.parametrize("case", list(MODES))
def test_shadow_modes(mcrt, gpu, case):
    sd, cfg, exp = R.skin_expectation("pose6_orbit_96x64", 6.0, **MODES[case])  # through the legs: 239 hits, 103 second-level
    reached, hits, second, pen = _counts(case, exp)
    assert hits >= 100 and second >= 20
    assert pen == {"soft_shadows_off": 0, "samples_1": 0, "samples_3": 3, "samples_8": 8, "samples_113": 19}[case]
    _check_both_forms(mcrt, sd, cfg, 6.0, exp, case)


@gpu_test
@pytest.mark.parametrize("bounces", [0, 1, 2, 3, 8])
def test_bounces(mcrt, gpu, bounces):
    sd, cfg, exp = R.skin_expectation("pose5_orbit_64x64_t16", 12.0, bounces=bounces)
    reached, hits, second, pen = _counts(f"{bounces} bounces", exp)
    if bounces == 0:  # the reference returns before it intersects: all constants
        assert (reached, hits) == (4096, 0) and (exp["rgba"] == 0).all() and (exp["distance"] == FLT_MAX).all()
    else:
        assert hits >= 100 and second >= 20
        deeper = R.skin_expectation("pose5_orbit_64x64_t16", 12.0, bounces=min(bounces + 1, 8))[2]
        if bounces < 3:  # every level the chains reach changes the colours
            assert not np.array_equal(exp["rgba"], deeper["rgba"])
    _check_both_forms(mcrt, sd, cfg, 12.0, exp, f"{bounces} bounces")


BOX_COUNTS = {"outer_back_face": (960, 88, 42, 7), "camera_inside": (80, 0, 0, 0), "null_and_empty": (1152, 130, 32, 6), "posed": (1296, 105, 9, 9),
              "seventy_boxes": (480, 78, 0, 0)}


@gpu_test
@pytest.mark.parametrize("name", L.BOX_CASES)
def test_box_scenes_at_their_floor(mcrt, gpu, name):
    sd, cfg, floor, exp = R.box_expectation(name)
    assert _counts(f"{name} floor {floor}", exp) == BOX_COUNTS[name]
    _check_both_forms(mcrt, sd, cfg, floor, exp, name)
    got = mcrt.TileRenderer.renderReflection(sd, cfg)  # ground=None: the scene's floor
    R.assert_reflection_equal(got, exp, name + " (ground=None)")


@gpu_test
@pytest.mark.parametrize("tile", [32, 16, 8, 7])
def test_tile_sizes(mcrt, gpu, tile):
    sd, cfg, exp = R.skin_expectation("pose0_default_96x64", 6.0)  # the tile size is the culling's granularity, never a value
    assert R.counts(exp)[1] >= 100
    _check_both_forms(mcrt, sd, R.config(cfg.width, cfg.height, tile), 6.0, exp, f"tile {tile}")


@gpu_test
@pytest.mark.parametrize("lead", [0, 1, 2])
def test_scalar_store_paths(mcrt, gpu, lead):
    """A width that is no multiple of 4, and planes `lead` elements off their allocation: the float planes 4 or 8 bytes off a
    16-byte boundary, rgba8 one or two bytes off a 4-byte boundary."""
    sd, cfg, exp = R.skin_expectation("pose3_orbit_70x50", 10.0)
    assert cfg.width % 4 and _counts("70x50 at 10", exp)[1] >= 100
    wide = R.skin_expectation("pose0_default_96x64", 6.0)
    for what, (sd_, cfg_, exp_), g in (("70x50", (sd, cfg, exp), 10.0), ("96x64", wide, 6.0)):
        ds = mcrt.DeviceScene(sd_)
        try:
            buf, got = _device_reflection(ds, cfg_, g, lead=lead)
            R.assert_reflection_equal(got, exp_, f"{what}, planes {lead} elements on")
            for k in PLANES:
                assert _untouched(buf[k][:lead]), f"{k}: written in front of the plane"
            ds.check()
        finally:
            ds.close()


@gpu_test
def test_plane_subsets_leave_the_other_planes_alone(mcrt, gpu):
    sd, cfg, exp = R.skin_expectation("pose3_orbit_70x50", 10.0)
    assert np.array_equal(exp["rgba8"], R.quantize(exp["rgba"])) and R.counts(exp)[1] >= 100
    ds = mcrt.DeviceScene(sd)
    try:
        subsets = [(a,) for a in PLANES] + [(a, b) for i, a in enumerate(PLANES) for b in PLANES[i + 1:]] + [PLANES]
        assert len(subsets) == 7
        for names in subsets:
            buf, got = _device_reflection(ds, cfg, 10.0, names)
            R.assert_reflection_equal(got, exp, "+".join(names))
            for k in PLANES:
                if k not in names:
                    assert _untouched(buf[k]), f"{k} was written although only {names} were asked for"
        none, c = abi.McrtReflection(None, None, None), cfg.to_c()
        assert mcrt._lib.load().mcrt_render_reflection_device(ds._h, C.byref(c), 10.0, C.byref(none), None) == abi.MCRT_ERR_INVALID
    finally:
        ds.close()


@gpu_test
def test_batch_of_five_scenes_at_five_heights_keeps_the_gaps(mcrt, gpu, oracle):
    cfg = R.config(64, 48, 32)
    cams = [(0.0, 20.0, 50.0), (60.0, 35.0, 40.0), (200.0, 25.0, 36.0), (310.0, 45.0, 32.0), (135.0, 20.0, 34.0)]
    sds = [L.skin_case("S64" if k % 2 else "S32", (k * 3) % 7, cams[k]) for k in range(5)]
    heights = [0.0, -0.5, 3.0, 10.0, 1.25]
    exps = [R.expected_reflection(oracle, sd, cfg, g) for sd, g in zip(sds, heights)]
    total = np.sum([R.counts(e) for e in exps], axis=0)
    print("five frames: reached, hits, second-level, penumbra:", total)
    assert total[1] >= 100 and total[2] >= 20 and all(R.counts(e)[1] > 0 for e in exps)
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        stride = px + 101  # odd frames start off a 16-byte boundary of distance and rgba8
        buf = _buffers(5, stride)
        mcrt.render_reflection_batch_device(handles, cfg, heights, frame_stride_pixels=stride, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES, 5, stride)
        for k in PLANES:
            gaps = buf[k].reshape(5, stride * COMPONENTS[k])[:, px * COMPONENTS[k]:]
            assert _untouched(gaps), f"{k}: the pixels between two frames were written"
        for i in range(5):
            R.assert_reflection_equal({k: v[i] for k, v in batch.items()}, exps[i], f"batch frame {i}")
        # a batch equals the same frames rendered singly
        for i, h in enumerate(handles):
            R.assert_reflection_equal({k: v[i] for k, v in batch.items()}, _device_reflection(h, cfg, heights[i])[1], f"batch frame {i} against its own call")
        # one handle listed twice, with two heights
        names = ("rgba", "distance")
        buf = _buffers(2, px, names)
        mcrt.render_reflection_batch_device([handles[3], handles[3]], cfg, [10.0, 0.0], stream=_stream(), **_ptrs(buf, names))
        torch.cuda.synchronize()
        twice = _frames(buf, cfg, names, 2)
        R.assert_reflection_equal({k: v[0] for k, v in twice.items()}, exps[3], "one handle, first height")
        R.assert_reflection_equal({k: v[1] for k, v in twice.items()}, R.expected_reflection(oracle, sds[3], cfg, 0.0), "one handle, second height")
        # the host wrapper, frame after frame
        host = mcrt.TileRenderer.renderReflectionBatch(sds, cfg, heights)
        for i in range(5):
            R.assert_reflection_equal({k: v[i] for k, v in host.items()}, exps[i], f"host frame {i}")
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_of_unposed_posed_and_hbm_scenes(mcrt, gpu):
    # an un-posed and a posed figure and seventy boxes in one launch (the HBM variant for all three), every frame at a height of
    # its own; each frame must be what its own call gives
    cfg = R.config(70, 45, 32)
    sds = [L.skin_case("S64", 0), L.skin_case("S64", 6, (135.0, 20.0, 34.0)), mcrt.SceneDesc(L.box_scene("seventy_boxes")[0])]
    heights = [6.0, 0.5, mcrt.scene_floor(sds[2])]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        buf = _buffers(3, cfg.width * cfg.height)
        mcrt.render_reflection_batch_device(handles, cfg, heights, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES, 3)
        for i, h in enumerate(handles):
            single = _device_reflection(h, cfg, heights[i])[1]
            assert (single["distance"] < FLT_MAX).sum() >= 20, f"frame {i} mirrors too little"
            R.assert_reflection_equal({k: v[i] for k, v in batch.items()}, single, f"mixed batch frame {i}")
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_batch_beyond_the_frames_of_one_launch(mcrt, gpu, oracle):
    n = 4096 + 1  # one launch takes 4096 frames (blockIdx.y)
    cfg = R.config(8, 8, 8)
    sds = [L.skin_case("S64", 6, (20.0, 80.0, 60.0)), L.skin_case("S64", 0, (135.0, 50.0, 34.0))]
    heights = [0.0, 10.0, 4.0]
    exps = [R.expected_reflection(oracle, sds[i % 2], cfg, heights[i % 3]) for i in range(6)]  # every (scene, height) pair
    print("4097 frames of 8 x 8:", [R.counts(e) for e in exps])
    assert all(R.counts(e)[0] == 64 for e in exps)
    for i in (0, 4095 % 6, 4096 % 6):
        assert R.counts(exps[i])[1] > 0, i  # the three frames looked at mirror something
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        buf = _buffers(n, px)
        mcrt.render_reflection_batch_device([handles[i % 2] for i in range(n)], cfg, [heights[i % 3] for i in range(n)], stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        got = _frames(buf, cfg, PLANES, n)
        for i in (0, 4095, 4096):
            R.assert_reflection_equal({k: v[i] for k, v in got.items()}, exps[i % 6], f"frame {i} of {n}")
        for k in PLANES:  # and every other frame is one of the six
            want = np.stack([exps[i % 6][k] for i in range(n)])
            assert np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), k
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_ground_none_is_the_scenes_floor(mcrt, gpu, oracle):
    cfg = R.config(64, 48, 32)
    sd = L.skin_case("S64", 4, (60.0, 35.0, 40.0))
    floor = mcrt.scene_floor(sd)
    assert floor == 9.5  # the pose lifts the figure: the plane is not the builder's y = 0
    exp = R.expected_reflection(oracle, sd, cfg, floor)
    assert _counts("pose 4 at its floor", exp)[1] >= 20
    R.assert_reflection_equal(mcrt.TileRenderer.renderReflection(sd, cfg), exp, "ground=None")
    R.assert_reflection_equal(mcrt.TileRenderer.renderReflection(sd, cfg, floor, planes=("rgba8",)), {"rgba8": exp["rgba8"]}, "rgba8 alone")
    both = mcrt.TileRenderer.renderReflectionBatch([sd, sd], cfg, None, planes=("distance", "rgba"))
    assert list(both) == ["rgba", "distance"]
    for i in range(2):
        R.assert_reflection_equal({k: v[i] for k, v in both.items()}, exp, f"batch wrapper frame {i}")


@gpu_test
def test_reflection_pass_between_two_renders_of_one_handle(mcrt, gpu):
    sd, rcfg, exp = R.skin_expectation("pose0_default_96x64", 6.0)
    cfg = abi.Config(width=96, height=64, samplesPerPixel=2)  # the reference's defaults otherwise: 3 bounces, soft shadows
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
        ds.render_reflection_device(rcfg, 6.0, stream=side.cuda_stream, **_ptrs(buf, PLANES))  # no wait for the render: it reads the scene alone
        ds.render_device(cfg, second.data_ptr(), 0, 1, abi.LAYOUT_FRAME, main.cuda_stream)
        ds.check()  # waits for all three
        torch.cuda.synchronize()
        scenes.assert_bit_equal(first.cpu().numpy(), single.cpu().numpy(), "beauty before the reflection pass")
        scenes.assert_bit_equal(second.cpu().numpy(), single.cpu().numpy(), "beauty after the reflection pass")
        assert float(single[..., 3].min().item()) > 0.0  # an opaque frame was rendered
        R.assert_reflection_equal({k: v[0] for k, v in _frames(buf, rcfg, PLANES).items()}, exp, "reflection pass beside the renders")
    finally:
        ds.close()


def _child(argv):
    """A fresh process: the frame of a skin case through the host form, saved as .npz (the development knobs are read once)."""
    import minecraftskin_raytracer_amd as M

    sd, cfg, _ = R.skin_expectation(argv[0], float(argv[1]))
    np.savez(argv[2], **M.TileRenderer.renderReflection(sd, cfg, float(argv[1])))


@gpu_test
@pytest.mark.parametrize("knob", ["MCRT_BUNDLE_DECISIONS", "MCRT_REFLECT_CULL"])
def test_without_a_development_knob_the_planes_are_the_same(mcrt, gpu, tmp_path, knob):
    sd, cfg, exp = R.skin_expectation("pose6_orbit_96x64", 6.0)
    assert R.counts(exp)[1] >= 100 and R.counts(exp)[2] >= 20
    default = mcrt.TileRenderer.renderReflection(sd, cfg, 6.0)
    out = str(tmp_path / "knob.npz")
    env = dict(os.environ, **{knob: "0"})
    subprocess.run([sys.executable, os.path.abspath(__file__), "pose6_orbit_96x64", "6.0", out], env=env, check=True, timeout=300)
    z = np.load(out)
    for k in PLANES:
        assert z[k].tobytes() == default[k].tobytes(), f"{knob}=0 changes {k}"
    R.assert_reflection_equal({k: z[k] for k in PLANES}, exp, f"{knob}=0")


@gpu_test
def test_full_hd_frame(mcrt, gpu, oracle):
    """1920 x 1080, pose 0, default camera, the floor at 0: the miss constants wherever the oracle's plane test says "not
    reached", and 16 tiles bit for bit — the 14 tiles that hold the most reflected hits (counted in the pass's own distance plane,
    which the oracle then has to confirm pixel by pixel), one corner tile and one tile of the tile row the horizon runs through."""
    w, h, tile = 1920, 1080, 32
    sd = L.skin_case("S64", 0)
    cfg = R.config(w, h, tile)
    ds = mcrt.DeviceScene(sd)
    try:
        got = _device_reflection(ds, cfg, 0.0)[1]
        ds.check()
    finally:
        ds.close()

    def rays_of(xs, ys):
        aspect = np.float32(w) / np.float32(h)
        return np.stack([oracle.camera_ray(sd.ptr, float((np.float32(x) + np.float32(0.5)) / np.float32(w)),
                                           float((np.float32(y) + np.float32(0.5)) / np.float32(h)), float(aspect)) for x, y in zip(xs, ys)])

    # The plane test per row: the camera's right vector is horizontal, so d.y has one sign along a pixel row (the normalisation
    # does not change a sign); the oracle's test at both ends and the middle of every row, and at every pixel of the rows around
    # the horizon
    assert float(sd.desc.camera_up[0]) == 0.0 and float(sd.desc.camera_up[2]) == 0.0
    cols = [0, w // 2, w - 1]
    reached_rows = np.zeros(h, bool)
    for y in range(h):
        r = G.plane_points(rays_of(cols, [y] * 3), 0.0)[0]
        assert r.all() or not r.any(), y
        reached_rows[y] = r[0]
    for y in range(536, 545):
        r = G.plane_points(rays_of(range(w), [y] * w), 0.0)[0]
        assert (r == reached_rows[y]).all(), y
    assert 400 < reached_rows.sum() < 700
    above = ~reached_rows
    assert (got["rgba"][above] == 0).all() and (got["rgba8"][above] == 0).all() and (got["distance"][above] == FLT_MAX).all()
    assert np.array_equal(got["rgba8"], R.quantize(got["rgba"]))
    hit = got["distance"] < FLT_MAX
    assert ((got["rgba"][..., 3] > 0) == hit).all()
    per_tile = {(tx, ty): int(hit[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile].sum()) for ty in range(34) for tx in range(60)}
    chosen = sorted(per_tile, key=per_tile.get, reverse=True)[:14] + [(0, 33), (30, 16)]
    assert len(set(chosen)) == 16
    total = np.zeros(4, np.int64)
    for tx, ty in chosen:
        x0, y0 = tx * tile, ty * tile
        tw, th = min(tile, w - x0), min(tile, h - y0)
        ys, xs = np.mgrid[y0:y0 + th, x0:x0 + tw]
        exp = R.expected_at(oracle, sd, cfg, rays_of(xs.ravel(), ys.ravel()), 0.0)
        total += R.counts(exp)
        tile_exp = {k: exp[k].reshape((th, tw) + exp[k].shape[1:]) for k in PLANES}
        R.assert_reflection_equal({k: got[k][y0:y0 + th, x0:x0 + tw] for k in PLANES}, tile_exp, f"tile ({tx}, {ty})")
    print("checked tiles: reached, hits, second-level, penumbra:", total, "hits in the frame:", int(hit.sum()))
    assert total[1] >= 5000 and total[2] >= 20


if __name__ == "__main__":
    _child(sys.argv[1:])
