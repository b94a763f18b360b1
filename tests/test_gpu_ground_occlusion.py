"""The ground-occlusion pass on the GPU (mcrt_render_ground_occlusion*) and the studio shot's floor-occlusion term: occlusion bit
for bit and the matte byte for byte against the CPU oracle (tests/ground_occlusion_checker.py) — skin frames at ground_y = 0 (the
plane passes through the 64x64 skin's outer leg boxes, so ray origins lie inside boxes) and at the scene's floor, the single,
batch and host forms, 113 samples (the draw limit and the atomic count), 64 samples (the ballot's full-wave branch), cameras
below the plane, clipped tiles, box scenes with more than 64 meshes and posed meshes, misaligned planes, radii <= 0, strides,
plane subsets, a pass beside the handle's render — and the blend with the term against numpy.

So that a plane of ones cannot pass, the two large skin frames assert that their expectation holds at least 100 pixels with
occlusion < 1, 5 with occlusion 0 and 40 with occlusion < 1 beside the figure (the oracle's counts at 8 samples, radius 3,
ground_y = 0: 152 / 7 / 50 and 207 / 25 / 73); the other cases print theirs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ground_occlusion_checker as GO  # noqa: E402
import layers_checker as L  # noqa: E402
import scenes  # noqa: E402
import shot_checker as S  # noqa: E402
from minecraftskin_raytracer_amd import abi  # noqa: E402

gpu_test = pytest.mark.gpu
SENTINEL = -12345.0
MATTE_SENTINEL = 77
PLANES = GO.PLANES


def _buffers(n, stride, names=PLANES):
    """Device planes for n frames `stride` pixels apart, filled with a sentinel."""
    return {k: (torch.full((n, stride), MATTE_SENTINEL, dtype=torch.uint8, device="cuda") if k == "matte"
                else torch.full((n, stride), SENTINEL, dtype=torch.float32, device="cuda")) for k in names}


def _ptrs(buf, names):
    return {f"{k}_ptr": buf[k].data_ptr() for k in names}


def _frames(buf, cfg, names):
    px = cfg.width * cfg.height
    return {k: buf[k].cpu().numpy()[:, :px].reshape(-1, cfg.height, cfg.width) for k in names}


def _untouched(t):
    return bool((t == (MATTE_SENTINEL if t.dtype == torch.uint8 else SENTINEL)).all().item())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device_pass(ds, cfg, ground, names=PLANES, stream=None):
    buf = _buffers(1, cfg.width * cfg.height)
    ds.render_ground_occlusion_device(cfg, ground, stream=stream if stream is not None else _stream(), **_ptrs(buf, names))
    torch.cuda.synchronize()
    return buf, {k: v[0] for k, v in _frames(buf, cfg, names).items()}


def _check_all_forms(mcrt, sd, cfg, ground, exp, what):
    """The one-shot host form, the device form and a batch of one handle listed twice against the expectation."""
    got = mcrt.TileRenderer.renderGroundOcclusion(sd, cfg, ground)
    assert list(got) == list(PLANES)
    GO.assert_planes_equal(got, exp, what)
    ds = mcrt.DeviceScene(sd)
    try:
        GO.assert_planes_equal(_device_pass(ds, cfg, ground)[1], exp, what + " (device form)")
        buf = _buffers(2, cfg.width * cfg.height)
        mcrt.render_ground_occlusion_batch_device([ds, ds], cfg, [ground, ground], stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES)
        for i in range(2):
            GO.assert_planes_equal({k: v[i] for k, v in batch.items()}, exp, f"{what} (batch frame {i})")
        ds.check()
    finally:
        ds.close()


def _assert_miss_constants(exp):
    miss = ~exp["reached"]
    assert (exp["occlusion"][miss] == 1.0).all() and (exp["matte"][miss] == 0).all()


FLOORS = ("zero", "floor")


@gpu_test
@pytest.mark.parametrize("floor", FLOORS)
@pytest.mark.parametrize("case", list(L.SKIN_CASES))
def test_skin_frames_equal_the_oracle(mcrt, gpu, oracle, case, floor):
    sd, cfg, exp = GO.skin_expectation(case, 0.0 if floor == "zero" else None)
    ground = 0.0 if floor == "zero" else mcrt.scene_floor(sd)
    below, zero = GO.counts(exp)
    print(case, floor, ground, "reached", int(exp["reached"].sum()), "occlusion < 1", below, "== 0", zero)
    _assert_miss_constants(exp)
    if floor == "zero" and case in ("pose6_orbit_96x64", "pose5_orbit_64x64_t16"):
        beside = int(((exp["occlusion"] < 1) & GO.beside_the_figure(oracle, sd, cfg)).sum())
        print(case, "< 1 beside the figure", beside)
        assert below >= 100 and zero >= 5 and beside >= 40
    if floor == "zero" and case == "pose3_orbit_70x50":
        assert not exp["reached"].any()  # the camera lies below the plane and looks up
    _check_all_forms(mcrt, sd, cfg, ground, exp, f"{case} at {ground}")


@gpu_test
def test_the_plane_through_the_legs(mcrt, gpu):
    sd, cfg, exp = GO.skin_expectation("pose3_orbit_70x50", 6.0)
    below, zero = GO.counts(exp)
    print("pose3 at 6", "reached", int(exp["reached"].sum()), "occlusion < 1", below, "== 0", zero)
    assert exp["reached"].any() and below >= 1
    _check_all_forms(mcrt, sd, cfg, 6.0, exp, "pose3_orbit_70x50 at 6")


@gpu_test
@pytest.mark.parametrize("samples,radius", [(113, 1.5), (64, 3.0), (1, 3.0), (3, 3.0)])
def test_sample_counts(mcrt, gpu, samples, radius):
    # 113: the draw limit, not a power of two — the LDS atomic; 64: a traced pixel fills a wave — the ballot's full-wave branch
    sd, cfg, exp = GO.skin_expectation("pose5_orbit_64x64_t16", 0.0, samples, radius)
    below, zero = GO.counts(exp)
    print(samples, radius, "occlusion < 1", below, "== 0", zero, "values", len(np.unique(exp["occlusion"])))
    assert below >= 40
    if samples >= 64:
        assert len(np.unique(exp["occlusion"])) > 10
    _check_all_forms(mcrt, sd, cfg, 0.0, exp, f"{samples} samples, radius {radius}")


@gpu_test
@pytest.mark.parametrize("name", L.BOX_CASES)
def test_box_scenes_at_their_floor(mcrt, gpu, name):
    sd, cfg, floor, exp = GO.box_expectation(name)
    below, zero = GO.counts(exp)
    print(name, "floor", floor, "reached", int(exp["reached"].sum()), "occlusion < 1", below, "== 0", zero)
    _check_all_forms(mcrt, sd, cfg, floor, exp, name)
    got = mcrt.TileRenderer.renderGroundOcclusion(sd, cfg)  # ground=None: the scene's floor
    GO.assert_planes_equal(got, exp, name + " (ground=None)")


def test_box_scenes_hold_occluded_pixels(mcrt):
    # the many-mesh scene (the mask's tail) and the posed one must have something to get wrong
    for name in ("seventy_boxes", "posed"):
        assert GO.counts(GO.box_expectation(name)[3])[0] >= 1, name


@gpu_test
def test_planes_off_their_alignment(mcrt, gpu):
    sd, cfg, exp = GO.skin_expectation("pose5_orbit_64x64_t16")
    px = cfg.width * cfg.height
    ds = mcrt.DeviceScene(sd)
    try:
        occ = torch.full((px + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        matte = torch.full((px + 8,), MATTE_SENTINEL, dtype=torch.uint8, device="cuda")
        assert occ.data_ptr() % 16 == 0 and matte.data_ptr() % 4 == 0
        ds.render_ground_occlusion_device(cfg, 0.0, occlusion_ptr=occ.data_ptr() + 4, matte_ptr=matte.data_ptr() + 1, stream=_stream())
        torch.cuda.synchronize()
        got = {"occlusion": occ.cpu().numpy()[1:px + 1].reshape(cfg.height, cfg.width), "matte": matte.cpu().numpy()[1:px + 1].reshape(cfg.height, cfg.width)}
        GO.assert_planes_equal(got, exp, "planes 4 bytes / 1 byte off")
        assert occ[0].item() == SENTINEL and _untouched(occ[px + 1:]) and matte[0].item() == MATTE_SENTINEL and _untouched(matte[px + 1:])
        ds.check()
    finally:
        ds.close()


@gpu_test
@pytest.mark.parametrize("radius", [0.0, -1.0])
def test_a_radius_that_is_not_positive_gives_ones(mcrt, gpu, radius):
    sd, cfg, _ = GO.skin_expectation("pose5_orbit_64x64_t16")
    c = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, aoSamples=8, aoRadius=radius)
    ds = mcrt.DeviceScene(sd)
    try:
        _, got = _device_pass(ds, c, 0.0)
        assert (got["occlusion"] == 1.0).all() and (got["matte"] == 0).all()
        ds.check()
    finally:
        ds.close()
    host = mcrt.TileRenderer.renderGroundOcclusion(sd, c, 0.0)
    assert (host["occlusion"] == 1.0).all() and (host["matte"] == 0).all()


@gpu_test
def test_batch_of_scenes_at_their_heights_keeps_the_gaps(mcrt, gpu, oracle):
    cfg = abi.Config(width=64, height=48, tileSize=32, aoSamples=8, aoRadius=3.0)
    cams = [(0.0, 20.0, 50.0), (60.0, 35.0, 40.0), (200.0, 25.0, 36.0), (310.0, 45.0, 32.0)]
    sds = [L.skin_case("S64" if k % 2 else "S32", (k * 3) % 7, cams[k]) for k in range(4)]
    heights = [0.0, -0.5, 3.0, 1.25]
    exps = [GO.expected_ground_occlusion(oracle, sd, cfg, g) for sd, g in zip(sds, heights)]
    print("batch: occlusion < 1 per frame", [GO.counts(e)[0] for e in exps])
    assert sum(GO.counts(e)[0] for e in exps) >= 100
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    try:
        px = cfg.width * cfg.height
        stride = px + 101  # odd frames start off a 16-byte boundary of the float plane and off a 4-byte boundary of the matte
        buf = _buffers(4, stride)
        mcrt.render_ground_occlusion_batch_device(handles, cfg, heights, frame_stride_pixels=stride, stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        batch = _frames(buf, cfg, PLANES)
        for k in PLANES:
            assert _untouched(buf[k][:, px:]), f"{k}: the pixels between two frames were written"
        for i in range(4):
            GO.assert_planes_equal({k: v[i] for k, v in batch.items()}, exps[i], f"batch frame {i}")
        # one handle listed twice, with two heights
        buf = _buffers(2, px)
        mcrt.render_ground_occlusion_batch_device([handles[3], handles[3]], cfg, [1.25, 0.0], stream=_stream(), **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        twice = _frames(buf, cfg, PLANES)
        GO.assert_planes_equal({k: v[0] for k, v in twice.items()}, exps[3], "one handle, first height")
        GO.assert_planes_equal({k: v[1] for k, v in twice.items()}, GO.expected_ground_occlusion(oracle, sds[3], cfg, 0.0), "one handle, second height")
        # the host wrapper, frame after frame
        host = mcrt.TileRenderer.renderGroundOcclusionBatch(sds, cfg, heights)
        for i in range(4):
            GO.assert_planes_equal({k: v[i] for k, v in host.items()}, exps[i], f"host frame {i}")
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_plane_subsets_leave_the_other_plane_alone(mcrt, gpu):
    sd, cfg, exp = GO.skin_expectation("pose6_orbit_96x64")
    ds = mcrt.DeviceScene(sd)
    try:
        for names in (("occlusion",), ("matte",), PLANES):
            buf, got = _device_pass(ds, cfg, 0.0, names)
            GO.assert_planes_equal(got, exp, "+".join(names))
            for k in PLANES:
                if k not in names:
                    assert _untouched(buf[k]), f"{k} was written although only {names} were asked for"
        none, c = abi.McrtGroundOcclusion(None, None), cfg.to_c()
        assert mcrt._lib.load().mcrt_render_ground_occlusion_device(ds._h, C.byref(c), 0.0, C.byref(none), None) == abi.MCRT_ERR_INVALID
        only = mcrt.TileRenderer.renderGroundOcclusion(sd, cfg, 0.0, planes="matte")
        assert list(only) == ["matte"] and (only["matte"] == exp["matte"]).all()
    finally:
        ds.close()


@gpu_test
def test_the_pass_beside_the_handles_render(mcrt, gpu, oracle):
    sd, cfg, exp = GO.skin_expectation("pose6_orbit_96x64")
    rcfg = abi.Config(width=cfg.width, height=cfg.height, tileSize=cfg.tileSize, samplesPerPixel=4, maxBounces=3, aoSamples=8, aoRadius=3.0)
    ref = oracle.render(sd.ptr, rcfg)
    ds = mcrt.DeviceScene(sd)
    try:
        frame = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        buf = _buffers(1, cfg.width * cfg.height)
        for _ in range(3):
            ds.render_device(rcfg, frame.data_ptr(), stream=_stream())
            ds.render_ground_occlusion_device(cfg, 0.0, stream=side.cuda_stream, **_ptrs(buf, PLANES))
        torch.cuda.synchronize()
        ds.check()
        GO.assert_planes_equal({k: v[0] for k, v in _frames(buf, cfg, PLANES).items()}, exp, "beside a render")
        scenes.assert_bit_equal(frame.cpu().numpy(), ref, "the render beside the pass")
    finally:
        ds.close()


# ---- the studio shot's floor-occlusion term ---------------------------------------------------------------------------
SHOT_CASE = "pose5_orbit_64x64_t16"


def _shot_config(name=SHOT_CASE):
    c = S.case_config(name)
    c.aoSamples, c.aoRadius = 8, 3.0
    return c


def _with_term(shot, o):
    return abi.Shot(shot.page, shot.pageColor, shot.shadowStrength, shot.reflectivity, shot.reflectionFade, floorOcclusion=o)


@gpu_test
@pytest.mark.parametrize("o", [0.5, 1.0, 0.0])
def test_composite_with_an_occlusion_plane_equals_the_numpy_blend(mcrt, gpu, oracle, o):
    sd, _, occ_exp = GO.skin_expectation(SHOT_CASE)
    cfg = _shot_config()
    shot = _with_term(S.SHOT, o)
    h, w = cfg.height, cfg.width
    ds = mcrt.DeviceScene(sd)
    try:
        F, vis, R, dR = S.own_planes(mcrt, [ds], cfg, [0.0])
        page = S.page_plane(oracle, sd, cfg, shot)
        occ = np.ascontiguousarray(occ_exp["occlusion"])
        dev = {k: torch.from_numpy(np.array(v, copy=True)).cuda() for k, v in dict(F=F, vis=vis, R=R, dR=dR, occ=occ[None]).items()}
        out = torch.zeros((1, h, w, 4), dtype=torch.float32, device="cuda")
        out8 = torch.zeros((1, h, w, 4), dtype=torch.uint8, device="cuda")
        mcrt.composite_shot_batch_device([ds], cfg, shot, dev["F"].data_ptr(), dev["vis"].data_ptr(), dev["R"].data_ptr(), dev["dR"].data_ptr(),
                                         out.data_ptr(), out8.data_ptr(), stream=_stream(), occlusion_ptr=dev["occ"].data_ptr())
        torch.cuda.synchronize()
        want = GO.compose(F[0], vis[0], R[0], dR[0], occ, page, shot)
        S.assert_shot_equal(out.cpu().numpy()[0], out8.cpu().numpy()[0], want, f"composite, o = {o}")
        plain = S.compose(F[0], vis[0], R[0], dR[0], page, S.SHOT)
        if o == 0.0:
            assert np.array_equal(scenes.bits(want), scenes.bits(plain))
        else:
            assert int((scenes.bits(want) != scenes.bits(plain)).any(axis=-1).sum()) >= 40
        # without the plane the term is absent whatever the strength
        mcrt.composite_shot_batch_device([ds], cfg, shot, dev["F"].data_ptr(), dev["vis"].data_ptr(), dev["R"].data_ptr(), dev["dR"].data_ptr(),
                                         out.data_ptr(), 0, stream=_stream())
        torch.cuda.synchronize()
        S.assert_shot_equal(out.cpu().numpy()[0], None, plain, f"composite without the plane, o = {o}")
        ds.check()
    finally:
        ds.close()


@gpu_test
def test_render_shot_with_the_term_equals_its_parts(mcrt, gpu, oracle):
    sd, _, occ_exp = GO.skin_expectation(SHOT_CASE)
    cfg = _shot_config()
    shot = _with_term(S.SHOT, 0.5)
    ds = mcrt.DeviceScene(sd)
    try:
        F, vis, R, dR = S.own_planes(mcrt, [ds], cfg, [0.0])
        _, occ = _device_pass(ds, cfg, 0.0, ("occlusion",))
        GO.assert_planes_equal(occ, occ_exp, "the pass under the shot's config")
        page = S.page_plane(oracle, sd, cfg, shot)
        want = GO.compose(F[0], vis[0], R[0], dR[0], occ["occlusion"], page, shot)
        # the host form, both outputs
        S.assert_shot_equal(mcrt.TileRenderer.renderShot(sd, cfg, shot, ground=0.0, rgba8=False), None, want, "renderShot f32")
        host8 = mcrt.TileRenderer.renderShot(sd, cfg, shot, ground=0.0)
        S.assert_shot_equal(None, host8, want, "renderShot rgba8")
        # the device form, in the caller's scratch
        need = mcrt.shot_scratch_bytes(cfg, shot, 1)
        assert need == mcrt.shot_scratch_bytes(cfg, S.SHOT, 1) + cfg.width * cfg.height * 4
        scratch = torch.zeros((need,), dtype=torch.uint8, device="cuda")
        out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        ds.render_shot_device(cfg, shot, 0.0, scratch.data_ptr(), need, out_f32_ptr=out.data_ptr(), stream=_stream())
        torch.cuda.synchronize()
        S.assert_shot_equal(out.cpu().numpy(), None, want, "render_shot_device")
        ds.check()
        # the floor is darker between and around the feet: at least 40 pixels differ from the shot without the term
        plain8 = mcrt.TileRenderer.renderShot(sd, cfg, S.SHOT, ground=0.0)
        differ = (host8 != plain8).any(axis=-1)
        print("pixels the term changes:", int(differ.sum()))
        assert int(differ.sum()) >= 40
        assert (host8.astype(np.int32) <= plain8.astype(np.int32)).all()  # it only darkens
    finally:
        ds.close()


@gpu_test
def test_recorded_shots_of_the_default_figure(mcrt, gpu):
    """tests/golden/ground_occlusion_shot_*.png: the default S64 figure's studio shot at ground 0.0 without the term and with
    floorOcclusion 0.5, as an MI355X rendered them.  Every value of a shot is defined bit for bit, so the bytes hold."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    want = {k: GO.read_png(os.path.join(golden, name)) for k, name in GO.GOLDEN_SHOTS.items()}
    cfg = GO.golden_shot_config()
    assert want["without"].shape == want["with"].shape == (cfg.height, cfg.width, 4)
    assert np.array_equal(want["side_by_side"], np.concatenate([want["without"], want["with"]], axis=1))
    darker = (want["without"] != want["with"]).any(axis=-1)
    assert int(darker.sum()) == 913 and (want["with"].astype(np.int32) <= want["without"].astype(np.int32)).all()
    ys, xs = np.nonzero(darker)
    assert ys.min() > cfg.height // 2  # the floor between and around the feet, in the lower half of the frame
    sd = scenes.skin_scene("S64", 0)
    for key, o in (("without", 0.0), ("with", 0.5)):
        got = mcrt.TileRenderer.renderShot(sd, cfg, abi.Shot(floorOcclusion=o), ground=0.0)
        bad = np.argwhere((got != want[key]).any(axis=-1))
        assert len(bad) == 0, f"shot {key} the term: {len(bad)} pixels differ from the recorded picture; first {tuple(bad[0])}"


@gpu_test
def test_strength_zero_through_the_new_entry_is_the_existing_entry(mcrt, gpu):
    sd, _, _ = GO.skin_expectation(SHOT_CASE)
    cfg = _shot_config()
    lib = mcrt._lib.load()
    c, s = cfg.to_c(), S.SHOT.to_c()
    h, w = cfg.height, cfg.width
    arr = (C.POINTER(abi.McrtSceneDesc) * 1)(sd.ptr)
    gy = (C.c_float * 1)(0.0)
    old, new = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    old8, new8 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    assert lib.mcrt_render_shot_batch(arr, 1, C.byref(c), C.byref(s), gy, abi.fptr(old), old8.ctypes.data_as(u8), 0) == 0
    assert lib.mcrt_render_shot_batch_occ(arr, 1, C.byref(c), C.byref(s), 0.0, gy, abi.fptr(new), new8.ctypes.data_as(u8), 0) == 0
    assert old.any() and np.array_equal(scenes.bits(old), scenes.bits(new)) and np.array_equal(old8, new8)
    # and with limits of the pass exceeded, which do not apply at strength 0
    cfg.aoSamples = 0
    c = cfg.to_c()
    again = np.zeros((h, w, 4), np.float32)
    assert lib.mcrt_render_shot_batch_occ(arr, 1, C.byref(c), C.byref(s), 0.0, gy, abi.fptr(again), None, 0) == 0
    assert np.array_equal(scenes.bits(old), scenes.bits(again))
