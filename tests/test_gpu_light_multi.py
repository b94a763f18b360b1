"""The light layers under extra lights on the GPU (mcrt_render_light_multi*): every plane — a visibility and a direct plane per
light, occlusion, the clamped sum — bit for bit (as uint32) against tests/light_multi_checker.py, which forms them from the CPU
oracle alone.

So that planes of constants cannot pass, every case first asserts on the ORACLE's expectation what it exercises
(light_multi_checker.assert_exercised): a floor of hit pixels and, in soft mode, for every extra disk light a floor of pixels in
that light's penumbra (0 < vis_k < 1).  The floors are stated per case below, chosen at or under what the oracle gives on the CPU
(the figures in the comments): 50 hits and 25 penumbra pixels on the 96 x 64 frames, as the existing suite asks of them; the small
frames hold less and say what."""
import numpy as np
import pytest
import torch

import extra_lights_checker as X
import layers_checker as L
import light_checker as LC
import light_multi_checker as LM
import scenes
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
POSE0 = "pose0_default_96x64"
SENTINEL = -12345.0
MAXL = abi.MAX_LIGHTS
COMPONENTS = {"visibility": 1, "direct": 4, "occlusion": 1, "combined": 4}
ALL = tuple((name, k) for name in ("visibility", "direct") for k in range(MAXL)) + (("occlusion", None), ("combined", None))
THREE = X.lights_key(X.CASES["three"])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Planes:
    """Device planes for n frames `stride` pixels apart, filled with a sentinel, `lead` floats in front of frame 0 of each; `asked`:
    (member, light index or None) pairs."""

    def __init__(self, cfg, asked=ALL, n=1, stride=None, lead=0):
        self.cfg, self.asked, self.n, self.lead = cfg, tuple(asked), n, lead
        self.px = cfg.width * cfg.height
        self.stride = self.px if stride is None else stride
        self.buf = {a: torch.full((lead + n * self.stride * COMPONENTS[a[0]],), SENTINEL, dtype=torch.float32, device="cuda") for a in self.asked}

    def args(self) -> dict:
        ptr = lambda a: self.buf[a].data_ptr() + 4 * self.lead if a in self.buf else 0  # noqa: E731
        return dict(visibility_ptrs=[ptr(("visibility", k)) for k in range(MAXL)], direct_ptrs=[ptr(("direct", k)) for k in range(MAXL)],
                    occlusion_ptr=ptr(("occlusion", None)), combined_ptr=ptr(("combined", None)))

    def frames(self, a):
        """(n, H, W[, 4]) of one asked plane"""
        c = COMPONENTS[a[0]]
        flat = self.buf[a].cpu().numpy()[self.lead:].reshape(self.n, self.stride * c)[:, :self.px * c]
        return flat.reshape((self.n, self.cfg.height, self.cfg.width) + ((c,) if c > 1 else ()))

    def gaps_untouched(self) -> bool:
        ok = True
        for a, t in self.buf.items():
            c = COMPONENTS[a[0]]
            host = t.cpu().numpy()
            ok = ok and (host[:self.lead] == SENTINEL).all() and (host[self.lead:].reshape(self.n, self.stride * c)[:, self.px * c:] == SENTINEL).all()
        return bool(ok)


def _assert_planes(planes: Planes, exps, what):
    """every asked plane of every frame against its frame's expectation"""
    for a in planes.asked:
        got = planes.frames(a)
        for i, exp in enumerate(exps):
            want = exp[a[0]] if a[1] is None else exp[a[0]][a[1]]
            scenes.assert_bit_equal(got[i], want, f"{what}: frame {i} {a[0]}{'' if a[1] is None else [a[1]]}")


def _device(mcrt, sd, cfg, lights, asked=ALL, lead=0):
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        planes = Planes(cfg, asked, lead=lead)
        ds.render_light_multi_device(cfg, stream=_stream(), **planes.args())
        torch.cuda.synchronize()
        ds.check()
        return planes
    finally:
        ds.close()


def _check_both_forms(mcrt, sd, cfg, lights, exp, what):
    LM.assert_constants(exp, len(lights))
    _assert_planes(_device(mcrt, sd, cfg, lights), [exp], what + " (device form)")
    got = mcrt.TileRenderer.renderLightMulti(sd, cfg, lights=lights)
    assert list(got) == list(abi.LIGHT_MULTI_NAMES) and got["visibility"].shape == (MAXL, cfg.height, cfg.width)
    LM.assert_equal(got, exp, what + " (one-shot form)")


# name -> (checker arguments, (floor of hits, floor of penumbra pixels per extra disk light)); in the comment what the oracle holds:
# hits, (penumbra pixels of the extra disk lights in order), hits whose combined differs from direct[0]
CASES = {
    "three_S8_ballot": (dict(name=POSE0, lights=THREE), (50, 25)),  # 551, (36, 87), 534
    "three_S3_atomics": (dict(name=POSE0, lights=THREE, samples=3), (50, 25)),  # 551, (30, 59), 530
    # the hard modes have no penumbra by construction; their test asks for 20 dark and 20 lit hits per extra light instead
    "three_hard": (dict(name=POSE0, lights=THREE, soft=False), (50, 0)),  # 551, dark (87, 113, 97), lit (464, 438, 454), 522
    "three_S1": (dict(name=POSE0, lights=THREE, samples=1), (50, 0)),  # the same
    "point_among_disks": (dict(name=POSE0, lights=X.lights_key(X.CASES["fill_left+kicker"])), (50, 25)),  # 551, (36,), 507
    "bright_front+negative": (dict(name=POSE0, lights=X.lights_key(X.CASES["bright_front+negative"])), (50, 25)),  # 551, (39, 50), 551
    "S113_several_passes_32x32": (dict(name=POSE0, lights=THREE, samples=113, size=(32, 32), tile=16), (50, 5)),  # 150, (8, 32), 144
    "posed_figure": (dict(name="pose5_orbit_64x64_t16", lights=THREE), (50, 25)),  # 1790, (194, 490), 986
    "1x1": (dict(name="pose0_1x1", lights=THREE), (1, 0)),  # one pixel, one hit
}


@pytest.mark.parametrize("case", list(CASES))
def test_cases_equal_the_checker(mcrt, gpu, case):
    kw, (min_hits, min_pen) = CASES[case]
    sd, cfg, exp = LM.skin_expectation(**kw)
    lights = X.lights_of(kw["lights"])
    hits, pen, changed = LM.assert_exercised(exp, lights, min_hits, min_pen, case)
    if not (kw.get("soft", True) and kw.get("samples", 8) > 1):  # the hard modes: every visibility is 0 or 1, and every extra light shadows something
        v = exp["visibility"][1:len(lights) + 1][:, exp["hit"]]
        assert ((v == 0) | (v == 1)).all() and ((v == 0).sum(axis=1) >= 20).all() and ((v == 1).sum(axis=1) >= 20).all(), case
    assert changed >= min(min_hits, 25) or case == "1x1"
    if case == "S113_several_passes_32x32":
        # 6 undecided hits fit a pass at S = 113 (8192 bytes of positions, 12 per sample), and a penumbra pixel is an undecided hit:
        # three of the four 16 x 16 tiles hold more of light 3's than that (the oracle: 9, 10, 8, 5), so their workgroups take several passes
        pen = exp["hit"] & (exp["visibility"][3] > 0) & (exp["visibility"][3] < 1)
        assert sum(int(pen[y:y + 16, x:x + 16].sum()) > 6 for y in (0, 16) for x in (0, 16)) >= 3
    _check_both_forms(mcrt, sd, cfg, lights, exp, case)


def test_unaligned_planes_on_a_frame_of_odd_width(mcrt, gpu):
    # 50 x 37 at tile 16, every plane 4 bytes off a 16-byte boundary: the scalar store path, a width that is no multiple of 4
    sd, cfg, exp = LM.skin_expectation(POSE0, THREE, size=(50, 37), tile=16)
    LM.assert_exercised(exp, X.CASES["three"], 50, 10, "50x37")  # the oracle: 187 hits, (11, 28) penumbra pixels
    planes = _device(mcrt, sd, cfg, X.CASES["three"], lead=1)
    assert all(t.data_ptr() % 16 == 0 for t in planes.buf.values())
    _assert_planes(planes, [exp], "50x37, planes offset by 4 bytes")
    assert planes.gaps_untouched()


SUBSETS = {
    "visibility2_alone": (("visibility", 2),),
    "combined_alone": (("combined", None),),
    "all_but_occlusion": tuple(a for a in ALL if a[0] != "occlusion"),
    "occlusion_alone": (("occlusion", None),),
}


@pytest.mark.parametrize("which", list(SUBSETS))
def test_plane_subsets(mcrt, gpu, which):
    sd, cfg, exp = LM.skin_expectation(POSE0, THREE)
    _assert_planes(_device(mcrt, sd, cfg, X.CASES["three"], SUBSETS[which]), [exp], which)
    names = tuple(dict.fromkeys(a[0] for a in SUBSETS[which]))
    ks = sorted({a[1] for a in SUBSETS[which] if a[1] is not None}) or None
    got = mcrt.TileRenderer.renderLightMulti(sd, cfg, lights=X.CASES["three"], planes=names, light_indices=ks)
    assert list(got) == [n for n in abi.LIGHT_MULTI_NAMES if n in names]
    for n, a in got.items():
        want = exp[n][list(ks)] if (n in abi.PER_LIGHT_NAMES and ks) else exp[n]
        scenes.assert_bit_equal(a, want, f"{which}: one-shot {n}")


def test_a_plane_of_an_absent_light_holds_the_constants(mcrt, gpu):
    lights = X.CASES["fill_left+kicker"]
    sd, cfg, exp = LM.skin_expectation(POSE0, X.lights_key(lights))
    planes = _device(mcrt, sd, cfg, lights, (("visibility", 3), ("direct", 3), ("visibility", 2)))
    assert (planes.frames(("visibility", 3)) == 1.0).all() and (planes.frames(("direct", 3)) == 0.0).all()
    _assert_planes(planes, [exp], "k = 3 on a two-light handle")


@pytest.mark.parametrize("view", ["boxes_unposed", "many_meshes_hbm"])
def test_scene_views_equal_the_checker(mcrt, gpu, oracle, view):
    import big_scene_cases as B
    from test_gpu_extra_lights import _box_case, _many_mesh_case

    if view == "boxes_unposed":
        sd, c = _box_case(mcrt)
        lights = (abi.Light((-20.0, 30.0, 25.0), (0.5, 0.5, 0.7, 1.0), 4.0), abi.Light((15.0, 10.0, 20.0), (0.8, 0.6, 0.4, 1.0), 0.0),
                  abi.Light((5.0, 40.0, -10.0), (0.3, 0.2, 0.2, 1.0), 8.0))
    else:
        sd, c, _ = _many_mesh_case()
        ctr = B.scene_centre(sd)
        lights = (abi.Light(tuple(float(v) for v in ctr + np.array([-30.0, 25.0, 30.0])), (0.6, 0.6, 0.8, 1.0), 4.0),
                  abi.Light(tuple(float(v) for v in ctr + np.array([20.0, -5.0, 25.0])), (0.7, 0.5, 0.4, 1.0), 0.0),
                  abi.Light(tuple(float(v) for v in ctr + np.array([0.0, 30.0, -20.0])), (0.4, 0.4, 0.3, 1.0), 10.0))
    cfg = LC.config(c.width, c.height, c.tileSize)
    exp = LM.expected_light_multi(oracle, sd, cfg, lights)
    # the existing suite's floor on these two scenes, 50 hits and 25 changed; the oracle: boxes 80 hits, (20, 0) penumbra pixels, 53
    # changed; many meshes 179, (24, 13), 156
    hits, pen, changed = LM.assert_exercised(exp, lights, 50, 0, view)
    assert changed >= 25
    _check_both_forms(mcrt, sd, cfg, lights, exp, view)


def test_batch_of_handles_with_0_to_3_lights(mcrt, gpu):
    sets = [(), (X.BRIGHT_FRONT,), X.CASES["fill_left+kicker"], X.CASES["three"]]
    exps = [LM.skin_expectation(POSE0, X.lights_key(s)) for s in sets]
    sd, cfg = exps[0][0], exps[0][1]
    handles = [mcrt.DeviceScene(sd) for _ in sets]
    try:
        for ds, s in zip(handles, sets):
            ds.set_extra_lights(s)
        order = [3, 0, 1, 2, 3]  # the three-light handle is listed twice
        planes = Planes(cfg, n=len(order), stride=cfg.width * cfg.height + 20)
        mcrt.render_light_multi_batch_device([handles[i] for i in order], cfg, frame_stride_pixels=planes.stride, stream=_stream(), **planes.args())
        torch.cuda.synchronize()
        _assert_planes(planes, [exps[i][2] for i in order], "batch")
        assert planes.gaps_untouched()
        for ds in handles:
            ds.check()
    finally:
        for ds in handles:
            ds.close()


def test_without_extra_lights_the_bytes_are_the_single_light_pass(mcrt, gpu):
    sd, cfg, exp = LC.skin_expectation(POSE0)
    ds = mcrt.DeviceScene(sd)
    try:
        px = cfg.width * cfg.height
        old = {k: torch.full((px * COMPONENTS[k],), SENTINEL, dtype=torch.float32, device="cuda") for k in LC.PLANES}
        ds.render_light_device(cfg, stream=_stream(), **{f"{k}_ptr": t.data_ptr() for k, t in old.items()})
        planes = Planes(cfg)
        ds.render_light_multi_device(cfg, stream=_stream(), **planes.args())
        torch.cuda.synchronize()
        assert torch.equal(planes.buf[("visibility", 0)].view(torch.int32), old["visibility"].view(torch.int32))
        assert torch.equal(planes.buf[("direct", 0)].view(torch.int32), old["direct"].view(torch.int32))
        assert torch.equal(planes.buf[("occlusion", None)].view(torch.int32), old["occlusion"].view(torch.int32))
        assert torch.equal(planes.buf[("combined", None)].view(torch.int32), old["direct"].view(torch.int32))  # clamp(D_0) = D_0
        LC.assert_light_equal({k: old[k].cpu().numpy().reshape(exp[k].shape) for k in LC.PLANES}, exp, "render_light_device")
    finally:
        ds.close()


@pytest.mark.parametrize("ao", [False, True])
def test_the_devices_beauty_frame_is_the_recomposition_of_its_planes(mcrt, gpu, ao):
    lights = X.CASES["three"]
    sd, cfg, exp = LM.skin_expectation(POSE0, THREE)
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        planes = Planes(cfg, (("combined", None), ("occlusion", None)))
        ds.render_light_multi_device(cfg, stream=_stream(), **planes.args())
        beauty = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
        bcfg = LC.beauty_config(cfg, ao=ao, intensity=0.7)
        ds.render_device_ex(bcfg, beauty.data_ptr(), 0, 0, 1, abi.LAYOUT_FRAME, _stream())
        torch.cuda.synchronize()
        ds.check()
    finally:
        ds.close()
    comb, occ = planes.frames(("combined", None))[0], planes.frames(("occlusion", None))[0]
    want = LC.recompose(comb, occ, 0.7) if ao else comb
    hit = exp["hit"]
    assert hit.sum() >= 500
    scenes.assert_bit_equal(beauty.cpu().numpy()[hit], want[hit], f"beauty frame, ao {ao}")


def test_the_lights_are_read_at_enqueue(mcrt, gpu):
    sd, cfg, exp = LM.skin_expectation(POSE0, THREE)
    _, _, plain = LM.skin_expectation(POSE0)
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(X.CASES["three"])
        lit = Planes(cfg, tuple(a for a in ALL if a[0] != "occlusion"))
        ds.render_light_multi_device(cfg, stream=_stream(), **lit.args())
        ds.set_extra_lights(())  # host state alone: the pass above keeps the lights it was enqueued with
        off = Planes(cfg, tuple(a for a in ALL if a[0] != "occlusion"))
        ds.render_light_multi_device(cfg, stream=_stream(), **off.args())
        torch.cuda.synchronize()
        _assert_planes(lit, [exp], "enqueued before set_extra_lights(())")
        _assert_planes(off, [plain], "enqueued after it")
    finally:
        ds.close()
