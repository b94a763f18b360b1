"""The light bake under extra lights on the GPU (mcrt_bake_light_multi*): position, normal, a visibility and a direct plane per
light, occlusion and the mean of the sub-samples' clamped sums, bit for bit (as uint32) against tests/light_multi_checker.py,
which forms them from the CPU oracle alone.

Every case first asserts on the ORACLE's expectation what it exercises (light_multi_checker.assert_bake_exercised): at least 50
live texels and, in soft mode, at least 25 texels in the penumbra of every extra disk light — far below what the oracle holds on
the figures here (the S64 figure at grid 2 under the three lights: 2719 live texels, 375 and 750 penumbra texels, 1204 texels whose
sum differs from the scene's own light's plane)."""
import numpy as np
import pytest
import torch

import bake_checker as B
import cape_checker as CK
import extra_lights_checker as X
import layers_checker as L
import light_multi_checker as LM
import scenes
import skin_paint_checker as S
import slim_checker as SL
from minecraftskin_raytracer_amd import abi

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
MAXL = abi.MAX_LIGHTS
COMPONENTS = {"position": 4, "normal": 4, "visibility": 1, "occlusion": 1, "direct": 4, "combined": 4}
ALL = ((("position", None), ("normal", None)) + tuple((name, k) for name in ("visibility", "direct") for k in range(MAXL))
       + (("occlusion", None), ("combined", None)))
THREE = X.lights_key(X.CASES["three"])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Planes:
    """Device planes for n frames `stride` texels apart, filled with a sentinel; `asked`: (member, light index or None) pairs."""

    def __init__(self, asked, n, stride):
        self.asked, self.n, self.stride = tuple(asked), n, stride
        self.buf = {a: torch.full((n * stride * COMPONENTS[a[0]],), SENTINEL, dtype=torch.float32, device="cuda") for a in self.asked}

    def args(self) -> dict:
        ptr = lambda a: self.buf[a].data_ptr() if a in self.buf else 0  # noqa: E731
        return dict(position_ptr=ptr(("position", None)), normal_ptr=ptr(("normal", None)), visibility_ptrs=[ptr(("visibility", k)) for k in range(MAXL)],
                    occlusion_ptr=ptr(("occlusion", None)), direct_ptrs=[ptr(("direct", k)) for k in range(MAXL)], combined_ptr=ptr(("combined", None)))

    def frame(self, a, i, n_texels):
        c = COMPONENTS[a[0]]
        flat = self.buf[a].cpu().numpy().reshape(self.n, self.stride * c)[i, :n_texels * c]
        return flat.reshape((n_texels,) + ((c,) if c > 1 else ()))

    def gap_untouched(self, i, n_texels) -> bool:
        return all(bool((t.cpu().numpy().reshape(self.n, self.stride * COMPONENTS[a[0]])[i, n_texels * COMPONENTS[a[0]]:] == SENTINEL).all())
                   for a, t in self.buf.items())


def _assert_frame(planes, i, n_texels, exp, what):
    for a in planes.asked:
        want = exp[a[0]] if a[1] is None else exp[a[0]][a[1]]
        scenes.assert_bit_equal(planes.frame(a, i, n_texels), want, f"{what}: {a[0]}{'' if a[1] is None else [a[1]]}")


def _device(ds, cfg, grid, asked=ALL):
    planes = Planes(asked, 1, ds.texels)
    ds.bake_light_multi_device(cfg, grid, stream=_stream(), **planes.args())
    torch.cuda.synchronize()
    ds.check()
    return planes


@pytest.mark.parametrize("grid, soft", [(1, True), (2, True), (2, False)])
def test_the_s64_figure_under_three_lights(mcrt, gpu, grid, soft):
    lights = X.CASES["three"]
    sd, cfg, exp = LM.bake_skin_expectation("S64", 0, grid, THREE, soft)
    live, pen, changed = LM.assert_bake_exercised(exp, lights, 50, 25 if soft else 0, f"grid {grid} soft {soft}")
    assert changed >= 500
    LM.assert_bake_constants(exp, len(lights))
    if not soft:  # shade()'s own test: without sub-samples every visibility would be 0 or 1; every extra light shadows and lights texels
        v = exp["visibility"][1:4][:, exp["live"]]
        assert ((v == 0).sum(axis=1) >= 100).all() and ((v == 1).sum(axis=1) >= 100).all()
    ds = mcrt.DeviceScene(sd)
    try:
        ds.set_extra_lights(lights)
        _assert_frame(_device(ds, cfg, grid), 0, ds.texels, exp, f"grid {grid} soft {soft} (device form)")
    finally:
        ds.close()
    got = mcrt.TileRenderer.bakeLightMulti(sd, cfg, grid, lights=lights)
    assert list(got) == list(abi.BAKE_MULTI_NAMES)
    LM.assert_equal(got, exp, f"grid {grid} soft {soft} (one-shot form)")


def test_without_extra_lights_the_bytes_are_the_single_light_bake(mcrt, gpu):
    sd, cfg, _, exp = B.case_expectation("s64_pose0")
    ds = mcrt.DeviceScene(sd)
    try:
        n = ds.texels
        old = {k: torch.full((n * COMPONENTS[k],), SENTINEL, dtype=torch.float32, device="cuda") for k in B.PLANES}
        ds.bake_light_device(cfg, 1, stream=_stream(), **{f"{k}_ptr": t.data_ptr() for k, t in old.items()})
        planes = _device(ds, cfg, 1)
        for a, k in ((("position", None), "position"), (("normal", None), "normal"), (("visibility", 0), "visibility"), (("occlusion", None), "occlusion"),
                     (("direct", 0), "direct"), (("combined", None), "direct")):  # (clamp(D_0) = D_0)
            assert torch.equal(planes.buf[a].view(torch.int32), old[k].view(torch.int32)), a
        B.assert_bake_equal({k: old[k].cpu().numpy().reshape(exp[k].shape) for k in B.PLANES}, exp, "bake_light_device")
        # position and normal alone, and with the occlusion: the single-light kernels write them
        for asked in ((("position", None), ("normal", None)), (("normal", None), ("occlusion", None))):
            sub = _device(ds, cfg, 1, asked)
            _assert_frame(sub, 0, n, exp, f"{[a[0] for a in asked]}")
    finally:
        ds.close()


def test_batch_of_s64_slim_and_64x32_handles_with_different_lights(mcrt, gpu, oracle):
    poses = mcrt.getBuiltinPoses()
    scenes_ = [L.skin_case("S64", 0), SL.reference_scene(SL.skin("synthetic"), poses[0]), L.skin_case("S32", 6), L.skin_case("S64", 0)]
    sets = [X.CASES["three"], (X.BRIGHT_FRONT,), X.CASES["fill_left+kicker"], ()]
    cfg = B.config()
    grid = 2
    exps = [LM.expected_bake_multi(oracle, sd, cfg, grid, s) for sd, s in zip(scenes_, sets)]
    for e, s in zip(exps[:3], sets[:3]):
        LM.assert_bake_exercised(e, s, 50, 25, f"{len(s)} extra lights")
    handles = [mcrt.DeviceScene(sd) for sd in scenes_]
    try:
        for ds, s in zip(handles, sets):
            ds.set_extra_lights(s)
        order = [0, 1, 2, 3, 1]  # the slim handle is listed twice
        sizes = [handles[i].texels for i in order]
        assert len(set(sizes)) == 3
        stride = max(sizes) + 37
        planes = Planes(ALL, len(order), stride)
        mcrt.bake_light_multi_batch_device([handles[i] for i in order], cfg, grid, texel_stride=stride, stream=_stream(), **planes.args())
        torch.cuda.synchronize()
        for f, i in enumerate(order):
            _assert_frame(planes, f, sizes[f], exps[i], f"batch frame {f} ({len(sets[i])} extra lights)")
            assert planes.gap_untouched(f, sizes[f]), f"the texels behind frame {f} were written"
        for ds in handles:
            ds.check()
    finally:
        for ds in handles:
            ds.close()


def test_a_caped_handle_through_its_texel_table(mcrt, gpu, oracle):
    lights = X.CASES["fill_left+kicker"]
    skin, cape, pose, look = L.unique_skin("S64"), CK.cape("marker"), mcrt.getBuiltinPoses()[3], CK.behind(150.0)
    sd = CK.reference_scene("S64", skin, cape, pose, 10.0, look)
    ds = mcrt.DeviceScene.for_skin("S64", pose, S.look_desc(look), cape=True)
    try:
        ds.set_skin(skin)
        ds.set_cape(cape)
        ds.set_extra_lights(lights)
        n = ds.texels
        assert n == 3264 + 372 and ds.blob() == mcrt.flatten(sd)
        cfg = B.config()
        exp = LM.expected_bake_multi(oracle, sd, cfg, 1, lights, blob=ds.blob())
        table = mcrt.texel_table(sd)
        assert np.array_equal(exp["table"], table) and np.array_equal(table[-372:, 0], np.full(372, 12))
        rows = np.flatnonzero(table[:, 0] == 12)  # the cape's texels
        assert exp["live"][rows].sum() >= 50 and (exp["combined"][rows].view(np.uint32) != exp["direct"][0][rows].view(np.uint32)).any(axis=-1).sum() >= 25
        planes = _device(ds, cfg, 1)
        _assert_frame(planes, 0, n, exp, "caped bake")
        for a in planes.asked:  # and once more, named by the table's rows
            want = exp[a[0]] if a[1] is None else exp[a[0]][a[1]]
            scenes.assert_bit_equal(planes.frame(a, 0, n)[rows], want[rows], f"the cape's rows of {a}")
    finally:
        ds.close()
