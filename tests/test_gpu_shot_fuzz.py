"""The studio shot against tests/shot_fuzz_cases.py on the GPU, everything bit for bit; the long sweep is tools/gpu_fuzz.py's mode
shot, which runs run_blend_case and run_shot_case of this file.

The blocks: 8 blend cases through composite_shot_batch_device against shot_checker.compose (three runs each: the leads of the
planes pin the kernel's sixteen alignment combinations, inputs go absent, one output is written alone), 4 whole shots against the
CPU oracle alone through every form of the entry points.  What a block holds is pinned on the CPU by
tests/test_shot_fuzz_cases.py; a test asserts its pin before it touches the device (the whole shots run one case per test).

The launch limits, each from the source so that a moved constant shows instead of hollowing the test: frames above kLayersGrid
workgroups of kBlock lanes (the kernel strides), kLayersBatchMaxFrames + 1 frames in one call, more batched blends than
kTableSlots without a host wait, a shot batch above the render's kBatchMaxFrames, and shots between renders that replay a
recorded launch graph, in both background modes.

Every output lies behind a lead, between gaps and in front of a tail of sentinels, which must keep their bytes."""

import numpy as np
import pytest
import torch

import resident_fuzz_cases as RF
import scenes
import shot_checker as S
import shot_fuzz_cases as SF
import skin_paint_checker as P
from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
f32 = np.float32
SENTINEL = -12345.0
BYTE_SENTINEL = 77
TAIL = 8  # sentinel elements behind the last frame of every output


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _place(planes, comps, stride, lead):
    """(n, px * comps) float32 → a device buffer with frame i `stride` pixels on behind `lead` floats, sentinels elsewhere; and the
    address of frame 0."""
    n, used = planes.shape
    host = np.full(lead + n * stride * comps, SENTINEL, f32)
    host[lead:].reshape(n, stride * comps)[:, :used] = planes
    t = _dev(host)
    assert t.data_ptr() % 16 == 0  # the lead alone decides the plane's alignment
    return t, t.data_ptr() + 4 * lead


class Outputs:
    """The two output planes of n frames in sentinel-filled allocations: a lead in front (floats / bytes), out_stride pixels from
    frame to frame, TAIL elements behind."""

    def __init__(self, n, px, stride, lead_f=0, lead_b=0, which="both"):
        self.n, self.px, self.stride, self.leads, self.which = n, px, stride, (lead_f, lead_b), which
        self.f = torch.full((lead_f + n * stride * 4 + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
        self.b = torch.full((lead_b + n * stride * 4 + TAIL,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.f.data_ptr() % 16 == 0 and self.b.data_ptr() % 16 == 0
        self.f_ptr = self.f.data_ptr() + 4 * lead_f if which in ("both", "f32") else 0
        self.b_ptr = self.b.data_ptr() + lead_b if which in ("both", "u8") else 0

    def compare(self, want, what) -> list:
        """want: (n, ..., 4) float32.  After a host wait."""
        lines = []
        want = np.ascontiguousarray(want).reshape(self.n, self.px * 4)
        for name, t, lead, sentinel, written in (("f32", self.f, self.leads[0], f32(SENTINEL), self.f_ptr), ("rgba8", self.b, self.leads[1], BYTE_SENTINEL, self.b_ptr)):
            a = t.cpu().numpy()
            if not written:
                if not (a == sentinel).all():
                    lines.append(f"MISMATCH {what}: plane {name} was not asked for and was written")
                continue
            body = a[lead:lead + self.n * self.stride * 4].reshape(self.n, self.stride * 4)
            if not ((a[:lead] == sentinel).all() and (a[lead + self.n * self.stride * 4:] == sentinel).all()):
                lines.append(f"MISMATCH {what}: plane {name}: written in front of or behind the frames")
            if not (body[:, self.px * 4:] == sentinel).all():
                lines.append(f"MISMATCH {what}: plane {name}: the pixels between two frames were written")
            got = body[:, :self.px * 4]
            if name == "f32":
                ne = (got.view(np.uint32) != want.view(np.uint32)).reshape(self.n, self.px, 4).any(axis=-1)
            else:
                ne = (got != S.quantize(want)).reshape(self.n, self.px, 4).any(axis=-1)
            if ne.any():
                i, p = (int(v) for v in np.argwhere(ne)[0])
                shown = want[i, 4 * p:4 * p + 4] if name == "f32" else S.quantize(want[i, 4 * p:4 * p + 4])
                lines.append(f"MISMATCH {what}: plane {name}: {int(ne.sum())} pixels differ; first frame {i} pixel {p}: {got[i, 4 * p:4 * p + 4]} vs {shown}")
        return lines


# ---- the blend ---------------------------------------------------------------------------------------------------------------------
def _coloured_handles(mcrt, colours):
    handles = []
    for bg in colours:
        sd = mcrt.MeshBuilder.buildDefaultScene()
        for i in range(4):
            sd.desc.background_color[i] = bg[i]
        handles.append(mcrt.DeviceScene(sd))
    return handles


def run_blend_case(mcrt, shared, case) -> list:
    """One blend case on the device, its three runs; the mismatches as texts (a HIP error raises).  shared: three open handles
    for the cases whose page does not read the scene."""
    own = _coloured_handles(mcrt, case["backgrounds"]) if case["page"] == "scene colour" else []
    try:
        three = own or shared
        n, px = case["n"], case["w"] * case["h"]
        handles = [three[i % 3] for i in range(n)]  # (the header allows a handle to be listed twice here)
        lines = []
        for r, run in enumerate(case["runs"]):
            F, vis, R, dR, shot = SF.run_inputs(case, run)
            leads = run["leads"]
            keep, ptr = [], {}
            for name, plane, comps in (("figure", F, 4), ("visibility", vis, 1), ("reflection", R, 4), ("distance", dR, 1)):
                ptr[name] = 0
                if plane is not None:
                    t, ptr[name] = _place(plane.reshape(n, px * comps), comps, case["in_stride"], leads[name])
                    keep.append(t)
            out = Outputs(n, px, case["out_stride"], leads["out"], leads["out8"], run["outputs"])
            mcrt.composite_shot_batch_device(handles, case["cfg"], shot, ptr["figure"], ptr["visibility"], ptr["reflection"], ptr["distance"],
                                             out.f_ptr, out.b_ptr, case["in_stride"], case["out_stride"], _stream())
            torch.cuda.synchronize()
            lines += out.compare(SF.expected_run(case, run), f"blend case {case['seed']} ({case['w']} x {case['h']} x {n}, page {case['page']}, "
                                 f"s, k, fade {case['shot_classes']}) run {r} (absent {run['absent']}, leads {leads})")
        return lines
    finally:
        for h in own:
            h.close()


@pytest.fixture(scope="module")
def shared_handles(mcrt, gpu):
    handles = _coloured_handles(mcrt, [(0.125, 0.5, 0.75, 1.0), (0.9, 0.1, 0.3, 1.0), (0.0, 1.0, 0.25, 1.0)])
    yield handles
    for h in handles:
        h.close()


def _report(lines):
    assert not lines, f"{len(lines)} mismatches:\n" + "\n".join(lines[:40])


@gpu_test
@pytest.mark.parametrize("first", list(SF.BLEND_BLOCKS))
def test_blend_block_equals_compose(mcrt, gpu, shared_handles, first):
    cases = SF.blend_block(first)
    assert SF.blend_census(cases) == SF.BLEND_BLOCKS[first], f"block {first}: the census is not the pinned one"
    lines = []
    for case in cases:
        lines += run_blend_case(mcrt, shared_handles, case)
    _report(lines)


# ---- whole shots -------------------------------------------------------------------------------------------------------------------
def _scratch(mcrt, cfg, shot, n):
    need = mcrt.shot_scratch_bytes(cfg, shot, n)
    return torch.full((need + 64,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda"), need


def shoot(mcrt, handles, cfg, shot, heights, gap=0, stream=None, what="") -> tuple:
    """render_shot_batch_device into sentinel-filled buffers → (Outputs, lines about the scratch); no host wait."""
    n, px = len(handles), cfg.width * cfg.height
    out = Outputs(n, px, px + gap)
    scratch, need = _scratch(mcrt, cfg, shot, n)
    mcrt.render_shot_batch_device(handles, cfg, shot, heights, scratch.data_ptr(), need, out.f_ptr, out.b_ptr, px + gap, _stream() if stream is None else stream)

    def scratch_kept():
        return [] if bool((scratch[need:] == BYTE_SENTINEL).all().item()) else [f"MISMATCH {what}: written behind the scratch"]

    return out, scratch_kept


def run_shot_case(mcrt, case, exps, tmp_dir) -> list:
    """One case of whole shots on the device: every call through its form, the refusals beside the deep configs, check() on
    every handle; the mismatches as texts (a HIP error raises)."""
    from test_png import decode_png

    sds = [SF.scene_desc(s) for s in case["scenes"]]
    heights = [SF.ground_height(s, sd) for s, sd in zip(case["scenes"], sds)]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    lines = []
    try:
        for ds, s in zip(handles, case["scenes"]):
            ds.set_background(s["background"])
        n = len(handles)
        for c, (call, per_scene) in enumerate(zip(case["calls"], exps)):
            cfg, shot, form = SF.call_config(case, call), call["shot"], call["form"]
            px = cfg.width * cfg.height
            want = np.stack([e["out"] for e in per_scene])
            what = f"shot case {case['seed']} call {c} ({form}, {call['skip']}, page {call['page']}, config {case['config']}{' deep' if call['deep'] else ''})"
            if form == "batch device":
                out, scratch_kept = shoot(mcrt, handles, cfg, shot, heights, call["gap"], what=what)
                torch.cuda.synchronize()
                lines += out.compare(want, what) + scratch_kept()
            elif form == "single device":
                for i, ds in enumerate(handles):
                    out = Outputs(1, px, px, which=("both", "u8", "f32")[i % 3])
                    scratch, need = _scratch(mcrt, cfg, shot, 1)
                    ds.render_shot_device(cfg, shot, heights[i], scratch.data_ptr(), need, out.f_ptr, out.b_ptr, _stream())
                    torch.cuda.synchronize()
                    lines += out.compare(want[i:i + 1], f"{what} scene {i}")
                    if not bool((scratch[need:] == BYTE_SENTINEL).all().item()):
                        lines.append(f"MISMATCH {what} scene {i}: written behind the scratch")
            elif form == "host":
                if n == 1:
                    got8 = mcrt.TileRenderer.renderShot(sds[0], cfg, shot, heights[0])[None]
                    got = mcrt.TileRenderer.renderShot(sds[0], cfg, shot, heights[0], rgba8=False)[None]
                else:
                    got8 = mcrt.TileRenderer.renderShotBatch(sds, cfg, shot, heights)
                    got = mcrt.TileRenderer.renderShotBatch(sds, cfg, shot, heights, rgba8=False)
                if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                    lines.append(f"MISMATCH {what}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} float pixels differ")
                if not np.array_equal(got8, S.quantize(want)):
                    lines.append(f"MISMATCH {what}: {int((got8 != S.quantize(want)).any(axis=-1).sum())} rgba8 pixels differ")
            else:
                for i, sd in enumerate(sds):
                    path = f"{tmp_dir}/shot_{case['seed']}_{c}_{i}.png"
                    if mcrt.render_shot_png(sd, cfg, path, shot, heights[i]) is not True:
                        lines.append(f"MISMATCH {what} scene {i}: render_shot_png failed")
                        continue
                    with open(path, "rb") as f:
                        img = np.asarray(decode_png(f.read())).reshape(cfg.height, cfg.width, 4)
                    if not np.array_equal(img, per_scene[i]["rgba8"]):
                        lines.append(f"MISMATCH {what} scene {i}: {int((img != per_scene[i]['rgba8']).any(axis=-1).sum())} png pixels differ")
            for refused, text in SF.refusals(case, call):
                try:
                    shoot(mcrt, handles, cfg, refused, heights)
                    torch.cuda.synchronize()
                    lines.append(f"MISMATCH {what}: a shot with s = {refused.shadowStrength}, k = {refused.reflectivity} was not refused")
                except mcrt._lib.McrtError as e:
                    if text not in str(e):
                        lines.append(f"MISMATCH {what}: refused with {e!s}, not with '{text}'")
        for ds in handles:
            ds.check()
    finally:
        for ds in handles:
            ds.close()
    return lines


@pytest.fixture(scope="module")
def checkers_built(mcrt, gpu, oracle):
    """What a process pays once, outside the tests' own time: the transparent checker's compilation and the skin layouts."""
    S.transparent_oracle()
    RF.layout("S64")
    RF.layout("S32")


# One case of a block of four per test: a whole block takes longer than the slowest test of tests/test_gpu_batch_fuzz.py (the time
# is the oracle's, on the CPU).  What the four hold together is tests/test_shot_fuzz_cases.py's part.
@gpu_test
@pytest.mark.parametrize("seed", list(SF.SHOT_CASES))
def test_shot_block_equals_the_oracle(mcrt, gpu, oracle, checkers_built, tmp_path, seed):
    case, exps, digest = SF.shot_case_expectation(oracle, seed)
    assert digest == SF.SHOT_CASES[seed], f"case {seed}: the oracle's census is not the pinned one"
    _report(run_shot_case(mcrt, case, exps, str(tmp_path)))


# ---- the launch limits -------------------------------------------------------------------------------------------------------------
class Blend:
    """All four inputs and both outputs of make_planes' planes for one composite call: uploaded and sentinel-filled by the
    constructor, enqueued by launch(), compared — behind a host wait — by compare()."""

    def __init__(self, cfg, shot, planes, page, in_gap, out_gap, what):
        self.cfg, self.shot, self.planes, self.page, self.what = cfg, shot, planes, page, what
        n, px = planes["F"].shape[0], cfg.width * cfg.height
        self.in_stride, self.keep, self.ptr = px + in_gap, [], {}
        for name, key, comps in (("figure", "F", 4), ("visibility", "vis", 1), ("reflection", "R", 4), ("distance", "dR", 1)):
            t, self.ptr[name] = _place(planes[key].reshape(n, px * comps), comps, self.in_stride, 0)
            self.keep.append(t)
        self.out = Outputs(n, px, px + out_gap)

    def launch(self, mcrt, handles, stream=None):
        p = self.ptr
        mcrt.composite_shot_batch_device(handles, self.cfg, self.shot, p["figure"], p["visibility"], p["reflection"], p["distance"], self.out.f_ptr,
                                         self.out.b_ptr, self.in_stride, self.out.stride, _stream() if stream is None else stream)

    def compare(self) -> list:
        p = self.planes
        return self.out.compare(S.compose(p["F"], p["vis"], p["R"], p["dR"], self.page, self.shot), self.what)


STRIDE_SHAPES = [(2048, 1025, 1, 0), (2049, 1024, 1, 0), (2097153, 1, 1, 0), (1, 2097153, 1, 0), (2048, 1025, 2, 3)]


@gpu_test
@pytest.mark.parametrize("shape", STRIDE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_the_kernel_strides_over_a_frame_above_8192_workgroups(mcrt, gpu, shared_handles, shape):
    """2048 x 1025: the first size whose lanes take a second trip, a power-of-two width (the shift of UDiv); 2049 x 1024: the
    n / d path of UDiv; 2 097 153 x 1: one pixel past the cap, exactly one lane strides; 1 x 2 097 153: width 1; and 2048 x 1025
    as two frames through the table, the outputs 3 pixels apart.  The page is the reference's gradient, so that every pixel's
    row and column enter the result."""
    w, h, n, out_gap = shape
    cap = SF.layers_grid() * SF.block_lanes()
    assert w * h > cap, f"{w} x {h} no longer exceeds kLayersGrid * kBlock = {cap} pixels: the kernel would not stride"
    assert w * h < 2 * cap
    g = np.random.default_rng([0x57D, w, h, n])
    shot, _ = SF.draw_shot(g, 4)  # s, k uniform, fade uniform * 60
    shot, cfg, _ = SF.draw_page(g, shot, w, h, "gradient")
    planes = SF.make_planes(g, 1, h, w, shot.reflectionFade)
    if n == 2:  # the second frame: the first one's pixels, 12 345 places on
        planes = {k: np.concatenate([planes[k], np.roll(planes[k].reshape((1, h * w) + planes[k].shape[3:]), 12345, axis=1).reshape(planes[k].shape)])
                  for k in ("F", "vis", "R", "dR")}
        assert planes["F"][0].tobytes() != planes["F"][1].tobytes()
    page = np.broadcast_to(S.gradient_plane(cfg), (n, h, w, 3))
    assert not np.array_equal(page[0, 0, 0], page[0, h // 2, w // 2])  # the gradient is there
    blend = Blend(cfg, shot, planes, page, 0, out_gap, f"{w} x {h} x {n}")
    blend.launch(mcrt, shared_handles[:n])
    torch.cuda.synchronize()
    _report(blend.compare())


@gpu_test
def test_4097_frames_in_one_call(mcrt, gpu):
    """kLayersBatchMaxFrames + 1 frames of 3 x 2 through the blend: three handles with backgrounds of their own listed in
    rotation, the page their colour (gradientBg off), other planes in every frame.  A wrong d_table + c0, or a wrong frame →
    scene mapping either side of 4095 | 4096, shows in the frames there."""
    n = SF.layers_batch_max_frames() + 1
    assert n > 4096
    g = np.random.default_rng(4097)
    colours = [(0.125, 0.5, 0.75, 1.0), (0.9, 0.1, 0.3, 1.0), (0.0, 1.0, 0.25, 1.0)]
    shot = abi.Shot(shadowStrength=0.6, reflectivity=0.35, reflectionFade=24.0)
    cfg = abi.Config(width=3, height=2, gradientBg=False)
    planes = SF.make_planes(g, n, 2, 3, shot.reflectionFade)
    assert len({planes["F"][i].tobytes() for i in (0, 4095, 4096)}) == 3
    page = np.broadcast_to(np.stack([np.asarray(colours[i % 3][:3], f32) for i in range(n)])[:, None, None, :], (n, 2, 3, 3))
    three = _coloured_handles(mcrt, colours)
    try:
        blend = Blend(cfg, shot, planes, page, 1, 2, f"{n} frames")
        blend.launch(mcrt, [three[i % 3] for i in range(n)])
        torch.cuda.synchronize()
        _report(blend.compare())
    finally:
        for h in three:
            h.close()


@gpu_test
def test_more_batched_blends_than_table_slots_without_a_wait(mcrt, gpu, shared_handles):
    """kTableSlots + 4 batched blends of 3 frames, back to back on one stream, each with inputs, outputs and a Shot of its own; one
    host wait at the end.  A table slot reused before its launch has read it shows as another call's frames."""
    calls = RF.table_slots() + 4
    assert calls > 8
    g = np.random.default_rng(12)
    w, h = 33, 17
    stream = torch.cuda.Stream()
    blends = []
    for c in range(calls):
        shot, _ = SF.draw_shot(g, 4)
        shot, cfg, _ = SF.draw_page(g, shot, w, h, ("gradient", "color")[c % 2])
        planes = SF.make_planes(g, 3, h, w, shot.reflectionFade)
        page = np.broadcast_to(S.gradient_plane(cfg), (3, h, w, 3)) if c % 2 == 0 else np.asarray(shot.pageColor, f32)
        blends.append(Blend(cfg, shot, planes, page, 5, 3, f"call {c} of {calls}"))
    assert len({b.planes["F"].tobytes() for b in blends}) == calls
    stream.wait_stream(torch.cuda.current_stream())  # the uploads and the sentinel fills; from here on nothing but the calls
    for b in blends:
        b.launch(mcrt, shared_handles, stream.cuda_stream)
    torch.cuda.synchronize()
    lines = []
    for b in blends:
        lines += b.compare()
    _report(lines)


def _upward_look(g):
    """A look from above the floor, so that the shadow and the mirror image are in the frame."""
    look = RF.make_look(g, distance=float(g.uniform(30.0, 50.0)), centred=True)
    look["camera_position"] = RF._orbit(float(g.uniform(-180, 180)), float(g.uniform(12.0, 35.0)), float(g.uniform(30.0, 50.0)), look["camera_target"])
    return look


@gpu_test
def test_a_shot_batch_above_the_renders_batch_limit(mcrt, gpu, oracle, checkers_built):
    """kBatchMaxFrames + 4 repaintable handles at 16 x 16: one batched repaint, one batched view change, one
    render_shot_batch_device with all four planes in use — the render takes two launch sequences while every scratch plane
    holds all n frames.  Against the library's own four calls plus compose; frames 0, 255 and the last against the oracle alone."""
    n = SF.batch_max_frames() + 4
    assert n > 256
    cfg = abi.Config(width=16, height=16, tileSize=16)
    shot = abi.Shot(shadowStrength=0.7, reflectivity=0.4, reflectionFade=40.0)
    g = np.random.default_rng(260)
    skins = [RF.make_skin(g, "S64", drop=k % 3) for k in range(16)]
    poses = np.stack([mcrt.getBuiltinPoses()[i % 7] for i in range(n)]).astype(f32)
    looks = [_upward_look(g) for _ in range(n)]
    heights = [0.0] * n
    stream = torch.cuda.Stream()
    handles = [mcrt.DeviceScene.for_skin("S64") for _ in range(n)]
    try:
        images = _dev(np.stack([skins[i % 16] for i in range(n)]))
        stream.wait_stream(torch.cuda.current_stream())
        mcrt.set_skins_batch_device(handles, images.data_ptr(), stream=stream.cuda_stream)
        mcrt.set_views_batch_device(handles, poses, [P.look_desc(k) for k in looks], stream.cuda_stream)
        with torch.cuda.stream(stream):
            out, scratch_kept = shoot(mcrt, handles, cfg, shot, heights, gap=5, stream=stream.cuda_stream, what="260 shots")
        torch.cuda.synchronize()
        F, vis, R, dR = S.own_planes(mcrt, handles, cfg, heights)
        assert len({F[i].tobytes() for i in range(n)}) >= n - 4, "the frames do not differ"
        shadowed = int(((vis < 1).reshape(n, -1).any(axis=1)).sum())
        mirrored = int(((R[..., 3] > 0).reshape(n, -1).any(axis=1)).sum())
        print(f"{n} frames: {shadowed} show shadow, {mirrored} a reflection")
        assert shadowed >= 50 and mirrored >= 50
        page = S.gradient_plane(cfg)
        lines = out.compare(S.compose(F, vis, R, dR, np.broadcast_to(page, (n,) + page.shape), shot), f"{n} shots") + scratch_kept()
        got = out.f.cpu().numpy()[:n * out.stride * 4].reshape(n, out.stride * 4)[:, :out.px * 4].reshape(n, 16, 16, 4)
        for i in (0, 255, n - 1):
            sd = P.reference_scene(skins[i % 16], poses[i], looks[i])
            exp = S.expected_shot(oracle, sd, cfg, shot, 0.0)
            if not np.array_equal(got[i].view(np.uint32), exp["out"].view(np.uint32)):
                lines.append(f"MISMATCH frame {i} against the oracle alone: {int((got[i].view(np.uint32) != exp['out'].view(np.uint32)).any(axis=-1).sum())} pixels differ")
        for ds in handles:
            ds.check()
        _report(lines)
    finally:
        for ds in handles:
            ds.close()


@gpu_test
def test_shots_between_replayed_renders(mcrt, gpu, oracle, checkers_built):
    """One repaintable handle, one config, one output buffer: renders until the launch graph is recorded and replayed, a shot,
    renders again — in reference mode, then in transparent mode — and a shot behind a view change without a host wait.  The shot's
    transparent figure must come from neither mode's recorded graph or plates, nor leave anything in them."""
    cfg = abi.Config(width=48, height=32, tileSize=16, samplesPerPixel=2, shadowSamples=8)
    g = np.random.default_rng(44)
    skin = np.array(RF.make_skin(g, "S64", drop=1))
    skin[..., 3] = np.where(skin[..., 3] >= 128, 255, 0)  # alpha 0 or 255: the reference frame's alpha is 1 everywhere
    pose, pose2 = mcrt.getBuiltinPoses()[6].astype(f32), mcrt.getBuiltinPoses()[2].astype(f32)
    look, look2 = _upward_look(g), _upward_look(g)
    shot = abi.Shot(shadowStrength=0.6, reflectivity=0.35, reflectionFade=30.0)
    sd, sd2 = P.reference_scene(skin, pose, look), P.reference_scene(skin, pose2, look2)
    reference = P.oracle_frame(oracle, skin, pose, cfg, look)
    transparent = S.transparent_oracle().render(sd.ptr, cfg, "transparent")[0]
    transparent2 = S.transparent_oracle().render(sd2.ptr, cfg, "transparent")[0]
    exp, exp2 = S.expected_shot(oracle, sd, cfg, shot, 0.0), S.expected_shot(oracle, sd2, cfg, shot, 0.0)
    assert (reference[..., 3] == 1).all() and (transparent[..., 3] == 0).sum() > 100 and exp["out"].tobytes() != exp2["out"].tobytes()
    for e in (exp, exp2):  # opaque, edge, shadowed and mirrored pixels (a penumbra needs a light with a radius: not asked for here)
        assert all(S.classes(e)[c] > 0 for c in (0, 1, 2, 4)), S.classes(e)
    px = cfg.width * cfg.height
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
    scratch, need = _scratch(mcrt, cfg, shot, 1)
    ds = mcrt.DeviceScene.for_skin("S64", pose, P.look_desc(look))

    def render(want, what):
        out.fill_(SENTINEL)
        ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, _stream())
        torch.cuda.synchronize()
        scenes.assert_bit_equal(out.cpu().numpy(), want, what)

    def shoot_here(want, what):
        out.fill_(SENTINEL)
        ds.render_shot_device(cfg, shot, 0.0, scratch.data_ptr(), need, out.data_ptr(), 0, _stream())
        torch.cuda.synchronize()
        scenes.assert_bit_equal(out.cpu().numpy(), want, what)
        assert bool((scratch[need:] == BYTE_SENTINEL).all().item())

    try:
        ds.set_skin(skin)
        renders = RF.record_at() + 1
        assert renders > 4
        for k in range(renders):
            render(reference, f"reference mode, render {k}")
        shoot_here(exp["out"], "the shot between replayed reference renders")
        for k in range(2):
            render(reference, f"reference mode behind the shot, render {k}")
        ds.set_background("transparent")
        for k in range(renders):
            render(transparent, f"transparent mode, render {k}")
        shoot_here(exp["out"], "the shot between replayed transparent renders")
        out.fill_(SENTINEL)
        ds.set_view_device(pose2, P.look_desc(look2), _stream())
        ds.render_shot_device(cfg, shot, 0.0, scratch.data_ptr(), need, out.data_ptr(), 0, _stream())  # no host wait in between
        torch.cuda.synchronize()
        scenes.assert_bit_equal(out.cpu().numpy(), exp2["out"], "the shot behind the view change")
        for k in range(2):
            render(transparent2, f"transparent mode, the new view, render {k}")
        ds.check()
    finally:
        ds.close()
