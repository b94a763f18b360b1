"""The shot as a cut-out against tests/cutout_fuzz_cases.py on the GPU, everything bit for bit; the long sweep is tools/gpu_fuzz.py's
mode cutout, which runs run_cutout_blend_case and run_cutout_shot_case of this file.

The blocks: 8 blend cases through composite_shot_batch_device against cutout_checker.compose_ex and bounds_of (three runs each:
the leads of the planes pin the kernel's sixteen alignment combinations, inputs — the occlusion among them — go absent, one
output is written alone, the boxes are asked for or not; the case with an opaque page, a black shadow and o > 0 takes the _occ
entry), 4 whole cut-outs against the CPU oracle alone through every form of the entry points.  What a block holds is pinned on
the CPU by tests/test_cutout_fuzz_cases.py; a test asserts its pin before it touches the device.

The shared grid, from the source so that a moved constant shows instead of hollowing the test: with bounds a launch shares
kBoundsGroups workgroups among its frames, and frame counts that leave a frame of four chunks three workgroups and two make the
lanes take several trips and the outside-in permutation act in a batch.  And more blends with bounds than kTableSlots, queued
without a host wait.

Every output lies behind a lead, between gaps and in front of a tail of sentinels, the boxes behind a lead and in front of one
more entry, which must keep their bytes."""

import numpy as np
import pytest
import torch

import cutout_checker as X
import cutout_fuzz_cases as CF
import ground_occlusion_checker as GO
import resident_fuzz_cases as RF
import shot_fuzz_cases as SF
import skin_paint_checker as P
import test_gpu_shot_fuzz as T
from minecraftskin_raytracer_amd import abi, api
from test_gpu_shot_fuzz import BYTE_SENTINEL, Outputs, _place, _report, _scratch, _stream, checkers_built, shared_handles  # noqa: F401 (fixtures)

gpu_test = pytest.mark.gpu
f32 = np.float32
BOX_SENTINEL = -777


class Boxes:
    """n boxes behind `lead` int32 and in front of one more entry, all sentinels; ptr: 0 where the run does not ask for them."""

    def __init__(self, n, lead=0, asked=True):
        self.n, self.lead, self.asked = n, lead, asked
        self.t = torch.full((lead + 4 * n + 4,), BOX_SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * lead if asked else 0

    def compare(self, want, what) -> list:
        """want: (n, 4) int32 (not read where the boxes were not asked for).  After a host wait."""
        a = self.t.cpu().numpy()
        body = a[self.lead:self.lead + 4 * self.n].reshape(self.n, 4)
        lines = []
        if not self.asked:
            return [] if (a == BOX_SENTINEL).all() else [f"MISMATCH {what}: boxes were not asked for and were written"]
        if not ((a[:self.lead] == BOX_SENTINEL).all() and (a[self.lead + 4 * self.n:] == BOX_SENTINEL).all()):
            lines.append(f"MISMATCH {what}: written in front of or behind the boxes")
        ne = (body != want).any(axis=1)
        if ne.any():
            i = int(np.argwhere(ne)[0][0])
            lines.append(f"MISMATCH {what}: {int(ne.sum())} boxes differ; first frame {i}: {body[i].tolist()} vs {want[i].tolist()}")
        return lines

    def untouched(self) -> bool:
        return bool((self.t == BOX_SENTINEL).all().item())


# ---- the blend ---------------------------------------------------------------------------------------------------------------------
class CutBlend:
    """One run of a blend case: uploaded and sentinel-filled by the constructor, enqueued by launch(), compared — behind a host
    wait — by compare()."""

    def __init__(self, case, r):
        self.case, self.run = case, case["runs"][r]
        run, n, px = self.run, case["n"], case["w"] * case["h"]
        F, vis, R, dR, occ, self.shot = CF.run_inputs(case, run)
        self.keep, self.ptr = [], {}
        for name, plane, comps in (("figure", F, 4), ("visibility", vis, 1), ("reflection", R, 4), ("distance", dR, 1), ("occlusion", occ, 1)):
            self.ptr[name] = 0
            if plane is not None:
                t, self.ptr[name] = _place(plane.reshape(n, px * comps), comps, case["in_stride"], run["leads"][name])
                self.keep.append(t)
        self.out = Outputs(n, px, case["out_stride"], run["leads"]["out"], run["leads"]["out8"], run["outputs"])
        self.boxes = Boxes(n, run["leads"]["boxes"], run["bounds"])
        self.what = (f"cut-out blend case {case['seed']} ({case['w']} x {case['h']} x {n}, {case['page_class']}, page {case['page']}, s, k, fade, o "
                     f"{case['shot_classes']}, C {run['C']}) run {r} (absent {run['absent']}, leads {run['leads']}, bounds {run['bounds']})")

    def launch(self, mcrt, handles, stream=None):
        p, case = self.ptr, self.case
        mcrt.composite_shot_batch_device(handles, case["cfg"], self.shot, p["figure"], p["visibility"], p["reflection"], p["distance"], self.out.f_ptr,
                                         self.out.b_ptr, case["in_stride"], case["out_stride"], _stream() if stream is None else stream, p["occlusion"],
                                         self.boxes.ptr)

    def compare(self) -> list:
        want = CF.expected_run(self.case, self.run)
        return self.out.compare(want, self.what) + self.boxes.compare(CF.box(want) if self.run["bounds"] else None, self.what)


def run_cutout_blend_case(mcrt, shared, case) -> list:
    """One blend case on the device, its three runs; the mismatches as texts (a HIP error raises).  shared: three open handles
    for the cases whose page does not read the scene."""
    own = T._coloured_handles(mcrt, case["backgrounds"]) if case["page"] == "scene colour" else []
    try:
        three = own or shared
        handles = [three[i % 3] for i in range(case["n"])]  # (the header allows a handle to be listed twice here)
        lines = []
        for r, run in enumerate(case["runs"]):
            blend = CutBlend(case, r)
            entry = api._shot_variant(blend.shot, run["bounds"])[0]
            if entry != ("_occ" if case["page_class"].startswith("opaque, black") else "_ex"):
                lines.append(f"MISMATCH {blend.what}: the call takes the entry '{entry}'")
            blend.launch(mcrt, handles)
            torch.cuda.synchronize()
            lines += blend.compare()
        return lines
    finally:
        for h in own:
            h.close()


@gpu_test
@pytest.mark.parametrize("first", list(CF.BLEND_BLOCKS))
def test_cutout_blend_block_equals_compose_ex(mcrt, gpu, shared_handles, first):
    cases = CF.blend_block(first)
    assert CF.blend_census(cases) == CF.BLEND_BLOCKS[first], f"block {first}: the census is not the pinned one"
    lines = []
    for case in cases:
        lines += run_cutout_blend_case(mcrt, shared_handles, case)
    _report(lines)


# ---- whole cut-outs ----------------------------------------------------------------------------------------------------------------
def shoot(mcrt, handles, cfg, shot, heights, gap=0, bounds=False, box_lead=0):
    """render_shot_batch_device into sentinel-filled buffers → (Outputs, Boxes, scratch, its size); no host wait."""
    n, px = len(handles), cfg.width * cfg.height
    out = Outputs(n, px, px + gap)
    boxes = Boxes(n, box_lead, bounds)
    scratch, need = _scratch(mcrt, cfg, shot, n)
    mcrt.render_shot_batch_device(handles, cfg, shot, heights, scratch.data_ptr(), need, out.f_ptr, out.b_ptr, px + gap, _stream(), boxes.ptr)
    return out, boxes, scratch, need


def _refused(mcrt, handles, heights, cfg, shot, bounds, text, what) -> list:
    """One shot that must be refused with `text`, and with outputs, scratch and boxes as they were."""
    n, px = len(handles), cfg.width * cfg.height
    out, boxes = Outputs(n, px, px), Boxes(n, 0, True)
    scratch = torch.full((64 * px * n + 64,), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
    lines = []
    try:
        mcrt.render_shot_batch_device(handles, cfg, shot, heights, scratch.data_ptr(), scratch.numel(), out.f_ptr, out.b_ptr, px, _stream(),
                                      boxes.ptr if bounds else 0)
        lines.append(f"MISMATCH {what}: {shot!r} under aoSamples {cfg.aoSamples}, shadowSamples {cfg.shadowSamples} was not refused")
    except (mcrt._lib.McrtError, ValueError) as e:
        if text not in str(e):
            lines.append(f"MISMATCH {what}: refused with {e!s}, not with '{text}'")
    torch.cuda.synchronize()
    if not (bool((out.f == T.SENTINEL).all().item()) and bool((out.b == BYTE_SENTINEL).all().item()) and bool((scratch == BYTE_SENTINEL).all().item())
            and boxes.untouched()):
        lines.append(f"MISMATCH {what}: the refused call ('{text}') wrote to its outputs, scratch or boxes")
    return lines


def _floats_and_bytes(got, got8, want, what) -> list:
    lines = []
    if got is not None and not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        lines.append(f"MISMATCH {what}: {int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())} float pixels differ")
    if got8 is not None and not np.array_equal(got8, X.quantize(want)):
        lines.append(f"MISMATCH {what}: {int((got8 != X.quantize(want)).any(axis=-1).sum())} rgba8 pixels differ")
    return lines


def _checked(handles, what) -> list:
    """check() on every handle: what it reports, as texts."""
    lines = []
    for i, ds in enumerate(handles):
        try:
            ds.check()
        except Exception as e:  # noqa: BLE001 (the library's error, whatever its class)
            lines.append(f"LIBRARY ERROR {what}: check() of handle {i}: {e!s}")
    return lines


def run_cutout_shot_case(mcrt, case, exps, tmp_dir) -> list:
    """One case of whole cut-outs on the device: every call through its form, check() on every handle behind every call and
    again behind the refusals beside it; the mismatches and the library's errors as texts, so that what was compared before an
    error is not lost."""
    sds = [CF.scene_desc(s) for s in case["scenes"]]
    heights = [SF.ground_height(s, sd) for s, sd in zip(case["scenes"], sds)]
    handles = [mcrt.DeviceScene(sd) for sd in sds]
    lines = []
    try:
        for ds, s in zip(handles, case["scenes"]):
            ds.set_background(s["background"])
        n = len(handles)
        for c, (call, per_scene) in enumerate(zip(case["calls"], exps)):
            cfg, shot, form = CF.call_config(case, call), call["shot"], call["form"]
            px = cfg.width * cfg.height
            cut = shot.page == "transparent"
            want = np.stack([e["out"] for e in per_scene])
            want_boxes = np.stack([e["bounds"] for e in per_scene])
            what = f"cut-out case {case['seed']} call {c} ({form}, {call['skip']}, {call['page']}, o {call['o']}, config {case['config']}{' deep' if call['deep'] else ''})"
            try:  # (a library error of one call is a finding like a mismatch: the comparisons made so far are kept)
                if form == "batch device":
                    out, boxes, scratch, need = shoot(mcrt, handles, cfg, shot, heights, call["gap"], cut, box_lead=c + 1)
                    torch.cuda.synchronize()
                    lines += out.compare(want, what) + boxes.compare(want_boxes, what)
                    if not bool((scratch[need:] == BYTE_SENTINEL).all().item()):
                        lines.append(f"MISMATCH {what}: written behind the scratch")
                elif form == "single device":
                    for i, ds in enumerate(handles):
                        out = Outputs(1, px, px, which=("both", "u8", "f32")[i % 3])
                        boxes = Boxes(1, i % 4, cut)
                        scratch, need = _scratch(mcrt, cfg, shot, 1)
                        ds.render_shot_device(cfg, shot, heights[i], scratch.data_ptr(), need, out.f_ptr, out.b_ptr, _stream(), boxes.ptr)
                        torch.cuda.synchronize()
                        lines += out.compare(want[i:i + 1], f"{what} scene {i}") + boxes.compare(want_boxes[i:i + 1], f"{what} scene {i}")
                        if not bool((scratch[need:] == BYTE_SENTINEL).all().item()):
                            lines.append(f"MISMATCH {what} scene {i}: written behind the scratch")
                elif form == "host":
                    if n == 1:
                        got8 = mcrt.TileRenderer.renderShot(sds[0], cfg, shot, heights[0], bounds=cut)
                        got = mcrt.TileRenderer.renderShot(sds[0], cfg, shot, heights[0], rgba8=False, bounds=cut)
                        got8, got = ((got8[0][None], got8[1][None]), (got[0][None], got[1][None])) if cut else (got8[None], got[None])
                    else:
                        got8 = mcrt.TileRenderer.renderShotBatch(sds, cfg, shot, heights, bounds=cut)
                        got = mcrt.TileRenderer.renderShotBatch(sds, cfg, shot, heights, rgba8=False, bounds=cut)
                    if cut:
                        for (_, b), name in ((got8, "rgba8"), (got, "float")):
                            if not np.array_equal(b, want_boxes):
                                lines.append(f"MISMATCH {what}: the boxes beside the {name} image: {b.tolist()} vs {want_boxes.tolist()}")
                        got8, got = got8[0], got[0]
                    lines += _floats_and_bytes(got, got8, want, what)
                elif form in ("png", "png crop"):
                    for i, sd in enumerate(sds):
                        path = f"{tmp_dir}/cutout_{case['seed']}_{c}_{i}.png"
                        if mcrt.render_shot_png(sd, cfg, path, shot, heights[i], crop=form == "png crop") is not True:
                            lines.append(f"MISMATCH {what} scene {i}: render_shot_png failed")
                            continue
                        x0, y0, x1, y1 = want_boxes[i].tolist()
                        rgba8 = per_scene[i]["rgba8"]
                        expect = rgba8[y0:y1, x0:x1] if form == "png crop" and x1 > x0 else rgba8  # an empty box: the whole frame
                        img = GO.read_png(path)
                        if img.shape != expect.shape or not np.array_equal(img, expect):
                            lines.append(f"MISMATCH {what} scene {i}: the file holds {img.shape}, expected {expect.shape}, or its pixels differ")
                else:  # the farm: every scene of the case in a slot of its own, with its own pose and look
                    models = ["slim" if s["kind"] == "slim" else "classic" for s in case["scenes"]]
                    batch = mcrt.SkinBatch(n, "S64", slim="slim" in models)
                    try:
                        looks = [None if s["look"] is None else P.look_desc(s["look"]) for s in case["scenes"]]
                        batch.set_views(np.stack([s["pose"] for s in case["scenes"]]).astype(f32), None if all(k is None for k in looks) else looks)
                        skins = np.stack([s["skin"] for s in case["scenes"]])
                        got8, b8 = batch.shots(skins, cfg, shot, ground=heights, bounds=True, models=models)
                        got, b = batch.shots(skins, cfg, shot, ground=heights, rgba8=False, bounds=True, models=models)
                        lines += _floats_and_bytes(got, got8, want, what)
                        if not (np.array_equal(b8, want_boxes) and np.array_equal(b, want_boxes)):
                            lines.append(f"MISMATCH {what}: the boxes: {b8.tolist()} and {b.tolist()} vs {want_boxes.tolist()}")
                    finally:
                        batch.close()
            except mcrt._lib.McrtError as e:
                lines.append(f"LIBRARY ERROR {what}: {e!s}")
            lines += _checked(handles, what)
            for r_cfg, refused, bounds, text in CF.refusals(case, call):
                lines += _refused(mcrt, handles, heights, r_cfg, refused, bounds, text, what)
            lines += _checked(handles, f"{what}, behind the refusals")
    finally:
        for ds in handles:
            ds.close()
    return lines


@pytest.fixture(scope="module")
def slim_layout_built(checkers_built):
    """Beside what checkers_built pays once per process: the slim model's skin layout."""
    RF.layout("slim")


# One case of a block of four per test, as tests/test_gpu_shot_fuzz.py does; what the four hold together is
# tests/test_cutout_fuzz_cases.py's part.
@gpu_test
@pytest.mark.parametrize("seed", list(CF.SHOT_CASES))
def test_cutout_block_equals_the_oracle(mcrt, gpu, oracle, slim_layout_built, tmp_path, seed):
    case, exps, digest = CF.shot_case_expectation(oracle, seed)
    assert digest == CF.SHOT_CASES[seed], f"case {seed}: the oracle's census is not the pinned one"
    _report(run_cutout_shot_case(mcrt, case, exps, str(tmp_path)))


# ---- the shared grid ---------------------------------------------------------------------------------------------------------------
GRID_W, GRID_H = 40, 20


@gpu_test
@pytest.mark.parametrize("n, share", [(600, 3), (700, 2)])
def test_bounds_with_a_share_of_the_grid_between_one_and_the_frames_chunks(mcrt, gpu, shared_handles, n, share):
    """Frames of 40 x 20 pixels are four chunks of kBlock pixels; with n frames a launch with bounds gives each
    kBoundsGroups / n workgroups — 3 (an odd gridDim.x) and 2: lanes take a second trip, and the chunks are taken from the
    outside in.  Frame i's only content is one pixel chosen by i % 9, its alpha 0.75 or the smallest denormal in turn: the first
    and the last pixel of the frame, of chunk 1 and of chunk 3, a pixel at x = 0 and one at x = 39 in the middle chunks, none."""
    block, px = SF.block_lanes(), GRID_W * GRID_H
    chunks = (px + block - 1) // block
    assert chunks == 4 and CF.bounds_groups() // n == share and 1 < share < chunks, "the constants moved: choose frame counts that share the grid again"
    pixels = [0, px - 1, block, 2 * block - 1, 3 * block, px - 1, 7 * GRID_W, 13 * GRID_W + GRID_W - 1, None]
    assert pixels[6] // block in (1, 2) and pixels[7] // block in (1, 2) and pixels[6] % GRID_W == 0 and pixels[7] % GRID_W == GRID_W - 1
    F = np.zeros((n, px, 4), f32)
    for i in range(n):
        if pixels[i % 9] is not None:
            F[i, pixels[i % 9]] = (0.25, 0.5, 1.0, 0.75 if (i // 9) % 2 == 0 else SF.DENORM_MIN)
    F = F.reshape(n, GRID_H, GRID_W, 4)
    want = CF.box(F)
    assert want[8].tolist() == [GRID_W, GRID_H, 0, 0] and want[1].tolist() == [GRID_W - 1, GRID_H - 1, GRID_W, GRID_H] and want[9 + 6].tolist() == [0, 7, 1, 8]
    t, ptr = _place(F.reshape(n, px * 4), 4, px, 0)
    out, boxes = Outputs(n, px, px + 1), Boxes(n, 1)
    mcrt.composite_shot_batch_device([shared_handles[i % 3] for i in range(n)], abi.Config(width=GRID_W, height=GRID_H), abi.Shot("transparent"), ptr,
                                     out_f32_ptr=out.f_ptr, out_rgba8_ptr=out.b_ptr, out_stride_pixels=px + 1, stream=_stream(), bounds_ptr=boxes.ptr)
    torch.cuda.synchronize()
    _report(out.compare(F, f"{n} frames, {share} workgroups each") + boxes.compare(want, f"{n} frames, {share} workgroups each"))


@gpu_test
def test_more_blends_with_bounds_than_table_slots_without_a_wait(mcrt, gpu, shared_handles):
    """kTableSlots + 2 blends with bounds of different transparent cases of several frames, back to back on one stream — the
    current one, behind the uploads and the sentinel fills —, each with planes, a Shot and boxes of its own; one host wait at the
    end.  A table slot or a box entry reused before its launch has read it shows as another call's frames."""
    calls = RF.table_slots() + 2
    assert calls > 8
    blends, seed = [], 1000
    while len(blends) < calls:
        case = CF.make_blend_case(seed)
        seed += 1
        if case["page_class"] == "transparent" and case["n"] >= 2 and case["page"] != "scene colour":
            blends.append(CutBlend(case, next(r for r, run in enumerate(case["runs"]) if run["bounds"])))
    assert len({b.case["F"].tobytes() for b in blends}) == calls
    for b in blends:  # from here on nothing but the calls
        b.launch(mcrt, [shared_handles[i % 3] for i in range(b.case["n"])])
    torch.cuda.synchronize()
    lines = []
    for b in blends:
        lines += b.compare()
    _report(lines)
