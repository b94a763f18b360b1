"""Randomised walks over the states of repaintable resident scenes against the CPU oracle, in the fixed blocks of
tests/resident_fuzz_cases.py (6 scripts each, one script per test); the long sweep is tools/gpu_fuzz.py's mode resident, which runs run_script of this
file.

A script's operations go through DeviceScene.for_skin, set_skin / set_skin_device / set_skins_batch_device, set_view /
set_view_device / set_views_batch_device, set_background, render_device_ex / render_batch_device, the single and the batched
passes and pick, on two streams without a host wait where the script has none.  Every checkpoint is compared: blobs byte for byte
with the host's flatten, frames bit for bit with the oracle's render of the reference-shaped scene (RGBA8 byte for byte through the
oracle's quantize), the planes of the passes bit for bit with the pass checkers on the full-table scene, ids and picks by
assert_ids_name_the_surfaces.  Outputs start 0 ... 2 pixels into sentinel-filled allocations, batched frames a gap apart; leads,
gaps and the skin images' buffers must keep their bytes.  check() on every handle before it closes.  A failing comparison collects
its text and the script goes on; a HIP error raises and ends the block.

No planes of constants can pass: before a script touches the device the ORACLE's census of it must be the pinned one
(resident_fuzz_cases.SCRIPTS, per script; tests/test_resident_fuzz_cases.py pins it on the CPU and says what a block holds).

Two fixed extras: more than kTableSlots table uploads in flight on 300 handles, and one handle on two lanes whose footprint goes
near, far, near under a replayed launch graph."""
import numpy as np
import pytest
import torch

import bake_checker as BC
import ground_checker as G
import layers_checker as L
import light_checker as LC
import reflection_checker as R
import resident_fuzz_cases as RF
import scenes
import skin_paint_checker as S
from minecraftskin_raytracer_amd import abi
from test_gpu_batch_fuzz import GROUND, LAYERS, REFLECTION, SENTINEL, Failures, _bytes_equal

gpu_test = pytest.mark.gpu
LIGHT = {"visibility": (torch.float32, 1), "occlusion": (torch.float32, 1), "direct": (torch.float32, 4)}
BAKE = {k: (torch.float32, c) for k, (_, c) in abi.BAKE_FORMATS.items()}
SPECS = {"layers": LAYERS, "ground": GROUND, "reflection": REFLECTION, "light": LIGHT, "bake": BAKE}
PASS_GAP = 37  # pixels (texels) between the frames of a batched pass


class Runner:
    """One script on the device."""

    def __init__(self, mcrt, oracle, script, exp):
        self.mcrt, self.oracle, self.script = mcrt, oracle, script
        self.exp = {}
        for i, c, v in exp:
            self.exp.setdefault(i, []).append((c, v))
        self.h = {}
        self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.pending, self.keep, self.buffers = [], [], {}
        self.fails = Failures()
        self.compared = {}
        self.what = f"script {script['seed']}"

    # ---- ordering -----------------------------------------------------------------------------------------------------------
    def behind_the_fills(self, k):
        """Stream k waits, on the device, for what torch has enqueued on its own stream: the sentinel fills and the uploads."""
        self.streams[k].wait_stream(torch.cuda.current_stream())
        return self.streams[k].cuda_stream

    def wait(self):
        """The host wait; then the comparisons that were put off."""
        torch.cuda.synchronize()
        todo, self.pending = self.pending, []
        for check in todo:
            check()
        self.keep = []

    def count(self, kind, n=1):
        self.compared[kind] = self.compared.get(kind, 0) + n

    # ---- operations ---------------------------------------------------------------------------------------------------------
    def create(self, op):
        M = self.mcrt
        if op["between"] == "plain":  # the pooled shell goes through the hands of a plain scene
            skin, pose, cfg = S.skin("synthetic_S64"), M.getBuiltinPoses()[3], RF.CONFIGS["default"]
            ds = M.DeviceScene(M.MeshBuilder.buildScene(skin, pose))
            try:
                out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")
                ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                self.fails.compare(lambda: scenes.assert_bit_equal(out.cpu().numpy(), S.oracle_frame(self.oracle, skin, pose, cfg), f"{self.what}: the plain scene in between"))
                ds.check()
            finally:
                ds.close()
        elif op["between"] == "other":  # ... or of the other skin kind
            other = "S32" if op["kind"] == "S64" else "S64"
            pose = M.getBuiltinPoses()[5]
            ds = M.DeviceScene.for_skin(other, pose)
            try:
                white = np.full((64 if other == "S64" else 32, 64, 4), 255, np.uint8)
                self.fails.compare(lambda: S.assert_blob_equal(ds.blob(), S.expected_blob(white, pose), f"{self.what}: the other kind in between"))
                ds.check()
            finally:
                ds.close()
        self.h[op["slot"]] = M.DeviceScene.for_skin(op["kind"], op["pose"], S.look_desc(op["look"]))

    def close(self, slot):
        ds = self.h.pop(slot)
        try:
            ds.check()
        finally:
            ds.close()

    def set_skin(self, op):
        handles = [self.h[s] for s in op["slots"]]
        if op["form"] == "host":
            handles[0].set_skin(op["skins"][0])
            return
        image = op["skins"][0].size
        if op["form"] == "device":
            host = np.full(image + 16, RF.SKIN_SENTINEL, np.uint8)
            off = op["offset"]
            host[off:off + image] = op["skins"][0].reshape(-1)
            dev = torch.from_numpy(host).cuda()
            handles[0].set_skin_device(dev.data_ptr() + off, self.behind_the_fills(op["stream"]))
        else:
            stride = image + op["gap"]
            host = np.full((len(handles), stride), RF.SKIN_SENTINEL, np.uint8)
            for i, skin in enumerate(op["skins"]):
                host[i, :image] = skin.reshape(-1)
            dev = torch.from_numpy(host).cuda()
            self.mcrt.set_skins_batch_device(handles, dev.data_ptr(), stride, self.behind_the_fills(op["stream"]))
        self.keep.append(dev)
        what = f"{self.what}: {op['form']} repaint of {op['slots']}"

        def unchanged():
            if not np.array_equal(dev.cpu().numpy(), host):
                self.fails.append(f"MISMATCH {what}: the launch wrote into the image buffer")

        self.pending.append(unchanged)

    def set_view(self, op):
        handles = [self.h[s] for s in op["slots"]]
        if op["form"] == "batch":
            poses = None if op["poses"] is None else np.stack(op["poses"]).astype(np.float32)
            looks = None if op["looks"] is None else [S.look_desc(k) for k in op["looks"]]
            self.mcrt.set_views_batch_device(handles, poses, looks, self.streams[op["stream"]].cuda_stream)
        elif op["form"] == "host":
            handles[0].set_view(op["poses"][0], S.look_desc(op["looks"][0]))
        else:
            handles[0].set_view_device(op["poses"][0], S.look_desc(op["looks"][0]), self.streams[op["stream"]].cuda_stream)

    def render(self, i, op):
        cfg = RF.CONFIGS[op["cfg"]]
        handles = [self.h[s] for s in op["slots"]]
        n, px, lead = len(handles), cfg.width * cfg.height, op["lead"]
        stride = px + (op["gap"] if op["batch"] else 0)
        want_f, want_u = op["outputs"] in ("both", "f32"), op["outputs"] in ("both", "u8")
        key = op["buffer"]
        if key is None or key not in self.buffers:
            bufs = (torch.empty((lead + n * stride, 4), dtype=torch.float32, device="cuda") if want_f else None,
                    torch.empty((lead + n * stride, 4), dtype=torch.uint8, device="cuda") if want_u else None, lead)
            if key is not None:
                self.buffers[key] = bufs
        else:
            bufs = self.buffers[key]  # the same pointers again: the launch parameters repeat
        f, u, lead = bufs
        expected = self.exp[i]
        what = f"{self.what}: op {i} render {op['cfg']} of {op['slots']}"

        def compare(sighting):
            for name, buf in (("float", f), ("rgba8", u)):
                if buf is None:
                    continue
                a = buf.cpu().numpy()
                if not (a[:lead] == SENTINEL[buf.dtype]).all():
                    self.fails.append(f"MISMATCH {what}: plane {name}: written in front of frame 0")
                for k in range(n):
                    at = lead + k * stride
                    if not (a[at + px:at + stride] == SENTINEL[buf.dtype]).all():
                        self.fails.append(f"MISMATCH {what}: plane {name}: the gap behind frame {k} was written")
                    frame, want = a[at:at + px].reshape(cfg.height, cfg.width, 4), expected[k][1][0]
                    if name == "float":
                        self.fails.compare(lambda: scenes.assert_bit_equal(frame, want, f"{what}: sighting {sighting} frame {k} plane float"))
                    else:
                        q = self.oracle.quantize(want).reshape(cfg.height, cfg.width, 4)
                        self.fails.compare(lambda: _bytes_equal(frame, q, f"{what}: sighting {sighting} frame {k} plane rgba8"))
                    self.count("frame")

        for sighting in range(op["repeat"]):
            for buf in (f, u):
                if buf is not None:
                    buf.fill_(SENTINEL[buf.dtype])
            stream = self.behind_the_fills(op["stream"])
            fp, up = (f.data_ptr() + lead * 16 if want_f else 0), (u.data_ptr() + lead * 4 if want_u else 0)
            if op["batch"]:
                self.mcrt.render_batch_device(handles, cfg, fp, up, stride, stream)
            else:
                handles[0].render_device_ex(cfg, fp, up, 0, 1, abi.LAYOUT_FRAME, stream)
            if op["wait"]:
                self.wait()
                compare(sighting)
            else:
                self.keep += [f, u]
                self.pending.append(lambda: compare(sighting))

    def do_pass(self, i, op):
        if op["sync"]:
            self.wait()
        which, cfg = op["which"], RF.CONFIGS[op["cfg"]]
        handles = [self.h[s] for s in op["slots"]]
        expected = self.exp[i]
        what = f"{self.what}: op {i} {which} {op['cfg']} of {op['slots']}"
        if which == "pick":
            xy = RF.pick_pixels(cfg)
            rec = handles[0].pick(cfg, xy)
            self.fails.compare(lambda: self.compare_pick(rec, xy, expected[0], what))
            self.count("pick")
            return
        spec, n = SPECS[which], len(handles)
        size = max(h.texels for h in handles) if which == "bake" else cfg.width * cfg.height
        stride = size + (PASS_GAP if op["batch"] else 0)
        buf = {k: torch.full((c + n * stride * c,), SENTINEL[t], dtype=t, device="cuda") for k, (t, c) in spec.items()}
        ptrs = {f"{k}_ptr": buf[k].data_ptr() + spec[k][1] * buf[k].element_size() for k in spec}  # every plane one pixel into its allocation
        stream = self.behind_the_fills(op["stream"])
        M = self.mcrt
        if op["batch"]:
            if which == "layers":
                M.render_layers_batch_device(handles, cfg, frame_stride_pixels=stride, stream=stream, **ptrs)
            elif which == "ground":
                M.render_ground_batch_device(handles, cfg, [op["ground"]] * n, frame_stride_pixels=stride, stream=stream, **ptrs)
            elif which == "reflection":
                M.render_reflection_batch_device(handles, cfg, [op["ground"]] * n, frame_stride_pixels=stride, stream=stream, **ptrs)
            elif which == "light":
                M.render_light_batch_device(handles, cfg, frame_stride_pixels=stride, stream=stream, **ptrs)
            else:
                M.bake_light_batch_device(handles, cfg, op["grid"], texel_stride=stride, stream=stream, **ptrs)
        elif which == "layers":
            handles[0].render_layers_device(cfg, stream=stream, **ptrs)
        elif which == "ground":
            handles[0].render_ground_device(cfg, op["ground"], stream=stream, **ptrs)
        elif which == "reflection":
            handles[0].render_reflection_device(cfg, op["ground"], stream=stream, **ptrs)
        elif which == "light":
            handles[0].render_light_device(cfg, stream=stream, **ptrs)
        else:
            handles[0].bake_light_device(cfg, op["grid"], stream=stream, **ptrs)
        texels = [h.texels for h in handles]

        def compare():
            for j in range(n):
                got = {}
                for k, (t, c) in spec.items():
                    a = buf[k].cpu().numpy()
                    if j == 0 and not (a[:c] == SENTINEL[t]).all():
                        self.fails.append(f"MISMATCH {what}: plane {k}: written in front of frame 0")
                    at = c + j * stride * c
                    used = texels[j] if which == "bake" else size
                    if not (a[at + used * c:at + stride * c] == SENTINEL[t]).all():
                        self.fails.append(f"MISMATCH {what}: plane {k}: the gap behind frame {j} was written")
                    shape = (used,) if which == "bake" else (cfg.height, cfg.width)
                    got[k] = a[at:at + used * c].reshape(shape + ((c,) if c > 1 else ()))
                c, want = expected[j]
                where = f"{what}: frame {j}"
                if which == "layers":
                    for k in ("depth", "normal", "albedo"):
                        self.fails.compare(lambda: scenes.assert_bit_equal(got[k], want[k], f"{where} plane {k}"))
                    self.fails.compare(lambda: L.assert_ids_name_the_surfaces(got["id"], want, self.scene_np(c["state"]), f"{where} plane id"))
                elif which == "ground":
                    self.fails.compare(lambda: G.assert_ground_equal(got, want, where))
                elif which == "reflection":
                    self.fails.compare(lambda: R.assert_reflection_equal(got, want, where))
                elif which == "light":
                    self.fails.compare(lambda: LC.assert_light_equal(got, want, where))
                else:
                    self.fails.compare(lambda: BC.assert_bake_equal(got, want, where))
                self.count(which)

        if op["wait"]:
            self.wait()
            compare()
        else:
            self.keep.append(buf)
            self.pending.append(compare)

    def scene_np(self, state):
        return S.full_table_scene(state["skin"], state["pose"], state["look"]).to_numpy()

    def compare_pick(self, rec, xy, expected, what):
        c, surf = expected
        at = (xy[:, 1], xy[:, 0])
        scenes.assert_bit_equal(rec["t"], surf["depth"][at], f"{what} t")
        scenes.assert_bit_equal(rec["normal"], surf["normal"][at], f"{what} normal")
        scenes.assert_bit_equal(rec["albedo"], surf["albedo"][at], f"{what} albedo")
        scenes.assert_bit_equal(rec["point"], surf["point"][at], f"{what} point")
        ids = np.stack([rec["mesh"], rec["face"], rec["tx"], rec["ty"]], axis=1)[:, None, :]
        sub = {k: surf[k][at][:, None] for k in ("hit", "mesh", "outer", "normal", "albedo")}
        L.assert_ids_name_the_surfaces(ids, sub, self.scene_np(c["state"]), f"{what} (pixel index, 0)")

    def blob(self, i, op):
        want = self.exp[i][0][1]
        got = self.h[op["slot"]].blob()  # (waits for the device)
        self.wait()
        self.fails.compare(lambda: S.assert_blob_equal(got, want, f"{self.what}: op {i} blob of {op['slot']}"))
        self.count("blob")

    def run(self) -> list:
        try:
            for i, op in enumerate(self.script["ops"]):
                kind = op["op"]
                if kind == "create":
                    self.create(op)
                elif kind == "close":
                    self.close(op["slot"])
                elif kind == "set_skin":
                    self.set_skin(op)
                elif kind == "set_view":
                    self.set_view(op)
                elif kind == "set_background":
                    self.h[op["slot"]].set_background(op["mode"])
                elif kind == "render":
                    self.render(i, op)
                elif kind == "pass":
                    self.do_pass(i, op)
                elif kind == "blob":
                    self.blob(i, op)
                elif kind == "sync":
                    self.wait()
            self.wait()
        finally:
            for ds in self.h.values():
                ds.close()
            self.h = {}
        return self.fails


def run_script(mcrt, oracle, script, exp, compared=None) -> list:
    """One script on the device; the mismatches as texts (a HIP error raises).  compared: a dict that gathers the checkpoints
    compared by kind."""
    r = Runner(mcrt, oracle, script, exp)
    fails = r.run()
    if compared is not None:
        for k, v in r.compared.items():
            compared[k] = compared.get(k, 0) + v
    return fails


def _report(fails):
    assert not fails, f"{len(fails)} mismatches:\n" + "\n".join(fails[:40])


@pytest.fixture(scope="module")
def checkers_built(mcrt, gpu, oracle):
    """What a process pays once, outside the tests' own time: the transparent checker, the skin layouts, torch's streams, and the
    first repaintable handle with its first repaint, view and render."""
    RF._transparent_checker()
    RF.layout("S64")
    RF.layout("S32")
    stream = torch.cuda.Stream()
    out = torch.zeros((32, 48, 4), dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    ds = mcrt.DeviceScene.for_skin("S64")
    try:
        ds.set_skin(S.skin("synthetic_S64"))
        ds.set_view(mcrt.getBuiltinPoses()[6])
        ds.render_device(RF.CONFIGS["default"], out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, stream.cuda_stream)
        torch.cuda.synchronize()
        ds.check()
    finally:
        ds.close()


# One script of a block of six per test: a whole block takes longer than the longest block test of tests/test_gpu_batch_fuzz.py
# (the time is the oracle's, on the CPU).  What the six hold together is tests/test_resident_fuzz_cases.py's part.
@gpu_test
@pytest.mark.parametrize("seed", list(RF.SCRIPTS))
def test_script_equals_the_oracle(mcrt, gpu, oracle, checkers_built, seed):
    script, exp, digest = RF.script_expectation(oracle, seed)
    assert digest == RF.SCRIPTS[seed], f"script {seed}: the oracle's census is not the pinned one"
    compared = {}
    fails = run_script(mcrt, oracle, script, exp, compared)
    print("script", seed, "compared:", compared)
    assert sum(compared.values()) >= len(exp)
    _report(fails)


@gpu_test
def test_more_table_uploads_than_slots_in_flight_on_three_hundred_handles(mcrt, gpu, oracle):
    """kTableSlots + 2 batch calls on 300 handles — repaints and views in turn — with no host wait in between; then blobs and frames
    0, 255, 256 and 299 of the last state."""
    n, cfg = 300, abi.Config(width=32, height=32)
    g = np.random.default_rng(300)
    calls = RF.table_slots() + 2
    skins = [[RF.make_skin(g, "S64") for _ in range(4)] for _ in range(calls)]  # four images per call, handle i takes image i % 4
    poses = [np.stack([mcrt.getBuiltinPoses()[(i + k) % 7] for i in range(n)]) for k in range(calls)]
    looks = [RF.make_look(g, distance=float(g.uniform(25, 40)), centred=True) for _ in range(calls)]
    stream = torch.cuda.Stream()
    handles = [mcrt.DeviceScene.for_skin("S64") for _ in range(n)]
    try:
        keep = []
        for k in range(calls):
            if k % 2 == 0:
                dev = torch.from_numpy(np.stack([skins[k][i % 4] for i in range(n)])).cuda()
                keep.append(dev)
                stream.wait_stream(torch.cuda.current_stream())
                mcrt.set_skins_batch_device(handles, dev.data_ptr(), stream=stream.cuda_stream)
            else:
                mcrt.set_views_batch_device(handles, poses[k], [S.look_desc(looks[k]) if i % 3 else None for i in range(n)], stream.cuda_stream)
        px = cfg.width * cfg.height
        out = torch.zeros((n, px, 4), dtype=torch.float32, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        mcrt.render_batch_device(handles, cfg, out.data_ptr(), 0, px, stream.cuda_stream)
        torch.cuda.synchronize()
        frames = out.cpu().numpy().reshape(n, cfg.height, cfg.width, 4)
        last_skin = calls - 1 if (calls - 1) % 2 == 0 else calls - 2
        last_view = calls - 1 if (calls - 1) % 2 == 1 else calls - 2
        for i in (0, 255, 256, 299):
            skin, pose, look = skins[last_skin][i % 4], poses[last_view][i], looks[last_view] if i % 3 else None
            S.assert_blob_equal(handles[i].blob(), S.expected_blob(skin, pose, look), f"handle {i}")
            scenes.assert_bit_equal(frames[i], S.oracle_frame(oracle, skin, pose, cfg, look), f"frame {i}")
        for h in handles:
            h.check()
    finally:
        for h in handles:
            h.close()


@gpu_test
def test_two_lanes_near_far_near_under_a_replayed_graph(mcrt, gpu, oracle):
    """set_lanes(2) on a frame of four tile rows: two per lane.  The workspace and the recorded graph are planned for the near
    view; the far view touches one tile, the second near view every tile again."""
    cfg = abi.Config(width=48, height=64, tileSize=16)
    g = np.random.default_rng(2)
    skin, pose = RF.make_skin(g, "S64"), mcrt.getBuiltinPoses()[6]
    near, far, near2 = RF._near(g), RF._far(g), RF._near(g)
    frames = {k: S.oracle_frame(oracle, skin, pose, cfg, look) for k, look in (("near", near), ("far", far), ("near2", near2))}
    out = torch.zeros((cfg.height, cfg.width, 4), dtype=torch.float32, device="cuda")

    def render(ds):
        out.fill_(-12345.0)
        ds.render_device(cfg, out.data_ptr(), 0, 1, abi.LAYOUT_FRAME, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    ds = mcrt.DeviceScene.for_skin("S64", pose, S.look_desc(near))
    try:
        ds.set_lanes(2)
        ds.set_skin(skin)
        for k in range(RF.record_at() + 1):
            scenes.assert_bit_equal(render(ds), frames["near"], f"near, render {k}")
        ds.set_view_device(None, S.look_desc(far), torch.cuda.current_stream().cuda_stream)
        scenes.assert_bit_equal(render(ds), frames["far"], "far")
        ds.set_view(None, S.look_desc(near2))
        scenes.assert_bit_equal(render(ds), frames["near2"], "near again")
        ds.set_view_device(None, S.look_desc(far), torch.cuda.current_stream().cuda_stream)
        scenes.assert_bit_equal(render(ds), frames["far"], "far again")
        S.assert_blob_equal(ds.blob(), S.expected_blob(skin, pose, far), "blob")
        ds.check()
    finally:
        ds.close()
