"""The seed tables' contents and the battery of tests/test_gpu_table_states.py — a helper, not a test.

Three per-device tables decide which code the hot kernels run: the window seed table (MCRT_SEED_TABLE), the table
of all seeds (MCRT_AO_SEED_TABLE) and the sample table (MCRT_SAMPLE_TABLE).  Here are

  * `word397`: what a seed table holds for a seed, independent of the library and exact;
  * the seeds at which the tables are probed;
  * STATES: the five combinations of tables a process can run with;
  * `battery()`: the renders and passes that every state runs, grouped by the handle that runs them, each item with what the
    handle must hold afterwards;
  * the census of the window-edge scenes (`edge_census`), which a CPU test holds against their labels."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import minecraftskin_raytracer_amd as M
from minecraftskin_raytracer_amd import abi

SEED_HALF = 1 << 24    # the window seed table: seeds -2^24 .. 2^24 - 1
SAMPLE_HALF = 1 << 22  # the sample table: seeds -2^22 .. 2^22 - 1
WINDOW_BYTES, FULL_BYTES, SAMPLE_BYTES = (1 << 25) * 4, 1 << 34, (1 << 23) * 128
FULL_TABLE_ROOM = 3 << 34  # the table of all seeds is built only where three times its size is free


def word397(seeds) -> np.ndarray:
    """State word 397 of std::mt19937's seeding of each seed: x = seed; for i in 1 .. 397: x = 1812433253 * (x ^ (x >> 30)) + i
    (mod 2^32) — vectorised in uint64, whose wrap-around keeps the low 32 bits exact."""
    x = (np.asarray(seeds).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    mask, mult = np.uint64(0xFFFFFFFF), np.uint64(1812433253)
    with np.errstate(over="ignore"):
        for i in range(1, 398):
            x = (mult * (x ^ (x >> np.uint64(30))) + np.uint64(i)) & mask
    return x.astype(np.uint32)


def window_probe_seeds() -> np.ndarray:
    """int64: the window's ends, around zero and 4096 random seeds inside."""
    g = np.random.default_rng(20250101)
    return np.concatenate([np.array([-SEED_HALF, -SEED_HALF + 1, -1, 0, 1, SEED_HALF - 1], np.int64), g.integers(-SEED_HALF, SEED_HALF, 4096)])


def full_probe_seeds() -> np.ndarray:
    """int64 in 0 .. 2^32 - 1: the range's ends, the boundaries of the 16 launches that fill the table (k << 28), the window's
    ends (2^24 and 2^32 - 2^24) with their neighbours, and 4096 random seeds."""
    g = np.random.default_rng(20250102)
    fixed = [0, 1, (1 << 32) - 1]
    for k in range(1, 16):
        fixed += [k << 28, (k << 28) - 1]
    for edge in (SEED_HALF, (1 << 32) - SEED_HALF):
        fixed += [edge - 1, edge, edge + 1]
    return np.concatenate([np.array(fixed, np.int64), g.integers(0, 1 << 32, 4096)])


# ---------------------------------------------------------------------------------------------------------------------
# the table states: the knobs of a child process, whether it opens with an AO render (which builds the table of all seeds
# before any pass asks for it), and the tables it then runs with
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class State:
    name: str
    seed_knob: str | None    # MCRT_SEED_TABLE
    full_knob: str | None    # MCRT_AO_SEED_TABLE
    sample_knob: str | None  # MCRT_SAMPLE_TABLE
    opens_with_ao: bool
    window: bool
    full: bool
    sample: bool

    def env(self) -> dict:
        return {"MCRT_SEED_TABLE": self.seed_knob, "MCRT_AO_SEED_TABLE": self.full_knob, "MCRT_SAMPLE_TABLE": self.sample_knob}


STATES = {s.name: s for s in (
    State("none", "0", "0", "0", False, False, False, False),
    State("all", None, None, "2", True, True, True, True),
    State("full-only", "0", None, "0", True, False, True, False),
    State("no-full", None, "0", "2", False, True, False, True),
    State("no-sample", None, None, "0", True, True, True, False),
)}
OPENING = abi.Config(width=32, height=32, aoEnabled=True)  # the opening render: AO on, the default soft shadows of 8 samples


# ---------------------------------------------------------------------------------------------------------------------
# the battery
# ---------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Item:
    """One call on a group's handle.  kind "render": `cfg` → {"frame"}; "pass": the `_device` form of `family` with `middle`
    (a ground height, a bake's grid) → the family's planes; "shot": render_shot_device → {"rgba8"}.  takes_full / takes_sample:
    the call makes the handle take the table of all seeds / the sample table where the device has or builds one."""
    key: str
    kind: str
    cfg: abi.Config
    takes_full: bool = False
    takes_sample: bool = False
    family: str = ""
    middle: tuple = ()
    expect: object = None  # parent: () -> what the CPU oracle or checker holds, see `check_item`


@dataclasses.dataclass
class Group:
    """A handle: `scene()` gives its description, `lights` its extra lights, `items` its calls in order."""
    key: str
    scene: object
    items: list
    lights: tuple = ()


def _render(key, cfg):
    ao = bool(cfg.aoEnabled) and int(cfg.aoSamples) > 0
    rows = bool(cfg.softShadows) and 2 <= int(cfg.shadowSamples) <= 8
    return Item(key, "render", cfg, takes_full=ao, takes_sample=rows)


BASE = dict(width=96, height=64, maxBounces=2, samplesPerPixel=4)
SHADOWS = [("s8", dict(shadowSamples=8)), ("s4", dict(shadowSamples=4)), ("s2", dict(shadowSamples=2)), ("s9", dict(shadowSamples=9)),
           ("s16", dict(shadowSamples=16)), ("hard", dict(softShadows=False))]


def _skin_renders(pose, order):
    """Rows (8, 4, 2 samples), engine (9, 16) and hard shadows; the same with AO of 8 samples and of 1; 9 bounces — the general
    per-level variants — with 4 and 16 samples and AO.  `order`: of the shadow settings, so that one handle meets a render the
    rows serve first and the other last."""
    import scenes

    items = [_render(label, abi.Config(**BASE, **kw)) for label, kw in order]
    for a in (8, 1):
        items += [_render(f"{label}_ao{a}", abi.Config(**BASE, **kw, aoEnabled=True, aoSamples=a)) for label, kw in order]
    items += [_render(f"b9_s{s}_ao", abi.Config(**dict(BASE, maxBounces=9), shadowSamples=s, aoEnabled=True, aoSamples=8)) for s in (4, 16)]
    return Group(f"skin_p{pose}", lambda: scenes.skin_scene("S64", pose), items)


# The two boxes of test_seed_table_window_and_recurrence_agree at a height y: a hit's shadow seed is about 67890 * y (the boxes
# reach 6 above and below y; x and z add less than 1.3e5), so the sample window's edge 2^22 lies at |y| = 61.8 and the seed
# window's edge 2^24 at |y| = 247.1.  Per height: where the hits' seeds lie relative to the sample window and to the seed
# window — "inside", "across" (hits on both sides of the edge) or "beyond".
EDGES = {0.0: ("inside", "inside"), 60.0: ("across", "inside"), -62.0: ("across", "inside"), 100.0: ("beyond", "inside"),
         247.0: ("beyond", "across"), -247.0: ("beyond", "across"), 400.0: ("beyond", "beyond"), -300.0: ("beyond", "beyond")}
EDGE_CFG = dict(width=96, height=64, maxBounces=3, samplesPerPixel=2, aoEnabled=True, aoSamples=4)


def edge_scene(height) -> "M.SceneDesc":
    import scenes

    tex = scenes.solid((0.8, 0.6, 0.4, 1.0))
    meshes = [scenes.build_box(tex, (0.0, height, 0.0), (8.0, 12.0, 4.0)), scenes.build_box(tex, (7.0, height + 2.0, 1.0), (3.0, 10.0, 3.0))]
    return M.SceneDesc(scenes.simple_scene(meshes, light=(5.0, height + 30.0, 30.0), cam_pos=(0.0, height + 2.0, 40.0), cam_target=(0.0, height, 0.0)))


def _in_window(seeds: np.ndarray, half: int) -> np.ndarray:
    return ((seeds.astype(np.int64) + half) & 0xFFFFFFFF) < 2 * half


def hit_shadow_seeds(oracle, sd, width, height) -> np.ndarray:
    """uint32: the shadow seeds (depth 0) of the primary hits of the pixel centres, as the pass checkers form them."""
    import layers_checker as L
    import light_checker as LC

    hits = oracle.intersect(sd.ptr, L.pixel_rays(oracle, sd.ptr, width, height))
    sums = LC.shadow_sums(hits["point"][hits["hit"] != 0].astype(np.float32))
    return np.array([oracle.seed_cast(float(s)) for s in sums], np.uint32)


def edge_census(oracle, height) -> dict:
    """{"sample": (hits inside the sample window, outside), "seed": (inside the seed window, outside)} of an edge scene."""
    seeds = hit_shadow_seeds(oracle, edge_scene(height), EDGE_CFG["width"], EDGE_CFG["height"])
    out = {}
    for name, half in (("sample", SAMPLE_HALF), ("seed", SEED_HALF)):
        inside = int(_in_window(seeds, half).sum())
        out[name] = (inside, len(seeds) - inside)
    return out


# whole-range seeds: the suite's fuzz cases at fixed seeds, frames cut to 96 x 64.  The wide cases scale scenes up to 1e6, so
# their shadow seeds cover the 32-bit range.  A handle passes the table of all seeds to `lit` only once it holds it, so each
# case opens with a small AO frame of its scene ("primer") and then renders as generated.
FUZZ_SEEDS = {"plain": range(1000, 1008), "bundle": range(7000, 7008), "wide": range(9000, 9008)}


@functools.lru_cache(maxsize=None)
def fuzz_case(group, seed):
    import fuzz_cases

    sd, cfg, what = {"plain": fuzz_cases.make_case, "bundle": fuzz_cases.make_bundle_case, "wide": fuzz_cases.make_wide_case}[group](seed)
    cfg = dataclasses.replace(cfg, width=min(int(cfg.width), 96), height=min(int(cfg.height), 64))
    primer = dataclasses.replace(cfg, width=24, height=16, samplesPerPixel=1, maxBounces=1, dofEnabled=False, aoEnabled=True,
                                 aoSamples=2, aoRadius=float(cfg.aoRadius))
    return sd, primer, cfg, what


PASS_SKIN, PASS_BOX = "pose6_orbit_96x64", "null_and_empty"
SHOT_SKIN = "pose0_33x17_t7"
BAKE_SKIN, BAKE_BOX = "s32_pose6", "two_boxes_q1"


def _pass_groups():
    """One skin case and one box case of each pass checker: the child builds scene and config by the checker's recipe, the
    parent takes the checker's own cached expectation (and holds its config against the recipe's)."""
    import bake_checker as B
    import ground_checker as G
    import ground_occlusion_checker as GO
    import layers_checker as L
    import light_checker as LC
    import reflection_checker as R
    import shot_checker as S

    kind, pose, camera, w, h, tile = L.SKIN_CASES[PASS_SKIN]
    _, bw, bh, btile = L.box_scene(PASS_BOX)

    def box():
        return M.SceneDesc(L.box_scene(PASS_BOX)[0])

    floor = M.scene_floor(box())
    skin_items = [
        Item("ground", "pass", abi.Config(width=w, height=h, tileSize=tile), family="ground", middle=(0.0,),
             expect=lambda: (G.skin_expectation(PASS_SKIN), G.assert_ground_equal)),
        Item("ground_occlusion", "pass", GO.case_config(PASS_SKIN), takes_full=True, family="ground_occlusion", middle=(0.0,),
             expect=lambda: (GO.skin_expectation(PASS_SKIN), GO.assert_planes_equal)),
        Item("light", "pass", LC.config(w, h, tile), takes_full=True, family="light", expect=lambda: (LC.skin_expectation(PASS_SKIN), LC.assert_light_equal)),
        Item("reflection", "pass", R.config(w, h, tile), family="reflection", middle=(6.0,),
             expect=lambda: (R.skin_expectation(PASS_SKIN, 6.0), R.assert_reflection_equal)),
    ]
    box_items = [
        Item("ground", "pass", abi.Config(width=bw, height=bh, tileSize=btile), family="ground", middle=(floor,),
             expect=lambda: (G.box_expectation(PASS_BOX), G.assert_ground_equal)),
        Item("ground_occlusion", "pass", abi.Config(width=bw, height=bh, tileSize=btile, aoSamples=8, aoRadius=3.0), takes_full=True,
             family="ground_occlusion", middle=(floor,), expect=lambda: (GO.box_expectation(PASS_BOX), GO.assert_planes_equal)),
        Item("light", "pass", LC.config(bw, bh, btile), takes_full=True, family="light", expect=lambda: (LC.box_expectation(PASS_BOX), LC.assert_light_equal)),
        Item("reflection", "pass", R.config(bw, bh, btile), family="reflection", middle=(floor,),
             expect=lambda: (R.box_expectation(PASS_BOX), R.assert_reflection_equal)),
    ]
    skind, spose, scamera, _, _, _ = L.SKIN_CASES[SHOT_SKIN]
    shot = Item("shot", "shot", S.case_config(SHOT_SKIN), takes_sample=True, middle=(0.0,), expect=lambda: (S.skin_expectation(SHOT_SKIN), None))
    bakes = []
    for name in (BAKE_SKIN, BAKE_BOX):
        case_kind, scene, kw = B.CASES[name]
        if case_kind == "skin":
            make = functools.partial(L.skin_case, *scene)
        else:
            make = functools.partial(lambda s, r: G.set_light(M.SceneDesc(B.box_scene(s)), None, r), scene, kw.get("radius"))
        item = Item("bake", "pass", B.config(), takes_full=True, family="bake", middle=(kw.get("grid", 1),),
                    expect=functools.partial(lambda n: ((lambda e: (e[0], e[1], e[3]))(B.case_expectation(n)), B.assert_bake_equal), name))
        bakes.append(Group(f"bake_{name}", make, [item]))
    return [Group("pass_skin", lambda: L.skin_case(kind, pose, camera), skin_items), Group("pass_box", box, box_items),
            Group("shot_skin", lambda: L.skin_case(skind, spose, scamera), [shot])] + bakes


def _extra_lights_group():
    import extra_lights_checker as X
    import layers_checker as L

    name = "pose0_default_96x64"
    lights = X.CASES["fill_left+kicker"]
    kind, pose, camera, w, h, tile = L.SKIN_CASES[name]
    item = _render("two_lights", X.config(w, h, tile, aoEnabled=False, aoSamples=4))
    item.expect = lambda: X.skin_expectation(name, X.lights_key(lights))
    return Group("extra_lights", lambda: L.skin_case(kind, pose, camera), [item], lights=tuple(lights))


@functools.lru_cache(maxsize=None)
def battery() -> tuple:
    groups = [_skin_renders(6, SHADOWS), _skin_renders(0, SHADOWS[::-1]), _extra_lights_group()]
    for height in EDGES:
        items = [_render(f"s{s}", abi.Config(**EDGE_CFG, shadowSamples=s)) for s in (4, 16)]
        groups.append(Group(f"edge_y{height:g}", functools.partial(edge_scene, height), items))
    for group, seeds in FUZZ_SEEDS.items():
        for seed in seeds:
            _, primer, cfg, _ = fuzz_case(group, seed)
            groups.append(Group(f"fuzz_{group}_{seed}", functools.partial(lambda g, s: fuzz_case(g, s)[0], group, seed), [_render("primer", primer), _render("case", cfg)]))
    groups += _pass_groups()
    assert len({g.key for g in groups}) == len(groups)
    return tuple(groups)


def expected_masks(state: State) -> dict:
    """{"group:item": the handle's tables() after the item} in `state`: the window table from creation on; the table of all
    seeds from the handle's first AO render or occlusion pass on; the sample table from its first render of 2 .. 8 soft-shadow
    samples on — each only where the state has that table."""
    out = {}
    for g in battery():
        full = sample = False
        for it in g.items:
            full, sample = full or it.takes_full, sample or it.takes_sample
            out[f"{g.key}:{it.key}"] = {"window": state.window, "full": state.full and full, "sample": state.sample and sample}
    return out
