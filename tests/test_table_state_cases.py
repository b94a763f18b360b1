"""What tests/test_gpu_table_states.py relies on, checked without a device: the reference recurrence of the seed tables'
words, the new entry points' declarations, and that the battery's window-edge scenes and wide fuzz cases really have hits on
the sides of the windows that their labels claim."""
import os

import numpy as np
import pytest

import table_state_cases as T

NEW_SYMBOLS = ("mcrt_device_tables_info", "mcrt_scene_tables", "mcrt_probe_seed_words")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcrt.h")


def test_word397_is_mt19937s_seeding():
    """numpy's RandomState(s) seeds by the same recurrence as std::mt19937(s): its state word 397."""
    seeds = [0, 1, 5489, 1 << 28, (1 << 28) - 1, 1 << 24, (1 << 32) - (1 << 24), 1 << 31, (1 << 32) - 1]
    want = np.array([np.random.RandomState(s).get_state()[1][397] for s in seeds], np.uint32)
    assert np.array_equal(T.word397(seeds), want)
    assert T.word397(np.array([-1, -(1 << 24)], np.int64)).tolist() == T.word397([(1 << 32) - 1, (1 << 32) - (1 << 24)]).tolist()  # two's complement
    g = np.random.default_rng(7)
    more = g.integers(0, 1 << 32, 64)
    assert np.array_equal(T.word397(more), np.array([np.random.RandomState(int(s)).get_state()[1][397] for s in more], np.uint32))


def test_probe_seed_lists():
    w, f = T.window_probe_seeds(), T.full_probe_seeds()
    assert len(w) == 6 + 4096 and w.min() == -T.SEED_HALF and w.max() == T.SEED_HALF - 1
    assert len(f) == 3 + 30 + 6 + 4096 and f.min() == 0 and f.max() == (1 << 32) - 1
    for k in range(1, 16):
        assert (k << 28) in f and (k << 28) - 1 in f
    shared = f[T._in_window(f.astype(np.uint32), T.SEED_HALF)]
    assert len(shared) >= 6  # 0, 1, 2^32 - 1, both ends' inner neighbours: seeds that both tables serve


def test_symbols_and_wrappers(mcrt):
    from minecraftskin_raytracer_amd import _lib

    lib = _lib.load()
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and f"int {name}(" in header, name
    for define in ("#define MCRT_TABLE_WINDOW 0", "#define MCRT_TABLE_FULL 1", "#define MCRT_TABLE_SAMPLE 2"):
        assert define in header
    for name in ("device_tables_info", "probe_seed_words", "sample_table_info"):
        assert name in mcrt.__all__ and callable(getattr(mcrt, name))
    assert callable(mcrt.DeviceScene.tables)
    with pytest.raises(ValueError):
        mcrt.probe_seed_words([T.SEED_HALF], "window")
    with pytest.raises(ValueError):
        mcrt.probe_seed_words([-T.SEED_HALF - 1], "window")
    with pytest.raises(ValueError):
        mcrt.probe_seed_words([-1], "full")
    with pytest.raises(ValueError):
        mcrt.probe_seed_words([0], "sample")


def test_figures_and_argument_checks_without_a_device(mcrt):
    """Before any render a process has no table: zero bytes and builds; the argument checks come before any device work."""
    import ctypes as C

    from minecraftskin_raytracer_amd import _lib

    lib = _lib.load()
    if mcrt.device_count() == 0:
        assert mcrt.device_tables_info() == {k: {"bytes": 0, "builds": 0} for k in ("window", "full", "sample")}
    assert mcrt.device_tables_info()["sample"] == mcrt.sample_table_info()
    assert mcrt.device_tables_info(7) == {k: {"bytes": 0, "builds": 0} for k in ("window", "full", "sample")}  # a device never used
    b, k, mask = C.c_size_t(), C.c_int(), C.c_int(-1)
    fn = lib.mcrt_device_tables_info
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    for which in (-1, 3):
        assert fn(0, which, C.byref(b), C.byref(k)) == 1 and lib.mcrt_last_error()
    assert fn(0, 1, None, None) == 0
    tables = lib.mcrt_scene_tables
    tables.restype, tables.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int)]
    block = (C.c_int32 * (1 << 18))()  # a zeroed handle, larger than any mcrt_scene: it holds nothing
    assert tables(None, C.byref(mask)) == 1 and tables(C.c_void_p(C.addressof(block)), None) == 1
    assert tables(C.c_void_p(C.addressof(block)), C.byref(mask)) == 0 and mask.value == 0
    probe = lib.mcrt_probe_seed_words
    u32_p = C.POINTER(C.c_uint32)
    probe.restype, probe.argtypes = C.c_int, [C.c_int, C.c_int, u32_p, C.c_int, u32_p]
    seeds, out = (C.c_uint32 * 2)(0, 1 << 24), (C.c_uint32 * 2)(7, 7)
    for args in ((0, 2, seeds, 1, out), (0, -1, seeds, 1, out), (0, 0, None, 1, out), (0, 0, seeds, 1, None), (0, 0, seeds, -1, out),
                 (0, 0, seeds, 2, out)):  # the sample table has no words; 2^24 lies outside the window
        assert probe(*args) == 1, args
    assert probe(0, 0, seeds, 0, out) == 0 and probe(0, 1, seeds, 0, out) == 0 and list(out) == [7, 7]


def test_the_states_and_the_battery():
    assert list(T.STATES) == ["none", "all", "full-only", "no-full", "no-sample"]
    for s in T.STATES.values():
        assert s.window == (s.seed_knob != "0") and s.full == (s.full_knob != "0") and s.sample == (s.sample_knob == "2")
        assert s.opens_with_ao == s.full  # the table of all seeds exists before any pass where the state has it
    groups = T.battery()
    keys = [f"{g.key}:{it.key}" for g in groups for it in g.items]
    assert len(set(keys)) == len(keys)
    for g in groups:
        for it in g.items:
            assert it.family == "bake" or (it.cfg.width <= 96 and it.cfg.height <= 64), (g.key, it.key)  # (a bake has texels, no frame)
    masks = T.expected_masks(T.STATES["all"])
    assert masks["skin_p6:s8"] == {"window": True, "full": False, "sample": True}
    assert masks["skin_p0:hard"] == {"window": True, "full": False, "sample": False} and masks["skin_p0:s2"]["sample"]
    assert masks["skin_p0:s16_ao8"] == {"window": True, "full": True, "sample": True}
    assert masks["pass_skin:ground"]["full"] is False and masks["pass_skin:ground_occlusion"]["full"] and not masks["pass_skin:reflection"]["sample"]
    assert not any(m["full"] or m["sample"] or m["window"] for m in T.expected_masks(T.STATES["none"]).values())
    assert all(m["full"] for k, m in T.expected_masks(T.STATES["full-only"]).items() if k.startswith("fuzz_"))


@pytest.mark.parametrize("height", list(T.EDGES))
def test_edge_scenes_have_hits_where_their_labels_say(oracle, height):
    census = T.edge_census(oracle, height)
    print(f"boxes at y = {height}: hits (inside, outside) the sample window {census['sample']}, the seed window {census['seed']}")
    for window, label in zip(("sample", "seed"), T.EDGES[height]):
        inside, outside = census[window]
        if label == "across":
            assert inside > 0 and outside > 0, (window, census)
        elif label == "inside":
            assert inside > 0 and outside == 0, (window, census)
        else:
            assert inside == 0 and outside > 0, (window, census)


def test_wide_cases_have_hits_outside_the_seed_window(oracle):
    inside = outside = 0
    for seed in T.FUZZ_SEEDS["wide"]:
        sd, _, cfg, _ = T.fuzz_case("wide", seed)
        seeds = T.hit_shadow_seeds(oracle, sd, cfg.width, cfg.height)
        i = int(T._in_window(seeds, T.SEED_HALF).sum())
        print(f"wide seed {seed}: {len(seeds)} hits, {i} inside the seed window, {len(seeds) - i} outside")
        inside, outside = inside + i, outside + len(seeds) - i
    assert outside > 0 and inside > 0, (inside, outside)
