"""The plane-family table of abi.py and the wrappers of api.py that are written once over it: the table against the structures and
against the values the public names had before it, the selection and its messages, the planes of a frame without pixels, the
refusals of the device forms and their order, and which C entry a shot takes.  No device: every check here comes before the
library does any device work."""
import ctypes as C
import itertools

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi, api

FLT_MAX = np.finfo(np.float32).max
F1, F4 = (np.float32, 1), (np.float32, 4)
# the values of the public names before the table, as literals: (names, formats as (dtype, components), the *_FORMATS dict itself)
GROUND_FORMATS = {"visibility": np.float32, "distance": np.float32, "matte": np.uint8}
GROUND_OCCLUSION_FORMATS = {"occlusion": np.float32, "matte": np.uint8}
BEFORE = {
    "layers": (("depth", "normal", "albedo", "id"), {"depth": F1, "normal": F4, "albedo": F4, "id": (np.int32, 4)}, None),
    "ground": (("visibility", "distance", "matte"), {"visibility": F1, "distance": F1, "matte": (np.uint8, 1)}, GROUND_FORMATS),
    "ground_occlusion": (("occlusion", "matte"), {"occlusion": F1, "matte": (np.uint8, 1)}, GROUND_OCCLUSION_FORMATS),
    "reflection": (("rgba", "rgba8", "distance"), {"rgba": F4, "rgba8": (np.uint8, 4), "distance": F1}, None),
    "light": (("visibility", "occlusion", "direct"), {"visibility": F1, "occlusion": F1, "direct": F4}, None),
    "bake": (("position", "normal", "visibility", "occlusion", "direct"),
             {"position": F4, "normal": F4, "visibility": F1, "occlusion": F1, "direct": F4}, None),
}
# what a plane holds where nothing is hit; every plane not listed holds 0
MISS = {("layers", "depth"): FLT_MAX, ("layers", "id"): (-1, 0, -1, -1), ("ground", "visibility"): 1, ("ground", "distance"): FLT_MAX,
        ("ground_occlusion", "occlusion"): 1, ("reflection", "distance"): FLT_MAX, ("light", "visibility"): 1, ("light", "occlusion"): 1,
        ("bake", "visibility"): 1, ("bake", "occlusion"): 1}
PUBLIC = {"layers": ("LAYER", "layer", abi.McrtLayers), "ground": ("GROUND", "ground", abi.McrtGround),
          "ground_occlusion": ("GROUND_OCCLUSION", "ground_occlusion", abi.McrtGroundOcclusion),
          "reflection": ("REFLECTION", "reflection", abi.McrtReflection), "light": ("LIGHT", "light", abi.McrtLightPlanes),
          "bake": ("BAKE", "bake", abi.McrtBakePlanes)}
FAMILIES = list(BEFORE)


def test_the_table_holds_the_six_families():
    assert list(abi.FAMILIES) == FAMILIES
    assert (abi.GROUND_MAX_SAMPLES, abi.GROUND_OCCLUSION_MAX_SAMPLES, abi.REFLECTION_MAX_BOUNCES, abi.LIGHT_MAX_SAMPLES, abi.BAKE_MAX_GRID) == (113, 113, 8, 113, 4)


@pytest.mark.parametrize("key", FAMILIES)
def test_structure_table_and_public_names_agree(key):
    family = abi.FAMILIES[key]
    names, formats, bare = BEFORE[key]
    upper, lower, struct = PUBLIC[key]
    assert family.struct is struct
    assert tuple(f[0] for f in struct._fields_) == family.names == names
    assert all(f[1] is C.c_void_p for f in struct._fields_) and C.sizeof(struct) == 8 * len(names)
    assert family.formats == formats and list(family.formats) == list(names)
    assert getattr(abi, upper + "_NAMES") == names
    public_formats = getattr(abi, upper + "_FORMATS")
    assert public_formats == (bare if bare is not None else formats) and list(public_formats) == list(names)
    assert getattr(abi, lower + "_names")(names[::-1]) == names


@pytest.mark.parametrize("key", FAMILIES)
def test_selection_is_canonical_and_refuses_with_the_familys_words(key):
    family = abi.FAMILIES[key]
    names = BEFORE[key][0]
    select = getattr(abi, PUBLIC[key][1] + "_names")
    for chosen in itertools.permutations(names, 2):
        assert select(chosen) == family.select(chosen) == tuple(n for n in names if n in chosen)
    assert select(names[-1]) == (names[-1],)  # a bare string is one name
    assert select(iter(names[::-1])) == names
    noun = "layer" if key == "layers" else "plane"
    with pytest.raises(ValueError, match=f"^no {noun} selected$"):
        select(())
    for bad in ("colour", 3, None):
        with pytest.raises(ValueError) as e:
            select((names[0], bad))
        assert str(e.value) == f"{noun}s must be taken from {names}, not {bad!r}"
    with pytest.raises(ValueError, match=f"^{noun}s must be taken from "):
        select("colour")


@pytest.mark.parametrize("key", FAMILIES)
def test_empty_planes_hold_the_miss_values(key):
    family = abi.FAMILIES[key]
    shape = () if key == "bake" else (3, 5)
    for name, (dtype, comps) in BEFORE[key][1].items():
        a = family.empty(name, 2, *shape)
        assert a.dtype == dtype and a.shape == (2,) + shape + ((comps,) if comps > 1 else ()) and a.flags["C_CONTIGUOUS"]
        want = np.broadcast_to(np.asarray(MISS.get((key, name), 0), dtype), a.shape)
        assert np.array_equal(a, want), (key, name)
        assert family.empty(name, 0, *shape).shape == (0,) + a.shape[1:]


@pytest.mark.parametrize("key, form", [("layers", "renderLayersBatch"), ("ground", "renderGroundBatch"), ("ground_occlusion", "renderGroundOcclusionBatch"),
                                       ("reflection", "renderReflectionBatch"), ("light", "renderLightBatch")])
def test_a_frame_without_pixels_keeps_the_empty_planes(mcrt, key, form):
    family = abi.FAMILIES[key]
    sd = mcrt.MeshBuilder.buildDefaultScene()
    out = getattr(mcrt.TileRenderer, form)([sd, sd], abi.Config(width=0, height=5))
    assert list(out) == list(BEFORE[key][0])
    for name, a in out.items():
        want = family.empty(name, 2, 5, 0)
        assert a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want)
    picked = getattr(mcrt.TileRenderer, form)([sd], abi.Config(width=4, height=5, tileSize=0), **{"layers" if key == "layers" else "planes": BEFORE[key][0][::-1][:1]})
    (name,) = picked  # tileSize 0: no tile either, and the planes hold the miss values at full size
    assert np.array_equal(picked[name], family.empty(name, 1, 5, 4))


# (function, family, takes ground, the stride's keyword and a value that is too small for the 16 x 8 frame)
BATCH_DEVICE_FORMS = [("render_layers_batch_device", "layers", False, "frame_stride_pixels", 127),
                      ("render_ground_batch_device", "ground", True, "frame_stride_pixels", 127),
                      ("render_ground_occlusion_batch_device", "ground_occlusion", True, "frame_stride_pixels", 127),
                      ("render_reflection_batch_device", "reflection", True, "frame_stride_pixels", 127),
                      ("render_light_batch_device", "light", False, "frame_stride_pixels", 127),
                      ("bake_light_batch_device", "bake", False, "texel_stride", -1)]


@pytest.mark.parametrize("function, key, takes_ground, stride_kw, small", BATCH_DEVICE_FORMS)
def test_batch_device_forms_refuse_in_order(mcrt, function, key, takes_ground, stride_kw, small):
    fn = getattr(mcrt, function)
    cfg = abi.Config(width=16, height=8)
    names = BEFORE[key][0]
    one = {f"{names[-1]}_ptr": 0x1000}
    at_least = "give at least one of " + ", ".join(f"{n}_ptr" for n in names)
    stride_text = "texel_stride must be >= 0" if key == "bake" else f"frame_stride_pixels {small} is smaller than width * height = 128"

    def call(scenes, ground, **kw):
        return fn(scenes, cfg, *((ground,) if takes_ground else ()), **kw)

    # everything wrong at once: the list is looked at first, then the pointers, then the ground, then the stride
    with pytest.raises(TypeError, match="^device_scenes must be DeviceScene objects$"):
        call([object()], None, **{stride_kw: small})
    with pytest.raises(ValueError) as e:
        call([], None, **{stride_kw: small})
    assert str(e.value) == at_least
    if takes_ground:
        with pytest.raises(ValueError) as e:
            call([], None, **one, **{stride_kw: small})
        assert str(e.value) == "ground heights are needed: a resident scene does not keep its description (see scene_floor)"
        with pytest.raises(ValueError, match="^1 ground heights for 0 scenes$"):
            call([], [float("nan")], **one, **{stride_kw: small})
    with pytest.raises(ValueError) as e:
        call([], 0.0, **one, **{stride_kw: small})
    assert str(e.value) == stride_text
    call([], 0.0, **one)  # no frames: the library has nothing to do, and needs no device for it
    # the single-handle form of the family words its refusals alike
    ds = object.__new__(mcrt.DeviceScene)
    ds._h = C.c_void_p()
    single = getattr(ds, function.replace("_batch_device", "_device"))
    with pytest.raises(ValueError) as e:
        single(cfg, *((float("nan"),) if takes_ground else ()))
    assert str(e.value) == at_least
    if takes_ground:
        with pytest.raises(ValueError, match="^ground must be finite$"):
            single(cfg, float("nan"), **one)


@pytest.mark.parametrize("function", ["render_batch_device", "render_shot_batch_device", "composite_shot_batch_device"])
def test_frame_batch_device_forms_refuse_in_order(mcrt, function):
    fn = getattr(mcrt, function)
    cfg = abi.Config(width=16, height=8)
    lead = {"render_batch_device": (), "render_shot_batch_device": (None, None, 0x1000, 64), "composite_shot_batch_device": (None, 0x1000)}[function]
    stride_kw = "out_stride_pixels" if function.startswith("composite") else "frame_stride_pixels"
    with pytest.raises(TypeError, match="^device_scenes must be DeviceScene objects$"):
        fn([object()], cfg, *lead, **{stride_kw: 127})
    with pytest.raises(ValueError, match="^give out_f32_ptr and/or out_rgba8_ptr$"):
        fn([], cfg, *lead, **{stride_kw: 127})
    if function == "render_shot_batch_device":  # its ground is None here
        with pytest.raises(ValueError, match="^ground heights are needed: a resident scene does not keep its description"):
            fn([], cfg, *lead, out_rgba8_ptr=0x2000, **{stride_kw: 127})
        lead = (None, 0.0, 0x1000, 64)
    with pytest.raises(ValueError) as e:
        fn([], cfg, *lead, out_rgba8_ptr=0x2000, **{stride_kw: 127})
    assert str(e.value) == f"{stride_kw} 127 is smaller than width * height = 128"
    if function != "render_batch_device":  # the shot itself comes last
        with pytest.raises(ValueError, match="^page must be "):
            fn([], cfg, abi.Shot(page="paper"), *lead[1:], out_rgba8_ptr=0x2000)


@pytest.mark.parametrize("shot, plain", [(abi.Shot(), ""), (abi.Shot(floorOcclusion=0.3), "_occ"), (abi.Shot(shadowColor=(0.2, 0, 0)), "_ex"),
                                         (abi.Shot(page="transparent"), "_ex"), (None, "")])
def test_the_shot_variant_is_decided_once(shot, plain):
    for asked in (False, True):
        variant, args = api._shot_variant(shot, asked)
        assert variant == ("_ex" if asked else plain)
        kinds = {"": (abi.McrtShot,), "_occ": (abi.McrtShot, float), "_ex": (abi.McrtShotEx,)}[variant]
        assert tuple(type(a) for a in args) == kinds
    if plain == "_occ":
        assert api._shot_variant(shot)[1][1] == 0.3
        assert api._shot_variant(shot, True)[1][0].floor_occlusion == pytest.approx(0.3)


def test_scratch_bytes_with_bounds_on_an_opaque_page_is_still_zero(mcrt):
    cfg = abi.Config(width=16, height=8)
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(), 2, bounds=True) == 0
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(floorOcclusion=0.3), 2, bounds=True) == 0
    opaque = mcrt.shot_scratch_bytes(cfg, abi.Shot(), 2)
    assert opaque == 2 * 16 * 8 * (16 + 16 + 4) and mcrt.shot_scratch_bytes(cfg, abi.Shot(page="transparent"), 2, bounds=True) == opaque
    assert mcrt.shot_scratch_bytes(cfg, abi.Shot(floorOcclusion=0.3), 2) == opaque + 2 * 16 * 8 * 4
