"""Every non-empty subset of a family's planes through its one-shot host form (mcrt_render_layers, mcrt_render_ground,
mcrt_render_ground_occlusion, mcrt_render_reflection, mcrt_render_light, mcrt_bake_light): each plane bit-equal to the same plane
of the all-planes request, which the families' own suites tie to the oracle, and the dict holding exactly the requested names in
canonical order.  The host forms place the wanted planes one after the other in one device buffer and download each to its own
host address; with a subset every plane lies elsewhere in that buffer than with all of them.

The frame is 33 x 17 at tileSize 16 — a ragged last tile in both axes, and 561 pixels: no multiple of 4, so a 4-byte or 1-byte
plane ends off a 16-byte boundary and the start of the plane behind it matters.  The built-in default scene at pose 1, the bake on
its texel pool at grid 1; 7 + 3 + 7 + 7 + 15 + 31 calls, milliseconds each."""
import itertools

import numpy as np
import pytest

from minecraftskin_raytracer_amd import abi

gpu_test = pytest.mark.gpu
CFG = dict(width=33, height=17, tileSize=16, shadowSamples=2, aoSamples=2, maxBounces=1)
FORMS = {"ground": "renderGround", "ground_occlusion": "renderGroundOcclusion", "reflection": "renderReflection", "light": "renderLight",
         "layers": "renderLayers", "bake": "bakeLight"}
CALLS = {"ground": 7, "ground_occlusion": 3, "reflection": 7, "light": 7, "layers": 15, "bake": 31}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@gpu_test
@pytest.mark.parametrize("key", list(FORMS))
def test_every_plane_subset_equals_the_all_planes_request(mcrt, gpu, key):
    family = abi.FAMILIES[key]
    sd = mcrt.MeshBuilder.buildDefaultScene(mcrt.getBuiltinPoses()[1])
    cfg = abi.Config(**CFG)
    form = getattr(mcrt.TileRenderer, FORMS[key])
    selector = "layers" if key == "layers" else "planes"

    def request(names):
        if key == "bake":
            return form(sd, cfg, grid=1, planes=names, device=gpu)
        return form(sd, cfg, **{selector: names}, device=gpu)

    full = request(family.names)
    assert tuple(full) == family.names
    # something was hit: the full request is not the planes of a frame (a pool) where nothing is
    blank = {k: family.empty(k, len(mcrt.texel_table(sd))) if key == "bake" else family.empty(k, 1, 17, 33)[0] for k in family.names}
    assert all(a.shape == blank[k].shape and a.dtype == blank[k].dtype for k, a in full.items())
    assert any(not _same_bits(a, blank[k]) for k, a in full.items())
    calls = 0
    for size in range(1, len(family.names) + 1):
        for chosen in itertools.combinations(family.names, size):
            got = request(chosen[::-1])  # asked for back to front: the dict comes in canonical order all the same
            calls += 1
            assert tuple(got) == chosen, (key, chosen)
            for name in chosen:
                assert _same_bits(got[name], full[name]), (key, chosen, name)
    assert calls == CALLS[key]
