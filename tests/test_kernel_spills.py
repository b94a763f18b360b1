"""Scalar-register spills of the render pipeline's hot kernels ("Scalar registers"), read from the built
library's kernel metadata by tools/kernel_spills.py.  No GPU: the figures are the compiler's.

The limits are the figures of the commit BEFORE the phases read their parameters on their own (profiles/sgpr_spills/
kernel_spills_before.txt), not this tree's: `primary`, `lit` and `resolve` — every view, and the batch entries that share
the bodies — may not spill more SGPRs than that commit's `primary_kernel<2>` (112), `lit_kernel<2>` (126) and
`resolve_kernel` (22) did, and may use no scratch where that commit's build of the same kernel used none.  What the tree
reaches is recorded in profiles/sgpr_spills/README.md, not asserted here."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "minecraftskin_raytracer_amd", "libmcrt.so")

SPILL_LIMIT = {"primary": 112, "lit": 126, "resolve": 22}
# bytes of scratch per lane of the kernels that had any before (the HBM and posed views of `primary` and `lit`); every
# other kernel of the three families had none
SCRATCH_BEFORE = {
    "primary_kernel<0>": 112, "primary_kernel<1>": 80, "primary_batch_kernel<0>": 144, "primary_batch_kernel<1>": 80,
    "lit_kernel<0>": 32, "lit_kernel<1>": 32, "lit_batch_kernel<0>": 32, "lit_batch_kernel<1>": 32,
}
EXPECTED = (["resolve_kernel", "resolve_batch_kernel", "resolve_transparent_kernel", "resolve_transparent_batch_kernel"] +
            [f"{k}_{form}<{v}>" for k in ("primary", "lit") for form in ("kernel", "batch_kernel") for v in (0, 1, 2)])


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_spills", os.path.join(ROOT, "tools", "kernel_spills.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert os.path.exists(LIB), "libmcrt.so is not built"
    return dict(tool.kernel_rows(LIB))


@pytest.mark.parametrize("name", EXPECTED)
def test_hot_kernels_spill_no_more_scalar_registers_than_before(rows, name):
    assert name in rows, f"{name} is not in the library's metadata: {sorted(rows)}"
    r = rows[name]
    family = name.split("_")[0]
    print(f"{name}: sgpr {r['sgpr']} spilled {r['sgpr_spill']} vgpr {r['vgpr']} scratch {r['scratch']}")
    assert r["sgpr_spill"] <= SPILL_LIMIT[family], f"{name} spills {r['sgpr_spill']} SGPRs, the limit of `{family}` is {SPILL_LIMIT[family]}"
    if SCRATCH_BEFORE.get(name, 0) == 0:
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane and had none"
