"""Register / scratch budgets of the FK forward kernels with sized box slots (csrc/kin.hip: gq_fk_forward_slots_kernel<KC>), read
from the built library's code-object metadata like tests/test_kernel_resources.py (no GPU needed).  The block has 12 wavefronts,
three per SIMD, so a wavefront may hold 512 / 3 = 170 registers; the budget of the four-slot kernel (160, nothing spilled) is the
budget of every sibling.  The two kernels that share the query's device code with its default of four slots, or not at all, must come out of the
build as they did before the slots became a template parameter."""
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")

UNCHANGED = {  # kernel -> (VGPRs, AGPRs, scratch bytes per lane) of the commit before
    "gq_sdf_wave_kernel<4>": (126, 0, 0),
    "gq_fk_forward_row_kernel": (100, 0, 0),
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_fk_forward_slot_kernels_fit_the_block():
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    slots = {k: v for k, v in res.items() if k.startswith("gq_fk_forward") and k not in ("gq_fk_forward_kernel", "gq_fk_forward_row_kernel")}
    assert sorted(slots) == [f"gq_fk_forward_slots_kernel<{kc}>" for kc in (1, 2, 3)], sorted(slots)
    for name, r in slots.items():
        assert r["vgpr"] + r["agpr"] <= 160 and r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["max_threads"] == 768, (name, r)
    for name, (vgpr, agpr, scratch) in UNCHANGED.items():
        r = res[name]
        assert (r["vgpr"], r["agpr"], r["scratch"]) == (vgpr, agpr, scratch), (name, r)
