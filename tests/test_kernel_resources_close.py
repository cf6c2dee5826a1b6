"""Register, scratch and LDS figures of gq_close_kernel, read from the built library's code-object metadata (no GPU needed), held to
what DESIGN 31 states for it: no scratch, at most 176 VGPRs (two wavefronts per SIMD: one block of eight wavefronts per CU is what
the launch asks for), at most 26 884 bytes of LDS (the frames, the coupling matrix and the keys of eight wavefronts)."""
import os
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
MAX_VGPR, MAX_LDS = 176, 26884


def test_close_kernel_resources():
    from kernel_resources import kernel_resources

    assert os.path.exists(LIB), "library not built"
    res = kernel_resources(LIB)
    assert "gq_close_kernel" in res, "gq_close_kernel is missing from the library"
    r = res["gq_close_kernel"]
    print(f"[gq_close_kernel] {r}")
    assert r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= MAX_VGPR, r
    assert r["lds_static"] <= MAX_LDS, r
