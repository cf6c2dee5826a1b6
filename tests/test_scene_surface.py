"""CPU-side checks of the scene term (E_scene on a signed-distance grid): C ABI and the struct's mirror, the host-only argument
check, registered ops, weight validation and the code-object metadata of the new kernels.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import pytest
import torch

from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_scene_check", 4), ("gq_scene_terms", 18), ("gq_scene_query", 7), ("gq_scene_total", 5)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    src = open(_C.HEADER_PATH).read()
    block = src[src.index("typedef struct gqSceneGrid"):src.index("} gqSceneGrid;")]
    for field in ("const float* values", "int nx, ny, nz", "float origin[3]", "float voxel"):
        assert field in block, field
    # the struct's size from its fields: a pointer, three ints, four floats, padded to the pointer's alignment
    p = ctypes.sizeof(ctypes.c_void_p)
    raw = p + 3 * ctypes.sizeof(ctypes.c_int) + 4 * ctypes.sizeof(ctypes.c_float)
    assert ctypes.sizeof(_C.SceneGrid) == (raw + p - 1) // p * p
    assert [f[0] for f in _C.SceneGrid._fields_] == ["values", "nx", "ny", "nz", "origin", "voxel"]
    assert _C.SceneGrid.nx.offset == p and _C.SceneGrid.origin.offset == p + 12 and _C.SceneGrid.voxel.offset == p + 24


def _grid(shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.SceneGrid()
    g.values = values  # never dereferenced: the check is host only
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(g, batch=4, n_links=14, n_samples=512):
    return _C.lib().gq_scene_check(ctypes.byref(g), batch, n_links, n_samples)


BAD = [
    (dict(shape=(1, 2, 2)), {}, b"nx"), (dict(shape=(2, 1, 2)), {}, b"ny"), (dict(shape=(2, 2, 1)), {}, b"nz"),
    (dict(shape=(1 << 10, 1 << 10, (1 << 8) + 1)), {}, b"nx*ny*nz"), (dict(shape=(1 << 20, 1 << 20, 2)), {}, b"nx*ny*nz"),
    (dict(voxel=0.0), {}, b"voxel"), (dict(voxel=-1.0), {}, b"voxel"), (dict(voxel=float("nan")), {}, b"voxel"),
    (dict(voxel=float("inf")), {}, b"voxel"), (dict(origin=(0.0, float("nan"), 0.0)), {}, b"origin"),
    (dict(origin=(float("inf"), 0.0, 0.0)), {}, b"origin"), (dict(values=None), {}, b"values"),
    ({}, dict(batch=0), b"batch"), ({}, dict(n_links=0), b"n_links"), ({}, dict(n_links=65), b"n_links"),
    ({}, dict(n_samples=0), b"n_samples"),
]


@pytest.mark.parametrize("grid_kw,call_kw,word", BAD)
def test_check_refuses_with_a_message_that_names_the_argument(grid_kw, call_kw, word):
    lib = _C.lib()
    assert _check(_grid()) == 0
    assert _check(_grid(shape=(1 << 10, 1 << 10, 1 << 8))) == 0  # exactly 2^28 nodes
    assert _check(_grid(), n_links=64) == 0
    assert _check(_grid(**grid_kw), **call_kw) != 0
    msg = lib.gq_last_error()
    assert b"scene" in msg and word in msg, msg


def test_check_refuses_a_null_grid():
    assert _C.lib().gq_scene_check(None, 4, 14, 512) != 0
    assert b"scene" in _C.lib().gq_last_error() and b"grid" in _C.lib().gq_last_error()


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    for name in ("scene_distance", "scene_terms", "scene_terms_backward"):
        assert hasattr(ns, name), name
    B, L, Ns, D = 5, 14, 70, 25
    origin = [0.0, 0.0, 0.0]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, LT, v = e(B, D), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(B, L, 3, 4), e(4, 5, 6)
        phi, grad, inside = ns.scene_distance(e(B, Ns, 3), v, origin, 0.1)
        assert phi.shape == (B, Ns) and grad.shape == (B, Ns, 3) and inside.shape == (B, Ns) and inside.dtype == torch.uint8
        es = ns.scene_terms(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, 0.01)
        assert es.shape == (B,)
        wrench, gRt = ns.scene_terms_backward(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, 0.01, e(B))
        assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12)
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.scene_distance(z(7, 3), z(2, 2, 2), origin, 0.1)
    with pytest.raises(NotImplementedError):
        ns.scene_terms(z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(2, 2, 2), origin, 0.1, 0.0)
    with pytest.raises(NotImplementedError):
        ns.scene_terms_backward(z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(2, 2, 2), origin, 0.1,
                                0.0, z(B))


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    B, L = 2, 14
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.scene_terms(torch.zeros(B, 25), None, None, torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 3, 3),
                        torch.zeros(B, L, 3, 4), torch.zeros(8, dtype=torch.uint8), None)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.scene_distance(torch.zeros(7, 3), None)


def test_merge_weights_knows_the_scene_term():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, SCENE_TERMS, TABLETOP_TERMS, TERM_NAMES, merge_weights

    assert SCENE_TERMS == ("E_scene",) and TABLETOP_TERMS == ("E_prior", "E_wall") and len(TERM_NAMES) == 5
    assert DEFAULT_WEIGHTS == {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}
    w = merge_weights(None)
    assert w["E_scene"] == 0.0
    assert merge_weights({"E_scene": 2.5})["E_scene"] == 2.5
    with pytest.raises(ValueError, match="E_scene"):
        merge_weights({"E_scene": -1.0})
    # what tests/test_tabletop_surface.py::test_stepper_refuses_unknown_weight_keys asserts still holds
    assert {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS and all(w[k] == 0.0 for k in TABLETOP_TERMS)
    w = merge_weights({"E_wall": 10, "E_prior": 2.5, "E_pen": 50})
    assert (w["E_wall"], w["E_prior"], w["E_pen"], w["E_dis"]) == (10.0, 2.5, 50.0, 100.0)
    for k in ("E_wall", "E_prior"):
        with pytest.raises(ValueError, match=k):
            merge_weights({k: -1.0})
    for bad in ("E_manipulativity", "e_wall", "wall", "e_scene", "scene"):
        with pytest.raises(ValueError, match=bad):
            merge_weights({bad: 1.0})


def test_new_kernel_resources():
    """The three new kernels: no scratch, and within the 64-register step (8 wavefronts per SIMD) they were built at: the fused
    kernel has 64 VGPRs with the 8 node values, 6 link sums and 9 K accumulators of a lane live at once."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "scene" in k}
    assert sorted(new) == ["gq_scene_kernel", "gq_scene_query_kernel", "gq_scene_total_kernel"], sorted(new)
    for name, r in new.items():
        assert "tabletop" not in name and "cloud" not in name
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64, (name, r)
