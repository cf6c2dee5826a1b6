"""CPU-side checks of the clutter scenes (one scene grid per object, composed on the device from posed part grids): C ABI and the
struct's mirror, the two host-only argument checks, registered ops, the code-object metadata of the four new kernels, and the
fp64 oracle's own self-checks.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _clutter_oracle as co
import _scene_oracle as so
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_clutter_check", 5), ("gq_clutter_terms", 19), ("gq_clutter_corridor_terms", 22), ("gq_clutter_query", 8),
                         ("gq_clutter_compose_check", 5), ("gq_clutter_compose", 10)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    # the single-grid siblings' arguments behind (grids, rows_per_grid)
    assert protos["gq_clutter_terms"][1][2:] == protos["gq_scene_terms"][1][1:]
    assert protos["gq_clutter_corridor_terms"][1][2:] == protos["gq_approach_terms"][1][1:]
    src = open(_C.HEADER_PATH).read()
    block = src[src.index("typedef struct gqClutterGrids"):src.index("} gqClutterGrids;")]
    for field in ("const float* values", "int n_grids, nx, ny, nz", "float origin[3]", "float voxel"):
        assert field in block, field
    # the struct's size from its fields: a pointer, four ints, four floats, padded to the pointer's alignment
    p = ctypes.sizeof(ctypes.c_void_p)
    raw = p + 4 * ctypes.sizeof(ctypes.c_int) + 4 * ctypes.sizeof(ctypes.c_float)
    assert ctypes.sizeof(_C.ClutterGrids) == (raw + p - 1) // p * p
    assert [f[0] for f in _C.ClutterGrids._fields_] == ["values", "n_grids", "nx", "ny", "nz", "origin", "voxel"]
    C = _C.ClutterGrids
    assert (C.n_grids.offset, C.nx.offset, C.nz.offset, C.origin.offset, C.voxel.offset) == (p, p + 4, p + 12, p + 16, p + 28)


def _grids(n_grids=3, shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.ClutterGrids()
    g.values = values  # never dereferenced: the checks are host only
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _grid(shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.SceneGrid()
    g.values = values
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(g, batch=12, rows_per_grid=4, n_links=14, n_samples=512):
    return _C.lib().gq_clutter_check(ctypes.byref(g), batch, rows_per_grid, n_links, n_samples)


GRID_BAD = [
    (dict(shape=(1, 2, 2)), b"nx"), (dict(shape=(2, 1, 2)), b"ny"), (dict(shape=(2, 2, 1)), b"nz"),
    (dict(shape=(1 << 10, 1 << 10, (1 << 8) + 1)), b"nx*ny*nz"), (dict(voxel=0.0), b"voxel"), (dict(voxel=float("nan")), b"voxel"),
    (dict(voxel=float("inf")), b"voxel"), (dict(origin=(0.0, float("nan"), 0.0)), b"origin"), (dict(values=None), b"values"),
]
BAD = [(kw, {}, w) for kw, w in GRID_BAD] + [
    (dict(n_grids=0), dict(batch=0, rows_per_grid=1), b"n_grids"), (dict(n_grids=65537), dict(batch=65537, rows_per_grid=1), b"n_grids"),
    ({}, dict(batch=0, rows_per_grid=0), b"batch"), ({}, dict(n_links=0), b"n_links"), ({}, dict(n_links=65), b"n_links"),
    ({}, dict(n_samples=0), b"n_samples"), ({}, dict(batch=3, rows_per_grid=0), b"rows_per_grid"),
    ({}, dict(batch=13), b"batch"), ({}, dict(batch=11), b"batch"), ({}, dict(rows_per_grid=3), b"batch"),
]


@pytest.mark.parametrize("grid_kw,call_kw,word", BAD)
def test_check_refuses_with_a_message_that_names_the_argument(grid_kw, call_kw, word):
    lib = _C.lib()
    assert _check(_grids()) == 0
    assert _check(_grids(n_grids=1), batch=4) == 0 and _check(_grids(n_grids=12), rows_per_grid=1) == 0
    assert _check(_grids(n_grids=65536), batch=65536, rows_per_grid=1) == 0
    assert _check(_grids(shape=(1 << 10, 1 << 10, 1 << 8))) == 0 and _check(_grids(), n_links=64) == 0
    assert _check(_grids(**grid_kw), **call_kw) != 0
    msg = lib.gq_last_error()
    assert b"clutter" in msg and word in msg, msg


def test_check_refuses_a_null_stack():
    lib = _C.lib()
    assert lib.gq_clutter_check(None, 4, 1, 14, 512) != 0
    assert b"clutter" in lib.gq_last_error() and b"grids" in lib.gq_last_error()
    assert lib.gq_clutter_compose_check(None, None, 0, None, 1.0) != 0
    assert b"clutter" in lib.gq_last_error() and b"out" in lib.gq_last_error()


def _compose_check(out=None, parts=(), base=None, far=0.02, n_parts=None):
    out = out or _grids()
    arr = (_C.SceneGrid * max(len(parts), 1))(*parts)
    return _C.lib().gq_clutter_compose_check(ctypes.byref(out), ctypes.cast(arr, ctypes.c_void_p) if parts else None,
                                             len(parts) if n_parts is None else n_parts, ctypes.byref(base) if base is not None else None, far)


def test_compose_check_refusals_and_limits():
    lib = _C.lib()
    ok = _grid()
    assert _compose_check(parts=[ok]) == 0 and _compose_check(base=ok) == 0 and _compose_check(parts=[ok] * 32, base=ok) == 0
    assert _compose_check(parts=[ok], far=-3.0) == 0

    def refused(*words, **kw):
        assert _compose_check(**kw) != 0
        msg = lib.gq_last_error()
        assert b"clutter" in msg and all(w in msg for w in words), msg

    refused(b"n_parts", parts=[ok] * 33)
    refused(b"n_parts", n_parts=-1)
    refused(b"base", parts=[])  # nothing to compose
    refused(b"parts", n_parts=2)  # a NULL array
    for far in (float("nan"), float("inf"), float("-inf")):
        refused(b"far", parts=[ok], far=far)
    for kw, word in GRID_BAD:
        refused(b"out", word, out=_grids(**kw), parts=[ok])
        refused(b"base", word, parts=[ok], base=_grid(**kw))
        refused(b"parts[2]", word, parts=[ok, ok, _grid(**kw), ok])
    refused(b"n_grids", out=_grids(n_grids=0), parts=[ok])
    refused(b"n_grids", out=_grids(n_grids=65537), parts=[ok])
    # the launch's own limit: n_grids x tiles of 4 x 4 x 16 nodes
    assert _compose_check(out=_grids(n_grids=128, shape=(256, 256, 256)), parts=[ok]) == 0  # 128 x 64 x 64 x 16 = 2^23 tiles
    refused(b"tiles", out=_grids(n_grids=129, shape=(256, 256, 256)), parts=[ok])


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    for name in ("scene_distance_set", "scene_terms_set", "scene_terms_set_backward", "approach_terms_set", "approach_terms_set_backward",
                 "scene_compose"):
        assert hasattr(ns, name), name
    # the schemas of the existing ops did not change: the stack is new ops, not a new argument
    twins = {"scene_distance": "scene_distance_set", "scene_terms": "scene_terms_set", "scene_terms_backward": "scene_terms_set_backward",
             "approach_terms": "approach_terms_set", "approach_terms_backward": "approach_terms_set_backward"}
    for name, twin in twins.items():  # (values, origin, voxel) in the same places
        a, b = getattr(ns, name).default._schema, getattr(ns, twin).default._schema
        assert [(x.name, str(x.type)) for x in a.arguments] == [(x.name, str(x.type)) for x in b.arguments], name
    B, L, Ns, D, G = 6, 14, 70, 25, 3
    origin, axis = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, LT, v = e(B, D), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(B, L, 3, 4), e(G, 4, 5, 6)
        phi, grad, inside = ns.scene_distance_set(e(B, Ns, 3), v, origin, 0.1)
        assert phi.shape == (B, Ns) and grad.shape == (B, Ns, 3) and inside.shape == (B, Ns) and inside.dtype == torch.uint8
        assert ns.scene_terms_set(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, 0.01).shape == (B,)
        wrench, gRt = ns.scene_terms_set_backward(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, 0.01, e(B))
        assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12)
        assert ns.approach_terms_set(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, 0.1, 4, 0.01).shape == (B,)
        wrench, gRt = ns.approach_terms_set_backward(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, 0.1, 4, 0.01, e(B))
        assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12)
        assert ns.scene_compose(v, origin, 0.1, e(G, 12), [e(3, 3, 3), e(2, 2, 2)], origin * 2, [0.1, 0.2], e(2, 12),
                                e(G, dtype=torch.int32), None, origin, 0.0, 0.02) is None
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.scene_distance_set(z(B, 7, 3), z(G, 2, 2, 2), origin, 0.1)
    with pytest.raises(NotImplementedError):
        ns.scene_terms_set(z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(G, 2, 2, 2), origin, 0.1, 0.0)
    with pytest.raises(NotImplementedError):
        ns.scene_compose(z(G, 2, 2, 2), origin, 0.1, z(G, 12), [z(2, 2, 2)], origin, [0.1], z(1, 12), None, None, origin, 0.0, 0.02)


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    with pytest.raises(RuntimeError, match="CUDA"):
        ops.scene_distance(torch.zeros(6, 7, 3), None)


def test_new_kernel_resources():
    """The four new kernels, and only those: no scratch, no spills, and the VGPR figures DESIGN 16 states -- the two row kernels at
    their single-grid siblings' 64 / 72 (the grid's index arithmetic is scalar), the query at 24, the compose at 26."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "clutter" in k}
    want = {"gq_clutter_kernel": 64, "gq_clutter_corridor_kernel": 72, "gq_clutter_query_kernel": 24, "gq_clutter_compose_kernel": 26}
    assert sorted(new) == sorted(want), sorted(new)
    for name, r in new.items():
        assert not any(w in name for w in ("scene", "approach", "tabletop", "cloud")), name
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] == want[name], (name, r)
    # the row kernels sit in their siblings' occupancy steps, with the siblings' LDS
    for a, b in (("gq_clutter_kernel", "gq_scene_kernel"), ("gq_clutter_corridor_kernel", "gq_approach_kernel")):
        assert (res[a]["vgpr"], res[a]["agpr"], res[a]["lds_static"]) == (res[b]["vgpr"], res[b]["agpr"], res[b]["lds_static"]), (a, b)


# -------------------------------------------------------------------------------------------------------------------
# the fp64 oracle's own self-checks
# -------------------------------------------------------------------------------------------------------------------
def test_oracle_one_part_identity_poses_is_phi_at_the_nodes():
    out = co.Out(2, (5, 4, 6), (-0.02, -0.015, -0.03), 0.01)
    part = so.random_field((6, 5, 7), (-0.031, -0.026, -0.035), 0.0125, 9)
    phi, info = co.compose(out, co.identity(2), [part], co.identity(1), None, None, far=1e30)
    want = so.phi(part, out.nodes())
    assert torch.isfinite(want).all() and info["inside"] == 1.0  # the part covers the output box
    assert torch.equal(phi[0], want) and torch.equal(phi[1], want)
    # a translated target sees the part moved the other way
    T = co.identity(1)
    T[0, :, 3] = torch.tensor([0.005, -0.0025, 0.0075])
    moved, _ = co.compose(co.Out(1, out.shape, out.origin, out.voxel), T, [part], co.identity(1), None, None, far=1e30)
    assert torch.equal(moved[0], so.phi(part, out.nodes() + T[0, :, 3].double()))


def test_oracle_exclude_removes_exactly_that_part():
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "random")
    full, _ = co.compose(out, tT, parts, pT, None, base, co.FAR)
    got, _ = co.compose(out, tT, parts, pT, ex, base, co.FAR)
    assert list(ex) == [0, -1, 2]
    for g, p in enumerate(int(e) for e in ex):
        one = co.Out(1, out.shape, out.origin, out.voxel)
        keep = [q for q in range(len(parts)) if q != p]
        want, _ = co.compose(one, tT[g:g + 1], [parts[q] for q in keep], pT[keep], None, base, co.FAR)
        assert torch.equal(got[g], want[0]), g
        if p >= 0:
            assert not torch.equal(got[g], full[g]), g  # the part was seen before it was left out
        else:
            assert torch.equal(got[g], full[g])
    assert (got >= full).all()


def test_oracle_nan_and_far():
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "affine")
    T = tT.clone()
    T[1, 2, 3] = float("nan")
    phi, _ = co.compose(out, T, parts, pT, ex, base, co.FAR)
    assert torch.isnan(phi[1]).all() and torch.isfinite(phi[0]).all() and torch.isfinite(phi[2]).all()
    assert float(phi[0].max()) <= co.FAR and float(phi[0].min()) < 0.0
    ref = np.asarray(co.compose(out, tT, parts, pT, ex, base, co.FAR)[0])
    assert np.array_equal(ref[0], phi[0].numpy()) and np.array_equal(ref[2], phi[2].numpy())
