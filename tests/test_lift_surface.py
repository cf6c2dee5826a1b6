"""CPU-side checks of the lift term (E_lift: the hand and the held object on the way out): C ABI, the host-only argument check,
registered ops, weight and gate validation, and the code-object metadata of the new kernel.  Nothing here needs a GPU."""
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
    for name, n_args in (("gq_lift_check", 15), ("gq_lift_terms", 30)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    # the entries the term stands on are what they were
    for name, n_args in (("gq_clutter_check", 5), ("gq_clutter_corridor_terms", 22), ("gq_scene_total", 5), ("gq_approach_terms", 21)):
        assert len(protos[name][1]) == n_args, name
    # the stack crosses as the gqClutterGrids the clutter entries take: no new struct
    assert [f[0] for f in _C.ClutterGrids._fields_] == ["values", "n_grids", "nx", "ny", "nz", "origin", "voxel"]


def _grids(n_grids=2, shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.ClutterGrids()
    g.values = values  # never dereferenced: the check is host only
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(g, batch=4, rows_per_grid=2, n_links=14, n_samples=512, n_obj=2, batch_each=2, M=100, height=0.05, retreat=0.02, n_stations=4,
           axis=(0.0, 0.0, 1.0), direction=(0.0, 0.6, 0.8), margin=0.01, object_margin=-0.005):
    vec = lambda v: None if v is None else ctypes.cast((ctypes.c_float * 3)(*v), ctypes.c_void_p)
    return _C.lib().gq_lift_check(None if g is None else ctypes.byref(g), batch, rows_per_grid, n_links, n_samples, n_obj, batch_each, M,
                                  height, retreat, n_stations, vec(axis), vec(direction), margin, object_margin)


NAN, INF = float("nan"), float("inf")
BAD = [
    # the stack and the launch's shapes: everything gq_clutter_check refuses
    (dict(shape=(1, 2, 2)), {}, b"nx"), (dict(shape=(2, 2, 1)), {}, b"nz"), (dict(voxel=0.0), {}, b"voxel"),
    (dict(origin=(0.0, NAN, 0.0)), {}, b"origin"), (dict(values=None), {}, b"values"), (dict(n_grids=0), {}, b"n_grids"),
    (dict(n_grids=3), {}, b"rows_per_grid"),
    ({}, dict(batch=0), b"batch"), ({}, dict(rows_per_grid=0), b"rows_per_grid"), ({}, dict(rows_per_grid=4), b"rows_per_grid"),
    ({}, dict(n_links=0), b"n_links"), ({}, dict(n_links=65), b"n_links"), ({}, dict(n_samples=0), b"n_samples"),
    # the objects
    ({}, dict(n_obj=3), b"batch_each"), ({}, dict(n_obj=0, batch_each=0), b"batch_each"), ({}, dict(batch_each=4), b"n_obj"),
    ({}, dict(n_obj=1 << 62, batch_each=4), b"n_obj"),  # n_obj * batch_each would overflow: the check divides
    ({}, dict(M=-1), b"n_object_points"), ({}, dict(M=(1 << 24) + 1), b"n_object_points"),
    # the carry
    ({}, dict(height=-0.01), b"height"), ({}, dict(height=NAN), b"height"), ({}, dict(height=INF), b"height"),
    ({}, dict(retreat=-0.01), b"retreat"), ({}, dict(retreat=NAN), b"retreat"), ({}, dict(retreat=INF), b"retreat"),
    ({}, dict(height=0.0, retreat=0.0), b"height + retreat"),
    ({}, dict(n_stations=0), b"n_stations"), ({}, dict(n_stations=33), b"n_stations"), ({}, dict(n_stations=-1), b"n_stations"),
    ({}, dict(axis=None), b"grasp_axis"), ({}, dict(axis=(0.0, 0.0, 0.0)), b"grasp_axis"), ({}, dict(axis=(0.0, NAN, 1.0)), b"grasp_axis"),
    ({}, dict(direction=None), b"direction"), ({}, dict(direction=(0.0, 0.0, 0.0)), b"direction"),
    ({}, dict(direction=(INF, 0.0, 0.0)), b"direction"),
    ({}, dict(margin=-0.01), b"margin"), ({}, dict(margin=NAN), b"margin"), ({}, dict(margin=INF), b"margin"),
    ({}, dict(object_margin=NAN), b"object_margin"), ({}, dict(object_margin=-INF), b"object_margin"),
]


@pytest.mark.parametrize("grid_kw,call_kw,word", BAD)
def test_check_refuses_with_a_message_that_names_the_argument(grid_kw, call_kw, word):
    lib = _C.lib()
    assert _check(_grids()) == 0
    assert _check(_grids(), n_stations=1) == 0 and _check(_grids(), n_stations=32) == 0 and _check(_grids(), n_links=64) == 0  # the limits
    assert _check(_grids(), M=0) == 0 and _check(_grids(), height=0.0) == 0 and _check(_grids(), retreat=0.0) == 0
    assert _check(_grids(), object_margin=-1.0) == 0 and _check(_grids(), margin=0.0) == 0
    assert _check(_grids(), direction=(0.0, -2.0, 0.0)) == 0  # used as given: not normalised, not refused
    assert _check(_grids(n_grids=1), rows_per_grid=4) == 0 and _check(_grids(), n_obj=4, batch_each=1) == 0
    assert _check(_grids(**grid_kw), **call_kw) != 0
    msg = lib.gq_last_error()
    assert b"lift" in msg and word in msg, msg


def test_check_takes_a_null_stack_for_the_parameters_alone():
    assert _check(None) == 0
    assert _check(None, rows_per_grid=1) == 0  # nothing to hold it against
    assert _check(None, n_stations=0) != 0 and b"lift: n_stations" in _C.lib().gq_last_error()
    assert _check(None, n_links=65) != 0 and b"n_links" in _C.lib().gq_last_error()


def test_ops_check_raises_value_errors():
    from graspqp_amd import ops

    ops.lift_check()
    ops.lift_check(None, 6, 14, 512, 3, 2, 100, 0.0, 0.1, 32, (0, 0, 1), (0, 0.6, 0.8), 0.01, -0.01)
    for kw, word in ((dict(height=0.0), "height"), (dict(stations=2.5), "n_stations"), (dict(direction=(0, 0, 0)), "direction"),
                     (dict(batch=4, n_obj=3, batch_each=2), "batch_each"), (dict(scene=object()), "scene")):
        with pytest.raises(ValueError, match=word):
            ops.lift_check(**kw)
    assert ops.lift_direction((0, 3, 4)) == [0.0, 0.6, 0.8]
    for bad in ((0, 0, 0), (0, float("nan"), 1), (1, 2)):
        with pytest.raises(ValueError, match="direction"):
            ops.lift_direction(bad)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    for name in ("lift_terms", "lift_terms_backward"):
        assert hasattr(ns, name), name
    B, L, Ns, D, M = 6, 14, 70, 25, 33
    origin, axis, u = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.6, 0.8]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, LT = e(B, D), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(B, L, 3, 4)
        for v in (e(4, 5, 6), e(3, 4, 5, 6)):  # one grid, or a stack
            el, eo = ns.lift_terms(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, u, 0.05, 0.02, 4, e(3, M, 3), 2, 0.01, -0.01)
            assert el.shape == (B,) and eo.shape == (B,)
            wrench, gRt = ns.lift_terms_backward(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, u, 0.05, 0.02, 4, e(3, M, 3), 2, 0.01,
                                                 -0.01, e(B))
            assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12)
    z = torch.zeros
    args = (z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(2, 2, 2), origin, 0.1, axis, u, 0.05, 0.02, 4,
            z(3, M, 3), 2, 0.0, 0.0)
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.lift_terms(*args)
    with pytest.raises(NotImplementedError):
        ns.lift_terms_backward(*args, z(B))


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    with pytest.raises(RuntimeError, match="CUDA"):
        ops.lift_terms(torch.zeros(2, 25), None, None, torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 3, 3), torch.zeros(2, 14, 3, 4),
                       torch.zeros(8, dtype=torch.uint8), None, (0.0, 0.0, 1.0), 0.05, 0.0, 4, None, 2)


def test_merge_weights_and_the_gates_know_the_lift_term():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, LIFT_TERMS, TERM_NAMES, TRACK_TERMS, merge_weights, select_tolerances

    assert LIFT_TERMS == ("E_lift",) and TRACK_TERMS == ("E_track",) and len(TERM_NAMES) == 5
    w = merge_weights(None)
    assert w["E_lift"] == 0.0 and "E_lift" not in DEFAULT_WEIGHTS  # no default weight
    assert {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS
    assert merge_weights({"E_lift": 2.5})["E_lift"] == 2.5
    with pytest.raises(ValueError, match="E_lift"):
        merge_weights({"E_lift": -1.0})
    for bad in ("e_lift", "lift", "E_carry"):
        with pytest.raises(ValueError, match=bad):
            merge_weights({bad: 1.0})
    names = TERM_NAMES + ("E_scene", "E_track", "E_lift")
    inf = float("inf")
    assert select_tolerances(names) == [inf] * 5 + [0.0, inf, 0.0]  # gated at 0 by default when it is on
    assert select_tolerances(names, {"E_lift": 1e-3}) == [inf] * 7 + [1e-3]
    with pytest.raises(ValueError, match="E_lift"):
        select_tolerances(TERM_NAMES, {"E_lift": 0.0})  # switched off


def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills; the row launches it was modelled on are still there."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "lift" in k}
    assert sorted(new) == ["gq_lift_kernel"], sorted(new)
    r = new["gq_lift_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["max_threads"] == 512
    assert "gq_approach_kernel" in res and "gq_clutter_corridor_kernel" in res
