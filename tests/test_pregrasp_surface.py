"""CPU-side checks of the pre-grasp term (E_pregrasp: the OPENED hand along the approach corridor, d = 0 included): C ABI, the
host-only argument check, registered ops, weight validation, the code-object metadata of the new kernel, and a self-check of the
oracle the GPU tests use.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ref_cpu  # noqa: F401

import _approach_oracle as ao
import _pregrasp_oracle as po
import _scene_oracle as so
from graspqp_amd import _C
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
VGPR_STEP = 80  # the registers gq_pregrasp_kernel was built at (6 wavefronts per SIMD)
G_SHAPE, G_ORIGIN, G_H = (100, 96, 104), (-0.5, -0.48, -0.52), 0.01


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_pregrasp_check", 9), ("gq_pregrasp_terms", 23)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    assert protos["gq_pregrasp_check"][1][2] is ctypes.c_int64  # rows_per_grid
    assert protos["gq_pregrasp_terms"][1][2] is ctypes.c_int64
    # the entries the term stands on are what they were
    for name, n_args in (("gq_scene_check", 4), ("gq_scene_total", 5), ("gq_approach_check", 7), ("gq_approach_terms", 21),
                         ("gq_clutter_check", 5), ("gq_clutter_corridor_terms", 22), ("gq_fk_backward", 20)):
        assert len(protos[name][1]) == n_args, name


def _grids(shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000, n_grids=1):
    g = _C.ClutterGrids()
    g.values = values  # never dereferenced: the check is host only
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(g, batch=4, rows_per_grid=4, n_links=14, n_samples=512, distance=0.1, n_stations=4, axis=(0.0, 0.0, 1.0), opening=0.5):
    ax = None if axis is None else ctypes.cast((ctypes.c_float * 3)(*axis), ctypes.c_void_p)
    return _C.lib().gq_pregrasp_check(ctypes.byref(g), batch, rows_per_grid, n_links, n_samples, distance, n_stations, ax, opening)


NAN, INF = float("nan"), float("inf")
BAD = [
    # everything gq_clutter_check refuses: the grid ...
    (dict(shape=(1, 2, 2)), {}, b"nx"), (dict(shape=(2, 1, 2)), {}, b"ny"), (dict(shape=(2, 2, 1)), {}, b"nz"),
    (dict(shape=(1 << 10, 1 << 10, (1 << 8) + 1)), {}, b"nx*ny*nz"), (dict(voxel=0.0), {}, b"voxel"), (dict(voxel=NAN), {}, b"voxel"),
    (dict(origin=(0.0, NAN, 0.0)), {}, b"origin"), (dict(values=None), {}, b"values"),
    (dict(n_grids=0), {}, b"n_grids"), (dict(n_grids=65537), dict(batch=65537, rows_per_grid=1), b"n_grids"),
    # ... and the launch
    ({}, dict(batch=0, rows_per_grid=1), b"batch"), ({}, dict(n_links=0), b"n_links"), ({}, dict(n_links=65), b"n_links"),
    ({}, dict(n_samples=0), b"n_samples"), ({}, dict(rows_per_grid=0), b"rows_per_grid"), ({}, dict(rows_per_grid=-1), b"rows_per_grid"),
    ({}, dict(rows_per_grid=1 << 31), b"rows_per_grid"), ({}, dict(rows_per_grid=3), b"batch"),
    (dict(n_grids=3), dict(batch=4, rows_per_grid=2), b"batch"),
    # everything gq_approach_check refuses, but for n_stations = 0
    ({}, dict(distance=0.0), b"distance"), ({}, dict(distance=-0.1), b"distance"), ({}, dict(distance=NAN), b"distance"),
    ({}, dict(distance=INF), b"distance"),
    ({}, dict(n_stations=33), b"n_stations"), ({}, dict(n_stations=-1), b"n_stations"),
    ({}, dict(axis=None), b"grasp_axis"), ({}, dict(axis=(0.0, 0.0, 0.0)), b"grasp_axis"), ({}, dict(axis=(0.0, NAN, 1.0)), b"grasp_axis"),
    ({}, dict(axis=(INF, 0.0, 0.0)), b"grasp_axis"),
    # the opening
    ({}, dict(opening=-0.01), b"opening"), ({}, dict(opening=1.01), b"opening"), ({}, dict(opening=NAN), b"opening"),
    ({}, dict(opening=INF), b"opening"),
]


@pytest.mark.parametrize("grid_kw,call_kw,word", BAD)
def test_check_refuses_with_a_message_that_names_the_argument(grid_kw, call_kw, word):
    lib = _C.lib()
    assert _check(_grids()) == 0
    assert _check(_grids(), n_stations=0) == 0 and _check(_grids(), n_stations=32) == 0  # the limits
    assert _check(_grids(), opening=0.0) == 0 and _check(_grids(), opening=1.0) == 0
    assert _check(_grids(), n_links=64) == 0
    assert _check(_grids(n_grids=3), batch=6, rows_per_grid=2) == 0
    assert _check(_grids(), axis=(0.0, -2.0, 0.0)) == 0  # used as given: not normalised, not refused
    assert _check(_grids(**grid_kw), **call_kw) != 0
    msg = lib.gq_last_error()
    assert b"pregrasp" in msg and word in msg, msg


def test_check_refuses_a_null_stack():
    ax = ctypes.cast((ctypes.c_float * 3)(0.0, 0.0, 1.0), ctypes.c_void_p)
    assert _C.lib().gq_pregrasp_check(None, 4, 4, 14, 512, 0.1, 4, ax, 0.5) != 0
    assert b"pregrasp" in _C.lib().gq_last_error() and b"grids" in _C.lib().gq_last_error()


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    for name in ("pregrasp_terms", "pregrasp_terms_backward"):
        assert hasattr(ns, name), name
    assert callable(ops.pregrasp_terms) and callable(ops.pregrasp_check) and callable(ops.default_open_joints)
    B, L, Ns, J = 6, 14, 70, 16
    origin, axis = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, q = e(B, 9 + J), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(J)
        for v in (e(4, 5, 6), e(3, 4, 5, 6)):  # one grid, a stack of three
            ep = ns.pregrasp_terms(hp, pts, lnk, 1, Rg, v, origin, 0.1, axis, 0.08, 4, 0.5, q, 0.01)
            assert ep.shape == (B,)
            g_theta, gRt = ns.pregrasp_terms_backward(hp, pts, lnk, 1, Rg, v, origin, 0.1, axis, 0.08, 4, 0.5, q, 0.01, e(B))
            assert g_theta.shape == (B, J) and gRt.shape == (B, 12)
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.pregrasp_terms(z(B, 9 + J), z(Ns, 3), z(Ns, dtype=torch.int32), 1, z(B, 3, 3), z(2, 2, 2), origin, 0.1, axis, 0.08, 4, 0.5,
                          z(J), 0.0)
    with pytest.raises(NotImplementedError):
        ns.pregrasp_terms_backward(z(B, 9 + J), z(Ns, 3), z(Ns, dtype=torch.int32), 1, z(B, 3, 3), z(2, 2, 2), origin, 0.1, axis, 0.08,
                                   4, 0.5, z(J), 0.0, z(B))


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    B, L = 2, 14
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.pregrasp_terms(torch.zeros(B, 25), None, None, torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 3, 3),
                           torch.zeros(B, L, 3, 4), torch.zeros(8, dtype=torch.uint8), None, (0.0, 0.0, 1.0), 0.1, 4, 0.5)


def test_default_open_joints_is_the_clamped_default_state():
    from graspqp_amd import ops

    for name in ("allegro", "shadow_hand", "panda"):
        spec = get_hand_spec(name)
        q = ops.default_open_joints(spec, "cpu").numpy()
        assert q.dtype == np.float32 and q.shape == (spec.n_dofs,)
        lo, hi = np.asarray(spec.joints_lower, np.float32), np.asarray(spec.joints_upper, np.float32)
        assert (q >= lo).all() and (q <= hi).all()
        np.testing.assert_array_equal(q, np.clip(np.asarray(spec.default_state, np.float32), lo, hi))


def test_merge_weights_knows_the_pregrasp_term():
    from graspqp_amd.stepper import (APPROACH_TERMS, DEFAULT_WEIGHTS, PREGRASP_TERMS, SCENE_TERMS, TABLETOP_TERMS, TERM_NAMES,
                                     merge_weights)

    assert PREGRASP_TERMS == ("E_pregrasp",) and APPROACH_TERMS == ("E_approach",) and SCENE_TERMS == ("E_scene",)
    assert len(TERM_NAMES) == 5
    assert DEFAULT_WEIGHTS == {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}
    w = merge_weights(None)
    assert w["E_pregrasp"] == 0.0 and w["E_approach"] == 0.0 and w["E_scene"] == 0.0
    assert list(w)[-1] == "E_pregrasp"
    assert merge_weights({"E_pregrasp": 2.5})["E_pregrasp"] == 2.5
    with pytest.raises(ValueError, match="E_pregrasp"):
        merge_weights({"E_pregrasp": -1.0})
    with pytest.raises(ValueError, match="E_pregrasp"):
        merge_weights({"E_pregrasp": float("nan")})
    assert {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS and all(w[k] == 0.0 for k in TABLETOP_TERMS)
    for bad in ("e_pregrasp", "pregrasp", "E_open"):
        with pytest.raises(ValueError, match=bad):
            merge_weights({bad: 1.0})


def test_stepper_signature_has_the_pregrasp_arguments():
    import inspect

    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.stepper import GraspStepper

    p = inspect.signature(GraspStepper.__init__).parameters
    assert p["pregrasp_opening"].default == 0.5
    for k in ("pregrasp_joints", "pregrasp_scene", "pregrasp_distance", "pregrasp_stations", "pregrasp_margin"):
        assert p[k].default is None, k
    p = inspect.signature(HandModel.set_pregrasp).parameters
    assert list(p)[1:] == ["distance", "stations", "opening", "open_joints", "margin", "scene"] and p["opening"].default == 0.5


def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills, within the register step DESIGN 21 states; every other kernel keeps its name."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "pregrasp" in k}
    assert sorted(new) == ["gq_pregrasp_kernel"], sorted(new)
    r = new["gq_pregrasp_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["vgpr"] + r["agpr"] <= VGPR_STEP, r
    assert r["lds_static"] <= 24 * 1024, r


# ---------------------------------------------------------------------------------------------------------------
# the oracle itself
# ---------------------------------------------------------------------------------------------------------------
def _case(Ns=64, B=3, seed=4):
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    pick = np.random.default_rng(Ns).permutation(512)[:Ns]
    pts, lnk = pts[pick], lnk[pick]
    F = so.multilinear(G_SHAPE, G_ORIGIN, G_H)
    gen = torch.Generator().manual_seed(seed)
    hp = torch.cat([0.1 * torch.randn(B, 3, generator=gen), torch.randn(B, 6, generator=gen),
                    torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)], 1).double()
    q = np.clip(np.asarray(spec.default_state, np.float64), spec.joints_lower, spec.joints_upper)
    return spec, pts, lnk, F, hp, q


def test_oracle_opening_zero_is_scene_plus_approach():
    """fp64: with alpha = 0 the opened hand is the hand, so E_pregrasp = (E_scene + K E_approach) / (K + 1), value and gradient."""
    spec, pts, lnk, F, hp, q = _case()
    D, K, margin = 0.08, 3, 0.01
    res = po.e_pregrasp(spec, pts, lnk, hp, q, 0.0, F, margin, D, K)
    sc = so.e_scene(spec, pts, lnk, hp, F, margin)
    ap = ao.e_approach(spec, pts, lnk, hp, F, margin, D, K)
    assert res["phi"].shape == (3, K + 1, 64) and res["active"].sum() >= 5 and res["active"].any(axis=(0, 2)).all()
    assert np.array_equal(res["active"][:, 0], sc["active"]) and np.array_equal(res["active"][:, 1:], ap["active"])
    np.testing.assert_allclose(res["E"], (sc["E"] + K * ap["E"]) / (K + 1), rtol=1e-12, atol=1e-12)
    want = (sc["grad"] + K * ap["grad"]) / (K + 1)
    assert np.abs(want[:, 9:]).max() > 0
    np.testing.assert_allclose(res["grad"], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_oracle_opening_one_has_no_joint_gradient():
    spec, pts, lnk, F, hp, q = _case()
    res = po.e_pregrasp(spec, pts, lnk, hp, q, 1.0, F, 0.01, 0.08, 3)
    assert res["active"].sum() >= 5 and np.abs(res["grad"][:, :9]).max() > 0
    assert (res["grad"][:, 9:] == 0).all()
    # the energy no longer depends on the joints at all
    hp2 = hp.clone()
    hp2[:, 9:] += 0.2
    np.testing.assert_array_equal(po.e_pregrasp(spec, pts, lnk, hp2, q, 1.0, F, 0.01, 0.08, 3)["E"], res["E"])


def test_oracle_no_station_is_the_scene_oracle_at_the_opened_pose():
    """K = 0: the one station d = 0, E_scene at the opened pose; the joint columns carry the chain-rule factor 1 - alpha."""
    spec, pts, lnk, F, hp, q = _case()
    alpha, margin = 0.25, 0.01
    res = po.e_pregrasp(spec, pts, lnk, hp, q, alpha, F, margin, 0.08, 0)
    assert res["phi"].shape == (3, 1, 64)
    ref = so.e_scene(spec, pts, lnk, po.opened_pose(hp, q, alpha), F, margin)
    assert ref["active"].sum() >= 5
    np.testing.assert_allclose(res["E"], ref["E"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(res["x"][:, 0], ref["x"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(res["grad"][:, :9], ref["grad"][:, :9], rtol=1e-12, atol=1e-12 * np.abs(ref["grad"]).max())
    np.testing.assert_allclose(res["grad"][:, 9:], (1 - alpha) * ref["grad"][:, 9:], rtol=1e-12, atol=1e-12 * np.abs(ref["grad"]).max())


def test_oracle_gradient_is_the_central_difference():
    """The rot6d and joint parts of the oracle's gradient against a central difference of the oracle's own energy, on one row."""
    spec, pts, lnk, F, hp, q = _case()
    alpha, margin, D, K = 0.5, 0.01, 0.08, 3
    res = po.e_pregrasp(spec, pts, lnk, hp, q, alpha, F, margin, D, K)
    row, h = 1, 1e-6
    assert np.abs(res["grad"][row, 9:]).max() > 0
    for j in range(3, hp.shape[1]):
        hp_p, hp_m = hp.clone(), hp.clone()
        hp_p[row, j] += h
        hp_m[row, j] -= h
        fd = 3.0 * (po.e_pregrasp(spec, pts, lnk, hp_p, q, alpha, F, margin, D, K)["E"][row] -
                    po.e_pregrasp(spec, pts, lnk, hp_m, q, alpha, F, margin, D, K)["E"][row]) / (2 * h)
        assert abs(fd - res["grad"][row, j]) <= 1e-6 * max(1.0, np.abs(res["grad"][row]).max()), (j, fd, res["grad"][row, j])


def test_oracle_stations_start_at_the_grasp_pose():
    """d_k = D k / K for k = 0..K: station 0 is the opened hand where it stands."""
    spec, pts, lnk, F, hp, q = _case(Ns=32, B=2, seed=9)
    D, K = 0.09, 3
    res = po.e_pregrasp(spec, pts, lnk, hp, q, 0.5, F, 0.01, D, K)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(po.opened_pose(hp, q, 0.5), torch.zeros(2, 1, dtype=torch.long))
    x0 = oh.get_surface_points().numpy()
    back = (oh.global_rotation @ oh.grasp_axis).numpy()
    for k in range(K + 1):
        np.testing.assert_allclose(res["x"][:, k], x0 - (D * k / K) * back[:, None], rtol=0, atol=1e-15)
