"""CPU-side checks of the approach term (E_approach: the scene grid along the hand's approach corridor): C ABI, the host-only
argument check, registered ops, weight validation, the code-object metadata of the new kernel, and a self-check of the oracle
the GPU tests use.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import ref_cpu  # noqa: F401

import _approach_oracle as ao
import _scene_oracle as so
from graspqp_amd import _C
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
VGPR_STEP = 72  # the registers gq_approach_kernel was built at (7 wavefronts per SIMD); 64 would spill


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_approach_check", 7), ("gq_approach_terms", 21)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    # the scene entries the term stands on are what they were
    for name, n_args in (("gq_scene_check", 4), ("gq_scene_terms", 18), ("gq_scene_query", 7), ("gq_scene_total", 5)):
        assert len(protos[name][1]) == n_args, name


def _grid(shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.SceneGrid()
    g.values = values  # never dereferenced: the check is host only
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(g, batch=4, n_links=14, n_samples=512, distance=0.1, n_stations=4, axis=(0.0, 0.0, 1.0)):
    ax = None if axis is None else ctypes.cast((ctypes.c_float * 3)(*axis), ctypes.c_void_p)
    return _C.lib().gq_approach_check(ctypes.byref(g), batch, n_links, n_samples, distance, n_stations, ax)


NAN, INF = float("nan"), float("inf")
BAD = [
    # everything gq_scene_check refuses
    (dict(shape=(1, 2, 2)), {}, b"nx"), (dict(shape=(2, 1, 2)), {}, b"ny"), (dict(shape=(2, 2, 1)), {}, b"nz"),
    (dict(shape=(1 << 10, 1 << 10, (1 << 8) + 1)), {}, b"nx*ny*nz"), (dict(voxel=0.0), {}, b"voxel"), (dict(voxel=NAN), {}, b"voxel"),
    (dict(origin=(0.0, NAN, 0.0)), {}, b"origin"), (dict(values=None), {}, b"values"),
    ({}, dict(batch=0), b"batch"), ({}, dict(n_links=0), b"n_links"), ({}, dict(n_links=65), b"n_links"),
    ({}, dict(n_samples=0), b"n_samples"),
    # the corridor
    ({}, dict(distance=0.0), b"distance"), ({}, dict(distance=-0.1), b"distance"), ({}, dict(distance=NAN), b"distance"),
    ({}, dict(distance=INF), b"distance"),
    ({}, dict(n_stations=0), b"n_stations"), ({}, dict(n_stations=33), b"n_stations"), ({}, dict(n_stations=-1), b"n_stations"),
    ({}, dict(axis=None), b"grasp_axis"), ({}, dict(axis=(0.0, 0.0, 0.0)), b"grasp_axis"), ({}, dict(axis=(0.0, NAN, 1.0)), b"grasp_axis"),
    ({}, dict(axis=(INF, 0.0, 0.0)), b"grasp_axis"),
]


@pytest.mark.parametrize("grid_kw,call_kw,word", BAD)
def test_check_refuses_with_a_message_that_names_the_argument(grid_kw, call_kw, word):
    lib = _C.lib()
    assert _check(_grid()) == 0
    assert _check(_grid(), n_stations=1) == 0 and _check(_grid(), n_stations=32) == 0  # the limits
    assert _check(_grid(), n_links=64) == 0
    assert _check(_grid(), axis=(0.0, -2.0, 0.0)) == 0  # used as given: not normalised, not refused
    assert _check(_grid(**grid_kw), **call_kw) != 0
    msg = lib.gq_last_error()
    assert b"approach" in msg and word in msg, msg


def test_check_refuses_a_null_grid():
    ax = ctypes.cast((ctypes.c_float * 3)(0.0, 0.0, 1.0), ctypes.c_void_p)
    assert _C.lib().gq_approach_check(None, 4, 14, 512, 0.1, 4, ax) != 0
    assert b"approach" in _C.lib().gq_last_error() and b"grid" in _C.lib().gq_last_error()


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    for name in ("approach_terms", "approach_terms_backward"):
        assert hasattr(ns, name), name
    B, L, Ns, D = 5, 14, 70, 25
    origin, axis = [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, LT, v = e(B, D), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(B, L, 3, 4), e(4, 5, 6)
        ea = ns.approach_terms(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, 0.08, 4, 0.01)
        assert ea.shape == (B,)
        wrench, gRt = ns.approach_terms_backward(hp, pts, lnk, L, Rg, LT, v, origin, 0.1, axis, 0.08, 4, 0.01, e(B))
        assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12)
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.approach_terms(z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(2, 2, 2), origin, 0.1, axis,
                          0.08, 4, 0.0)
    with pytest.raises(NotImplementedError):
        ns.approach_terms_backward(z(B, D), z(Ns, 3), z(Ns, dtype=torch.int32), L, z(B, 3, 3), z(B, L, 3, 4), z(2, 2, 2), origin, 0.1,
                                   axis, 0.08, 4, 0.0, z(B))


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    B, L = 2, 14
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.approach_terms(torch.zeros(B, 25), None, None, torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 3, 3),
                           torch.zeros(B, L, 3, 4), torch.zeros(8, dtype=torch.uint8), None, (0.0, 0.0, 1.0), 0.1, 4)


def test_merge_weights_knows_the_approach_term():
    from graspqp_amd.stepper import APPROACH_TERMS, DEFAULT_WEIGHTS, SCENE_TERMS, TABLETOP_TERMS, TERM_NAMES, merge_weights

    assert APPROACH_TERMS == ("E_approach",) and SCENE_TERMS == ("E_scene",) and TABLETOP_TERMS == ("E_prior", "E_wall")
    assert len(TERM_NAMES) == 5
    assert DEFAULT_WEIGHTS == {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}
    w = merge_weights(None)
    assert w["E_approach"] == 0.0 and w["E_scene"] == 0.0
    assert merge_weights({"E_approach": 2.5})["E_approach"] == 2.5
    with pytest.raises(ValueError, match="E_approach"):
        merge_weights({"E_approach": -1.0})
    assert {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS and all(w[k] == 0.0 for k in TABLETOP_TERMS)
    for bad in ("e_approach", "approach", "E_corridor"):
        with pytest.raises(ValueError, match=bad):
            merge_weights({bad: 1.0})


def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills, within the register step DESIGN 15 states."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "approach" in k}
    assert sorted(new) == ["gq_approach_kernel"], sorted(new)
    for name, r in new.items():
        assert "scene" not in name and "tabletop" not in name and "cloud" not in name
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= VGPR_STEP, (name, r)


def test_oracle_with_one_station_is_the_scene_oracle_at_the_retreated_pose():
    """fp64: E_approach with K = 1 at (t, R, theta) is E_scene at (t - D R a, R, theta), to 1e-12 in value and in d/dt,
    d/dtheta.  The rot6d part differs by the derivative of the shift -D R a, so it is held to a central difference of the
    approach oracle itself, on one row."""
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    pick = np.random.default_rng(64).permutation(512)[:64]
    pts, lnk = pts[pick], lnk[pick]
    F = so.multilinear((100, 96, 104), (-0.5, -0.48, -0.52), 0.01)
    B, D, margin = 3, 0.08, 0.01
    gen = torch.Generator().manual_seed(4)
    hp = torch.cat([0.1 * torch.randn(B, 3, generator=gen), torch.randn(B, 6, generator=gen),
                    torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)], 1).double()
    res = ao.e_approach(spec, pts, lnk, hp, F, margin, D, 1)
    assert res["inside"].all() and res["active"].sum() >= 5 and res["phi"].shape == (B, 1, 64)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.clone(), torch.zeros(B, 1, dtype=torch.long))
    back = (oh.global_rotation @ oh.grasp_axis).detach()
    hp2 = hp.clone()
    hp2[:, :3] -= D * back
    ref = so.e_scene(spec, pts, lnk, hp2, F, margin)
    np.testing.assert_allclose(res["E"], ref["E"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(res["active"][:, 0], ref["active"])
    for cols in (slice(0, 3), slice(9, None)):
        a, b = res["grad"][:, cols], ref["grad"][:, cols]
        assert np.abs(a).max() > 0
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max())
    assert np.abs(res["grad"][:, 3:9] - ref["grad"][:, 3:9]).max() > 1e-6 * np.abs(ref["grad"][:, 3:9]).max()
    row, h = 1, 1e-6
    for j in range(3, 9):
        hp_p, hp_m = hp.clone(), hp.clone()
        hp_p[row, j] += h
        hp_m[row, j] -= h
        fd = 3.0 * (ao.e_approach(spec, pts, lnk, hp_p, F, margin, D, 1)["E"][row] -
                    ao.e_approach(spec, pts, lnk, hp_m, F, margin, D, 1)["E"][row]) / (2 * h)
        assert abs(fd - res["grad"][row, j]) <= 1e-6 * max(1.0, np.abs(res["grad"][row]).max()), (j, fd, res["grad"][row, j])


def test_oracle_stations_and_mean():
    """d_k = D k / K for k = 1..K (no station at 0), and E is the mean over the stations of the per-station hinge sums."""
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    pts, lnk = pts[:32], lnk[:32]
    F = so.affine((100, 96, 104), (-0.5, -0.48, -0.52), 0.01)
    gen = torch.Generator().manual_seed(9)
    hp = torch.cat([0.05 * torch.randn(2, 3, generator=gen), torch.randn(2, 6, generator=gen),
                    torch.tensor(spec.default_state)[None].repeat(2, 1)], 1).double()
    D, K, margin = 0.09, 3, 0.01
    res = ao.e_approach(spec, pts, lnk, hp, F, margin, D, K)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.clone(), torch.zeros(2, 1, dtype=torch.long))
    x0 = oh.get_surface_points().numpy()
    back = (oh.global_rotation @ oh.grasp_axis).numpy()
    for k in range(1, K + 1):
        np.testing.assert_allclose(res["x"][:, k - 1], x0 - (D * k / K) * back[:, None], rtol=0, atol=1e-15)
    per = [so.e_scene(spec, pts, lnk, torch.cat([hp[:, :3] - (D * k / K) * torch.tensor(back), hp[:, 3:]], 1), F, margin)["E"]
           for k in range(1, K + 1)]
    np.testing.assert_allclose(res["E"], sum(per) / K, rtol=1e-12, atol=1e-14)
