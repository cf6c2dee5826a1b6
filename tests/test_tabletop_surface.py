"""CPU-side checks of the tabletop terms (E_prior / E_wall in the stepper): C ABI, registered ops, weight validation, the
shared hand-surface sampler and the code-object metadata of the new kernel.  Nothing here needs a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name in ("gq_tabletop_check", "gq_tabletop_terms", "gq_tabletop_total"):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert len(protos["gq_tabletop_check"][1]) == 3
    assert len(protos["gq_tabletop_terms"][1]) == 22
    src = open(_C.HEADER_PATH).read()
    assert "core/energy.py:68-78" in src[src.index("tabletop terms"):src.index("gq_tabletop_check(")]


@pytest.mark.parametrize("args,word", [((0, 14, 512), b"batch"), ((-3, 14, 512), b"batch"), ((4, 0, 512), b"n_links"),
                                       ((4, -1, 512), b"n_links"), ((4, 14, 0), b"n_samples"), ((4, 14, -7), b"n_samples")])
def test_check_rejects_empty_shapes_with_a_message(args, word):
    lib = _C.lib()
    assert lib.gq_tabletop_check(4, 14, 512) == 0
    assert lib.gq_tabletop_check(*args) != 0
    msg = lib.gq_last_error()
    assert b"tabletop" in msg and word in msg, msg


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops  # noqa: F401

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "tabletop_terms") and hasattr(ns, "tabletop_terms_backward")
    B, L, Ns, D = 5, 14, 70, 25
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        hp, pts, lnk, Rg, LT = e(B, D), e(Ns, 3), e(Ns, dtype=torch.int32), e(B, 3, 3), e(B, L, 3, 4)
        e_prior, e_wall = ns.tabletop_terms(hp, pts, lnk, L, Rg, LT, [0.0, 0.0, 1.0], 0.0)
        assert e_prior.shape == (B,) and e_wall.shape == (B,)
        wrench, gRt, gR = ns.tabletop_terms_backward(hp, pts, lnk, L, Rg, LT, [0.0, 0.0, 1.0], 0.0, e(B), e(B))
        assert wrench.shape == (B, L, 6) and gRt.shape == (B, 12) and gR.shape == (B, 9)
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.tabletop_terms(torch.zeros(B, D), torch.zeros(Ns, 3), torch.zeros(Ns, dtype=torch.int32), L, torch.zeros(B, 3, 3),
                          torch.zeros(B, L, 3, 4), [0.0, 0.0, 1.0], 0.0)


def test_cpu_tensors_are_refused():
    from graspqp_amd import ops

    B, L = 2, 14
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.tabletop_terms(torch.zeros(B, 25), None, None, torch.zeros(B, 4, dtype=torch.long), torch.zeros(B, 3, 3),
                           torch.zeros(B, L, 3, 4), torch.zeros(8, dtype=torch.uint8), [0.0, 0.0, 1.0])


def test_stepper_refuses_unknown_weight_keys():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, TABLETOP_TERMS, merge_weights

    w = merge_weights(None)
    assert {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS and all(w[k] == 0.0 for k in TABLETOP_TERMS)
    w = merge_weights({"E_wall": 10, "E_prior": 2.5, "E_pen": 50})
    assert (w["E_wall"], w["E_prior"], w["E_pen"], w["E_dis"]) == (10.0, 2.5, 50.0, 100.0)
    for k in ("E_wall", "E_prior"):
        with pytest.raises(ValueError, match=k):
            merge_weights({k: -1.0})
    for bad in ("E_manipulativity", "e_wall", "wall"):
        with pytest.raises(ValueError, match=bad):
            merge_weights({bad: 1.0})


def _old_surface_samples(spec, n_surface_points):
    """The expressions HandModel._surface_handle held before the sampler moved to utils/meshes.py, written out."""
    from graspqp_amd.utils import meshes as mesh_utils

    fvs = [spec.link_faces(l).astype(np.float64) for l in range(spec.n_links)]
    areas = [0.5 * np.linalg.norm(np.cross(f[:, 1] - f[:, 0], f[:, 2] - f[:, 0]), axis=1).sum() if len(f) else 0.0 for f in fvs]
    tot = sum(areas)
    counts = [int(a / tot * n_surface_points) for a in areas]
    counts[0] += n_surface_points - sum(counts)
    pts, lnk = [], []
    for l, (f, k) in enumerate(zip(fvs, counts)):
        if k == 0 or len(f) == 0:
            continue
        dense = mesh_utils.sample_surface(f, 100 * k, seed=42)
        pts.append(mesh_utils.farthest_point_sampling(dense, k))
        lnk.append(np.full(k, l, dtype=np.int32))
    return np.concatenate(pts).astype(np.float32), np.concatenate(lnk)


@pytest.mark.parametrize("hand_name,n", [("allegro", 96), ("schunk2", 64)])
def test_extracted_sampler_returns_the_arrays_hand_model_used(hand_name, n):
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.utils import meshes as mesh_utils

    spec = get_hand_spec(hand_name)
    pts, lnk = mesh_utils.hand_surface_samples(spec, n)
    pts_old, lnk_old = _old_surface_samples(spec, n)
    assert pts.dtype == np.float32 and lnk.dtype == np.int32 and pts.shape == (n, 3) and lnk.shape == (n,)
    assert np.array_equal(pts, pts_old) and np.array_equal(lnk, lnk_old)
    assert (np.diff(lnk) >= 0).all() and lnk.min() >= 0 and lnk.max() < spec.n_links


def test_new_kernel_resources():
    """The two new kernels: no scratch, and within the 64-register step (8 wavefronts per SIMD) they were built at."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "tabletop" in k}
    assert sorted(new) == ["gq_tabletop_kernel", "gq_tabletop_total_kernel"], sorted(new)
    for r in new.values():
        assert r["scratch"] == 0, r
        assert r["vgpr"] + r["agpr"] <= 64, r
