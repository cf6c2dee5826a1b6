"""Exact grasp-quality metrics on the device: the BVLS kernel (ops.lsq_box_exact / ScipyLsqSolver), the fused span metrics
(ops.span_exact, GRASPQP_SCIPY / GRASPQP_EUCLIDIAN_SCIPY forms) and HandModel's entropies, against scipy and the
reference's own answers stored in tests/golden."""
import os

import numpy as np
import pytest
import torch
from scipy.optimize import lsq_linear

pytestmark = pytest.mark.gpu

from graspqp_amd import ops  # noqa: E402
from graspqp_amd.metrics import (EucledianFrictionConeSpanMetric, OverallFrictionConeSpanMetric, ScipyLsqSolver,  # noqa: E402
                                 SpanMetricWrapper, SQPLsqSolver)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bvls(A, b, lo, hi):
    return lsq_linear(A.astype(np.float64), b.astype(np.float64), bounds=(lo, hi), method="bvls")


def _check_rows(A, b, lo, hi, x, v, st):
    """value within 1e-6 v* + 1e-9 (1 + |b|^2) of fp64 BVLS; x feasible with a small fp64 projected gradient."""
    A64, b64, x64 = A.double().cpu().numpy(), b.double().cpu().numpy(), x.double().cpu().numpy()
    v, st = v.double().cpu().numpy(), st.cpu().numpy()
    assert (st >= 0).all(), st.min()
    for r in range(A64.shape[0]):
        ref = _bvls(A64[r], b64[r], lo, hi).cost
        bb = float(b64[r] @ b64[r])
        assert abs(v[r] - ref) <= 1e-6 * ref + 1e-9 * (1 + bb), (r, v[r], ref)
        xr = x64[r]
        assert (xr >= lo - 1e-9 * max(1, abs(lo))).all() and (xr <= hi + 1e-9 * max(1, abs(hi))).all()
        g = A64[r].T @ (A64[r] @ xr - b64[r])
        pg = np.where(xr <= lo, np.minimum(g, 0), np.where(xr >= hi, np.maximum(g, 0), g))
        an = np.linalg.norm(A64[r])
        assert np.abs(pg).max() <= 1e-4 * an * (an * np.abs(xr).max() + np.sqrt(bb)) + 1e-12, (r, np.abs(pg).max())


def _span_A(B, n, k, g):
    d = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    cp = d * (0.05 + 0.01 * torch.randn(B, n, 1, generator=g))
    cn = torch.nn.functional.normalize(d + 0.3 * torch.randn(B, n, 3, generator=g), dim=-1)
    cog = 0.005 * torch.randn(B, 3, generator=g)
    return cp, cn, cog


def _F(cp, cn, cog, k, mu=0.2, tw=5.0):
    """grasp matrix (B,6,n k) of the friction-cone metric (span.py:167-205, 25-38) in fp32 torch"""
    B, n, _ = cn.shape
    b1 = torch.full((B, n, 3), 3 ** -0.5, device=cn.device)
    dot = (b1 * cn).sum(-1) / (cn.norm(dim=-1) + 1e-6)
    b1[..., 1] -= 2 * (dot > 0.9).float()
    t1 = torch.linalg.cross(cn, b1)
    t2 = torch.linalg.cross(cn, t1)
    c = (1 - mu ** 2) ** 0.5
    if k == 4:
        dirs = [mu * t1 + c * cn, mu * t2 + c * cn, -mu * t1 + c * cn, -mu * t2 + c * cn]
    else:
        a = [2 * np.pi / k * i for i in range(k)]
        dirs = [mu * (np.cos(x) * t1 + np.sin(x) * t2) + c * cn for x in a]
    f = torch.stack(dirs, -2).flatten(-3, -2) / k
    r = (cp - cog.unsqueeze(1)).repeat_interleave(k, dim=-2)
    return torch.cat([f, torch.linalg.cross(r, f) * tw], -1).mT.contiguous()


@pytest.mark.parametrize("m,nz", [(1, 1), (3, 16), (6, 48), (8, 96), (6, 128), (8, 128), (8, 3)])
@pytest.mark.parametrize("bounds", [(0.0, 50.0), (1.0, 21.0), (-1e4, 1e4)])
def test_lsq_exact_random_against_scipy_bvls(m, nz, bounds):
    g = torch.Generator().manual_seed(m * 1000 + nz)
    B = 64
    A = torch.randn(B, m, nz, generator=g)
    b = torch.randn(B, m, generator=g) * 2
    s = ScipyLsqSolver.from_mat(A.cuda(), b.cuda())  # outputs go to the device the solver was built for, as in the reference
    v, x = s.solve(A.cuda(), b.cuda(), min_bound=bounds[0], max_bound=bounds[1], return_solution=True)
    assert v.dtype == torch.float32 and v.device.type == "cuda" and x.shape == (B, nz) and not v.requires_grad
    _check_rows(A, b, *bounds, x, v, s.last_status)


@pytest.mark.parametrize("n,k", [(4, 4), (12, 4), (12, 8), (16, 8), (24, 4)])
@pytest.mark.parametrize("bounds,basis", [((1.0, 21.0), "zero"), ((0.0, 50.0), "euclid")])
def test_lsq_exact_span_shaped(n, k, bounds, basis):
    g = torch.Generator().manual_seed(7 * n + k)
    F = _F(*_span_A(32, n, k, g), k)
    if basis == "zero":
        b = torch.zeros(32, 6)
    else:
        b = torch.cat([torch.eye(6), -torch.eye(6)])[torch.arange(32) % 12]
    x, v, st = ops.lsq_box_exact(F.cuda(), b.cuda(), *bounds)
    _check_rows(F, b, *bounds, x, v, st)


def test_lsq_exact_degenerate_cases():
    g = torch.Generator().manual_seed(3)
    A = torch.randn(6, 4, 32, generator=g)
    A[0, :, 5] = 0  # zero column
    A[1, :, 7] = A[1, :, 3]  # duplicate columns (coincident contacts)
    A[1, :, 8] = A[1, :, 3]
    A[2] = torch.randn(4, 2, generator=g) @ torch.randn(2, 32, generator=g)  # rank 2
    A[3, :, 16:] = 0
    b = torch.randn(6, 4, generator=g)
    b[5] = 0
    x, v, st = ops.lsq_box_exact(A.cuda(), b.cuda(), -1.0, 2.0)
    _check_rows(A, b, -1.0, 2.0, x, v, st)
    # m > nz
    A2 = torch.randn(8, 8, 3, generator=g)
    b2 = torch.randn(8, 8, generator=g)
    x, v, st = ops.lsq_box_exact(A2.cuda(), b2.cuda(), 0.0, 1.0)
    _check_rows(A2, b2, 0.0, 1.0, x, v, st)
    # lower == upper: x is the bound, zero iterations
    x, v, st = ops.lsq_box_exact(A2.cuda(), b2.cuda(), 0.5, 0.5)
    assert (x == 0.5).all() and (st == 0).all()
    ref = 0.5 * ((A2.double() @ torch.full((8, 3, 1), 0.5, dtype=torch.float64)).squeeze(-1) - b2.double()).pow(2).sum(-1)
    torch.testing.assert_close(v.double().cpu(), ref, rtol=1e-6, atol=1e-9)
    # refused at the C entry
    with pytest.raises(RuntimeError, match="lower"):
        ops.lsq_box_exact(A2.cuda(), b2.cuda(), 1.0, 0.0)
    with pytest.raises(RuntimeError, match="finite"):
        ops.lsq_box_exact(A2.cuda(), b2.cuda(), 0.0, float("inf"))


def test_lsq_exact_nan_row_fp64_and_large_batch():
    g = torch.Generator().manual_seed(4)
    B = 4096
    A = torch.randn(B, 6, 48, generator=g, dtype=torch.float64)
    b = torch.randn(B, 6, generator=g, dtype=torch.float64)
    A[17, 2, 9] = float("nan")
    x, v, st = ops.lsq_box_exact(A.cuda(), b.cuda(), 0.0, 50.0)
    assert v.dtype == torch.float64 and x.dtype == torch.float64
    assert torch.isnan(v[17]) and int(st[17]) == -2
    keep = torch.ones(B, dtype=torch.bool)
    keep[17] = False
    assert (st[keep.cuda()] >= 0).all()
    # neighbours are unchanged by the NaN row
    x2, v2, st2 = ops.lsq_box_exact(A[16:19:2].cuda(), b[16:19:2].cuda(), 0.0, 50.0)
    assert torch.equal(v2, v[16:19:2]) and torch.equal(x2, x[16:19:2])
    sel = torch.arange(0, B, 97)
    sel = sel[sel != 17]
    _check_rows(A[sel], b[sel], 0.0, 50.0, x[sel.cuda()], v[sel.cuda()], st[sel.cuda()])
    # bitwise reproducible
    x3, v3, st3 = ops.lsq_box_exact(A.cuda(), b.cuda(), 0.0, 50.0)
    assert torch.equal(torch.nan_to_num(v3), torch.nan_to_num(v)) and torch.equal(st3, st)


def test_kat_solver_golden():
    d = np.load(os.path.join(GOLD, "kat_solver.npz"))
    A, b = torch.tensor(d["A"]).cuda(), torch.tensor(d["b"]).cuda()
    s = ScipyLsqSolver.from_mat(A, b)
    v, x = s(A, b, min_bound=float(d["min_bound"]), max_bound=float(d["max_bound"]), init=0.1, return_solution=True)
    assert abs(float(v[0]) - float(d["value"][0])) < 1e-4


def test_solver_4d_and_b_broadcast():
    g = torch.Generator().manual_seed(5)
    A = torch.randn(3, 12, 6, 16, generator=g).cuda()
    b = torch.randn(1, 12, 6, generator=g).cuda()
    s = ScipyLsqSolver.from_mat(A, b)
    v, x = s.solve(A, b, min_bound=0.0, max_bound=50.0, return_solution=True)
    assert v.shape == (3, 12) and x.shape == (3, 12, 16)
    v1 = s.solve(A[1:2], b, min_bound=0.0, max_bound=50.0)
    assert torch.equal(v1[0], v[1])
    assert not issubclass(ScipyLsqSolver, SQPLsqSolver)


@pytest.mark.parametrize("name", ["span_n4_k4", "span_n12_k4", "span_n16_k4", "span_n12_k8"])
def test_overall_exact_against_reference_golden(name):
    d = np.load(os.path.join(GOLD, name + ".npz"))
    k = int(d["n_cone_vecs"])
    fn = SpanMetricWrapper(OverallFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver, "friction": float(d["friction"]),
                                                          "max_limit": float(d["max_limit"]), "n_cone_vecs": k})
    cp = torch.tensor(d["contact_pts"]).cuda().requires_grad_()
    e, x = fn(contact_pts=cp, contact_normals=torch.tensor(d["contact_normals"]).cuda(), sdf=None,
              cog=torch.tensor(d["cog"]).cuda(), with_solution=True, svd_gain=float(d["svd_gain"]))
    assert fn.exact and not e.requires_grad and x.shape == d["x_sum"].shape
    np.testing.assert_allclose(e.cpu().numpy(), d["e_fc"], rtol=1e-5)


@pytest.mark.parametrize("n,k", [(12, 4), (12, 8), (16, 4), (16, 8)])
def test_euclidean_against_reference_golden(n, k):
    d = np.load(os.path.join(GOLD, f"span_euclid_n{n}_k{k}.npz"))
    m = EucledianFrictionConeSpanMetric(solver_cls=ScipyLsqSolver, friction=float(d["friction"]), n_cone_vecs=k)
    cp, cn, cog = (torch.tensor(d[key]).cuda() for key in ("contact_pts", "contact_normals", "cog"))
    res, basis, svd, xs = m(cp, cn, cog)
    assert res.shape == (cp.shape[0], 12) and basis.shape == (cp.shape[0], 12, 6) and svd.shape == (cp.shape[0], 1)
    assert xs.shape == (cp.shape[0], 12, n) and (m._cache["status"] >= 0).all()
    r = res.double().cpu().numpy()
    assert np.abs(r - d["values_bvls"]).max() <= 2e-6
    assert (r <= d["values_ref"] + 2e-6).all()  # never worse than the reference's trf
    np.testing.assert_allclose(svd[:, 0].cpu().numpy(), d["svd"], rtol=1e-5)
    fn = SpanMetricWrapper(EucledianFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver, "friction": 0.2, "n_cone_vecs": k})
    e = fn(contact_pts=cp, contact_normals=cn, cog=cog, svd_gain=0.1)
    e_bvls = 2.0 * (d["values_bvls"].mean(-1) + 0.01) * np.exp(-0.1 * d["svd"])
    np.testing.assert_allclose(e.double().cpu().numpy(), e_bvls, rtol=1e-5)


def test_fused_op_matches_solver_path_and_is_reproducible():
    g = torch.Generator().manual_seed(9)
    cp, cn, cog = (t.cuda() for t in _span_A(64, 12, 8, g))
    F = _F(cp, cn, cog, 8)
    val, xs, svd, st = ops.span_exact(cp, cn, cog, 8, 0.2, 5.0, 12, 0.0, 50.0)
    b = torch.cat([torch.eye(6), -torch.eye(6)]).cuda()
    s = ScipyLsqSolver()
    v2, x2 = s.solve(F.unsqueeze(1).expand(-1, 12, -1, -1).contiguous(), b.unsqueeze(0).expand(64, -1, -1),
                     min_bound=0.0, max_bound=50.0, return_solution=True)
    torch.testing.assert_close(val, v2, rtol=1e-4, atol=1e-7)  # F built by torch here: last-bit differences
    val2, xs2, svd2, st2 = ops.span_exact(cp, cn, cog, 8, 0.2, 5.0, 12, 0.0, 50.0)
    assert torch.equal(val, val2) and torch.equal(xs, xs2) and torch.equal(svd, svd2) and torch.equal(st, st2)


def test_fused_op_large_batch():
    g = torch.Generator().manual_seed(11)
    B = 32 * 1024
    cp, cn, cog = (t.cuda() for t in _span_A(B, 12, 8, g))
    val, xs, svd, st = ops.span_exact(cp, cn, cog, 8, 0.2, 5.0, 12, 0.0, 50.0)
    torch.cuda.synchronize()
    assert (st >= 0).all(), int(st.min())
    sel = torch.arange(0, B, B // 256)
    F = _F(cp[sel], cn[sel], cog[sel], 8).double().cpu().numpy()  # torch-built F: allow its rounding
    basis = np.concatenate([np.eye(6), -np.eye(6)])
    v = val[sel].double().cpu().numpy()
    for r in range(len(sel)):
        for i in (0, 5, 7, 11):
            ref = _bvls(F[r], basis[i], 0.0, 50.0).cost
            assert abs(v[r, i] - ref) <= 1e-5 * ref + 1e-8, (r, i, v[r, i], ref)


def test_calculate_energy_with_exact_wrapper_and_fused_route_unchanged():
    from graspqp_amd.core.energy import _fusable, calculate_energy
    from graspqp_amd.core.hand_model import get_hand_model
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF
    from graspqp_amd.utils import meshes

    pd = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0})
    ex = SpanMetricWrapper(OverallFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver, "friction": 0.2, "max_limit": 20.0})
    eu = SpanMetricWrapper(EucledianFrictionConeSpanMetric, {"solver_cls": ScipyLsqSolver, "friction": 0.2})
    assert not pd.exact and ex.exact and eu.exact
    g = torch.Generator().manual_seed(2)
    cp, cn, cog = (t.cuda() for t in _span_A(16, 4, 4, g))
    e0 = pd(contact_pts=cp, contact_normals=cn, cog=cog)
    cfg = dict(ops.FC_DEFAULTS)
    cfg.update(friction=0.2, n_cone_vecs=4, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0)
    e1, _ = ops.fc_energy(cp, cn, cog, **cfg)
    assert torch.equal(e0, e1)  # the PDIPM wrapper still takes the loop's op, bit for bit
    ee = ex(contact_pts=cp, contact_normals=cn, cog=cog)
    assert (ee <= e0 * (1 + 1e-4)).all()  # the exact optimum is never above the PDIPM iterate
    # class surface: a scene, the composed route for the exact wrappers, the fused one for the PDIPM wrapper
    be, n = 4, 4
    fv = meshes.icosphere(3, 0.05)
    sp = meshes.surface_points(fv, 400, oversample=8)
    hm = get_hand_model("allegro", device="cuda")
    om = ObjectModel(batch_size_each=be, num_samples=400)
    om.initialize_from_meshes([fv], surface_points_list=[sp])
    t = torch.nn.functional.normalize(torch.randn(be, 3, generator=g), dim=-1) * 0.12
    hp = torch.cat([t, torch.randn(be, 6, generator=g), torch.tensor(hm.spec.default_state)[None].float().expand(be, -1)], 1)
    idx = torch.randint(hm.n_contact_candidates, (be, n), generator=g)
    for fn, fused in ((pd, True), (ex, False), (eu, False)):
        hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
        assert _fusable(hm, om, fn, "gendexgrasp", []) == fused
        losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=[], svd_gain=0.1)
        assert losses["E_fc"].shape == (be,) and torch.isfinite(losses["E_fc"]).all()
        assert losses["E_fc"].requires_grad == fused
        total = sum(losses.values())
        total.sum().backward()
        assert torch.isfinite(hm.hand_pose.grad).all() and hm.hand_pose.grad.abs().sum() > 0


def test_entropies_match_fp64_restatement():
    from scipy.spatial.transform import Rotation

    from graspqp_amd.core.hand_model import get_hand_model

    for hand in ("allegro", "ability_hand"):
        hm = get_hand_model(hand, device="cuda")
        g = torch.Generator().manual_seed(1)
        B = 512
        lo, hi = hm.joints_lower.cpu(), hm.joints_upper.cpu()
        q = lo + (hi - lo) * torch.rand(B, lo.numel(), generator=g) * 1.1 - 0.05 * (hi - lo)
        hp = torch.cat([0.08 * torch.randn(B, 3, generator=g), torch.randn(B, 6, generator=g), q], 1)
        hm.set_parameters(hp.cuda(), torch.zeros(B, 4, dtype=torch.long, device="cuda"))
        je = hm.joint_entropy()
        te, re = hm.pose_entropy()
        assert je.dim() == 0 and te.dim() == 0 and re.dim() == 0

        def H(v, a, b):
            c = torch.histc(v, 32, a, b)
            p = c / c.sum()
            return float(-(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))).sum())

        hp64 = hp.double()
        je_ref = sum(H(hp64[:, 9 + j], float(lo[j]), float(hi[j])) for j in range(lo.numel())) / lo.numel()
        te_ref = sum(H(hp64[:, i], -0.1, 0.1) for i in range(3)) / 3
        x = torch.nn.functional.normalize(hp64[:, 3:6], dim=-1)
        y = hp64[:, 6:9] - (x * hp64[:, 6:9]).sum(-1, keepdim=True) * x
        y = torch.nn.functional.normalize(y, dim=-1)
        R = torch.stack([x, y, torch.linalg.cross(x, y)], -1).numpy()
        v = torch.tensor(Rotation.from_matrix(R).as_rotvec())
        r = v.norm(dim=-1)
        sph = [r, torch.acos(v[:, 2] / r), torch.sign(v[:, 1]) * torch.acos(v[:, 0] / v[:, :2].norm(dim=-1))]
        lim = [(0, np.pi), (0, np.pi), (-np.pi, np.pi)]
        re_ref = sum(H(sph[i], *lim[i]) for i in range(3)) / 3
        assert abs(float(je) - je_ref) < 1e-5 and abs(float(te) - te_ref) < 1e-5 and abs(float(re) - re_ref) < 1e-5, \
            (hand, float(je), je_ref, float(te), te_ref, float(re), re_ref)


def test_register_budget_of_the_exact_kernels():
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources()
    names = [k for k in res if "exact_kernel" in k]
    assert len(names) == 4, names
    for k in names:
        assert res[k]["scratch"] == 0, (k, res[k])
        assert res[k]["vgpr"] + res[k]["agpr"] <= 168, (k, res[k])  # 3 wavefronts per SIMD (DESIGN: exact metrics)
