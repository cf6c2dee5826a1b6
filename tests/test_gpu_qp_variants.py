"""Every box-QP kernel variant against the fp64 oracle (oracle/ref_cpu/qp.py), step by step.

The box-QP is a dispatch table (csrc/qp.hip gq_launch_iter / gq_launch_bwd, csrc/qp_lr.hip):
  dense Q   nz <= 16 / 32 / 48 / 64      gq_qp_iter_kernel<NZ>, gq_qp_bwd_kernel<NZ>       (register Cholesky)
            65 <= nz <= 128              gq_qp_dense_iter_kernel, gq_qp_dense_bwd_kernel   (matrix in LDS)
  low rank  m <= 6 | m in {7, 8}  x  nz <= 64 | nz > 64
                                         gq_qp_lr_iter_kernel<M,NC>, gq_qp_lr_bwd_kernel<M,NC>  (Woodbury)
The parametrisations below reach every row, on both sides of every boundary.

Comparisons are made where they are well conditioned, so that the tolerances can be tight:
  * forward at a FIXED iteration count (eps = 0: the stop rule cannot end the loop early): fp32 and fp64 iterates agree
    to a few ulps times the conditioning; the tolerance is derived per case from the oracle's own fp32 run on the same
    inputs, under an absolute ceiling;
  * converged forward against an independent optimum (scipy's BVLS) and the fp64 KKT residuals of the HIP multipliers;
  * backward at a FIXED KKT state taken from the fp64 oracle, against ``_solve_kkt_box`` in fp64, with a per-row bound
    from the fp32 conditioning of Q + diag(d_u + d_l);
  * autograd to every input at k = 2, 3 and the fused force-closure path at non-default settings.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import qp as oqp  # noqa: E402
from ref_cpu import span as ospan  # noqa: E402

from _scenes import hetero_contacts, lsq_box_problem, spd_box_qp  # noqa: E402

U32 = 2.0**-24  # fp32 unit round-off
KS = (1, 2, 3, 5)  # fixed PDIPM iteration counts of the forward comparisons
RIDGE = 1e-4  # SQPLsqSolver's Q = A'A + 1e-4 I (oracle lsq_box_qp)

DENSE_NZ = (1, 7, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 72, 100, 127, 128)
LR_M = (1, 3, 6, 7, 8)
LR_NZ = (1, 5, 24, 63, 64, 65, 96, 128)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return ops


def _cu(*ts):
    return tuple(t.float().cuda().contiguous() for t in ts)


def _rowerr(a, ref):
    """per-row inf-norm error of ``a`` relative to the inf norm of the fp64 reference row"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return ((a - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).numpy()


def _lsq_Qp(A, b):
    """the oracle's Q = A'A + ridge I and p = -A'b, in A's precision (oracle lsq_box_qp)"""
    nz = A.shape[2]
    Q = A.transpose(1, 2) @ A + RIDGE * torch.eye(nz, dtype=A.dtype)
    return Q, -(A.transpose(1, 2) @ b.unsqueeze(-1)).squeeze(-1)


# ---------------------------------------------------------------------------------------------------------------
# 1 + 2: forward at a fixed iteration count, every variant
# ---------------------------------------------------------------------------------------------------------------
# Errors after k iterations, per row, in the inf norm, relative to the size of the terms of the equation each satisfies:
# x against max(|x|, |slack|) (x + s_u = upper: with bounds at +-1e4 x inherits fp32 round-off of the bounds' size), lam
# against max(|lam|, |Q x| + |p|) (stationarity; lam -> 0 where no bound is active), slack against |slack|.
# Tolerance: NOISE_MULT x the oracle's own fp32 error on the same inputs (per case, batch max), within [FWD_FLOOR, FWD_CEIL].
NOISE_MULT = 16.0  # measured on the MI355X: HIP / oracle-fp32 error <= 8.4 (dense lam, nz = 100, B = 1, k = 3)
FWD_FLOOR = 2e-6  # ~ 30 ulps: below this a case's fp32 noise estimate is itself round-off
FWD_CEIL = 2e-3  # measured: largest HIP error under the ceiling 2e-4 (dense x and lam, k = 5)


def _fwd_errors(xls, o64, Q, p):
    x64 = o64[0]
    gs = (Q @ x64.unsqueeze(-1)).squeeze(-1).abs().amax(-1) + p.abs().amax(-1)
    out = []
    s_abs, l_abs = o64[2].abs().amax(-1), o64[1].abs().amax(-1)
    for t, r, scale in zip(xls, o64, (torch.maximum(x64.abs().amax(-1), s_abs), torch.maximum(l_abs, gs), s_abs)):
        t = t.detach().double().cpu()
        out.append(((t - r).abs().amax(-1) / scale.clamp_min(1e-30)).max().item())
    return out


def _check_fixed_iter(what, hip, o64, o32, n_hip, n64, Q, p, lam_ceil=FWD_CEIL):
    assert int(n_hip) == int(n64), f"{what}: n_iter {int(n_hip)} != oracle {int(n64)}"
    for t in hip:
        assert torch.isfinite(t).all(), f"{what}: non-finite output"
    for name, e, e32, ceil in zip(("x", "lam", "slack"), _fwd_errors(hip, o64, Q, p), _fwd_errors(o32, o64, Q, p),
                                  (FWD_CEIL, lam_ceil, FWD_CEIL)):
        tol = min(max(NOISE_MULT * e32, FWD_FLOOR), ceil)
        assert e <= tol, f"{what}: {name} err {e:.3g} > tol {tol:.3g} (oracle fp32 noise {e32:.3g})"


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("nz", DENSE_NZ)
def test_dense_fixed_iterations(gq, nz, B):
    Q, p, lo, up = spd_box_qp(B, nz, seed=1000 + nz + B)
    Qc, pc, lc, uc = _cu(Q, p, lo, up)
    for k in KS:
        lim = k + 1  # > k: the not-improved rule cannot fire either
        o64 = oqp.pdipm_forward_box(Q, p, lo, up, eps=0.0, maxIter=k, notImprovedLim=lim)
        o32 = oqp.pdipm_forward_box(Q.float(), p.float(), lo.float(), up.float(), eps=0.0, maxIter=k, notImprovedLim=lim)
        x, lam, slack, nit = torch.ops.graspqp_amd.box_qp(Qc, pc, lc, uc, 0.0, k, lim)
        _check_fixed_iter(f"dense nz={nz} B={B} k={k}", (x, lam, slack), o64[:3], o32[:3], nit.item(), o64[3], Q, p)


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("bounds", [(1.0, 21.0), (-1e4, 1e4)])
@pytest.mark.parametrize("m,nz", [(m, nz) for m in LR_M for nz in LR_NZ])
def test_lowrank_fixed_iterations(gq, m, nz, bounds, B):
    lo_s, up_s = bounds
    A, b = lsq_box_problem(B, m, nz, seed=2000 + 10 * nz + m + B, lower=lo_s, upper=up_s)
    Ac, bc = _cu(A, b)
    Q, p = _lsq_Qp(A, b)
    Q32, p32 = _lsq_Qp(A.float(), b.float())
    lo, up = torch.full((B, nz), lo_s, dtype=torch.float64), torch.full((B, nz), up_s, dtype=torch.float64)
    # the raw op uses qpth's notImprovedLim = 3, as the oracle's lsq_box_qp does.  With bounds at +-1e4 a single row's
    # residual can reach fp32 round-off by iteration 3, and the rule may then end the fp32 loop one iteration before the
    # fp64 one (measured: n_iter 4 vs 5 at m = 1, nz >= 64, B = 1, k = 5); k <= 3 leaves it no room to fire.
    for k in KS if up_s - lo_s < 1e3 else KS[:3]:
        o64 = oqp.pdipm_forward_box(Q, p, lo, up, eps=0.0, maxIter=k)
        o32 = oqp.pdipm_forward_box(Q32, p32, lo.float(), up.float(), eps=0.0, maxIter=k)
        x, lam, slack, nit = torch.ops.graspqp_amd.lsq_box_qp(Ac, bc, lo_s, up_s, RIDGE, 0.0, k)
        # bounds at +-1e4: the initial point (d = 1) puts lam at ~|h| = 1e4 and the next iterates cancel it down to the
        # size of the gradient terms, so lam carries fp32 round-off of the bounds' size.  The kernel reproduces the
        # oracle's own fp32 error there to three digits (measured on the MI355X, e.g. 206 vs 206 relative to |Q x| + |p|
        # at m = 1, nz = 128, k = 2): lam is held to the oracle-noise rule only, without the ceiling.
        _check_fixed_iter(f"low-rank m={m} nz={nz} bounds={bounds} B={B} k={k}", (x, lam, slack), o64[:3], o32[:3],
                          nit.item(), o64[3], Q, p, lam_ceil=FWD_CEIL if up_s - lo_s < 1e3 else float("inf"))


# ---------------------------------------------------------------------------------------------------------------
# 3: converged forward against an independent optimum (BVLS) and the fp64 KKT residuals of the HIP multipliers
# ---------------------------------------------------------------------------------------------------------------
def _bvls(R, t, lo, up):
    """argmin 1/2 |R x - t|^2 in the box, scipy's bounded-variable least squares in fp64, row by row"""
    from scipy.optimize import lsq_linear

    xs = [lsq_linear(R[i].numpy(), t[i].numpy(), bounds=(lo[i].numpy(), up[i].numpy()), method="bvls", tol=1e-14,
                     max_iter=1000).x for i in range(R.shape[0])]
    return torch.tensor(np.stack(xs), dtype=torch.float64)


def _check_converged(what, Q, p, lo, up, x, lam, slack, x_star):
    x, lam, slack = (t.detach().double().cpu() for t in (x, lam, slack))
    nz = x.shape[1]

    def f(v):
        return 0.5 * (v.unsqueeze(1) @ Q @ v.unsqueeze(-1)).squeeze(-1).squeeze(-1) + (p * v).sum(-1)

    f_star = f(x_star)
    scale = (Q @ x_star.unsqueeze(-1)).squeeze(-1).abs().amax(-1) + p.abs().amax(-1)  # size of the gradient terms
    bw = (up - lo).abs().amax(-1)
    gap = ((f(x) - f_star).abs() / (scale * bw)).max().item()
    lu, ll, su, sl = lam[:, :nz], lam[:, nz:], slack[:, :nz], slack[:, nz:]
    stat = ((Q @ x.unsqueeze(-1)).squeeze(-1) + p + lu - ll).abs().amax(-1) / scale
    prim = torch.maximum((x + su - up).abs().amax(-1), (-x + sl + lo).abs().amax(-1)) / bw
    comp = (lam * slack).abs().amax(-1) / (scale * bw)
    sign = torch.minimum(lam.amin(-1) / scale, slack.amin(-1) / bw)
    assert stat.max() <= CONV_KKT, f"{what}: stationarity {stat.max():.3g}"
    assert prim.max() <= CONV_KKT, f"{what}: primal feasibility {prim.max():.3g}"
    assert comp.max() <= CONV_KKT, f"{what}: complementarity {comp.max():.3g}"
    assert sign.min() >= 0.0, f"{what}: negative multiplier or slack {sign.min():.3g}"
    # x itself is not compared: along the directions the ridge alone pins down (low rank) it is ill-determined
    assert gap <= CONV_GAP, f"{what}: objective gap {gap:.3g}"


# relative to the gradient scale |Q x*| + |p| times the box width: fp32 PDIPM run to its noise floor
CONV_GAP = 1e-3  # measured: dense <= 1.4e-4 (nz = 128), low rank <= 6e-8
CONV_KKT = 1e-4  # measured: stationarity <= 3.4e-7, primal <= 3.9e-6, complementarity <= 2.7e-5 (dense nz = 100)


@pytest.mark.parametrize("nz", [7, 16, 33, 64, 100, 128])
def test_dense_converged_against_bvls(gq, nz):
    Q, p, lo, up = spd_box_qp(16, nz, seed=3000 + nz, cond=(1e1, 1e2))
    L = torch.linalg.cholesky(Q)  # 1/2 x'Qx + p'x = 1/2 |L'x + L^-1 p|^2 + const
    x_star = _bvls(L.transpose(1, 2), -torch.linalg.solve_triangular(L, p.unsqueeze(-1), upper=False).squeeze(-1), lo, up)
    x, lam, slack, _ = torch.ops.graspqp_amd.box_qp(*_cu(Q, p, lo, up), 1e-6, 64, 3)
    _check_converged(f"dense nz={nz}", Q, p, lo, up, x, lam, slack, x_star)


@pytest.mark.parametrize("m,nz", [(3, 5), (6, 24), (6, 96), (8, 63), (7, 65), (8, 128)])
def test_lowrank_converged_against_bvls(gq, m, nz):
    A, b = lsq_box_problem(16, m, nz, seed=4000 + nz + m)
    B = A.shape[0]
    lo, up = torch.full((B, nz), 1.0, dtype=torch.float64), torch.full((B, nz), 21.0, dtype=torch.float64)
    # 1/2 |A x - b|^2 + ridge/2 |x|^2 = 1/2 |[A; sqrt(ridge) I] x - [b; 0]|^2
    R = torch.cat([A, (RIDGE**0.5) * torch.eye(nz, dtype=torch.float64).expand(B, nz, nz)], 1)
    x_star = _bvls(R, torch.cat([b, torch.zeros(B, nz, dtype=torch.float64)], 1), lo, up)
    x, lam, slack, _ = torch.ops.graspqp_amd.lsq_box_qp(*_cu(A, b), 1.0, 21.0, RIDGE, 1e-6, 64)
    Q, p = _lsq_Qp(A, b)
    _check_converged(f"low-rank m={m} nz={nz}", Q, p, lo, up, x, lam, slack, x_star)


# ---------------------------------------------------------------------------------------------------------------
# 4: backward at a fixed KKT state
# ---------------------------------------------------------------------------------------------------------------
BWD_C = 8.0  # multiple of the per-row first-order fp32 bound (below); measured ratio <= 2.2 (dx), 1.3 (dlam)
BWD_FLOOR = 1e-6
BWD_CAP = 1e-2  # dense fp32 Cholesky: the bound reaches ~2e-3 on late iterates (d up to 1e10)
LR_BWD_CAP = 1e-5  # low-rank route: Woodbury system and rhs - A'y in fp64; measured <= 1.8e-7


def _kkt_state(Q, p, lo, up, it):
    """(lam, slack) of the fp64 oracle's iterate ``it`` (fixed count, eps = 0), rounded to fp32"""
    hist = []
    oqp.pdipm_forward_box(Q, p, lo, up, eps=0.0, maxIter=it + 1, notImprovedLim=it + 2, history=hist)
    return hist[it]["z"].float().double(), hist[it]["s"].float().double()


def _bwd_bounds(Q, d, dx):
    """Per-row first-order fp32 error bounds of dx = M^-1 r, M = Q + diag(d_u + d_l), and of dlam = d * (G dx), each
    relative to its inf norm.  Cholesky is backward stable in the Jacobi-scaled sense (van der Sluis): with D = diag(M),
    S = D^-1/2 M D^-1/2,  |dx_i - dx^_i| <~ u |S^-1|_2 |D^1/2 dx|_2 / sqrt(D_i)."""
    nz = Q.shape[-1]
    Dg = torch.diagonal(Q, dim1=1, dim2=2) + d[:, :nz] + d[:, nz:]
    M = Q + torch.diag_embed(d[:, :nz] + d[:, nz:])
    S = M / torch.sqrt(Dg[:, :, None] * Dg[:, None, :])
    s_inv = 1.0 / torch.linalg.eigvalsh(S)[:, 0]
    w = U32 * s_inv * torch.linalg.norm(torch.sqrt(Dg) * dx, dim=-1)  # (B,)
    ex = w / Dg.sqrt().amin(-1) / dx.abs().amax(-1)
    dlam = d * torch.cat([dx, -dx], 1)
    el = w * (d / torch.cat([Dg, Dg], 1).sqrt()).amax(-1) / dlam.abs().amax(-1)
    return ex.numpy(), el.numpy()


def _check_bwd(what, Q, lam, slack, gx, dx_h, dl_h, cap=BWD_CAP):
    d = lam.clamp_min(1e-8) / slack.clamp_min(1e-8)
    nz = Q.shape[-1]
    z0 = torch.zeros(Q.shape[0], 2 * nz, dtype=torch.float64)
    dx, _, dlam = oqp._solve_kkt_box(Q, d, gx, z0, z0)
    bx, bl = _bwd_bounds(Q, d, dx)
    for name, h, r, bound in (("dx", dx_h, dx, bx), ("dlam", dl_h, dlam, bl)):
        e = _rowerr(h, r)
        tol = np.clip(BWD_C * bound, BWD_FLOOR, cap)
        bad = np.flatnonzero(e > tol)
        assert bad.size == 0, (f"{what}: {name} rows {bad[:4].tolist()} err {e[bad[:4]].tolist()} > tol "
                               f"{tol[bad[:4]].tolist()}")


@pytest.mark.parametrize("it", [1, 6])  # early (moderate d = lam / slack) and late (d over ~12 decades)
@pytest.mark.parametrize("nz", [1, 7, 16, 17, 32, 33, 48, 64, 65, 100, 128])
def test_dense_backward_at_fixed_kkt_state(gq, nz, it):
    Q, p, lo, up = spd_box_qp(32, nz, seed=5000 + nz, cond=(1e1, 1e3))
    lam, slack = _kkt_state(Q, p, lo, up, it)
    gx = torch.randn(Q.shape[0], nz, generator=torch.Generator().manual_seed(nz), dtype=torch.float64).float().double()
    dx_h, dl_h = torch.ops.graspqp_amd.box_qp_backward(*_cu(Q, lam, slack, gx))
    _check_bwd(f"dense nz={nz} it={it}", Q, lam, slack, gx, dx_h, dl_h)


@pytest.mark.parametrize("it", [1, 6])
@pytest.mark.parametrize("m,nz", [(1, 1), (3, 24), (6, 63), (6, 64), (6, 65), (6, 128), (7, 5), (8, 64), (7, 65), (8, 96)])
def test_lowrank_backward_at_fixed_kkt_state(gq, m, nz, it):
    A, b = lsq_box_problem(32, m, nz, seed=6000 + nz + m)
    B = A.shape[0]
    Q, p = _lsq_Qp(A, b)
    lo, up = torch.full((B, nz), 1.0, dtype=torch.float64), torch.full((B, nz), 21.0, dtype=torch.float64)
    lam, slack = _kkt_state(Q, p, lo, up, it)
    gx = torch.randn(B, nz, generator=torch.Generator().manual_seed(nz), dtype=torch.float64).float().double()
    dx_h, dl_h = torch.ops.graspqp_amd.lsq_box_qp_backward(*_cu(A, lam, slack, gx), RIDGE)
    _check_bwd(f"low-rank m={m} nz={nz} it={it}", Q, lam, slack, gx, dx_h, dl_h, LR_BWD_CAP)


# ---------------------------------------------------------------------------------------------------------------
# 5: autograd to every input at a fixed iteration count
# ---------------------------------------------------------------------------------------------------------------
GRAD_TOL = 1e-4  # per-row normwise, relative; dense box_qp / QPFunction measured <= 2.3e-5 (k = 3)
LSQ_GRAD_TOL = 2e-3  # lsq_box_qp / SQPLsqSolver: cond(A'A + 1e-4 I) up to ~4e4, measured <= 3.4e-4 (k = 3)


def _grad_err(what, g_hip, g_ref, tol=GRAD_TOL):
    e = (torch.linalg.norm((g_hip.detach().double().cpu() - g_ref).flatten(1), dim=1)
         / torch.linalg.norm(g_ref.flatten(1), dim=1).clamp_min(1e-30)).max().item()
    assert e <= tol, f"{what}: gradient err {e:.3g}"


def _upstream(B, nz, seed):
    return torch.randn(B, nz, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float().double()


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("nz", [7, 32, 48, 64, 100])
def test_box_qp_autograd_every_input(gq, nz, k):
    B = 16
    Q, p, lo, up = spd_box_qp(B, nz, seed=7000 + nz, cond=(1e1, 1e3))
    w = _upstream(B, nz, nz + k)
    ins = [t.float().cuda().requires_grad_() for t in (Q, p, lo, up)]
    x, _, _ = gq.box_qp(*ins, eps=0.0, max_iter=k, not_improved_lim=3)
    (x * w.float().cuda()).sum().backward()
    Qo, po, loo, upo = (t.clone().requires_grad_() for t in (Q, p, lo, up))
    G = torch.cat([torch.eye(nz, dtype=torch.float64), -torch.eye(nz, dtype=torch.float64)])
    xo = oqp.QPFunction(eps=0.0, maxIter=k, box_form=True)(Qo, po, G, torch.cat([upo, -loo], 1))
    (xo * w).sum().backward()
    for name, h, r in zip(("Q", "p", "lower", "upper"), ins, (Qo, po, loo, upo)):
        _grad_err(f"box_qp nz={nz} k={k} d/d{name}", h.grad, r.grad)

    # the qpth-shaped QPFunction(Q, p, G, h): gradient wrt h
    from graspqp_amd.metrics import QPFunction

    hg = torch.cat([up, -lo], 1).float().cuda().requires_grad_()
    xq = QPFunction(maxIter=k, eps=0.0)(Q.float().cuda(), p.float().cuda(), G.float().cuda(), hg)
    (xq * w.float().cuda()).sum().backward()
    ho = torch.cat([up, -lo], 1).requires_grad_()
    (oqp.QPFunction(eps=0.0, maxIter=k, box_form=True)(Q, p, G, ho) * w).sum().backward()
    _grad_err(f"QPFunction nz={nz} k={k} d/dh", hg.grad, ho.grad)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("m,nz", [(3, 5), (6, 24), (6, 96), (8, 63), (7, 65), (8, 128)])
def test_lsq_autograd_A_and_b(gq, m, nz, k):
    from graspqp_amd.metrics import SQPLsqSolver

    B = 16
    A, b = lsq_box_problem(B, m, nz, seed=8000 + nz + m)
    w, v = _upstream(B, nz, nz), _upstream(B, 1, m)[:, 0]
    Ao, bo = A.clone().requires_grad_(), b.clone().requires_grad_()
    val_o, xo = oqp.lsq_box_qp(Ao, bo, 1.0, 21.0, eps=0.0, maxIter=k, box_form=True)
    ((xo * w).sum() + (val_o * v).sum()).backward()

    Ah, bh = (t.float().cuda().requires_grad_() for t in (A, b))
    x = gq.lsq_box_qp(Ah, bh, 1.0, 21.0, ridge=RIDGE, eps=0.0, max_iter=k)
    val = 0.5 * ((bh - (Ah @ x.unsqueeze(-1)).squeeze(-1)) ** 2).sum(-1)
    ((x * w.float().cuda()).sum() + (val * v.float().cuda()).sum()).backward()
    _grad_err(f"lsq_box_qp m={m} nz={nz} k={k} d/dA", Ah.grad, Ao.grad, LSQ_GRAD_TOL)
    _grad_err(f"lsq_box_qp m={m} nz={nz} k={k} d/db", bh.grad, bo.grad, LSQ_GRAD_TOL)

    As, bs = (t.float().cuda().requires_grad_() for t in (A, b))
    solver = SQPLsqSolver.from_mat(As.detach(), bs.detach())
    solver._max_iter, solver._eps = k, 0.0  # the fixed iteration count (reference defaults: 12, 5e-2)
    val_s, xs = solver.solve(As, bs, min_bound=1.0, max_bound=21.0, return_solution=True)
    ((xs * w.float().cuda()).sum() + (val_s * v.float().cuda()).sum()).backward()
    _grad_err(f"SQPLsqSolver m={m} nz={nz} k={k} d/dA", As.grad, Ao.grad, LSQ_GRAD_TOL)
    _grad_err(f"SQPLsqSolver m={m} nz={nz} k={k} d/db", bs.grad, bo.grad, LSQ_GRAD_TOL)


# ---------------------------------------------------------------------------------------------------------------
# 6: the fused force-closure path at non-default settings
# ---------------------------------------------------------------------------------------------------------------
FC_CFGS = (dict(friction=0.5, torque_weight=1.0, max_limit=5.0, svd_gain=0.3, values_gain=1.0),
           dict(friction=0.3, torque_weight=2.0, max_limit=10.0, svd_gain=0.05, values_gain=3.0))
FC_TOL_E = 1e-5  # measured <= 3.0e-6 (k = 3)
FC_TOL_G = 1e-5  # measured <= 1.8e-6


@pytest.mark.parametrize("cfg", range(len(FC_CFGS)))
@pytest.mark.parametrize("k_it", [1, 3])
@pytest.mark.parametrize("n,kc", [(5, 3), (16, 4), (13, 5), (11, 6), (8, 8), (16, 8)])  # nz = 15, 64, 65, 66, 64, 128
def test_fc_energy_non_default_settings(gq, n, kc, k_it, cfg):
    B = 16
    FC_CFG = FC_CFGS[cfg]
    pts, nrm, cog = (t.float().double() for t in hetero_contacts(B, n, seed=9000 + n * kc))
    po = pts.clone().requires_grad_()
    eo, xso = ospan.e_fc(po, nrm, cog, svd_gain=FC_CFG["svd_gain"], values_gain=FC_CFG["values_gain"], k=kc,
                         mu=FC_CFG["friction"], torque_weight=FC_CFG["torque_weight"], max_limit=FC_CFG["max_limit"],
                         eps=0.0, maxIter=k_it, box_form=True)
    ge = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    (eo * ge).sum().backward()
    pg = pts.float().cuda().requires_grad_()
    e, xs = gq.fc_energy(pg, nrm.float().cuda(), cog.float().cuda(), n_cone_vecs=kc, eps=0.0, max_iter=k_it, **FC_CFG)
    (e * ge.float().cuda()).sum().backward()
    what = f"fc_energy n={n} k={kc} it={k_it} cfg={cfg}"
    er = (e.detach().double().cpu() - eo.detach()).abs() / eo.detach().abs()
    assert er.max() <= FC_TOL_E, f"{what}: E_fc rel err {er.max():.3g}"
    _grad_err(f"{what} d/dcontact_pts", pg.grad.double().cpu(), po.grad, FC_TOL_G)
