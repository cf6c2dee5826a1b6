"""The fc tail asks for its iterate before k* is known: slot, last snapshot, or back to the table.

The tail of the fused step (csrc/fcstep_dev.h::gq_fc_tail_body) requests two candidates with its first loads -- the slot
in which the head keeps the row's best iterate among iterations 0 .. max_iter - 2 (iteration bi_a) and the snapshot of
the last iteration -- while other wavefronts of its block replay qpth's batch-global stop rule.  Once k* is known the row
takes the last snapshot (k* is the last iteration and that iterate improved the row's residual), else the slot
(bi_a <= k*), else it goes back to memory for the snapshot of the best iterate among 0..k*.  Three settings of eps on the
same contacts take the code through all of it:

  default   the rule stops at the last iteration or the one before: no row goes back to the table;
  huge      the rule stops at iteration 0 (n_iter == 1): every row with bi_a > 0 goes back for snapshot 0;
  mid-way   an eps at which the rule stops in the middle: rows served by the slot and rows that go back, in one launch.

The contacts are those of Allegro grasps on a superquadric after 100 MALA* steps (the benchmark's workload; from there on
its rows converge slowly enough for the default eps to let all or all but one of the iterations count).  Every case is
compared with oracle/ref_cpu in fp64 at the same eps, row by row: E_fc and F x under the rule of tests/_parity.py with its
default bounds (within twice the oracle's own fp32 noise on the same inputs, floor 1e-4, ceiling 5e-3), the contact
gradient to 2e-2 of its norm over the batch as in test_gpu_parity.py and under the same rule on every row whose gradient
the oracle reproduces in fp32.  x itself -- 48 variables of which F fixes
6 directions -- is pinned to 1e-6 against the best iterate that the library's box QP selects from its snapshot table on
the same F and eps; a neighbouring snapshot is off by 1e-3 and more, a wrong one by 1e-1.

k* of a launch is what gq_fc_step reports (n_iter - 1).  The best iteration of every row among the first max_iter - 1 and
among all iterations, and the eps of the mid-way case, come from the library's own box-QP entry point on the step's
grasp matrix (gq_lsq_boxqp_forward: the same PDIPM loop, per-row best iteration as an output): eps is searched on a
geometric grid for a stop iteration in the middle that both neighbouring grid values share, so that the fp64 oracle
stops at the same iteration.  8 rows go through the tail that replays the stop rule beside the row
(gq_fc_tail_kernel<1, 4>; eight consecutive rows of the 260, around a slow one), 260 rows through the large-batch tail
that reads k* from memory (gq_fc_tail_kernel<1, 0>, stop rule in the head's epilogue).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import span as ospan  # noqa: E402

from _parity import assert_tail_within_fp32_noise, rel_err  # noqa: E402

N, K, MAX_ITER = 12, 4, 12
FC = dict(friction=0.2, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0)
EPS_DEFAULT = 5e-2
EPS_HUGE = 1e30


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return ops


def _contacts(gq, B):
    """contact points, outward object normals, cog of B Allegro grasps on a superquadric after 100 MALA* steps"""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from bench import make_initial_state
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.stepper import GraspStepper
    from graspqp_amd.utils import meshes

    spec = get_hand_spec("allegro")
    fv = meshes.superquadric(0)
    sp = meshes.surface_points(fv, 700, oversample=4, seed=42)
    st = GraspStepper(gq.HandHandle(spec), gq.MeshSet([fv]), torch.tensor(sp)[None], B, N, seed=1)
    hp, idx = make_initial_state(spec, fv, B, N, 1000)
    st.reset(hp.cuda(), idx.cuda())
    for _ in range(100):
        st.step()
    st.flush()
    torch.cuda.synchronize()
    return tuple(t.detach().float().cpu().double() for t in (st.cpts, st.obj_normal, st.cog))


def _view(ws, ptr, count):
    off = int(ptr.value) - ws.data_ptr()
    return ws[off:off + 4 * count].view(torch.float32)


def _fc_step(gq, pts, nrm, cog, eps):
    """gq_fc_step with w_dis = 0, w_fc = 1 -> (E_fc, x, dE_fc/d contact points, n_iter, F)"""
    from graspqp_amd import _C

    B = pts.shape[0]
    f = lambda t: t.float().cuda().contiguous()
    p, nr, cg = f(pts), f(nrm), f(cog)
    d2 = torch.full((B, N), 1e-4, device="cuda")
    sgn = torch.ones(B, N, dtype=torch.int32, device="cuda")
    closest = (p - 0.01 * nr).contiguous()
    hand_n = (-nr).contiguous()
    obj_normal, g_cpts, g_cnrm = torch.empty_like(p), torch.empty_like(p), torch.empty_like(p)
    e = torch.empty(B, device="cuda")
    xs = torch.empty(B, N, device="cuda")
    nit = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = gq._size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), N, K, MAX_ITER)
    ws = gq._ws(nb, p.device).zero_()
    _C.call("gq_fc_step", _C.f32(d2), _C.i32(sgn), _C.f32(nr), _C.f32(closest), _C.f32(p), _C.f32(hand_n), _C.f32(cg), B, N, K,
            FC["friction"], FC["torque_weight"], FC["max_limit"], FC["svd_gain"], FC["values_gain"], float(eps), MAX_ITER,
            0.0, 1.0, _C.f32(obj_normal), _C.f32(g_cpts), _C.f32(g_cnrm), _C.f32(e), _C.f32(xs), _C.i32(nit), _C.ptr(ws), nb,
            _C.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(obj_normal, nr)
    Fp, xp, _, _ = gq.fc_peek(ws, B, N, K)
    x = _view(ws, xp, B * N * K).view(B, N * K).clone()
    F = _view(ws, Fp, B * 6 * N * K).view(B, 6, N * K).clone()
    return e.cpu().double(), x.cpu().double(), g_cpts.cpu().double(), int(nit.item()), F


def _qp_stop(gq, F, eps, lim, max_iter=MAX_ITER):
    """the library's box QP on the step's grasp matrix -> (n_iter, per-row best iteration among 0..k*)"""
    from graspqp_amd import _C

    B, m, nz = F.shape
    x = torch.empty(B, nz, device="cuda")
    lam, slack = torch.empty(B, 2 * nz, device="cuda"), torch.empty(B, 2 * nz, device="cuda")
    bi = torch.zeros(B, dtype=torch.int32, device="cuda")
    nit = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nb = gq._qp_ws(B, nz, max_iter, F.device)
    _C.call("gq_lsq_boxqp_forward", _C.f32(F), None, None, None, 1.0, FC["max_limit"] + 1.0, B, m, nz, 1e-4, float(eps),
            int(max_iter), int(lim), _C.f32(x), _C.f32(lam), _C.f32(slack), _C.i32(bi), _C.i32(nit), _C.ptr(ws), nb, _C.stream_ptr())
    _qp_stop.x = x  # the solver's own best iterate among 0..k* of every row
    return int(nit.item()), bi.cpu().numpy()


class _Case:
    pass


_CACHE = {}


def _mid_eps(gq, F, bi_a):
    """eps on a geometric grid at which the rule stops mid-way, with the same stop iteration at both neighbouring grid
    values and as many rows as possible on either side of it -> (eps or None, rows on the smaller side)"""
    grid = [10.0 ** (e / 4.0) for e in range(-24, 25)]  # 1e-6 .. 1e6, four values per decade
    n_at = [_qp_stop(gq, F, e, 3)[0] for e in grid]
    eps_mid, best = None, 0
    for i in range(1, len(grid) - 1):
        ks = n_at[i] - 1
        if 2 <= ks <= MAX_ITER - 3 and n_at[i - 1] == n_at[i] == n_at[i + 1]:
            score = min(int((bi_a > ks).sum()), int((bi_a <= ks).sum()))
            if score > best:
                eps_mid, best = grid[i], score
    return eps_mid, best


def _scene(gq, B):
    """inputs, best iterations and the mid-way eps of a batch, computed once per batch size.  The 8 rows are eight
    consecutive rows of the 260: a batch stops when its SLOWEST row has converged, and eight rows on their own stop two
    or three iterations early, so the eight are taken around a slow row of the large batch."""
    if B in _CACHE:
        return _CACHE[B]
    s = _Case()
    if B == 260:
        s.pts, s.nrm, s.cog = _contacts(gq, B)
        rows = slice(0, B)
    else:
        big = _scene(gq, 260)
        rows, best = None, -1
        for r0 in range(0, 260 - B + 1, B):
            Fc = big.F[r0:r0 + B].contiguous()
            if _qp_stop(gq, Fc, EPS_DEFAULT, 3)[0] >= MAX_ITER - 1:
                score = _mid_eps(gq, Fc, big.bi_a[r0:r0 + B])[1]
                if score > best:
                    rows, best = slice(r0, r0 + B), score
        assert rows is not None, "no eight consecutive rows run to the last iterations at the default eps"
        s.pts, s.nrm, s.cog = big.pts[rows], big.nrm[rows], big.cog[rows]
    _, _, _, _, s.F = _fc_step(gq, s.pts, s.nrm, s.cog, EPS_DEFAULT)
    n_all, s.bi_all = _qp_stop(gq, s.F, 0.0, 1000)  # no stop condition can fire: the best iteration over all of them ...
    n_a, s.bi_a = _qp_stop(gq, s.F, 0.0, 1000, MAX_ITER - 1)  # ... and over all but the last: the slot's
    assert n_all == MAX_ITER and n_a == MAX_ITER - 1
    s.eps_mid, _ = _mid_eps(gq, s.F, s.bi_a)
    assert s.eps_mid is not None, "no eps stops the rule mid-way with a margin and rows on both sides"
    _CACHE[B] = s
    return s


def _oracle(s, eps, dtype):
    p = s.pts.to(dtype).clone().requires_grad_()
    kw = dict(mu=FC["friction"], k=K, max_limit=FC["max_limit"], torque_weight=FC["torque_weight"], eps=eps, maxIter=MAX_ITER,
              box_form=True)
    val, svd, x, F = ospan.span_metric(p, s.nrm.to(dtype), s.cog.to(dtype), **kw)
    e = FC["values_gain"] * (val + 1e-2) * torch.exp(-FC["svd_gain"] * svd)
    e.sum().backward()
    Fx = (F @ x.unsqueeze(-1)).squeeze(-1)
    return e.detach().double().numpy(), Fx.detach().double().numpy(), p.grad.double().numpy()


def _row_err(a, ref):
    return np.abs(a - ref).max(-1) / np.abs(ref).max(-1)


@pytest.mark.parametrize("B", [8, 260])
@pytest.mark.parametrize("case", ["default", "huge", "mid"])
def test_tail_commit_and_fallback(gq, B, case):
    s = _scene(gq, B)
    eps = {"default": EPS_DEFAULT, "huge": EPS_HUGE, "mid": s.eps_mid}[case]
    e, x, g, n_iter, _ = _fc_step(gq, s.pts, s.nrm, s.cog, eps)
    ks, last = n_iter - 1, MAX_ITER - 1
    from_last = (s.bi_all == last) if ks == last else np.zeros(B, dtype=bool)
    from_slot = ~from_last & (s.bi_a <= ks)
    n_last, n_slot, n_redo = int(from_last.sum()), int(from_slot.sum()), int((~from_last & ~from_slot).sum())
    print(f"B={B} {case}: eps {eps:.3g} n_iter {n_iter} rows served by the last snapshot {n_last} / the slot {n_slot} / "
          f"the table {n_redo}; best iteration of the rows, histogram {np.bincount(s.bi_all, minlength=MAX_ITER).tolist()}")
    if case == "default":
        assert ks >= last - 1 and n_redo == 0, f"default eps: k* = {ks}, {n_redo} rows go back to the table"
    elif case == "huge":
        assert n_iter == 1 and n_redo == int((s.bi_a > 0).sum()) and n_redo > 0
    else:
        assert 2 <= ks <= MAX_ITER - 3 and n_redo > 0 and n_slot > 0, (ks, n_redo, n_slot)
    # x, sharp: the library's box QP on the same F at the same eps runs the same PDIPM loop and selects each row's best
    # iterate among 0..k* from the snapshot table by itself.  The step's x must be that iterate: 1e-6 of the row's
    # largest entry leaves room for nothing but a different rounding of the same arithmetic in the two kernels, while
    # neighbouring snapshots differ by 1e-3 and more.
    n_qp, _ = _qp_stop(gq, s.F, eps, 3)
    x_qp = _qp_stop.x.cpu().double().numpy()
    dx = _row_err(x.numpy(), x_qp)
    print(f"   x against the box QP's own best iterate: rows bit-identical {int((dx == 0).sum())} of {B}, max row err {dx.max():.3g}")
    assert n_qp == n_iter
    assert dx.max() <= 1e-6, f"x B={B} {case}: row {int(dx.argmax())} is not the best iterate among 0..k* ({dx.max():.3g})"
    # against the fp64 oracle: E_fc, F x (the well-determined part of x: F fixes 6 directions of the 48, the ridge 1e-4
    # the rest) row by row, each under the rule of _parity.py with its default bounds
    e64, fx64, g64 = _oracle(s, eps, torch.float64)
    e32, fx32, g32 = _oracle(s, eps, torch.float32)
    Fx = (s.F.cpu().double() @ x.unsqueeze(-1)).squeeze(-1).numpy()
    rowg = lambda a: np.linalg.norm((a - g64).reshape(B, -1), axis=1) / np.linalg.norm(g64.reshape(B, -1), axis=1)
    re_, rf, rg = rel_err(e.numpy(), e64), _row_err(Fx, fx64), rowg(g.numpy())
    ne, nf, ng = rel_err(e32, e64), _row_err(fx32, fx64), rowg(g32)
    print(f"   E_fc rel err median {np.median(re_):.3g} max {re_.max():.3g} (oracle fp32 noise max {ne.max():.3g}); "
          f"F x row err median {np.median(rf):.3g} max {rf.max():.3g} (noise max {nf.max():.3g}); "
          f"gradient row err median {np.median(rg):.3g} max {rg.max():.3g} (noise max {ng.max():.3g})")
    assert_tail_within_fp32_noise(re_, ne, f"E_fc B={B} {case}")
    assert_tail_within_fp32_noise(rf, nf, f"F x B={B} {case}")
    # the gradient: the batch bound of test_gpu_parity.py, and row by row the rule of _parity.py, under that same 2e-2 as ceiling, on
    # the rows this oracle can judge singly -- those on which its own fp32 run stays under the rule's ceiling.  (The
    # gradient passes through the KKT solve at the iterate; on the rows near a change of the active set the oracle's fp32
    # run is off by 1e-1 and more from its fp64 run.  Those rows are held by x above, of which the gradient is a function.)
    ge = np.linalg.norm(g.numpy() - g64) / np.linalg.norm(g64)
    stable = ng < 5e-3
    print(f"   gradient: batch {ge:.3g}; rows the oracle judges singly {int(stable.sum())} of {B}, max row err on them {rg[stable].max():.3g}")
    assert ge < 2e-2, ge
    assert stable.sum() >= B // 2
    assert_tail_within_fp32_noise(rg[stable], ng[stable], f"gradient B={B} {case}", ceiling=2e-2)  # the gradient's own bound
