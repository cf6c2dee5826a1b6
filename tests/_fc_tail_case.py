"""One gq_fc_step launch on recorded contacts with every output of the tail kept -- shared by
tools/make_golden_fc_tail.py (which records the parent's bits) and tests/test_gpu_fc_tail_candidates.py."""
import ctypes

import numpy as np
import torch

N, K = 12, 4
FC = dict(friction=0.2, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0)
W_DIS, W_FC = 0.5, 1.0  # w_dis != 0: the tail ADDS its part to the head's E_dis gradient
SENTINEL = 12345.0
OUTPUTS = ("e_fc", "val", "svd", "x", "x_sum", "g_cpts", "n_iter")


def _view(ws, ptr, count):
    off = int(ptr.value) - ws.data_ptr()
    return ws[off:off + 4 * count].view(torch.float32)


def run(gq, pts, nrm, cog, eps, max_iter):
    """gq_fc_step on B rows -> dict of numpy arrays (OUTPUTS) + F.  e_fc, x_sum and the workspace's x, val, svd are
    pre-filled with SENTINEL; g_cpts is the head's E_dis part plus the tail's E_fc part."""
    from graspqp_amd import _C

    B = pts.shape[0]
    f = lambda t: torch.as_tensor(t).float().cuda().contiguous()
    p, nr, cg = f(pts), f(nrm), f(cog)
    d2 = torch.full((B, N), 1e-4, device="cuda")
    sgn = torch.ones(B, N, dtype=torch.int32, device="cuda")
    closest = (p - 0.01 * nr).contiguous()
    hand_n = (-nr).contiguous()
    obj_normal, g_cpts, g_cnrm = (torch.full_like(p, SENTINEL) for _ in range(3))
    e = torch.full((B,), SENTINEL, device="cuda")
    xs = torch.full((B, N), SENTINEL, device="cuda")
    nit = torch.zeros(1, dtype=torch.int32, device="cuda")
    nb = gq._size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), N, K, max_iter)
    ws = gq._ws(nb, p.device).zero_()
    Fp, xp, vp, sp = gq.fc_peek(ws, B, N, K)
    x, val, svd = _view(ws, xp, B * N * K), _view(ws, vp, B), _view(ws, sp, B)
    for t in (x, val, svd):
        t.fill_(SENTINEL)
    _C.call("gq_fc_step", _C.f32(d2), _C.i32(sgn), _C.f32(nr), _C.f32(closest), _C.f32(p), _C.f32(hand_n), _C.f32(cg), B, N, K,
            FC["friction"], FC["torque_weight"], FC["max_limit"], FC["svd_gain"], FC["values_gain"], float(eps), int(max_iter),
            W_DIS, W_FC, _C.f32(obj_normal), _C.f32(g_cpts), _C.f32(g_cnrm), _C.f32(e), _C.f32(xs), _C.i32(nit), _C.ptr(ws), nb,
            _C.stream_ptr())
    torch.cuda.synchronize()
    out = {"e_fc": e, "val": val, "svd": svd, "x": x.view(B, N * K), "x_sum": xs, "g_cpts": g_cpts, "n_iter": nit}
    out = {k: v.detach().cpu().numpy().copy() for k, v in out.items()}
    out["F"] = _view(ws, Fp, B * 6 * N * K).view(B, 6, N * K).clone()
    return out


def best_iterations(gq, F, max_iter):
    """per-row best iteration among 0 .. max_iter - 1 (no stop condition can fire), from the library's own box QP on the
    step's grasp matrix, as tests/test_gpu_fc_tail_slot.py derives it"""
    from graspqp_amd import _C

    B, m, nz = F.shape
    x = torch.empty(B, nz, device="cuda")
    lam, slack = torch.empty(B, 2 * nz, device="cuda"), torch.empty(B, 2 * nz, device="cuda")
    bi = torch.zeros(B, dtype=torch.int32, device="cuda")
    nit = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws, nb = gq._qp_ws(B, nz, max_iter, F.device)
    _C.call("gq_lsq_boxqp_forward", _C.f32(F), None, None, None, 1.0, FC["max_limit"] + 1.0, B, m, nz, 1e-4, 0.0,
            int(max_iter), 1000, _C.f32(x), _C.f32(lam), _C.f32(slack), _C.i32(bi), _C.i32(nit), _C.ptr(ws), nb, _C.stream_ptr())
    torch.cuda.synchronize()
    assert int(nit.item()) == max_iter
    return bi.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
