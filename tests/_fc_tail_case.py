"""One gq_fc_step launch on recorded contacts with every output of the tail kept -- shared by
tools/make_golden_fc_tail.py (which records the parent's bits) and tests/test_gpu_fc_tail_candidates.py."""
import numpy as np
import torch

N, K = 12, 4
FC = dict(friction=0.2, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0)
W_DIS, W_FC = 0.5, 1.0  # w_dis != 0: the tail ADDS its part to the head's E_dis gradient
SENTINEL = 12345.0
OUTPUTS = ("e_fc", "val", "svd", "x", "x_sum", "g_cpts", "n_iter")


def run(gq, pts, nrm, cog, eps, max_iter):
    """gq_fc_step on B rows -> dict of numpy arrays (OUTPUTS) + F.  e_fc, x_sum and the workspace's x, val, svd are
    pre-filled with SENTINEL; g_cpts is the head's E_dis part plus the tail's E_fc part.  The launch is that of
    tests/_fc_step_case.py::run at these settings, with its guard rows."""
    import _fc_step_case as fsc

    assert fsc.SENTINEL == SENTINEL
    d2, sgn, obj_dir, closest, hand_n = fsc.plain_contact_inputs(pts, nrm)
    out = fsc.run(gq, N, K, FC, eps, max_iter, W_DIS, W_FC, d2, sgn, obj_dir, closest, pts, hand_n, cog)
    return {k: out[k] for k in OUTPUTS + ("F",)}


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
