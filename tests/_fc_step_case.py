"""One gq_fc_step launch with every parameter open and every output kept, and the scenes of
tests/test_gpu_fc_step_routes.py (plain torch + the oracle; the launch itself needs the GPU).

run() is the parametrised form of tests/_fc_tail_case.py::run, which delegates to it.  Every output the caller owns is
allocated with ONE GUARD ROW beyond the B rows the call is told of and pre-filled with SENTINEL, as are the workspace's x,
val and svd (without a guard row: the library lays the workspace out); 256 guard bytes follow the workspace.  After the
launch no sentinel may be left in a row < B and every guard must be untouched: a head block or a tail that runs a row
>= B, or a row that nobody stores, shows here whatever the test compares afterwards.
"""
import ctypes

import numpy as np
import torch

FC_DEFAULT = dict(friction=0.2, torque_weight=5.0, max_limit=20.0, svd_gain=0.1, values_gain=2.0)
SENTINEL = 12345.0
WS_GUARD = 256  # bytes behind the workspace
WS_GUARD_BYTE = 0xA5
OUTPUTS = ("e_fc", "val", "svd", "x", "x_sum", "obj_normal", "g_cpts", "g_cnrm", "n_iter")


def _view(ws, ptr, count):
    off = int(ptr.value) - ws.data_ptr()
    return ws[off:off + 4 * count].view(torch.float32)


class Workspace:
    """a zero-filled fc workspace (zeroed ONCE: the head's block counter must return to zero by itself) + guard bytes"""

    def __init__(self, gq, B, n, k, max_iter):
        self.key = (B, n, k, max_iter)
        self.nb = gq._size_call("gq_fc_workspace_bytes", ctypes.c_int64(B), n, k, max_iter)
        self.buf = gq._ws(self.nb + WS_GUARD, torch.device("cuda"))
        self.buf[:self.nb].zero_()
        self.buf[self.nb:].fill_(WS_GUARD_BYTE)


def run(gq, n, k, fc, eps, max_iter, w_dis, w_fc, dist_sq, sign, obj_dir, closest, pts, hand_normals, cog, ws=None):
    """gq_fc_step on B rows -> dict of numpy arrays (OUTPUTS, rows < B) + "F" (device tensor) + "ws" (the Workspace, to
    launch again on it).  Raises AssertionError when a sentinel is left in a row < B or a guard was written."""
    from graspqp_amd import _C

    B = pts.shape[0]
    f = lambda t: torch.as_tensor(t).float().cuda().contiguous()
    d2, od, cl, p, hn, cg = f(dist_sq), f(obj_dir), f(closest), f(pts), f(hand_normals), f(cog)
    sg = torch.as_tensor(sign).to(torch.int32).cuda().contiguous()
    assert d2.shape == sg.shape == (B, n) and p.shape == od.shape == cl.shape == hn.shape == (B, n, 3) and cg.shape == (B, 3)
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")
    obj_normal, g_cpts, g_cnrm = full(B + 1, n, 3), full(B + 1, n, 3), full(B + 1, n, 3)
    e, xs = full(B + 1), full(B + 1, n)
    nit = torch.tensor([-1, -7], dtype=torch.int32, device="cuda")  # second word: guard
    if ws is None:
        ws = Workspace(gq, B, n, k, max_iter)
    assert ws.key == (B, n, k, max_iter)
    Fp, xp, vp, sp = gq.fc_peek(ws.buf[:ws.nb], B, n, k)
    x, val, svd = _view(ws.buf, xp, B * n * k), _view(ws.buf, vp, B), _view(ws.buf, sp, B)
    for t in (x, val, svd):
        t.fill_(SENTINEL)
    _C.call("gq_fc_step", _C.f32(d2), _C.i32(sg), _C.f32(od), _C.f32(cl), _C.f32(p), _C.f32(hn), _C.f32(cg), B, n, k,
            fc["friction"], fc["torque_weight"], fc["max_limit"], fc["svd_gain"], fc["values_gain"], float(eps), int(max_iter),
            float(w_dis), float(w_fc), _C.f32(obj_normal), _C.f32(g_cpts), _C.f32(g_cnrm), _C.f32(e), _C.f32(xs), _C.i32(nit),
            _C.ptr(ws.buf), ws.nb, _C.stream_ptr())
    torch.cuda.synchronize()
    dev = {"e_fc": e, "x_sum": xs, "obj_normal": obj_normal, "g_cpts": g_cpts, "g_cnrm": g_cnrm}
    for name, t in dev.items():
        assert bool((t[B] == SENTINEL).all()), f"{name}: the guard row behind the {B} rows was written"
        left = (t[:B] == SENTINEL).reshape(B, -1).any(1)
        assert not bool(left.any()), f"{name}: the sentinel is left in rows {torch.nonzero(left).flatten().tolist()[:8]}"
    for name, t in (("x", x.view(B, n * k)), ("val", val.view(B, 1)), ("svd", svd.view(B, 1))):
        left = (t == SENTINEL).any(1)
        assert not bool(left.any()), f"{name}: the sentinel is left in rows {torch.nonzero(left).flatten().tolist()[:8]}"
    assert int(nit[1].item()) == -7, "n_iter: the word behind it was written"
    assert bool((ws.buf[ws.nb:] == WS_GUARD_BYTE).all()), "the bytes behind the workspace were written"
    out = {"e_fc": e[:B], "val": val, "svd": svd, "x": x.view(B, n * k), "x_sum": xs[:B], "obj_normal": obj_normal[:B],
           "g_cpts": g_cpts[:B], "g_cnrm": g_cnrm[:B], "n_iter": nit[:1]}
    out = {name: t.detach().cpu().numpy().copy() for name, t in out.items()}
    out["F"] = _view(ws.buf, Fp, B * 6 * n * k).view(B, 6, n * k).clone()
    out["ws"] = ws
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def plain_contact_inputs(pts, nrm):
    """the contact-term inputs of a contact that touches: sign +1, one distance, the hand normal opposite to the object's
    -> (dist_sq, sign, obj_dir, closest, hand_normals) for run()"""
    p, nr = torch.as_tensor(pts).float(), torch.as_tensor(nrm).float()
    B, n = p.shape[:2]
    return torch.full((B, n), 1e-4), torch.ones(B, n, dtype=torch.int32), nr, p - 0.01 * nr, -nr


# ---------------------------------------------------------------------------------------------------------------
# section 1: general contact-term inputs around contacts of _scenes.hetero_contacts
# ---------------------------------------------------------------------------------------------------------------
def general_contact_inputs(pts, nrm, seed):
    """Contact-term inputs in general position for the contacts (pts, nrm = OUTWARD object normals), every value fp32-exact
    in fp64 -> dict(dist_sq, sign, obj_dir, closest, hand_normals):

      sign          +-1, mixed within every row (contact outside / inside the object)
      obj_dir       sign * nrm: unit vectors of either orientation; the outward normal the step has to form is sign * obj_dir
      dist_sq       log-uniform in [1e-10, 1e-3], one contact in eight exactly 0
      hand_normals  random unit vectors, unrelated to the object's
      closest       pts - sign * sqrt(dist_sq) * obj_dir + a tangential offset of 1e-4 .. 3e-4 (never zero)
    """
    g = torch.Generator().manual_seed(seed)
    B, n, _ = pts.shape
    dt = torch.float64
    sign = torch.where(torch.rand(B, n, generator=g) < 0.5, -1, 1).to(torch.int32)
    sign[:, 0], sign[:, 1] = 1, -1  # mixed within every row whatever the draw
    sg = sign.to(dt).unsqueeze(-1)
    obj_dir = (sg * nrm.to(dt)).float().to(dt)
    d2 = 10.0 ** (-10.0 + 7.0 * torch.rand(B, n, generator=g, dtype=dt))
    d2[torch.rand(B, n, generator=g) < 0.125] = 0.0
    d2[:, 2] = 0.0  # an exact zero in every row
    d2 = d2.float().to(dt)
    hand = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g, dtype=dt), dim=-1).float().to(dt)
    t = torch.linalg.cross(obj_dir, torch.randn(B, n, 3, generator=g, dtype=dt), dim=-1)
    t = torch.nn.functional.normalize(t, dim=-1) * (1e-4 + 2e-4 * torch.rand(B, n, 1, generator=g, dtype=dt))
    closest = (pts.to(dt) - sg * d2.sqrt().unsqueeze(-1) * obj_dir + t).float().to(dt)
    return dict(dist_sq=d2, sign=sign, obj_dir=obj_dir, closest=closest, hand_normals=hand)


def contact_term_closed_form(c, pts, w_dis, dtype):
    """w_dis dE_dis/dp and w_dis dE_dis/dnH of csrc/fc_dev.h::gq_contact_term in ``dtype`` on the CPU:
    e = exp(1 + vC.nH), root = sqrt(d2 + 1e-8), g_p = w e / root (p - closest), g_n = w e root vC, vC = sign * obj_dir"""
    d2, od, cl, hn, p = (t.to(dtype) for t in (c["dist_sq"], c["obj_dir"], c["closest"], c["hand_normals"], pts))
    vC = c["sign"].to(dtype).unsqueeze(-1) * od
    e = torch.exp(1.0 + (vC * hn).sum(-1, keepdim=True))
    root = torch.sqrt(d2 + 1e-8).unsqueeze(-1)
    return w_dis * e / root * (p - cl), w_dis * e * root * vC


# ---------------------------------------------------------------------------------------------------------------
# section 2: a batch of copies of an early row E with one late row H somewhere
# ---------------------------------------------------------------------------------------------------------------
STOP_SHAPES = ((12, 4), (13, 5))
STOP_EPS, STOP_MAX_ITER = 5e-2, 12
_stop_scene = {}


def oracle_fc(pts, nrm, cog, k, eps, max_iter, dtype, fc=FC_DEFAULT):
    """the oracle's E_fc with the step's constant upstream 1 -> (e, d e.sum() / d pts, x_sum, n_iter), fp64 numpy"""
    from ref_cpu import qp as oqp
    from ref_cpu import span as ospan

    p = pts.to(dtype).clone().requires_grad_()
    e, xs = ospan.e_fc(p, nrm.to(dtype), cog.to(dtype), svd_gain=fc["svd_gain"], values_gain=fc["values_gain"], k=k,
                       mu=fc["friction"], torque_weight=fc["torque_weight"], max_limit=fc["max_limit"], eps=eps,
                       maxIter=max_iter, box_form=True)
    n_iter = int(oqp.LAST["n_iter"])
    e.sum().backward()
    return e.detach().double().numpy(), p.grad.double().numpy(), xs.detach().double().numpy(), n_iter


def stop_scene(n, k):
    """(pts, nrm, cog) of two rows [E, H] of hetero_contacts(64, n, 9000 + n k), rounded to fp32: E has the smallest
    stand-alone n_iter of the 64 (fp64 oracle, default eps and maxIter), H the largest that is still < maxIter.
    -> (pts (2,n,3), nrm, cog (2,3), n_iter of E alone, n_iter of H alone)"""
    if (n, k) not in _stop_scene:
        from _scenes import hetero_contacts

        pts, nrm, cog = (t.float().double() for t in hetero_contacts(64, n, seed=9000 + n * k))
        alone = np.array([oracle_fc(pts[r:r + 1], nrm[r:r + 1], cog[r:r + 1], k, STOP_EPS, STOP_MAX_ITER, torch.float64)[3]
                          for r in range(64)])
        e_row = int(alone.argmin())
        late = np.where(alone < STOP_MAX_ITER, alone, -1)
        h_row = int(late.argmax())
        rows = [e_row, h_row]
        _stop_scene[(n, k)] = (pts[rows], nrm[rows], cog[rows], int(alone[e_row]), int(alone[h_row]))
    return _stop_scene[(n, k)]
