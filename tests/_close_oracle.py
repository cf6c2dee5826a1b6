"""Finger closing (include/graspqp_hip.h, "finger closing") written in torch on top of tests/_scene_oracle.py: the kinematics and the
samples of ``hand_oracle``, the grid's own trilinear interpolant of ``phi`` / ``locate`` (the analytic shape is never the
reference), the direction, the per-link minimum with the lowest-index tie-break, touch, stop masks and the clamped update.
Everything runs in the dtype asked for: float64 is the oracle, float32 the oracle's own rounding noise.  The inputs the device
holds in float32 (step, joint limits, direction, pose) are rounded to float32 first, in either dtype.  Nothing here needs a GPU."""
import numpy as np
import torch

import ref_cpu  # noqa: F401
from ref_cpu import kin

import _scene_oracle as so
from _scene_oracle import FACE, NEAR  # noqa: F401
from graspqp_amd import ops


def direction_delta(v, step):
    """(B,JA) command, (JA) step -> (B,JA) increments: u = v / step, m = max |u|, Delta = step u / m; a row with m = 0 or with a
    non-finite u does not move."""
    u = v / step
    m = u.abs().amax(1)
    ok = torch.isfinite(u).all(1) & (m > 0)
    safe = torch.where(ok, m, torch.ones_like(m))
    return torch.where(ok[:, None], step * (u / safe[:, None]), torch.zeros_like(u))


def link_minima(ph, lnk, L):
    """ph (B,Ns) with +inf where a sample takes no part -> (m (B,L), index (B,L) with -1, second (B,L) the second smallest value)."""
    B = ph.shape[0]
    m = torch.full((B, L), float("inf"), dtype=ph.dtype)
    second = torch.full((B, L), float("inf"), dtype=ph.dtype)
    idx = np.full((B, L), -1, np.int64)
    for l in range(L):
        cols = np.nonzero(lnk == l)[0]
        if cols.size == 0:
            continue
        v = ph[:, cols]
        ml = v.min(1).values
        first = np.argmax((v == ml[:, None]).numpy(), axis=1)  # numpy: the first occurrence, i.e. the lowest sample index
        has = ml < float("inf")  # the test grids hold finite values: +inf is "no sample takes part"
        m[:, l] = ml
        idx[:, l] = np.where(has.numpy(), cols[first], -1)
        if cols.size > 1:
            second[:, l] = v.topk(2, dim=1, largest=False).values[:, 1]
    return m, idx, second


def sample_world(oh, theta, R, t):
    """-> (x (B,Ns,3) world positions of the samples, T (B,L,4,4) link transforms) at the actuated joints theta"""
    T = oh.fk(theta)
    Tl = T[:, torch.as_tensor(oh.surface_link, dtype=torch.long)]
    c = torch.as_tensor(oh.surface_points, dtype=theta.dtype)
    xh = (Tl[..., :3, :3] @ c[None, :, :, None]).squeeze(-1) + Tl[..., :3, 3]
    return xh @ R.transpose(1, 2) + t[:, None], T


def stack_phi(fields, x):
    """phi (B,Ns) of the rows' own grids (row b reads fields[b // (B / G)]), +inf where the sample takes no part"""
    B, G = x.shape[0], len(fields)
    assert B % G == 0
    rows = B // G
    ph = torch.cat([so.phi(fields[g], x[g * rows:(g + 1) * rows], use_grid=True) for g in range(G)], 0)
    return torch.where(torch.isfinite(ph) | (ph == float("-inf")), ph, torch.full_like(ph, float("inf")))


def close(spec, pts, lnk, hp, direction, fields, S, step, tau, dtype=torch.float64):
    """The procedure on (B,9+JA) poses -> dict of numpy arrays.  Final state: theta (B,JA), touch_step (B,L), joint_stop (B,JA), phi
    (B,L), sample (B,L), point (B,L,3), normal (B,L,3).  For the guards and the hand-computed facts: M (S+1,B,L) every evaluated m_l,
    thetas (S+1,B,JA), T (S+1,B,L,4,4), second (B,L) the second smallest phi of the link at the final state, face (B,L) the distance
    of the point's coordinates to the nearest cell face in cell units, delta (B,JA)."""
    lnk = np.asarray(lnk)
    oh = so.hand_oracle(spec, pts, lnk, dtype)
    hp = hp.detach().float().to(dtype)
    B, JA, L = hp.shape[0], spec.n_dofs, spec.n_links
    R, t = kin.special_gramschmidt(hp[:, 3:9]), hp[:, :3]
    theta = hp[:, 9:].clone()
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dtype)
    step_t, lo, hi = f32(step), f32(spec.joints_lower), f32(spec.joints_upper)
    delta = direction_delta(direction.detach().float().to(dtype), step_t)
    bits = ops.close_stop_masks_host(spec)
    masks = torch.tensor([[bool((int(bits[a]) >> l) & 1) for l in range(L)] for a in range(JA)])
    touched = torch.zeros(B, L, dtype=torch.bool)
    tstep = torch.full((B, L), -1, dtype=torch.long)
    jstop = torch.full((B, JA), -1, dtype=torch.long)
    Ms, thetas, Ts = [], [], []
    for s in range(S + 1):
        x, T = sample_world(oh, theta, R, t)
        m, idx, second = link_minima(stack_phi(fields, x), lnk, L)
        Ms.append(m), thetas.append(theta.clone()), Ts.append(T)
        new = ~touched & (m <= tau)
        tstep = torch.where(new, torch.full_like(tstep, s), tstep)
        touched = touched | new
        stopped = (touched[:, None, :] & masks[None]).any(-1)
        jstop = torch.where(stopped & (jstop < 0), torch.full_like(jstop, s), jstop)
        if s < S:
            nt = torch.minimum(torch.maximum(theta + delta, lo), hi)
            theta = torch.where(stopped | (delta == 0), theta, nt)
    # the final state: x, m, idx, second are those of evaluation S
    has = idx >= 0
    pick = torch.as_tensor(np.where(has, idx, 0))
    point = torch.gather(x, 1, pick[..., None].expand(B, L, 3))
    pg = point.clone().requires_grad_()
    G, rows = len(fields), B // len(fields)
    val = torch.cat([so.phi(fields[g], pg[g * rows:(g + 1) * rows], use_grid=True) for g in range(G)], 0)
    hast = torch.as_tensor(has)
    torch.where(hast, val, torch.zeros_like(val)).sum().backward()
    grad = torch.where(hast[..., None], pg.grad, torch.zeros_like(pg.grad))
    norm = grad.norm(dim=-1, keepdim=True)
    normal = torch.where(norm > 0, grad / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(grad))
    face = np.full((B, L), np.inf)
    for g in range(G):
        u = so.locate(fields[g], point[g * rows:(g + 1) * rows])[3]
        face[g * rows:(g + 1) * rows] = (u - u.round()).abs().amin(-1).numpy()
    point = torch.where(hast[..., None], point, torch.zeros_like(point))
    n64 = lambda a: a.double().numpy()
    return dict(theta=n64(theta), touch_step=tstep.numpy(), joint_stop=jstop.numpy(), phi=n64(m), sample=idx, point=n64(point),
                normal=n64(normal), M=n64(torch.stack(Ms)), thetas=n64(torch.stack(thetas)), T=n64(torch.stack(Ts)), second=n64(second),
                face=np.where(has, face, np.inf), delta=n64(delta), masks=masks.numpy())


def undecidable(ref, tau):
    """(B) bool: rows where some evaluated |m_l - tau|, up to and including the link's first touch, is below NEAR -- one flipped
    touch changes everything after it."""
    M, ts = ref["M"], ref["touch_step"]
    s = np.arange(M.shape[0])[:, None, None]
    before = (ts[None] < 0) | (s <= ts[None])
    with np.errstate(invalid="ignore"):
        close_call = np.isfinite(M) & (np.abs(M - tau) < NEAR)
    return (before & close_call).any(axis=(0, 2))
