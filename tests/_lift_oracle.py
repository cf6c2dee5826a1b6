"""The lift term's contract (include/graspqp_hip.h, "lift clearance") written in torch on top of tests/_scene_oracle.py: station
k = 1..K is the rigid body "hand + held object" carried by (k / K) (H u - D R a),
E_lift = (1/K) sum_k [ sum_s max(m_h - phi(x_w^k), 0) + sum_j max(m_o - phi(x^{j,k}), 0) ].
Everything runs in the dtype of its inputs (float64 for the oracle)."""
import numpy as np
import torch

from _scene_oracle import FACE, NEAR, hand_oracle, locate, phi


def carry(oh, H, D, K, u, dtype):
    """(B,K,3): the translation of station k = 1..K, (k / K) (H u - D R a); differentiable w.r.t. oh.hand_pose through R."""
    back = oh.global_rotation @ oh.grasp_axis.to(dtype)  # (B,3): R a
    s = torch.arange(1, K + 1, dtype=dtype) / K
    uu = torch.as_tensor(np.asarray(u, dtype=np.float64), dtype=dtype)
    return s[None, :, None] * (H * uu[None, None, :] - D * back[:, None, :])


def _hinge(field, x, margin):
    p = phi(field, x)
    inside, _, _, u = locate(field, x.detach())
    h = torch.where(inside, torch.relu(margin - torch.where(inside, p, torch.zeros_like(p))), torch.zeros_like(p))
    ud = u.detach()
    face = (ud - ud.round()).abs().amin(-1) if x.shape[-2] else ud.new_zeros(ud.shape[:-1])
    pd = p.detach()
    return h, dict(phi=pd.numpy(), inside=inside.numpy(), active=(inside & (pd < margin)).numpy(), face=face.numpy(),
                   x=x.detach().numpy())


def e_lift(spec, pts, lnk, hp, fields, m_h, m_o, H, D, K, u, object_points, batch_each, scale=3.0, dtype=torch.float64):
    """``fields``: a Field, or a list of G Fields (row b reads fields[b // (B / G)]); ``object_points`` (n_obj,M,3), object frame,
    M = 0 allowed; row b carries object b // batch_each.  -> dict: E (B), E_object (B) the object's share, grad (B,D)
    d (scale sum E) / d hand_pose, grad_object (B,D) the same of the object's share alone, and ``hand`` / ``object``: per station
    point (B,K,Ns) / (B,K,M) phi, inside, active, face (distance of the coordinates to the nearest cell face, in cell units) and
    x (...,3)."""
    fields = list(fields) if isinstance(fields, (list, tuple)) else [fields]
    oh = hand_oracle(spec, pts, lnk, dtype)
    hp = hp.detach().to(dtype).clone().requires_grad_()
    B = hp.shape[0]
    oh.set_parameters(hp, torch.zeros(B, 1, dtype=torch.long))
    c = carry(oh, H, D, K, u, dtype)  # (B,K,3)
    xh = oh.get_surface_points()[:, None] + c[:, :, None, :]  # (B,K,Ns,3)
    P = torch.as_tensor(np.asarray(object_points, dtype=np.float64), dtype=dtype)
    assert P.dim() == 3 and P.shape[2] == 3 and P.shape[0] * batch_each == B and B % len(fields) == 0
    xo = P.repeat_interleave(batch_each, 0)[:, None] + c[:, :, None, :]  # (B,K,M,3)
    rpg = B // len(fields)
    hh, ho, ih, io = [], [], [], []
    for g, F in enumerate(fields):
        rows = slice(g * rpg, (g + 1) * rpg)
        a, b = _hinge(F, xh[rows], m_h)
        hh.append(a), ih.append(b)
        a, b = _hinge(F, xo[rows], m_o)
        ho.append(a), io.append(b)
    cat = lambda parts: {k: np.concatenate([q[k] for q in parts], 0) for k in parts[0]}
    E_hand, E_obj = torch.cat(hh).sum((-1, -2)) / K, torch.cat(ho).sum((-1, -2)) / K
    E = E_hand + E_obj
    zero = torch.zeros_like(hp)
    g_obj = torch.autograd.grad((scale * E_obj).sum(), hp, retain_graph=True, allow_unused=True)[0] if E_obj.requires_grad else None
    g_all = torch.autograd.grad((scale * E).sum(), hp, allow_unused=True)[0] if E.requires_grad else None
    return dict(E=E.detach().numpy(), E_object=E_obj.detach().numpy(), grad=(zero if g_all is None else g_all).detach().numpy(),
                grad_object=(zero if g_obj is None else g_obj).detach().numpy(), hand=cat(ih), object=cat(io))


def guards(res, m_h, m_o):
    """The conditions on the INPUTS over all B (Ns + M) K station points: -> (nearest cell face in cell units, nearest
    |phi - margin| of the points inside the volume, against the set's own margin)."""
    face, near = np.inf, np.inf
    for part, m in ((res["hand"], m_h), (res["object"], m_o)):
        if part["phi"].size == 0:
            continue
        ins = part["inside"]
        face = min(face, float(part["face"].min()))
        if ins.any():
            near = min(near, float(np.abs(part["phi"][ins] - m).min()))
    return face, near


__all__ = ["FACE", "NEAR", "carry", "e_lift", "guards"]
