"""The approach term's contract (include/graspqp_hip.h, "approach clearance") written in torch on top of tests/_scene_oracle.py:
station k = 1..K is the whole hand moved back by d_k = D k / K along R a, E_approach = (1/K) sum_k sum_s max(margin - phi, 0).
Everything runs in the dtype of its inputs (float64 for the oracle)."""
import numpy as np
import torch

from _scene_oracle import FACE, NEAR, hand_oracle, locate, phi


def station_points(oh, D, K):
    """(B,K,Ns,3) world positions of the surface samples at the stations, from the oracle hand's own surface points and
    global_rotation @ grasp_axis; differentiable w.r.t. oh.hand_pose."""
    x = oh.get_surface_points()  # (B,Ns,3)
    back = oh.global_rotation @ oh.grasp_axis.to(x.dtype)  # (B,3): R a
    d = D * torch.arange(1, K + 1, dtype=x.dtype) / K
    return x[:, None] - d[None, :, None, None] * back[:, None, None, :]


def e_approach(spec, pts, lnk, hp, field, margin, D, K, scale=3.0, dtype=torch.float64):
    """-> dict: E (B) E_approach, grad (B,D) d (scale sum E) / d hand_pose, and per station point (B,K,Ns): phi, inside, active,
    face (distance of the coordinates to the nearest cell face, in cell units); x (B,K,Ns,3)."""
    oh = hand_oracle(spec, pts, lnk, dtype)
    hp = hp.detach().to(dtype).clone().requires_grad_()
    oh.set_parameters(hp, torch.zeros(hp.shape[0], 1, dtype=torch.long))
    x = station_points(oh, D, K)
    p = phi(field, x)
    inside, _, _, u = locate(field, x.detach())
    hinge = torch.where(inside, torch.relu(margin - torch.where(inside, p, torch.zeros_like(p))), torch.zeros_like(p))
    E = hinge.sum((-1, -2)) / K
    if E.requires_grad:
        (scale * E).sum().backward()
    ud = u.detach()
    face = (ud - ud.round()).abs().amin(-1)
    pd = p.detach()
    g = oh.hand_pose.grad
    return dict(E=E.detach().numpy(), grad=(torch.zeros_like(hp) if g is None else g).detach().numpy(), phi=pd.numpy(),
                inside=inside.numpy(), active=(inside & (pd < margin)).numpy(), face=face.numpy(), x=x.detach().numpy())


def guards(res, margin):
    """The two conditions on the INPUTS over all B Ns K station points: -> (nearest cell face in cell units, nearest
    |phi - margin| of the points inside the volume)."""
    ins = res["inside"]
    near = np.abs(res["phi"][ins] - margin).min() if ins.any() else np.inf
    return float(res["face"].min()), float(near)


__all__ = ["FACE", "NEAR", "station_points", "e_approach", "guards"]
