"""The pre-grasp term's contract (include/graspqp_hip.h, "pre-grasp clearance") written in torch on top of tests/_scene_oracle.py:
the joints are opened to theta_o = (1 - alpha) theta + alpha q_o, root pose and R unchanged; station k = 0..K is the opened hand
moved back by d_k = D k / K along R a (K = 0: the one station d = 0), E_pregrasp = 1/(K+1) sum_k sum_s max(margin - phi, 0).
Autograd runs to hand_pose THROUGH the opened pose.  Everything runs in the dtype of its inputs (float64 for the oracle)."""
import numpy as np
import torch

from _scene_oracle import FACE, NEAR, hand_oracle, locate, phi


def opened_pose(hp, open_joints, opening):
    """(B,D) hand_pose -> the pose of the opened hand: the first nine entries as they are, the joints (1 - alpha) theta + alpha q_o;
    differentiable w.r.t. hp."""
    q = torch.as_tensor(np.asarray(open_joints, dtype=np.float64), dtype=hp.dtype)
    return torch.cat([hp[:, :9], (1.0 - opening) * hp[:, 9:] + opening * q[None]], dim=1)


def station_points(oh, D, K):
    """(B,K+1,Ns,3) world positions of the surface samples of the oracle hand (already at the opened pose) at the stations
    k = 0..K."""
    x = oh.get_surface_points()  # (B,Ns,3)
    back = oh.global_rotation @ oh.grasp_axis.to(x.dtype)  # (B,3): R a
    d = D * torch.arange(0, K + 1, dtype=x.dtype) / max(K, 1)
    return x[:, None] - d[None, :, None, None] * back[:, None, None, :]


def e_pregrasp(spec, pts, lnk, hp, open_joints, opening, field, margin, D, K, scale=3.0, dtype=torch.float64):
    """-> dict: E (B) E_pregrasp, grad (B,D) d (scale sum E) / d hand_pose, and per station point (B,K+1,Ns): phi, inside, active,
    face (distance of the coordinates to the nearest cell face, in cell units); x (B,K+1,Ns,3).  What _approach_oracle.e_approach
    returns, with K + 1 stations."""
    oh = hand_oracle(spec, pts, lnk, dtype)
    hp = hp.detach().to(dtype).clone().requires_grad_()
    oh.set_parameters(opened_pose(hp, open_joints, opening), torch.zeros(hp.shape[0], 1, dtype=torch.long))
    x = station_points(oh, D, K)
    p = phi(field, x)
    inside, _, _, u = locate(field, x.detach())
    hinge = torch.where(inside, torch.relu(margin - torch.where(inside, p, torch.zeros_like(p))), torch.zeros_like(p))
    E = hinge.sum((-1, -2)) / (K + 1)
    if E.requires_grad:
        (scale * E).sum().backward()
    ud = u.detach()
    face = (ud - ud.round()).abs().amin(-1)
    pd = p.detach()
    g = hp.grad
    return dict(E=E.detach().numpy(), grad=(torch.zeros_like(hp) if g is None else g).detach().numpy(), phi=pd.numpy(),
                inside=inside.numpy(), active=(inside & (pd < margin)).numpy(), face=face.numpy(), x=x.detach().numpy())


def guards(res, margin):
    """The two conditions on the INPUTS over all B Ns (K+1) station points: -> (nearest cell face in cell units, to be held
    against FACE; nearest |phi - margin| of the points inside the volume, against NEAR)."""
    ins = res["inside"]
    near = np.abs(res["phi"][ins] - margin).min() if ins.any() else np.inf
    return float(res["face"].min()), float(near)


__all__ = ["FACE", "NEAR", "opened_pose", "station_points", "e_pregrasp", "guards"]
