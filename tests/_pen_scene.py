"""The scene of test_gpu_parity.py::test_hand_penetration_and_self_penetration with P = 1024 surface points per object, and
the fp64 oracle of the hand-penetration query PER POINT on it: the distance, the winning link, the second-best link's
distance and the gradient d dis / d x_h in the hand frame -- for tests/test_gpu_pen_backward.py.

Run as a script (python tests/_pen_scene.py) it measures the nudge baseline that test uses: the oracle's own
(dis, link, gvec), cast to fp32, at the surface points and at the points moved by 3e-6 m (the fp32 position noise) in random
directions, both fed to the fp64 backward oracle of tests/_pen_backward_oracle.py; printed is the norm-wise difference of
the two (wrench, gRt) results."""
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":
    _root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    sys.path[:0] = [_root, os.path.join(_root, "oracle"), os.path.dirname(os.path.abspath(__file__))]

from ref_cpu import models as omodels  # noqa: E402
from ref_cpu import sdf as osdf  # noqa: E402

from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

N_OBJ, BE, P = 2, 3, 1024


def scene():
    """-> spec, face-vertex lists, surface points (n_obj,P,3) fp32, hand_pose (B,D) fp32, contact indices."""
    spec = get_hand_spec("allegro")
    B = N_OBJ * BE
    fvs = [meshes.icosphere(2, 0.05), meshes.superquadric(5, 24, 12)]
    sps = np.stack([meshes.surface_points(f, P, oversample=4) for f in fvs]).astype(np.float32)
    g = torch.Generator().manual_seed(11)  # _rand_pose(spec, B, 11, spread=0.03) of test_gpu_parity.py
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=g, dtype=torch.float64), dim=-1) * 0.03
    six = torch.randn(B, 6, generator=g, dtype=torch.float64)
    th = torch.tensor(spec.default_state, dtype=torch.float64)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=g, dtype=torch.float64)
    hp = torch.cat([t, six, th], 1)
    hp[:, 9:] += 0.4
    idx = torch.randint(spec.n_contact_candidates, (B, 4), generator=torch.Generator().manual_seed(2))
    return spec, fvs, sps, hp.float(), idx


def point_oracle(spec, hand_pose, idx, x):
    """fp64, at the fp32 pose and the points x (B,P,3) widened to fp64 -> dict of numpy arrays: dis (B,P) = the max over the
    per-link stack of OracleHand.cal_distance, winner (B,P) = its arg-max as a link id, second (B,P) = the runner-up link's
    distance, g_h (B,P,3) = autograd's d dis / d x rotated into the hand frame, g_h = g_x R."""
    oh = omodels.OracleHand(spec, torch.float64)
    oh.set_parameters(hand_pose.double(), idx)
    x = torch.as_tensor(x, dtype=torch.float64).clone().requires_grad_()
    B, N, _ = x.shape
    R = oh.global_rotation
    xh = (x - oh.global_translation.unsqueeze(1)) @ R
    stack, ids = [], []
    for l, fv in enumerate(oh.link_faces):  # the loop of OracleHand.cal_distance, keeping the stack
        if fv.shape[0] == 0:
            continue
        T = oh.current_status[:, l]
        xl = (xh - T[:, :3, 3].unsqueeze(1)) @ T[:, :3, :3]
        d2, sgn, _, _ = osdf.compute_sdf(xl.reshape(-1, 3), fv)
        stack.append((torch.sqrt(d2 + 1e-8) * (-sgn)).reshape(B, N))
        ids.append(l)
    stack = torch.stack(stack, 0)
    dis, arg = stack.max(0)
    assert torch.equal(dis.detach(), oh.cal_distance(x.detach())), "the stack must be the one of OracleHand.cal_distance"
    dis.sum().backward()
    g_h = x.grad @ R.detach()
    top2 = stack.detach().topk(2, dim=0).values
    return {"dis": dis.detach().numpy(), "winner": np.asarray(ids)[arg.numpy()].astype(np.int32), "second": top2[1].numpy(),
            "g_h": g_h.numpy(), "Rg": R.detach().numpy().reshape(B, 9), "n_links": len(oh.link_faces)}


def fp32_triple(o):
    """(dis, link, gvec) of the oracle as the backward kernel reads them; link = 0 and gvec = 0 where nothing penetrates."""
    pos = o["dis"] > 0
    return (o["dis"].astype(np.float32), np.where(pos, o["winner"], 0).astype(np.int32),
            np.where(pos[..., None], o["g_h"], 0.0).astype(np.float32))


def normwise(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def nudge_baseline(seed=0, eps=3e-6):
    import _pen_backward_oracle as pbo

    spec, _, sps, hp, idx = scene()
    x = np.repeat(sps.astype(np.float64), BE, 0)
    d = np.random.default_rng(seed).normal(size=x.shape)
    d *= eps / np.linalg.norm(d, axis=-1, keepdims=True)
    o0, o1 = point_oracle(spec, hp, idx, x), point_oracle(spec, hp, idx, x + d)
    out = []
    for o in (o0, o1):
        dis, link, gvec = fp32_triple(o)
        out.append(pbo.oracle(sps, hp.numpy(), o0["Rg"].astype(np.float32), link, gvec, o0["n_links"], BE, dis=dis, w_pen=100.0))
    both = (o0["dis"] > 1e-5) & (o1["dis"] > 1e-5)
    off = np.abs(o0["dis"][..., None] * o0["g_h"] - o1["dis"][..., None] * o1["g_h"]).max(-1)[both]
    return {"wrench": normwise(out[1][0], out[0][0]), "gRt": normwise(out[1][1], out[0][1]), "penetrating": int((o0["dis"] > 1e-5).sum()),
            "offset_moved_beyond_5e-6": int((off > 5e-6).sum()), "offset_max": float(off.max())}


if __name__ == "__main__":
    import time

    t0 = time.time()
    for s in range(3):
        print(s, nudge_baseline(s), f"{time.time() - t0:.1f} s")
