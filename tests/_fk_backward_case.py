"""Seeded inputs of one gq_fk_backward call, the call itself through the C ABI and its check against the oracle, shared by
tests/test_gpu_fk_backward_block.py, tests/test_gpu_kinematics_limits.py and tools/make_golden_fk_backward.py (which records
the outputs of a given library).

Inputs are numpy arrays from np.random.RandomState (a frozen stream); the kinematic state (Rg, link_T, node frames) comes
from gq_fk_forward on the same pose, or from the fixture.  Every gradient input and the energy / accept tail are optional,
as in the C ABI."""
import ctypes

import numpy as np
import torch

GRAD_INPUTS = ("g_cpts", "g_cnrm", "g_spheres", "g_wrench", "g_Rt", "g_theta", "g_R")
WEIGHTS = dict(w_dis=100.0, w_fc=1.0, w_pen=100.0, w_spen=10.0, w_joints=1.0)
N_TERMS = 5


def make_inputs(spec, B, n, seed, joint_scale=None):
    """Pose near the default state with some joints beyond their limits (E_joints and its gradient are non-zero), contact
    indices, all seven gradient inputs, the contact records of the energy tail and the accepted state of the accept step.
    joint_scale (JA,): the joint noise and the excursion beyond the limits in units of a +-0.3 rad joint (hands with
    millimetre prismatic joints); None = 1, the stream of draws is the same either way."""
    r = np.random.RandomState(seed)
    f = lambda *s: r.standard_normal(s).astype(np.float32)
    JA = spec.n_dofs  # actuated joints = pose dimension - 9
    L, S, D = spec.n_links, spec.n_spheres, 9 + JA
    t = f(B, 3)
    t = 0.12 * t / np.linalg.norm(t, axis=1, keepdims=True)
    lo, hi = np.asarray(spec.joints_lower, np.float32), np.asarray(spec.joints_upper, np.float32)
    sc = np.ones(JA, np.float32) if joint_scale is None else np.asarray(joint_scale, np.float32)
    th = np.clip(np.asarray(spec.default_state, np.float32)[None, :JA] + 0.3 * (sc * f(B, JA)), lo - 0.2 * sc, hi + 0.2 * sc)
    inp = dict(hand_pose=np.concatenate([t, f(B, 6), th], 1).astype(np.float32),
               idx=r.randint(0, spec.n_contact_candidates, (B, n)).astype(np.int64),
               g_cpts=f(B, n, 3), g_cnrm=f(B, n, 3), g_spheres=f(B, max(S, 1), 3)[:, :S], g_wrench=f(B, L, 6), g_Rt=f(B, 12),
               g_theta=f(B, JA), g_R=f(B, 9),
               dist_sq=(1e-3 * r.rand(B, n)).astype(np.float32), sign=(2 * r.randint(0, 2, (B, n)) - 1).astype(np.int32),
               e_fc=r.rand(B).astype(np.float32), e_pen=r.rand(B).astype(np.float32), e_spen=r.rand(B).astype(np.float32),
               u_accept=r.rand(B).astype(np.float32), z=f(B), step=r.randint(1, 400, B).astype(np.int64),
               energy_old=(40.0 + 80.0 * r.rand(B)).astype(np.float32), pose_old=f(B, D), grad_old=f(B, D),
               idx_old=r.randint(0, spec.n_contact_candidates, (B, n)).astype(np.int64), terms_old=f(N_TERMS, B))
    # the Metropolis test must go both ways in every fixture: rows 0 and 1 come from far above any new total, row 2 from zero,
    # the others from the range of the totals (about 8 per contact at these weights)
    inp["energy_old"] = (n * (7.5 + 2.5 * r.rand(B))).astype(np.float32)
    inp["energy_old"][:2], inp["energy_old"][2] = 1e4, 0.0
    for k in ("obj_dir", "hand_normals"):
        v = f(B, n, 3)
        inp[k] = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    return inp


def forward_state(C, hand, inp):
    """Rg (B,9), link_T (B,L,12) and the node frames (B,J,12) of gq_fk_forward on the inputs' pose, as numpy arrays."""
    hp, ix = torch.tensor(inp["hand_pose"]).cuda(), torch.tensor(inp["idx"]).cuda()
    B, n = ix.shape
    dev = hp.device
    Rg, LT = torch.empty(B, 9, device=dev), torch.empty(B, hand.L, 12, device=dev)
    cp, cn = torch.empty(B, n, 3, device=dev), torch.empty(B, n, 3, device=dev)
    ws, nb = hand.fk_ws(B, dev)
    C.call("gq_fk_forward", hand.handle, C.f32(hp), C.i64(ix), B, n, C.f32(Rg), C.f32(LT), C.f32(cp), C.f32(cn), None, 0.0,
           None, None, None, None, C.ptr(ws), nb, C.stream_ptr())
    torch.cuda.synchronize()
    N = hand.spec.n_nodes  # tree joints (coupled hands: more than the pose carries)
    W = ws[: B * N * 48].view(torch.float32).view(B, N, 12)
    return dict(Rg=Rg.cpu().numpy(), link_T=LT.cpu().numpy(), node_W=W.cpu().numpy().copy())


def run_backward(C, hand, inp, present=GRAD_INPUTS, tail=True, reset_mask=None, slots=1, slot_ctr=(0, 1)):
    """One gq_fk_backward launch on `inp` (make_inputs + forward_state).  present: the gradient inputs that are handed over;
    tail: with the fused energy and accept tail.  reset_mask (B,) uint8: rows accepted unconditionally.  slots / slot_ctr: the
    ring of accept draws -- inp["u_accept"] is then (slots, B) and slot_ctr the device counter pair before the launch (the
    proposal has advanced [1]); the pair after the launch comes back as "slot_ctr".  -> dict of numpy outputs."""
    cu = {k: torch.tensor(np.ascontiguousarray(v)).cuda() for k, v in inp.items()}
    B, n = inp["idx"].shape
    D = inp["hand_pose"].shape[1]
    ws, nb = hand.fk_ws(B, cu["hand_pose"].device)
    ws.zero_()
    ws[: B * hand.spec.n_nodes * 48].view(torch.float32).copy_(cu["node_W"].reshape(-1))
    opt = lambda k: C.f32(cu[k]) if (k in present and cu[k].numel() > 0) else None
    gp = torch.full((B, D), float("nan"), device="cuda")
    keep = []
    en = ac = None
    if tail:
        jlo = torch.tensor(np.asarray(hand.spec.joints_lower, np.float32)).cuda()
        jhi = torch.tensor(np.asarray(hand.spec.joints_upper, np.float32)).cuda()
        terms_new = torch.zeros(N_TERMS, B, device="cuda")
        terms_new[1], terms_new[2], terms_new[3] = cu["e_fc"], cu["e_pen"], cu["e_spen"]
        total = torch.zeros(B, device="cuda")
        en = C.RowEnergyDesc()
        en.dist_sq, en.sign, en.obj_dir, en.hand_normals = (cu[k].data_ptr() for k in ("dist_sq", "sign", "obj_dir", "hand_normals"))
        en.joints_lower, en.joints_upper = jlo.data_ptr(), jhi.data_ptr()
        en.e_fc, en.e_pen, en.e_spen = (terms_new[i].data_ptr() for i in (1, 2, 3))
        en.n = n
        for k, v in WEIGHTS.items():
            setattr(en, k, v)
        en.e_dis, en.e_joints, en.total = terms_new[0].data_ptr(), terms_new[4].data_ptr(), total.data_ptr()
        accept = torch.full((B,), 7, dtype=torch.uint8, device="cuda")
        temperature = torch.zeros(B, device="cuda")
        energy, pose, grad, idx, terms = (cu[k].clone() for k in ("energy_old", "pose_old", "grad_old", "idx_old", "terms_old"))
        ac = C.AcceptDesc()
        rm = None if reset_mask is None else torch.tensor(np.ascontiguousarray(reset_mask, dtype=np.uint8)).cuda()
        assert cu["u_accept"].numel() == slots * B
        ac.u_accept, ac.z, ac.step = cu["u_accept"].data_ptr(), cu["z"].data_ptr(), cu["step"].data_ptr()
        ac.reset_mask = None if rm is None else rm.data_ptr()
        ac.starting_temperature, ac.decay, ac.annealing_period = 18.0, 0.95, 30
        ac.energy, ac.pose, ac.idx, ac.grad = energy.data_ptr(), pose.data_ptr(), idx.data_ptr(), grad.data_ptr()
        ac.accept, ac.temperature = accept.data_ptr(), temperature.data_ptr()
        ac.n_terms, ac.terms_new, ac.terms = N_TERMS, terms_new.data_ptr(), terms.data_ptr()
        slot_ctr = torch.tensor(list(slot_ctr), dtype=torch.int32, device="cuda")  # default: one slot of draws, the proposal has advanced [1]
        ac.slot_ctr, ac.slots = slot_ctr.data_ptr(), slots
        keep = [jlo, jhi, rm]
    C.call("gq_fk_backward", hand.handle, C.f32(cu["hand_pose"]), C.i64(cu["idx"]), B, n, C.f32(cu["Rg"]), C.f32(cu["link_T"]),
           opt("g_cpts"), opt("g_cnrm"), opt("g_spheres"), opt("g_wrench"), opt("g_Rt"), opt("g_theta"), opt("g_R"), C.f32(gp),
           ctypes.byref(en) if tail else None, ctypes.byref(ac) if tail else None, C.ptr(ws), nb, C.stream_ptr())
    torch.cuda.synchronize()
    del keep
    out = dict(grad_pose=gp.cpu().numpy())
    if tail:
        out.update(e_dis=terms_new[0].cpu().numpy(), e_joints=terms_new[4].cpu().numpy(), total=total.cpu().numpy(),
                   accept=accept.cpu().numpy(), pose=pose.cpu().numpy(), grad=grad.cpu().numpy(), idx=idx.cpu().numpy(),
                   terms=terms.cpu().numpy(), energy=energy.cpu().numpy(), temperature=temperature.cpu().numpy(),
                   terms_new=terms_new.cpu().numpy(), slot_ctr=slot_ctr.cpu().numpy())
    return out


def oracle_grad(spec, inp, present, tail, seed, dtype=torch.float64):
    """-> (d loss / d hand_pose by autograd through oracle/ref_cpu in `dtype`, the inputs with g_wrench / g_Rt replaced by those
    of the loss).  Loss: sum(cp . g_cpts) + sum(cn . g_cnrm) + sum(spheres . g_spheres) + sum(R . g_R) + sum(theta . g_theta) +
    a linear energy on link-fixed points (its hand-frame link wrenches (f, x cross f) are the kernel's g_wrench) + a linear
    energy on world points seen from the hand frame (its [gsum, K] is the kernel's g_Rt) + w_joints E_joints with the tail.
    The random constants of the loss are drawn in fp64 and cast, so every dtype differentiates the same loss."""
    from ref_cpu import kin as okin
    from ref_cpu import models as omodels

    B, n = inp["idx"].shape
    L = spec.n_links
    td = lambda k: torch.tensor(inp[k], dtype=dtype)
    hp = td("hand_pose").requires_grad_()
    oh = omodels.OracleHand(spec, dtype)
    oh.set_parameters(hp, torch.tensor(inp["idx"]))
    T, R, t = oh.current_status, oh.global_rotation, oh.global_translation
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)
    q, w = 0.02 * rn(L, 3, 3), rn(B, L, 3, 3)  # three link-fixed points per link, a constant force on each
    x = (T[:, :, None, :3, :3] @ q[None, :, :, :, None]).squeeze(-1) + T[:, :, None, :3, 3]
    P, d = 0.1 * rn(B, 8, 3), rn(B, 8, 3)      # world points, constant hand-frame gradients
    xh = (P - t[:, None]) @ R
    inp = dict(inp)
    inp["g_wrench"] = torch.cat([w.sum(2), torch.cross(x.detach(), w, dim=-1).sum(2)], -1).float().numpy()
    inp["g_Rt"] = torch.cat([d.sum(1), torch.einsum("bpk,bpj->bkj", xh.detach(), d).reshape(B, 9)], 1).float().numpy()
    sph = okin.sphere_centers_world(spec, T, R, t)
    terms = dict(g_cpts=lambda: (oh.contact_points * td("g_cpts")).sum(), g_cnrm=lambda: (oh.contact_normals * td("g_cnrm")).sum(),
                 g_spheres=lambda: (sph * td("g_spheres")).sum() if spec.n_spheres else hp.sum() * 0.0,
                 g_wrench=lambda: (x * w).sum(), g_Rt=lambda: (xh * d).sum(), g_theta=lambda: (hp[:, 9:] * td("g_theta")).sum(),
                 g_R=lambda: (R.reshape(B, 9) * td("g_R")).sum())
    loss = hp.sum() * 0.0
    for k in present:
        loss = loss + terms[k]()
    if tail:
        lo, hi = (torch.tensor(np.asarray(a, np.float64)).to(dtype) for a in (spec.joints_lower, spec.joints_upper))
        loss = loss + WEIGHTS["w_joints"] * (torch.relu(hp[:, 9:] - hi) + torch.relu(lo - hp[:, 9:])).sum()
    loss.backward()
    return hp.grad.numpy(), inp


def check(C, spec, hand, B, n, seed, present=GRAD_INPUTS, tail=True, joint_scale=None, fp32_floor=False):
    """gq_fk_backward on make_inputs against the fp64 oracle: 1e-4 on the norm, rtol 2e-3 / atol 2e-4 per element, E_joints,
    the accept flags.  fp32_floor: the same oracle in float32 on the same inputs gives the noise floor of an fp32 evaluation
    (its error against the fp64 run); the kernel is allowed the larger of the tolerances above and 4 x that floor -- 2 x because
    two independent fp32 evaluations can sit on opposite sides of the truth, 2 x for another association order and fused
    multiply-adds.  -> the inputs (with the forward state), the outputs and the measured errors."""
    from _parity import rel_err

    inp0 = make_inputs(spec, B, n, seed, joint_scale)
    go, inp = oracle_grad(spec, inp0, present, tail, seed + 1000)
    inp.update(forward_state(C, hand, inp))
    out = run_backward(C, hand, inp, present=present, tail=tail)
    gg = out["grad_pose"]
    nrm = np.linalg.norm(gg - go) / np.linalg.norm(go)
    print(f"{spec.name} B={B} n={n} present={present} tail={tail}: norm-wise {nrm:.3g}, max abs {np.abs(gg - go).max():.3g}, "
          f"max rel {rel_err(gg, go, 1e-2).max():.3g}")
    err = dict(norm=nrm, max_abs=np.abs(gg - go).max(), floor_norm=0.0, floor_abs=0.0)
    if not fp32_floor:
        assert nrm < 1e-4
        np.testing.assert_allclose(gg, go, rtol=2e-3, atol=2e-4)
    else:
        g32, _ = oracle_grad(spec, inp0, present, tail, seed + 1000, dtype=torch.float32)
        err["floor_norm"] = np.linalg.norm(g32 - go) / np.linalg.norm(go)
        err["floor_abs"] = np.abs(g32 - go).max()
        print(f"{spec.name}: fp32 oracle against its fp64 self: norm-wise {err['floor_norm']:.3g}, max abs {err['floor_abs']:.3g}")
        assert nrm < max(1e-4, 4 * err["floor_norm"])
        allowed = np.maximum(2e-4 + 2e-3 * np.abs(go), 4 * err["floor_abs"])
        bad = np.abs(gg - go) > allowed
        assert not bad.any(), f"{bad.sum()} elements beyond max(rtol 2e-3 / atol 2e-4, 4 x fp32 floor {err['floor_abs']:.3g})"
    if tail:
        assert set(out["accept"].tolist()) <= {0, 1} and np.isfinite(out["total"]).all()
        th = inp["hand_pose"][:, 9:].astype(np.float64)
        ej = np.maximum(th - np.asarray(spec.joints_upper, np.float64), 0) + np.maximum(np.asarray(spec.joints_lower, np.float64) - th, 0)
        np.testing.assert_allclose(out["e_joints"], ej.sum(1), rtol=1e-5, atol=1e-6)
    return inp, out, err
