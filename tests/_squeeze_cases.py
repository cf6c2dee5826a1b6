"""Inputs and the fp64 oracle of the squeeze tests, shared by tests/test_squeeze_body_host.py (CPU) and tests/test_gpu_squeeze.py.

The oracle is ``ref_cpu.export.get_req_joint_velocities`` (the reference's hand_model.py:1155-1218) on an ``OracleHand`` and an
``OracleObject`` (an icosphere of 5 cm) with fp64 autograd, driven as core/energy.py:80-87 drives it: the contacts move along
``normal.detach() * |distance|.clamp(min=tau)``.  Its damping is the default argument of ``ref_cpu.export.pinv``; another damping is
that same function with the other argument (``damping_of``).

The term has two kinks, and every case keeps clear of both (``assert_guards``, on the oracle's numbers): no contact with
|sqrt(d2 + 1e-8) - tau| < 1e-5 m, none with d2 < 1e-10.  Every case has contacts above tau and contacts at the clamp: the root
translation of row b is set so that its contact 0 lies 2 mm (even b) or 15 mm (odd b) off the sphere.  Nothing here needs a GPU."""
import contextlib
import functools
import types

import numpy as np
import torch

import ref_cpu  # noqa: F401
from ref_cpu import export as oexp
from ref_cpu import models as omodels
from ref_cpu import sdf as osdf

import _pregrasp_cases as pc
from graspqp_amd.utils import meshes

TAU, LAM, RADIUS = 5e-3, 1e-3, 0.05
KINK, MIN_D2 = 1e-5, 1e-10
spec_of, set_synthetic_root = pc.spec_of, pc.set_synthetic_root


@functools.lru_cache(maxsize=None)
def sphere():
    fv = meshes.icosphere(1, RADIUS).astype(np.float32)
    return fv, meshes.surface_points(fv, 64, oversample=8).astype(np.float32)


@contextlib.contextmanager
def damping_of(lam):
    """``ref_cpu.export.pinv`` with damping ``lam`` for the calls inside (get_req_joint_velocities takes its default)."""
    old = oexp.pinv
    oexp.pinv = lambda A, l=lam: old(A, l)
    try:
        yield
    finally:
        oexp.pinv = old


def _travel(oh, oo):
    dist, cn = oo.cal_distance(oh.contact_points)
    return dist, cn


def guards(dist, tau):
    """(nearest |s - tau|, smallest d2, contacts above tau, contacts at the clamp) from the oracle's signed distances."""
    s = dist.detach().abs()  # = sqrt(d2 + 1e-8)
    return float((s - tau).abs().min()), float((s * s - 1e-8).min()), int((s > tau).sum()), int((s <= tau).sum())


def assert_guards(dist, tau, tag):
    near, d2, free, clamped = guards(dist, tau)
    print(f"[{tag}] guards: nearest |s - tau| {near:.2e} m, smallest d2 {d2:.2e}, {free} contacts above tau, {clamped} at the clamp")
    assert near >= KINK and d2 >= MIN_D2 and free > 0 and clamped > 0, tag


@functools.lru_cache(maxsize=None)
def inputs(name, B, n, tau=TAU, seed0=None):
    """Seeded float32 (hand_pose (B,D), contact_idx (B,n)) whose contacts pass the guards on the sphere."""
    spec = spec_of(name)
    fv, sp = sphere()
    oo = omodels.OracleObject([fv], [sp], B, torch.float64)
    seed0 = 1000 * n + B if seed0 is None else seed0
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        hp = pc.pose(spec, B, seed, spread=0.0)
        idx = torch.randint(spec.n_contact_candidates, (B, n), generator=gen)
        out = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen, dtype=torch.float64), dim=-1)
        off = torch.where(torch.arange(B) % 2 == 0, 2e-3, 1.5e-2).double()
        oh = omodels.OracleHand(spec, torch.float64)
        oh.set_parameters(hp.double(), idx)
        hp[:, :3] += (out * (RADIUS + off)[:, None] - oh.contact_points[:, 0]).float()
        oh.set_parameters(hp.double(), idx)
        dist, _ = _travel(oh, oo)
        near, d2, free, clamped = guards(dist, tau)
        if near >= KINK and d2 >= MIN_D2 and free > 0 and clamped > 0:
            return hp, idx
    raise AssertionError("no seeded pose passes the guards")


def oracle(name, hp, idx, up, tau=TAU, lam=LAM):
    """-> dict: E (B), theta (B,JA), grad (B,D) of sum(up E), dist (B,n) signed, all fp64 numpy / torch."""
    spec = spec_of(name)
    fv, sp = sphere()
    B = hp.shape[0]
    oh = omodels.OracleHand(spec, torch.float64)
    oo = omodels.OracleObject([fv], [sp], B, torch.float64)
    hp64 = hp.double().clone().requires_grad_()
    oh.set_parameters(hp64, idx)
    dist, cn = _travel(oh, oo)
    with damping_of(lam):
        th, res = oexp.get_req_joint_velocities(oh, cn.detach() * dist.unsqueeze(-1).abs().clamp(min=tau), idx)
    E = res.mean(-1)
    (g,) = torch.autograd.grad((E * torch.as_tensor(up, dtype=torch.float64)).sum(), hp64)
    return dict(E=E.detach().numpy(), theta=th.detach().numpy(), grad=g.numpy(), dist=dist.detach())


def assert_populated(ref, tau, tag, prismatic_only=False):
    """Both sides of every gradient comparison are populated: contacts above tau and at the clamp, and non-zero joint, rotation and
    contact-point (= root translation: only the contact points move with it) parts of the oracle gradient.  All-prismatic hands:
    the joint part is skipped (their Jacobian does not depend on the joints; what is left of it is the contact-point path)."""
    assert_guards(ref["dist"], tau, tag)
    g = ref["grad"]
    assert np.linalg.norm(g[:, :3]) > 0 and np.linalg.norm(g[:, 3:9]) > 0, tag
    assert prismatic_only or np.linalg.norm(g[:, 9:]) > 0, tag


def assert_close(E, theta, grad, ref, tag, prismatic_only=False):
    """The bounds of tests/test_gpu_alt_energies.py for this quantity: values rtol 2e-3 / atol 1e-9, theta rtol 2e-3 / atol 2e-5,
    gradients norm-wise 1e-3 overall and 2e-3 per part (joints, root rotation, root translation = the contact-point path)."""
    E, g, go = np.asarray(E, np.float64), np.asarray(grad, np.float64), ref["grad"]
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    print(f"[{tag}] E max rel err {np.max(np.abs(E - ref['E']) / np.abs(ref['E'])):.2e}, gradient rel err {rel(g, go):.2e}, "
          f"translation {rel(g[:, :3], go[:, :3]):.2e}, rotation {rel(g[:, 3:9], go[:, 3:9]):.2e}, joints {rel(g[:, 9:], go[:, 9:]):.2e} "
          f"(norms {np.linalg.norm(go[:, :3]):.2e} {np.linalg.norm(go[:, 3:9]):.2e} {np.linalg.norm(go[:, 9:]):.2e})")
    np.testing.assert_allclose(E, ref["E"], rtol=2e-3, atol=1e-9)
    if theta is not None:
        err = np.abs(np.asarray(theta, np.float64) - ref["theta"])
        print(f"[{tag}] theta max abs err {err.max():.2e} (max |theta| {np.abs(ref['theta']).max():.2e})")
        np.testing.assert_allclose(theta, ref["theta"], rtol=2e-3, atol=2e-5)
    assert np.linalg.norm(g - go) <= 1e-3 * np.linalg.norm(go), tag
    assert np.linalg.norm(g[:, :3] - go[:, :3]) <= 2e-3 * np.linalg.norm(go[:, :3]), (tag, "contact points")
    assert np.linalg.norm(g[:, 3:9] - go[:, 3:9]) <= 2e-3 * np.linalg.norm(go[:, 3:9]), (tag, "root rotation")
    if not prismatic_only:
        assert np.linalg.norm(g[:, 9:] - go[:, 9:]) <= 2e-3 * np.linalg.norm(go[:, 9:]), (tag, "joints")


# ---- the parts of one row, for the host program: leaves are the joints, R and the contact points ---------------------------
def oracle_parts(spec, theta, R, idx, p, up, tau=TAU, lam=LAM):
    """theta (1,JA), R (1,3,3), p (1,n,3) world contact points, fp64 -> E, theta_dot (JA), dE/dtheta (JA), dE/dR (3,3), dE/dp (n,3)
    of up E, with get_req_joint_velocities on a stand-in that carries exactly what it reads (spec, global_rotation, hand_pose)."""
    fv, _ = sphere()
    th = torch.as_tensor(theta, dtype=torch.float64).clone().requires_grad_()
    Rl = torch.as_tensor(R, dtype=torch.float64).clone().requires_grad_()
    pl = torch.as_tensor(p, dtype=torch.float64).clone().requires_grad_()
    hand = types.SimpleNamespace(spec=spec, global_rotation=Rl, hand_pose=torch.cat([torch.zeros(1, 9, dtype=torch.float64), th], 1))
    d2, sgn, nrm, cls = osdf.compute_sdf(pl.reshape(-1, 3), torch.as_tensor(fv, dtype=torch.float64))
    dist = (torch.sqrt(d2 + 1e-8) * (-sgn)).reshape(1, -1)
    cn = (nrm * sgn.unsqueeze(1)).reshape(1, -1, 3)
    with damping_of(lam):
        thd, res = oexp.get_req_joint_velocities(hand, cn.detach() * dist.unsqueeze(-1).abs().clamp(min=tau), idx)
    E = res.mean(-1)
    gt, gR, gp = torch.autograd.grad((E * up).sum(), (th, Rl, pl))
    return dict(E=float(E.detach()), theta=thd[0].detach().numpy(), g_theta=gt[0].numpy(), g_R=gR[0].numpy(), g_p=gp[0].numpy(),
                d2=d2.detach().numpy(), normal=cn[0].detach().numpy(), closest=cls.detach().numpy(), dist=dist.detach())
