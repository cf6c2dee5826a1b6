"""Inputs and the reference of the payload-holding tests, shared by tests/test_hold_body_host.py (CPU), tests/test_gpu_hold.py and
tests/test_hold_surface.py.  Nothing here needs a GPU.

The reference is a restatement of the term (include/graspqp_hip.h, "payload holding") in torch at a chosen dtype: the cone
matrix F on the inward normals, per (row, load) the SAME loop as the kernel's, ``ref_cpu.qp.pdipm_forward_box(Q, p, 0, u, eps=0,
maxIter=T, notImprovedLim=T+1)`` with a batch of one (so it returns that problem's own best iterate and no stop rule fires), then
V, r, the contact forces, the envelope gradient and J' R' f with ``ref_cpu.export.contact_jacobian``.  fp64 is the reference, the
same code in fp32 is the noise the bounds are scaled by, and scipy's BVLS gives the exact optimum.

A case is 8 rows = 4 objects x 2 rows on one hand; the contact points and normals are synthetic (the launch takes them as inputs;
the hand's pose matters for the joint torques only), on a sphere of 5 cm about ``cog``, built so that every regime of the box QP
occurs (``assert_populated``):
  object 0  contacts spread around the sphere, a 0.2 kg load: carried, E at the ridge floor, free columns
  object 1  the same contacts, a 5 kg load against the same force bound: columns at the upper bound
  object 2  all contacts within 25 degrees of +x and the load pulling along -x, away from them: x = 0, E = 1, zero gradient
  object 3  contacts around the sphere, 1 kg with its centre of mass 2 cm off (a torque load)
With n = 1 the cone matrix has rank 3 < 6 whatever the regime.  Loads 1..7 add accelerations of up to 6 m/s^2 to the weight."""
import functools

import numpy as np
import torch

import ref_cpu  # noqa: F401
from ref_cpu import export as oexp
from ref_cpu import kin
from ref_cpu import qp as oqp

import _pregrasp_cases as pc

MU, TW, RIDGE, T, MAX_FORCE, RADIUS = 0.5, 5.0, 1e-4, 16, 4.0, 0.05
B, BE = 8, 2
NK = [(1, 4), (3, 4), (12, 4), (5, 8), (12, 8)]  # nz = 4, 12, 48, 40, 96: one and two column slots, the second filled to lane 31
LOADS = (1, 3, 8)
HANDS = ("allegro", "ability_hand", "panda")
ACC = ((0, 0, 0), (3, 0, 0), (0, -3, 2), (0, 0, 6), (-4, 1, 0), (2, 2, -2), (0, 5, 0), (-1, -1, -5))
spec_of, set_synthetic_root = pc.spec_of, pc.set_synthetic_root


def loads(L):
    """(4,L,6) CPU float32 through ops.hold_loads: the four objects of the docstring."""
    from graspqp_amd import ops

    a = ACC[:L]
    away = (0.2 * np.array(a, np.float64)).tolist()  # object 2: gravity along -x, the accelerations only tilt the pull a little
    return torch.cat([ops.hold_loads([0.2, 5.0], accelerations=a), ops.hold_loads([0.3], up=(1.0, 0.0, 0.0), accelerations=away),
                      ops.hold_loads([1.0], accelerations=a, com_offset=(0.02, 0.0, 0.0))], 0)


@functools.lru_cache(maxsize=None)
def inputs(name, n, seed=0):
    """Seeded float32 tensors: hand_pose (B,D), idx (B,n), contact_pts (B,n,3), obj_normal (B,n,3, outward, unit), cog (B,3)."""
    spec = spec_of(name)
    hp = pc.pose(spec, B, 7 + seed, spread=0.1)
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=torch.Generator().manual_seed(100 * n + seed))
    return (hp, idx) + geometry(n)


@functools.lru_cache(maxsize=None)
def geometry(n):
    """contact_pts, obj_normal, cog of a case: they do not depend on the hand."""
    gen = torch.Generator().manual_seed(100 * n + 1)
    cog = (0.01 * torch.randn(B // BE, 3, generator=gen)).repeat_interleave(BE, 0)
    d = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=gen), dim=-1)
    if n >= 3:  # the first three contacts 120 degrees apart in a vertical plane, one of them below the object: its normal force
        for b in range(B):  # carries the weight, so the light load can be carried whatever the friction
            phi = float(torch.rand(1, generator=gen)) * 2 * np.pi
            hor = torch.tensor([np.cos(phi), np.sin(phi), 0.0], dtype=torch.float32)
            ang = torch.tensor([-0.5, 1.0 / 6.0, 5.0 / 6.0]) * np.pi + 0.1 * torch.randn(3, generator=gen)
            d[b, :3] = torch.cos(ang)[:, None] * hor + torch.sin(ang)[:, None] * torch.tensor([0.0, 0.0, 1.0])
            d[b, :3] += 0.05 * torch.randn(3, 3, generator=gen)
        d = torch.nn.functional.normalize(d, dim=-1)
    side = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0]) + 0.25 * (torch.rand(BE, n, 3, generator=gen) - 0.5), dim=-1)
    d[2 * BE:3 * BE] = side  # object 2: within 25 degrees of +x
    cp = cog[:, None] + RADIUS * d
    nrm = torch.nn.functional.normalize(d + 0.05 * torch.randn(B, n, 3, generator=gen), dim=-1)
    nrm[2 * BE:3 * BE] = side
    return cp.float().contiguous(), nrm.float().contiguous(), cog.float().contiguous()


def cone_matrix(cp, nrm_out, cog, k, mu=MU, tw=TW):
    """F (B,6,n k) of csrc/fc_dev.h's cone column on the INWARD normals, in the dtype of ``cp``; column i = contact i // k, edge i % k.
    Also the guard of the column's one branch: the smallest |dot - 0.9| over the contacts."""
    dt = cp.dtype
    n = -nrm_out.to(dt)
    is3 = 0.57735026918962576
    b1 = torch.full_like(n, is3)
    dot = (b1 * n).sum(-1) / (n.norm(dim=-1) + 1e-6)
    b1[..., 1] = torch.where(dot > 0.9, b1[..., 1] - 2.0, b1[..., 1])
    t1 = torch.linalg.cross(n, b1, dim=-1)
    t2 = torch.linalg.cross(n, t1, dim=-1)
    cc = float(np.sqrt(1.0 - mu * mu))
    cols = []
    for e in range(k):
        if k == 4:
            s = mu if e < 2 else -mu
            dr = s * t2 if e & 1 else s * t1
        else:
            ang = 6.283185307179586 / k * e
            dr = mu * (float(np.cos(ang)) * t1 + float(np.sin(ang)) * t2)
        f = (dr + cc * n) / k
        tau = tw * torch.linalg.cross(cp - cog.to(dt)[:, None], f, dim=-1)
        cols.append(torch.cat([f, tau], -1))  # (B,n,6)
    F = torch.stack(cols, 2)  # (B,n,k,6)
    return F.reshape(F.shape[0], -1, 6).transpose(1, 2).contiguous(), float((dot - 0.9).abs().min())


def loop(F, w, u, ridge=RIDGE, iters=T):
    """x (nz) of one problem: the shared PDIPM loop, batch of one, no stop rule."""
    nz = F.shape[1]
    Q = F.T @ F + ridge * torch.eye(nz, dtype=F.dtype)
    p = F.T @ w
    x, _, _, _ = oqp.pdipm_forward_box(Q[None], p[None], torch.zeros(1, nz, dtype=F.dtype), torch.full((1, nz), u, dtype=F.dtype), eps=0.0,
                                       maxIter=iters, notImprovedLim=iters + 1)
    return x[0]


def exact(F, w, u, ridge=RIDGE):
    """The exact optimum of one problem (fp64 numpy in, x out) by scipy's BVLS on the ridge-augmented least-squares form."""
    from scipy.optimize import lsq_linear

    nz = F.shape[1]
    A = np.concatenate([F, np.sqrt(ridge) * np.eye(nz)], 0)
    return lsq_linear(A, -np.concatenate([w, np.zeros(nz)]), bounds=(0.0, u), method="bvls", tol=1e-14).x


def evaluate(F, w, x, ridge=RIDGE):
    r = F @ x + w
    return r, float(r @ r + ridge * (x @ x))


@functools.lru_cache(maxsize=None)
def solved(n, k, L, dtype=torch.float64, iters=T, max_force=MAX_FORCE, with_exact=False):
    """The part of the reference that does not depend on the hand (computed once per case and shared): E (B), resid (B,L),
    x (B,L,nz), force (B,L,n,3), g (B,n,3) = dE/dcontact_pts, guard, rank; with_exact also E_exact (B) at the BVLS optimum."""
    cp, nrm, cog = geometry(n)
    F, guard = cone_matrix(cp.to(dtype), nrm.to(dtype), cog.to(dtype), k)
    lw = loads(L).to(dtype)
    w = torch.cat([lw[..., :3], TW * lw[..., 3:]], -1)  # (4,L,6)
    nz = n * k
    out = dict(E=np.zeros(B), resid=np.zeros((B, L)), x=np.zeros((B, L, nz)), force=np.zeros((B, L, n, 3)), g=np.zeros((B, n, 3)),
               guard=guard, E_exact=np.zeros(B), wnorm=np.zeros((B, L)))
    for b in range(B):
        for l in range(L):
            wl = w[b // BE, l]
            x = loop(F[b], wl, max_force, RIDGE, iters)
            r, V = evaluate(F[b], wl, x)
            ww = float(wl @ wl)
            out["E"][b] += V / ww / L
            out["resid"][b, l] = float(r.norm()) / np.sqrt(ww)
            out["wnorm"][b, l] = float(lw[b // BE, l, :3].norm())
            out["x"][b, l] = x.double().numpy()
            f = F[b][:3].T * x[:, None]  # (nz,3)
            out["force"][b, l] = f.reshape(n, k, 3).sum(1).double().numpy()
            gt = (2.0 / (L * ww)) * r[3:][None, :] * x[:, None]  # (nz,3) dE/dtau_i
            out["g"][b] += (TW * torch.linalg.cross(F[b][:3].T, gt, dim=-1)).reshape(n, k, 3).sum(1).double().numpy()
            if with_exact:
                xe = exact(F[b].double().numpy(), wl.double().numpy(), max_force)
                out["E_exact"][b] += evaluate(F[b].double(), wl.double(), torch.as_tensor(xe))[1] / ww / L
    out["rank"] = int(np.linalg.matrix_rank(F[0].double().numpy()))
    out["F"] = F.double().numpy()
    return out


def reference(name, n, k, L, dtype=torch.float64, iters=T, max_force=MAX_FORCE, with_exact=False):
    """``solved`` plus torque (B,L,JA) = J_act' R' force on the hand ``name``; numpy fp64 arrays."""
    spec = spec_of(name)
    hp, idx = inputs(name, n)[:2]
    out = dict(solved(n, k, L, dtype, iters, max_force, with_exact))
    R = kin.special_gramschmidt(hp[:, 3:9].to(dtype))
    Jc = oexp.contact_jacobian(spec, hp[:, 9:].to(dtype), idx)  # (B,n,3,JA)
    fh = torch.einsum("bji,blcj->blci", R, torch.as_tensor(out["force"]).to(dtype))  # R' f
    out["torque"] = torch.einsum("bcia,blci->bla", Jc, fh).double().numpy()
    return out


def regimes(ref, max_force=MAX_FORCE):
    """(row, load) pairs per regime: carried (resid < 2 %, a free column), saturated (a column within 1 % of the bound, resid > 10 %),
    nothing (every column < 1e-3 of the bound, resid > 0.999)."""
    x, r = ref["x"], ref["resid"]
    free = ((x > 0.02 * max_force) & (x < 0.98 * max_force)).any(-1)
    return dict(carried=int(((r < 0.02) & free).sum()), saturated=int((((x > 0.99 * max_force).any(-1)) & (r > 0.1)).sum()),
                nothing=int((((x < 1e-3 * max_force).all(-1)) & (r > 0.999)).sum()))


def assert_populated(ref, n, tag):
    reg = regimes(ref)
    print(f"[{tag}] regimes (row, load) pairs: {reg}, rank of F {ref['rank']}, cone-branch guard {ref['guard']:.2e}, |g| per row "
          f"{np.linalg.norm(ref['g'].reshape(B, -1), axis=1).round(4).tolist()}")
    assert ref["guard"] > 1e-3, tag  # no contact near the one branch of the cone column
    assert reg["saturated"] > 0 and reg["nothing"] > 0, (tag, reg)
    if n == 1:
        assert ref["rank"] < 6, tag  # the rank-deficient regime
    else:
        assert reg["carried"] > 0, (tag, reg)
    assert np.linalg.norm(ref["g"]) > 0 and np.abs(ref["torque"]).max() > 0, tag
    zero = ref["resid"].min(1) > 0.999  # rows where no load is held at all: E = 1, zero gradient
    assert zero.any() and np.abs(ref["E"][zero] - 1).max() < 1e-3 and np.linalg.norm(ref["g"][zero]) < 1e-3, tag
