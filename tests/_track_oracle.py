"""The fp64 oracle of the approach tracking term and its seeded cases, shared by the CPU tests (test_track_oracle.py,
test_track_body_host.py) and tests/test_gpu_track.py.  Nothing here needs a GPU or an asset.

The oracle is a batched torch restatement of the iteration of include/graspqp_hip.h ("approach tracking"): waypoint i = 0..T at
d_i = D (T - i) / T, q warm-started from the waypoint before (the first from ``q_start``), U updates of the reach term's update
(``_reach_oracle.solve``), one more FK for e_i and E_i = |e_i|^2; E_track the mean.  The gradient is autograd's with every q_i
detached.  The arms, the kinematics and the pools of poses are those of tests/_reach_oracle.py.

Cases: ``q_start`` is the float32-rounded station-K winner of ``_reach_oracle.pool(name, n_seeds, stations=2)``.  A row is STABLE
when the oracle alone says so: ``q_start`` perturbed by +-1e-6 with a seeded sign pattern (clipped to the limits) moves E_track by
at most a quarter of the comparison bound 2e-3 E + 1e-10 and the path by at most 1e-4.  Only stable rows are compared, and at most
4 of a pool's 64 rows may be left out."""
import functools

import numpy as np
import torch

import _reach_oracle as ro
from _reach_oracle import F64, LAM, RHO, AXIS, POOL, POOL_EACH

STATIONS = 2          # the reach pools the start configurations come from
SHAPES = ((8, 3), (4, 2))  # (T, U)
SEEDS = (1, 4)
E_RTOL, E_ATOL = 2e-3, 1e-10
MAX_LEFT_OUT = 4


def e_bound(E):
    return E_RTOL * np.asarray(E) + E_ATOL


def track(arm, pose9, base_T, batch_each, q_start, T, U, axis=AXIS, distance=0.10, lam=LAM, rho=RHO, up=None):
    """pose9 (B,9), base_T (n_obj,3,4), q_start (B,N) -> dict: E (B), Ei (B,T+1), q (B,T+1,N), worst (B), step (B), grad (B,9) =
    d sum(up E) / d pose9 with every q_i held fixed, clamped (B) = whether some q_i has a joint on a limit, e (B,T+1,6)."""
    pose = torch.as_tensor(np.asarray(pose9), dtype=F64).clone().requires_grad_()
    B = pose.shape[0]
    R = ro.gramschmidt(pose[:, 3:9])
    a = torch.as_tensor(axis, dtype=F64)
    base = ro._T44(base_T)[torch.arange(B) // int(batch_each)]
    q = torch.as_tensor(np.asarray(q_start), dtype=F64).clone()
    Ra = R @ a
    Ei, qs, es, step = [], [], [], torch.zeros(B, dtype=F64)
    for i in range(T + 1):
        d = distance * (T - i) / T
        ps = pose[:, :3] - d * Ra
        qn = ro.solve(arm, base, ps.detach(), R.detach(), q, U, lam, rho)
        step = torch.maximum(step, (qn - q).abs().amax(-1))
        q = qn
        Tee, _, _ = ro.fk(arm, q, base)
        e = ro.error(Tee, ps, R, rho)
        Ei.append((e * e).sum(-1))
        qs.append(q)
        es.append(e.detach())
    Ei, qs = torch.stack(Ei, 1), torch.stack(qs, 1)
    E = Ei.sum(-1) / (T + 1)
    upt = torch.ones(B, dtype=F64) if up is None else torch.as_tensor(np.asarray(up), dtype=F64)
    (g,) = torch.autograd.grad((E * upt).sum(), pose)
    lo, hi = torch.as_tensor(arm.lower, dtype=F64), torch.as_tensor(arm.upper, dtype=F64)
    clamped = ((qs <= lo) | (qs >= hi)).any(-1).any(-1)
    return dict(E=E.detach().numpy(), Ei=Ei.detach().numpy(), q=qs.numpy(), worst=Ei.detach().amax(-1).numpy(), step=step.numpy(),
                grad=g.numpy(), clamped=clamped.numpy(), e=torch.stack(es, 1).numpy())


def closed_form_grad(pose9, e, T, axis=AXIS, distance=0.10, rho=RHO, up=None):
    """The gradient as the kernel forms it, in fp64: per waypoint g_p = 2 c e_p on p*_i = t - d_i R a and the torque 2 c rho e_w on
    R* = R, c = up / (T+1), gathered in the gRt layout and chained through the Gram-Schmidt map (``_reach_oracle.pose_grad_of_gRt``)."""
    pose9, e = np.asarray(pose9, np.float64), np.asarray(e, np.float64)
    B = pose9.shape[0]
    a = np.asarray(axis, np.float64)
    out = np.zeros((B, 9))
    for b in range(B):
        R = ro.gramschmidt(torch.as_tensor(pose9[b:b + 1, 3:9], dtype=F64))[0].numpy()
        c = (1.0 if up is None else float(up[b])) / (T + 1)
        gRt, tau_h = np.zeros(12), np.zeros(3)
        for i in range(T + 1):
            d = distance * (T - i) / T
            gh = R.T @ (2 * c * e[b, i, :3])
            gRt[:3] -= gh
            gRt[3:] += np.outer(gh, -d * a).ravel()
            tau_h += R.T @ (2 * c * rho * e[b, i, 3:])
        hx, hy, hz = 0.5 * tau_h
        gRt[3 + 1] -= hz; gRt[3 + 2] += hy; gRt[3 + 3] += hz; gRt[3 + 5] -= hx; gRt[3 + 6] -= hy; gRt[3 + 7] += hx
        out[b] = ro.pose_grad_of_gRt(gRt, pose9[b])
    return out


def stable(arm, pose9, base_T, batch_each, q_start, T, U, ref, axis=AXIS, distance=0.10, seed=0):
    """q_start +- 1e-6 (seeded signs, clipped to the limits) moves E by at most a quarter of the E bound and the path by <= 1e-4."""
    rng = np.random.default_rng(4242 + seed)
    sign = np.where(rng.random(np.shape(q_start)) < 0.5, -1.0, 1.0)
    qp = np.clip(np.asarray(q_start, np.float64) + 1e-6 * sign, arm.lower, arm.upper)
    alt = track(arm, pose9, base_T, batch_each, qp, T, U, axis, distance)
    return (np.abs(alt["E"] - ref["E"]) <= 0.25 * e_bound(ref["E"])) & (np.abs(alt["q"] - ref["q"]).max((1, 2)) <= 1e-4)


def _kinds_present(arm, ref, st):
    """A stable row with a clamped joint, one with E > 1e-3, one with E < 1e-10 (short3: its three joints never get there, the kind
    is not asked of it)."""
    kinds = [st & ref["clamped"], st & (ref["E"] > 1e-3)]
    if arm.n_joints >= 6:
        kinds.append(st & (ref["E"] < 1e-10))
    return kinds


@functools.lru_cache(maxsize=None)
def pool(name, n_seeds=1, T=8, U=3):
    """The 64 rows of ``_reach_oracle.pool(name, n_seeds, stations=2)`` with q_start = float32 of its station-K winner, the oracle
    and which rows are stable.  Cached and shared: read-only."""
    rp = ro.pool(name, n_seeds, STATIONS)
    arm = rp["arm"]
    q_start = rp["ref"]["q"][:, STATIONS].astype(np.float32)
    ref = track(arm, rp["pose9"], rp["base_T"], POOL_EACH, q_start, T, U, rp["axis"], rp["distance"], up=rp["up"])
    st = stable(arm, rp["pose9"], rp["base_T"], POOL_EACH, q_start, T, U,
                track(arm, rp["pose9"], rp["base_T"], POOL_EACH, q_start, T, U, rp["axis"], rp["distance"]), rp["axis"], rp["distance"])
    return dict(arm=arm, pose9=rp["pose9"], base_T=rp["base_T"], q_start=q_start, ref=ref, stable=st, batch_each=POOL_EACH, T=T, U=U,
                distance=rp["distance"], up=rp["up"], name=name, axis=rp["axis"], n_seeds=n_seeds)


@functools.lru_cache(maxsize=None)
def case(name, n_seeds=1, T=8, U=3):
    """Eight rows of the pool, four per object (batch_each = 4), in the manner of ``_reach_oracle.case``: first a stable row of every
    kind and a row that is not stable (if the pool has one), then the pool's rows in order.  The oracle's numbers are the pool's."""
    pl = pool(name, n_seeds, T, U)
    st, ref = pl["stable"], pl["ref"]
    first = lambda m: [int(np.flatnonzero(m)[0])] if m.any() else []
    order = sum((first(m) for m in _kinds_present(pl["arm"], ref, st)), []) + first(~st) + list(range(POOL))
    rows = [[], []]
    for b in order:
        if b not in rows[b // POOL_EACH] and len(rows[b // POOL_EACH]) < 4:
            rows[b // POOL_EACH].append(b)
    sel = np.array(sorted(rows[0]) + sorted(rows[1]))
    out = dict(pl)
    out.update(pose9=pl["pose9"][sel], stable=st[sel], up=pl["up"][sel], q_start=pl["q_start"][sel], batch_each=4, rows=sel,
               ref={k: v[sel] for k, v in ref.items()})
    return out


def rows_case(name, n_seeds, B, batch_each, T, U):
    """A shape case: B rows in objects of ``batch_each`` rows whose bases alternate between the pool's two (so the groups of one
    wavefront have different bases), every object's rows drawn in order from the half of the pool that was generated for its base;
    the oracle and the stable rows for exactly these."""
    pl = pool(name, n_seeds, 8, 3)
    arm, n_obj = pl["arm"], B // batch_each
    taken, sel = [0, 0], []
    for o in range(n_obj):
        h = o % 2
        sel += list(range(h * POOL_EACH + taken[h], h * POOL_EACH + taken[h] + batch_each))
        taken[h] += batch_each
    assert n_obj * batch_each == B and max(taken) <= POOL_EACH
    sel = np.array(sel)
    base_T = np.stack([pl["base_T"][o % 2] for o in range(n_obj)])
    pose9, q_start, up = pl["pose9"][sel], pl["q_start"][sel], pl["up"][sel]
    ref = track(arm, pose9, base_T, batch_each, q_start, T, U, pl["axis"], pl["distance"], up=up)
    st = stable(arm, pose9, base_T, batch_each, q_start, T, U, track(arm, pose9, base_T, batch_each, q_start, T, U, pl["axis"], pl["distance"]),
                pl["axis"], pl["distance"])
    return dict(arm=arm, pose9=pose9, base_T=base_T, q_start=q_start, ref=ref, stable=st, batch_each=batch_each, T=T, U=U,
                distance=pl["distance"], up=up, name=name, axis=pl["axis"], n_seeds=n_seeds)


def compared_set(cs, tag="", kinds=True):
    """The stable rows of a case, with what every compared set must contain (``kinds`` = False: a shape case drawn for its lane
    mapping, not for its kinds of row; at least one row must still be stable)."""
    m, ref = cs["stable"], cs["ref"]
    print(f"[{tag}] stable {int(m.sum())} of {len(m)} rows; E {np.array2string(ref['E'], precision=2)}; clamped {ref['clamped'].astype(int)}")
    names = ["a clamped joint", "E > 1e-3", "E < 1e-10"]
    for kind, what in zip(_kinds_present(cs["arm"], ref, m) if kinds else [m], names if kinds else ["anything"]):
        assert kind.any(), (tag, "no stable row with " + what)
    return m


def ratios(E, grad9, q, step, cs, tag="", kinds=True):
    """The figures of the comparison on the stable rows, each as a share of its bound: E against 2e-3 E_64 + 1e-10, the pose
    gradient norm-wise against 1e-3 (translation and rotation part against 2e-3), track_q against 1e-3, track_step against 2e-3."""
    m, ref = compared_set(cs, tag, kinds), cs["ref"]
    E, g, go, Eo = np.asarray(E, np.float64)[m], np.asarray(grad9, np.float64)[m][:, :9], ref["grad"][m], ref["E"][m]
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    out = dict(E=np.max(np.abs(E - Eo) / e_bound(Eo)), grad=rel(g, go) / 1e-3, grad_t=rel(g[:, :3], go[:, :3]) / 2e-3,
               grad_r=rel(g[:, 3:], go[:, 3:]) / 2e-3)
    if q is not None:
        out["q"] = np.abs(np.asarray(q, np.float64)[m] - ref["q"][m]).max() / 1e-3
    if step is not None:
        out["step"] = np.abs(np.asarray(step, np.float64)[m] - ref["step"][m]).max() / 2e-3
    print(f"[{tag}] share of the bound: " + ", ".join(f"{k} {v:.2e}" for k, v in out.items()))
    return out


def assert_close(E, grad9, q, step, cs, tag="", kinds=True):
    out = ratios(E, grad9, q, step, cs, tag, kinds)
    for k, v in out.items():
        assert v <= 1.0, (tag, k, v)
    return out
