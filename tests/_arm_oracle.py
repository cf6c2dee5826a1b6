"""The fp64 oracle of the arm clearance term (include/graspqp_hip.h, "arm clearance"), shared by test_arm_oracle.py,
test_arm_body_host.py, test_arm_surface.py and test_gpu_arm.py.  Nothing here needs a GPU or an asset.

A torch restatement that takes the joints q as an INPUT, as the launch does: link frames W_j(q) multiplied left to right, sphere
points x_s = W_l c_s, the hinge max(margin + r - phi, 0) on the row's grid (the fields and phi of _scene_oracle.py), the mean over
the stations; g_q from f_s = -grad phi and the columns z_j x (x_s - o_j) / z_j; y = (J J' + lambda_a I)^-1 J g_q with the columns
of the joints ON a limit zeroed; the pose gradient through p*_k = t - d_k R a and the torque rho y_w.  The joint limits are rounded to
float32 before "on a limit" is decided, as the device holds them (with double limits the clamped flag of a float32 q flips).
``dtype`` is the precision of the kinematics, the points, the field and the columns; the Gram matrix and the solve are always fp64:
dtype = float32 is the oracle's own rounding noise, the measure the bounds of the GPU test rest on.

The arms, bases and pools are those of _reach_oracle.py; the joints fed to the term are the reach oracle's winners, rounded to
float32 once."""
import functools

import numpy as np
import torch

import _reach_oracle as ro
import _scene_oracle as so

F64 = torch.float64
MARGIN, RADIUS, SPACING, LAM_A = 0.01, 0.05, 0.08, 1e-6
SHAPE, ORIGIN, VOXEL = (24, 24, 20), (-0.6, -0.6, -0.4), 0.1  # the far ends of some arm configurations lie outside: free space
# the affine field phi = n . x - c is a tilted board ABOVE the object (free space below it); the offset c per arm is chosen so that
# every pool holds rows without an active sphere and rows with several links in collision
AFFINE_N = (-0.36, 0.48, -0.8)
AFFINE_C = {"elbow6": -0.45, "arm7": -0.6, "gantry6": -0.2, "short3": 0.0, "chain8": -0.35}


@functools.lru_cache(maxsize=None)
def arm_spec(name, n_seeds=1):
    """The arm of _reach_oracle with its link spheres (radius 0.05, one every 0.08 m)."""
    return ro.arm_spec(name, n_seeds).with_link_spheres(RADIUS, SPACING)


def one_sphere(arm):
    """The same arm with ONE sphere, on the last link."""
    return arm.with_spheres([arm.n_joints - 1], [[0.02, 0.0, 0.01]], [RADIUS])


def full_spheres(arm, seed=3):
    """The same arm with 64 spheres: seeded links, centres within 0.1 m of the link origin, radii 0.03 .. 0.08; float32-exact."""
    rng = np.random.default_rng(seed)
    link = np.sort(rng.integers(0, arm.n_joints, 64))
    link[0], link[-1] = 0, arm.n_joints - 1
    centre = rng.uniform(-0.1, 0.1, (64, 3)).astype(np.float32).astype(np.float64)
    radius = rng.uniform(0.03, 0.08, 64).astype(np.float32).astype(np.float64)
    return arm.with_spheres(link, centre, radius)


def field(kind, name="elbow6", seed=0):
    """The test grids: about 24 x 24 x 20 nodes at 0.1 m around the object, covering most of the arm."""
    if kind == "affine":
        return so.affine(SHAPE, ORIGIN, VOXEL, n=AFFINE_N, c=AFFINE_C[name])
    if kind == "multilinear":
        return so.multilinear(SHAPE, ORIGIN, VOXEL, c=(0.05, 0.3, -0.2, 0.4, 0.35, -0.3, 0.2, 0.6))
    if kind == "random":
        return so.random_field(SHAPE, ORIGIN, VOXEL, 11 + seed, amp=0.3)
    raise KeyError(kind)


def link_frames(arm, q, base, dtype=F64):
    """q (P,N), base (P,4,4) -> link frames W (P,N,4,4) = base X_0 ... X_j (left to right) and the hand-root pose (P,4,4)."""
    eye = torch.eye(4, dtype=dtype)
    Tc, W = base.to(dtype), []
    for j in range(arm.n_joints):
        a = torch.as_tensor(arm.joint_axis[j], dtype=dtype)
        Mo = eye.repeat(q.shape[0], 1, 1)
        if arm.joint_type[j] == 1:
            Kh = ro._hat(a)
            Mo[:, :3, :3] = torch.eye(3, dtype=dtype) + torch.sin(q[:, j])[:, None, None] * Kh + (1 - torch.cos(q[:, j]))[:, None, None] * (Kh @ Kh)
        else:
            Mo[:, :3, 3] = q[:, j, None] * a
        Tc = Tc @ ro._T44(arm.joint_T[j]).to(dtype) @ Mo
        W.append(Tc)
    return torch.stack(W, 1), Tc @ ro._T44(arm.tool_T).to(dtype)


def _phi_rows(fields, rows_per_grid, x, K1):
    """phi (P,Ns) and inside (P,Ns) of the points x (P,Ns,3); problem p belongs to row p // K1, which reads grid row // rows_per_grid"""
    P = x.shape[0]
    grid = (torch.arange(P) // K1) // int(rows_per_grid)
    phi = torch.zeros(x.shape[:2], dtype=x.dtype)
    inside = torch.zeros(x.shape[:2], dtype=torch.bool)
    face = torch.zeros(x.shape[:2], dtype=x.dtype)
    for g, f in enumerate(fields):
        m = grid == g
        if m.any():
            ins, _, _, u = so.locate(f, x[m].detach())
            p = so.phi(f, x[m])
            phi = phi.index_put((torch.nonzero(m)[:, 0],), torch.where(ins, p, torch.zeros_like(p)))
            inside[m] = ins
            ud = torch.nan_to_num(u.detach())
            face[m] = (ud - ud.round()).abs().amin(-1)
    return phi, inside, face


def arm_terms(arm, q, pose9, base_T, batch_each, fields, margin=MARGIN, lam=LAM_A, rho=ro.RHO, axis=ro.AXIS, distance=0.10, up=None,
              dtype=F64):
    """q (B,K+1,N), pose9 (B,9), base_T (n_obj,3,4), fields: a list of G test grids (B divisible by G) -> dict of numpy arrays:
    E (B), Ek (B,K+1), grad (B,9) = d sum(up E) / d pose9, y (B,K+1,6) = [y_p ; rho y_w], gq (B,K+1,N), x (B,K+1,Ns,3), phi, inside,
    active, face (B,K+1,Ns), frozen (B,K+1,N), sig2 (B,K+1) = sigma_min^2 of the 6 x N matrix J with the frozen columns zeroed."""
    q = torch.as_tensor(np.asarray(q), dtype=dtype)
    B, K1, N = q.shape
    K, P, Ns = K1 - 1, B * K1, arm.n_spheres
    base = ro._T44(base_T)[torch.arange(B) // int(batch_each)].to(dtype)
    base_p = base[:, None].expand(B, K1, 4, 4).reshape(P, 4, 4)
    W, Tee = link_frames(arm, q.reshape(P, N), base_p, dtype)
    link = torch.as_tensor(arm.sphere_link, dtype=torch.long)
    ctr = torch.as_tensor(arm.sphere_centre, dtype=dtype)
    rad = torch.as_tensor(arm.sphere_radius, dtype=dtype)
    Wl = W[:, link]  # (P,Ns,4,4)
    x = ((Wl[..., :3, :3] @ ctr[None, :, :, None])[..., 0] + Wl[..., :3, 3]).detach().requires_grad_()
    phi, inside, face = _phi_rows(fields, B // len(fields), x, K1)
    h = torch.where(inside, torch.relu((margin + rad)[None] - phi), torch.zeros_like(phi))
    Ek = h.sum(-1)
    f = torch.autograd.grad(Ek.sum(), x)[0] if Ek.requires_grad else torch.zeros_like(x)  # -grad phi where active
    x = x.detach()
    rev = torch.as_tensor(arm.joint_type == 1)
    org = W[:, :, :3, 3]
    axs = W[:, :, :3, :3] @ torch.as_tensor(arm.joint_axis, dtype=dtype)[None, :, :, None]
    axs = axs[..., 0]  # (P,N,3)
    col = torch.where(rev[None, :, None, None], torch.linalg.cross(axs[:, :, None].expand(P, N, Ns, 3), x[:, None] - org[:, :, None], dim=-1),
                      axs[:, :, None].expand(P, N, Ns, 3))
    on = (link[None, :] >= torch.arange(N)[:, None]).to(dtype)  # (N,Ns)
    gq = ((col * f[:, None]).sum(-1) * on[None]).sum(-1)  # (P,N)
    pee = Tee[:, :3, 3]
    Jv = torch.where(rev[None, :, None], torch.linalg.cross(axs, pee[:, None] - org, dim=-1), axs)
    Jw = rho * rev[None, :, None].to(dtype) * axs
    q32 = q.reshape(P, N).to(torch.float32)
    lo32, hi32 = torch.as_tensor(arm.lower.astype(np.float32)), torch.as_tensor(arm.upper.astype(np.float32))
    frozen = ~((lo32 < q32) & (q32 < hi32))
    J = (torch.cat([Jv, Jw], -1) * (~frozen)[:, :, None].to(dtype)).transpose(1, 2).to(F64)  # (P,6,N)
    A = J @ J.transpose(1, 2)
    y = torch.linalg.solve(A + lam * torch.eye(6, dtype=F64), J @ gq.to(F64)[:, :, None])[:, :, 0]
    sig2 = torch.linalg.eigvalsh(A)[:, 0].clamp_min(0.0)
    yk = torch.cat([y[:, :3], rho * y[:, 3:]], -1).reshape(B, K1, 6)
    # the pose gradient: dE_k/dp*_k = y_p through p*_k = t - d_k R a; the torque tau pairs with R as <hat(tau) R / 2, R>
    pose = torch.as_tensor(np.asarray(pose9), dtype=F64).clone().requires_grad_()
    R = ro.gramschmidt(pose[:, 3:9])
    a = torch.as_tensor(axis, dtype=F64)
    d = torch.tensor([distance * k / K if K else 0.0 for k in range(K1)], dtype=F64)
    ps = pose[:, None, :3] - d[None, :, None] * (R @ a)[:, None, :]
    upt = (torch.ones(B, dtype=F64) if up is None else torch.as_tensor(np.asarray(up), dtype=F64)) / K1
    tau = (upt[:, None, None] * yk[:, :, 3:]).sum(1)
    s = (upt[:, None, None] * yk[:, :, :3] * ps).sum() + (0.5 * (ro._hat(tau) @ R.detach()) * R).sum()
    (g9,) = torch.autograd.grad(s, pose)
    E = Ek.detach().reshape(B, K1).to(F64).sum(-1) / K1
    r = lambda t, *sh: t.detach().reshape(B, K1, *sh).to(F64).numpy()
    pd = phi.detach()
    return dict(E=E.numpy(), Ek=r(Ek), grad=g9.numpy(), y=yk.numpy(), gq=r(gq, N), x=r(x, Ns, 3), phi=r(pd, Ns),
                inside=inside.reshape(B, K1, Ns).numpy(), active=(inside & (pd < (margin + rad)[None])).reshape(B, K1, Ns).numpy(),
                face=r(face, Ns), frozen=frozen.reshape(B, K1, N).numpy(), sig2=sig2.reshape(B, K1).numpy(), h=r(h, Ns))


def guard_rows(res, arm, margin, random=False):
    """The conditions on the INPUTS, per row: every sphere inside the volume has |margin + r - phi| >= NEAR and, on a random field,
    every coordinate of every sphere lies at least FACE cells from a cell face.  -> (ok (B) bool, nearest (B), face (B))"""
    ins = res["inside"]
    near = np.where(ins, np.abs((margin + arm.sphere_radius)[None, None] - res["phi"]), np.inf).min((1, 2))
    face = res["face"].min((1, 2))
    return (near >= so.NEAR) & ((face >= so.FACE) if random else True), near, face


def guards(res, arm, margin, random=False):
    """... of a whole case -> (ok, nearest, face)"""
    ok, near, face = guard_rows(res, arm, margin, random)
    return bool(ok.all()), float(near.min()), float(face.min())


def coverage(res, arm):
    """Per row: no active sphere; all spheres active or >= 2 links with an active sphere; a joint on a limit; a sphere outside."""
    act = res["active"]
    links = np.array([[len(set(arm.sphere_link[a.any(0)])) for a in [act[b]]][0] for b in range(act.shape[0])])
    return dict(none=~act.any((1, 2)), many=act.all((1, 2)) | (links >= 2), limit=res["frozen"].any((1, 2)), outside=(~res["inside"]).any((1, 2)))


def reach_q(name, stations, n_seeds=1):
    """The joints the term is fed: the winners of the reach oracle on the pool of _reach_oracle, rounded to float32 (and kept inside
    the float32 limits, as the reach launch leaves them)."""
    pl = ro.pool(name, n_seeds, stations)
    arm = pl["arm"]
    q = np.clip(pl["ref"]["q"].astype(np.float32), arm.lower.astype(np.float32), arm.upper.astype(np.float32))
    return pl, q.astype(np.float64)


@functools.lru_cache(maxsize=None)
def pool(name, stations=0, kind="affine", spheres="link"):
    """The 64 rows of the reach pool with the arm term's oracle on ``kind`` of field, and which rows meet the guards.  Read-only."""
    pl, q = reach_q(name, stations)
    arm = arm_spec(name)
    arm = {"link": arm, "one": one_sphere(arm), "full": full_spheres(arm)}[spheres]
    fld = field(kind, name)
    res = arm_terms(arm, q, pl["pose9"], pl["base_T"], pl["batch_each"], [fld], distance=pl["distance"], up=pl["up"])
    ok, _, _ = guard_rows(res, arm, MARGIN, kind == "random")
    return dict(pl, arm=arm, q=q, field=fld, res=res, kind=kind, guarded=ok)


@functools.lru_cache(maxsize=None)
def case(name, stations=0, kind="affine", spheres="link"):
    """Eight rows of the pool THAT MEET THE GUARDS, four per object (batch_each = 4): first one row of every kind of ``coverage`` the
    pool has, then a row with a non-zero gradient, then the pool's rows in order.  The oracle's numbers are the pool's.  Read-only."""
    pl = pool(name, stations, kind, spheres)
    res, cov, ok = pl["res"], coverage(pl["res"], pl["arm"]), pl["guarded"]
    first = lambda m: [int(np.flatnonzero(m & ok)[0])] if (m & ok).any() else []
    order = sum((first(m) for m in cov.values()), []) + first(np.abs(res["grad"]).sum(-1) > 0) + [b for b in range(ro.POOL) if ok[b]]
    rows = [[], []]
    for b in order:
        if b not in rows[b // ro.POOL_EACH] and len(rows[b // ro.POOL_EACH]) < 4:
            rows[b // ro.POOL_EACH].append(b)
    sel = np.array(sorted(rows[0]) + sorted(rows[1]))
    assert len(sel) == 8
    return dict(pl, pose9=pl["pose9"][sel], q=pl["q"][sel], up=pl["up"][sel], batch_each=4, rows=sel,
                res={k: v[sel] for k, v in res.items()})


def assert_coverage(res, arm, tag=""):
    cov = coverage(res, arm)
    print(f"[{tag}] rows without an active sphere {int(cov['none'].sum())}, with several links / all spheres active {int(cov['many'].sum())}, "
          f"with a joint on a limit {int(cov['limit'].sum())}, with a sphere outside the volume {int(cov['outside'].sum())}")
    for k, m in cov.items():
        assert m.any(), (tag, f"no row of the kind {k!r}")


def assert_close(E, grad9, cs, tag=""):
    """The bounds of the GPU test and of the host program: per row |E - E_64| <= 1e-5 m; per row with a non-zero gradient the pose
    gradient norm-wise within 1e-3 |g_64|.  -> (worst |dE|, worst relative gradient error)"""
    res = cs["res"]
    E, g = np.asarray(E, np.float64), np.asarray(grad9, np.float64)[:, :9]
    dE = np.abs(E - res["E"])
    gn = np.linalg.norm(res["grad"], axis=-1)
    nz = gn > 0
    rel = np.linalg.norm(g - res["grad"], axis=-1)[nz] / gn[nz]
    print(f"[{tag}] worst |E - E_64| = {dE.max():.2e} m (bound 1e-5); gradient rows {int(nz.sum())}, worst rel err "
          f"{(rel.max() if nz.any() else 0.0):.2e} (bound 1e-3)")
    assert (dE <= 1e-5).all(), (tag, E, res["E"])
    assert (np.linalg.norm(g[~nz], axis=-1) == 0).all(), (tag, "a gradient where the oracle has none")
    assert (rel <= 1e-3).all(), (tag, rel)
    return float(dE.max()), float(rel.max() if nz.any() else 0.0)
