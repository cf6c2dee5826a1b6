"""The fp64 oracle of the reach term on its own (tests/_reach_oracle.py), no GPU.

1. The settled share: the comparison with the kernel is restricted to settled rows (E at M and at 2M updates agree to 1e-3 relative,
   or both are below 1e-12).  That cap is a condition: at least 3/4 of the generated cases of every arm are settled, for every
   (seeds, stations) the GPU test runs, and every pool holds the three kinds of row a compared set needs.
2. The definition of the gradient: on settled out-of-range rows whose winning configuration has no joint on a limit, the gradient
   with the final q held fixed equals a central difference of the fully converged E (M = 400) to 1e-4 norm-wise -- the envelope
   theorem: there dq = 0 means J'e = 0, E is stationary in q.  "Fully converged" is checked, not assumed: update 401 moves no joint
   by more than 1e-10 (past the outer boundary a stretched arm ends in a two-cycle about the singular configuration, whose E repeats
   without being stationary).  (With a joint ON its limit the fixed point of the clamped iteration
   satisfies c_j . (J J' + lambda I)^-1 e = 0 for the free joints, not c_j . e = 0: it is not the constrained minimiser, and the
   gradient is an approximation there, as it is wherever the iteration has not converged.)
3. The log map and its gradient are finite at e = 0."""
import numpy as np
import pytest
import torch

import _reach_oracle as ro


@pytest.mark.parametrize("n_seeds,stations", [(1, 0), (4, 0), (1, 2), (4, 2)])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_three_quarters_of_the_generated_cases_are_settled(name, n_seeds, stations):
    pl = ro.pool(name, n_seeds, stations)
    share = pl["settled"].mean()
    print(f"[{name} S={n_seeds} K={stations}] settled {int(pl['settled'].sum())} of {ro.POOL} (generator seed {pl['seed']})")
    assert share >= 0.75
    cs = ro.case(name, n_seeds, stations)
    assert cs["pose9"].shape == (8, 9) and (cs["rows"][:4] < ro.POOL_EACH).all() and (cs["rows"][4:] >= ro.POOL_EACH).all()
    ro.compared_set(cs, name)


def _converged(arm, base, ps, Rs, n_iter=400):
    q = ro.solve(arm, base, ps, Rs, torch.as_tensor(arm.seeds[:1], dtype=ro.F64).expand(ps.shape[0], -1), n_iter)
    Tee, _, _ = ro.fk(arm, q, base)
    e = ro.error(Tee, ps, Rs, ro.RHO)
    return (e * e).sum(-1), e, q


def _under_actuated(name):
    """short3, and gantry4: the first four joints of gantry6 (three prismatic axes and the wrist's yaw) with its tool."""
    if name == "short3":
        return ro.arm_spec(name)
    types, Ts, axes, lo, hi, tool = ro.arm_arrays("gantry6")
    return ro.ArmSpec(types[:4], Ts[:4], axes[:4], lo[:4], hi[:4], tool)


@pytest.mark.parametrize("name", ["short3", "gantry4"])
def test_envelope_gradient_equals_the_central_difference_of_the_converged_energy(name):
    """Out of range without the outer boundary and without a clamp: arms of fewer than six joints, whose targets are reachable
    poses turned by 0.2 .. 0.4 rad and moved by about 1 .. 3 cm -- six conditions on three or four joints, two kinds of chain
    (all revolute; prismatic axes with one revolute joint).  For an arm of six or more joints an unreachable target is either past
    a limit (the clamped case of the module docstring) or past the singular boundary, where only an excess below about
    lambda / 0.1 m, E < 1e-6, reaches a fixed point at all; the generator's own out-of-range rows are of these two kinds, which is
    why the targets are built here.  Every row must qualify.  Three things are compared: the oracle's autograd gradient
    (``ro.reach(...)["grad"]``, final q detached), the closed form 2 e_p / 2 rho e_w that the kernel implements, and the central
    difference of the converged energy."""
    arm = _under_actuated(name)
    N = arm.n_joints
    rng = np.random.default_rng(31)
    n = 4
    base34 = ro.T((-0.4, 0.05, -0.2), (0, 0, 0.7))[None, :3]  # fp64: a float32 base is a rotation to 6e-8 only, and the closed form
                                                              # equals autograd through the log map ON the manifold
    base = ro._T44(base34)[[0] * n]
    ps, Rs = torch.zeros(n, 3, dtype=ro.F64), torch.zeros(n, 3, 3, dtype=ro.F64)
    for b in range(n):
        Tw = arm.fk(arm.lower + (0.3 + 0.4 * rng.random(N)) * (arm.upper - arm.lower), base[0, :3].numpy())
        w = rng.normal(size=3)
        w *= rng.uniform(0.2, 0.4) / np.linalg.norm(w)
        Rs[b] = torch.linalg.matrix_exp(ro._hat(torch.as_tensor(w))) @ torch.as_tensor(Tw[:3, :3])
        ps[b] = torch.as_tensor(Tw[:3, 3] + rng.normal(size=3) * 0.012)
    Rs = ro.gramschmidt(torch.cat([Rs[:, :, 0], Rs[:, :, 1]], 1))  # exactly what the pose's rot6d entries stand for
    E, e, q = _converged(arm, base, ps, Rs)
    _, _, q1 = _converged(arm, base, ps, Rs, 401)  # a fixed point, not the two-cycle of a stretched arm past the outer boundary
    E24, _, _ = _converged(arm, base, ps, Rs, ro.M)
    E48, _, _ = _converged(arm, base, ps, Rs, 2 * ro.M)
    lo, hi = torch.as_tensor(arm.lower), torch.as_tensor(arm.upper)
    free = ~((q <= lo) | (q >= hi)).any(-1)
    ok = torch.as_tensor(ro.settled(E24.numpy(), E48.numpy())) & (E > 1e-6) & free & ((q1 - q).abs().amax(-1) <= 1e-10)
    print(f"[{name}] out-of-range rows, settled, at a fixed point at M = 400, no joint on a limit: {ok.tolist()}")
    assert ok.all()
    # the oracle's autograd gradient of the pose against the closed form, carried to the pose as gq_fk_backward carries gRt
    pose9 = torch.cat([ps, Rs[:, :, 0], Rs[:, :, 1]], 1).numpy()
    ref = ro.reach(arm, pose9, base34, n, n_iter=400)
    assert np.allclose(ref["E"], E.numpy(), rtol=1e-9)
    for b in range(n):
        R = Rs[b].numpy()
        gp, tau = 2 * e[b, :3].numpy(), 2 * ro.RHO * e[b, 3:].numpy()
        th = R.T @ tau
        K9 = 0.5 * np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
        want = ro.pose_grad_of_gRt(np.concatenate([-R.T @ gp, K9.ravel()]), pose9[b])
        err = np.linalg.norm(ref["grad"][b] - want) / np.linalg.norm(ref["grad"][b])
        print(f"[{name}] row {b}: autograd of the oracle vs closed form {err:.2e}")
        assert err <= 1e-9
    h = 1e-5
    for b in range(n):
        g = torch.cat([2 * e[b, :3], 2 * ro.RHO * e[b, 3:]])  # dE/dp* = 2 e_p, torque 2 rho e_w = 2 rho^2 log
        cd = torch.zeros(6, dtype=ro.F64)
        for i in range(6):
            d = torch.zeros(6, dtype=ro.F64)
            d[i] = h
            vals = []
            for sgn in (1.0, -1.0):
                Rp = torch.linalg.matrix_exp(ro._hat(sgn * d[3:])) @ Rs[b]
                vals.append(_converged(arm, base[b:b + 1], ps[b:b + 1] + sgn * d[:3], Rp[None])[0][0])
            cd[i] = (vals[0] - vals[1]) / (2 * h)
        err = float(torch.linalg.norm(g - cd) / torch.linalg.norm(cd))
        print(f"[{name}] row {b}: E {float(E[b]):.3e}, |g| {float(torch.linalg.norm(cd)):.3e}, envelope vs central difference {err:.2e}")
        assert err <= 1e-4


def test_log_map_and_gradient_are_finite_at_zero_error():
    arm = ro.arm_spec("elbow6")
    q = torch.as_tensor(arm.seeds[:1], dtype=ro.F64)
    base = torch.eye(4, dtype=ro.F64)[None]
    Tee, _, _ = ro.fk(arm, q, base)
    ps, Rs = Tee[:, :3, 3].clone().requires_grad_(), Tee[:, :3, :3].clone().requires_grad_()
    e = ro.error(Tee.detach(), ps, Rs, ro.RHO)
    E = (e * e).sum()
    gp, gR = torch.autograd.grad(E, (ps, Rs))
    assert float(E.detach()) == 0.0 and torch.isfinite(gp).all() and torch.isfinite(gR).all() and float(gR.abs().max()) == 0.0
    # and the oracle's pose gradient on a reachable row is finite and small
    cs = ro.case("gantry6", 1, 0)
    assert np.isfinite(cs["ref"]["grad"]).all()
