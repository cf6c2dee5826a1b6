"""The oracle of the arm clearance term against the thing it claims to be, on the CPU (tests/_arm_oracle.py; no GPU).

1. The formula y = (J J' + lambda_a I)^-1 J g_q against central differences of E_arm along the CONVERGED reach iteration (400
   updates, restarted from q) under a small motion of the target, on the reachable rows without a joint on a limit of elbow6, arm7 and
   chain8: relative error <= 2 lambda_a / sigma_min^2(J) + 1e-6 at lambda_a = 1e-6 and 1e-8.
2. Every compared case holds a row with no active sphere, a row with all spheres or >= 2 links active, a row with a joint on a
   limit and a sphere outside the volume.
3. The guards on the inputs hold per sphere: |margin + r - phi| >= 2e-5 (and, on the random field, >= 1e-4 cells from a face).
Also printed: the oracle's own float32 rounding noise (float32 kinematics, points, field and columns, fp64 solve), the measure the
bounds of the GPU test rest on."""
import numpy as np
import pytest
import torch

import _arm_oracle as ao
import _reach_oracle as ro

EPS = 1e-6  # the step of the central differences: metres and radians


def _exp_so3(w):
    return torch.linalg.matrix_exp(ro._hat(w))


def _tracked_energy(arm, fld, base, ps, Rs, q0):
    """E_arm of one station at the joints the reach iteration converges to from q0 for the targets (ps, Rs)"""
    q = ro.solve(arm, base, ps, Rs, q0, n_iter=400)
    Tee, _, _ = ro.fk(arm, q, base)
    err = ro.error(Tee, ps, Rs, ro.RHO).norm(dim=-1)
    n = q.shape[0]
    res = ao.arm_terms(arm, q[:, None].numpy(), np.tile([0, 0, 0, 1, 0, 0, 0, 1, 0], (n, 1)), base[:, :3].numpy(), 1, [fld])
    return res["Ek"][:, 0], err.numpy()


@pytest.mark.parametrize("lam", [1e-6, 1e-8])
@pytest.mark.parametrize("name", ["elbow6", "arm7", "chain8"])
def test_formula_is_the_derivative_along_the_tracked_target(name, lam):
    pl = ao.pool(name, 0, "affine")
    arm, fld, ref = pl["arm"], pl["field"], pl["ref"]
    B = ro.POOL
    q = pl["q"][:, 0]
    res = ao.arm_terms(arm, pl["q"], pl["pose9"], pl["base_T"], pl["batch_each"], [fld], lam=lam)
    ao.assert_coverage(res, arm, f"{name} pool")
    rows = np.flatnonzero(ao.guard_rows(res, arm, ao.MARGIN)[0] & (ref["E"] < 1e-10) & ~res["frozen"].any((1, 2)) & (np.abs(res["y"]).sum((1, 2)) > 0))
    assert len(rows) >= 8, (name, "too few reachable, unclamped rows with a gradient", len(rows))
    base = ro._T44(pl["base_T"])[torch.as_tensor(rows) // pl["batch_each"]]
    qt = torch.as_tensor(q[rows], dtype=ro.F64)
    Tee, _, _ = ro.fk(arm, qt, base)
    ps0, Rs0 = Tee[:, :3, 3], Tee[:, :3, :3]  # the pose the arm IS at: the reached target up to 1e-5, and e = 0 exactly
    fd = np.zeros((len(rows), 6))
    for i in range(6):
        d = torch.zeros(6, dtype=ro.F64)
        d[i] = EPS
        Ep, ep = _tracked_energy(arm, fld, base, ps0 + d[:3], _exp_so3(d[None, 3:]) @ Rs0, qt)
        Em, em = _tracked_energy(arm, fld, base, ps0 - d[:3], _exp_so3(-d[None, 3:]) @ Rs0, qt)
        assert max(ep.max(), em.max()) < 1e-9, (name, "the iteration did not converge", ep.max(), em.max())
        fd[:, i] = (Ep - Em) / (2 * EPS)
    # the same q, the base of each row: y = [dE/dp* ; torque]
    y = res["y"][rows, 0]
    nrm = np.linalg.norm(fd, axis=-1)
    rel = np.linalg.norm(y - fd, axis=-1) / np.maximum(nrm, 1e-300)
    bound = 2 * lam / res["sig2"][rows, 0] + 1e-6
    print(f"[{name} lambda_a={lam:g}] {len(rows)} rows; rel err max {rel.max():.2e}, worst share of the bound {np.max(rel / bound):.2f}; "
          f"sigma_min^2 {res['sig2'][rows, 0].min():.1e} .. {res['sig2'][rows, 0].max():.1e}")
    assert (nrm > 0).all()
    assert (rel <= bound).all(), (name, lam, rel / bound)


@pytest.mark.parametrize("stations", [0, 2])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_cases_cover_the_kinds_and_meet_the_guards(name, stations):
    for kind in ("affine", "multilinear", "random"):
        cs = ao.case(name, stations, kind)
        ok, near, face = ao.guards(cs["res"], cs["arm"], ao.MARGIN, kind == "random")
        print(f"[{name} K={stations} {kind}] {int((~cs['guarded']).sum())} of {len(cs['guarded'])} pool rows left out by the guards; spheres {cs['arm'].n_spheres}; nearest |margin + r - phi| {near:.1e}, face {face:.1e}")
        assert ok
        assert 6 <= cs["arm"].n_spheres <= 64
        if kind == "affine":
            ao.assert_coverage(cs["res"], cs["arm"], f"{name} K={stations} {kind}")
        else:  # the fields without a free half space: both kinds of sphere, and a sphere outside the volume
            act, ins = cs["res"]["active"], cs["res"]["inside"]
            assert act.any() and (ins & ~act).any() and (~ins).any()


def test_float32_noise_of_the_oracle():
    """What the bounds of the GPU test rest on: the oracle in float32 (fp64 solve) against itself in fp64, all five pools."""
    worst_E, worst_g = 0.0, 0.0
    for name in ro.ARM_NAMES:
        for kind in ("affine", "random"):
            pl = ao.pool(name, 0, kind)
            r32 = ao.arm_terms(pl["arm"], pl["q"], pl["pose9"], pl["base_T"], pl["batch_each"], [pl["field"]], up=pl["up"], dtype=torch.float32)
            r64, ok = pl["res"], pl["guarded"]  # the rows that meet the guards on the inputs
            print(f"[{name} {kind}] {int((~ok).sum())} of {len(ok)} pool rows do not meet the guards on the inputs and are left out")
            assert ok.sum() >= 56  # the guards leave out a few rows of a pool, never a kind of row
            assert (r32["active"][ok] == r64["active"][ok]).all(), (name, kind, "an active set differs")
            dE = np.abs(r32["E"] - r64["E"])[ok].max()
            gn = np.linalg.norm(r64["grad"], axis=-1)
            nz = (gn > 0) & ok
            dg = (np.linalg.norm(r32["grad"] - r64["grad"], axis=-1)[nz] / gn[nz])
            print(f"[{name} {kind}] float32 oracle: |dE| max {dE:.1e} m; gradient rel err max {dg.max():.1e}, median {np.median(dg):.1e}")
            worst_E, worst_g = max(worst_E, dE), max(worst_g, dg.max())
    # a quarter of the bounds of the GPU test (1e-5 m, 1e-3): beyond that the bound would have to follow the oracle's noise
    assert worst_E <= 2.5e-6 and worst_g <= 2.5e-4, (worst_E, worst_g)
