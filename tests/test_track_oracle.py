"""The fp64 oracle of the approach tracking term (tests/_track_oracle.py) checked on its own, without a GPU:

1. the share of STABLE rows of every pool (at most 4 of 64 may be left out) and the kinds of row every compared set must hold;
2. the closed-form gradient the kernel implements (per waypoint 2 c e_p on the target position, the torque 2 c rho e_w on the target
   rotation, gathered in the gRt layout) equals autograd's with every q_i detached;
3. the envelope statement: where every waypoint has reached a fixed point with no joint on a limit, that gradient IS the gradient of
   the path energy -- the warm start drops out.  Checked on short3 with T = 4, U = 100 on the rows whose E agrees at U and U + 1
   updates to 1e-9 (a two-cycle repeats at U and U + 2, not at U + 1): central differences of E_track in the nine pose entries with
   h = 1e-6, relative error <= 1e-4, the bound of test_reach_oracle.py for the same theorem.  The other arms run the same check on
   every row that meets the rule and print the count; zero rows is an answer and is printed as such."""
import numpy as np
import pytest

import _reach_oracle as ro
import _track_oracle as to


@pytest.mark.parametrize("T,U", to.SHAPES)
@pytest.mark.parametrize("n_seeds", to.SEEDS)
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_pools_are_stable_and_hold_every_kind_of_row(name, n_seeds, T, U):
    pl = to.pool(name, n_seeds, T, U)
    st, ref = pl["stable"], pl["ref"]
    kinds = to._kinds_present(pl["arm"], ref, st)
    print(f"[{name} S={n_seeds} T={T} U={U}] stable {int(st.sum())} of {ro.POOL}; clamped {int(kinds[0].sum())}, E > 1e-3 {int(kinds[1].sum())}, "
          f"E < 1e-10 {int(kinds[2].sum()) if len(kinds) > 2 else 'not asked (three joints)'}")
    assert ro.POOL - int(st.sum()) <= to.MAX_LEFT_OUT
    assert all(k.any() for k in kinds)
    assert (name == "short3") == (len(kinds) == 2)
    to.compared_set(to.case(name, n_seeds, T, U), f"case {name} S={n_seeds} T={T} U={U}")  # the eight-row case holds them too
    # the path stays inside the limits, the first waypoint starts from q_start
    arm = pl["arm"]
    assert (ref["q"] >= arm.lower).all() and (ref["q"] <= arm.upper).all()
    assert (ref["step"] >= np.abs(ref["q"][:, 0] - pl["q_start"]).max(-1) - 1e-15).all()
    assert np.allclose(ref["worst"], ref["Ei"].max(-1)) and np.allclose(ref["E"], ref["Ei"].mean(-1))


@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_closed_form_gradient_equals_autograd(name):
    pl = to.pool(name, 4, 8, 3)
    ref = pl["ref"]
    g = to.closed_form_grad(pl["pose9"], ref["e"], pl["T"], pl["axis"], pl["distance"], up=pl["up"])
    err = np.linalg.norm(g - ref["grad"]) / np.linalg.norm(ref["grad"])
    print(f"[{name}] closed form vs autograd (q_i detached): {err:.2e}")
    assert err <= 1e-9


def _envelope(name, n_seeds=1, T=4, U=100, h=1e-6):
    """-> (rows that meet the U against U + 1 rule with no joint on a limit, per-row |cd - g|, per-row |g|, per-row largest joint
    move of update U + 1 over the waypoints)"""
    pl = to.pool(name, n_seeds, 4, 2)
    arm, pose9, q0 = pl["arm"], pl["pose9"].astype(np.float64), pl["q_start"]
    base = pl["base_T"][np.arange(ro.POOL) // ro.POOL_EACH]  # a base per row, batch_each = 1
    run = lambda p, b, q, u: to.track(arm, p, b, 1, q, T, u, pl["axis"], pl["distance"])
    r0, r1 = run(pose9, base, q0, U), run(pose9, base, q0, U + 1)
    ok = np.flatnonzero((np.abs(r0["E"] - r1["E"]) <= 1e-9) & ~r0["clamped"] & ~r1["clamped"])
    if len(ok) == 0:
        return ok, np.zeros(0), np.zeros(0), np.zeros(0)
    # all 18 perturbed copies of the qualifying rows in one batch
    P = np.tile(pose9[ok], (18, 1))
    for c in range(9):
        P[(2 * c) * len(ok):(2 * c + 1) * len(ok), c] += h
        P[(2 * c + 1) * len(ok):(2 * c + 2) * len(ok), c] -= h
    E = run(P, np.tile(base[ok], (18, 1, 1)), np.tile(q0[ok], (18, 1)), U)["E"].reshape(9, 2, len(ok))
    cd = ((E[:, 0] - E[:, 1]) / (2 * h)).T
    g = r0["grad"][ok]
    return ok, np.linalg.norm(cd - g, axis=-1), np.linalg.norm(g, axis=-1), np.abs(r0["q"][ok] - r1["q"][ok]).max((1, 2))


def test_envelope_on_short3():
    ok, err, gn, _ = _envelope("short3")
    rel = err / gn
    print(f"[short3] {len(ok)} rows settled by the U against U+1 rule with no joint on a limit; envelope vs central difference, worst "
          f"relative error {rel.max():.2e} (|g| {gn.min():.2e} .. {gn.max():.2e})")
    assert len(ok) >= 6
    assert (rel <= 1e-4).all()


@pytest.mark.parametrize("name", [n for n in ro.ARM_NAMES if n != "short3"])
def test_envelope_on_the_other_arms(name):
    """Every row that meets the rule.  Two things differ from short3.  These arms reach most targets, where E and its gradient
    vanish: the comparison carries the absolute floor 1e-9 of a central difference with h = 1e-6 in fp64 (rounding eps E / h <= 1e-10
    for E <= 1 m^2, truncation h^2 times a third derivative of order one), below which a relative error says nothing.  And the
    rule on E is a weak proxy for the theorem's premise when E itself is of the order 1e-8: on elbow6 5 of the 52 rows that meet it
    (E 5e-16 .. 7e-8) are NOT at a fixed point -- near a singular configuration update 101 still moves a joint by 1e-6 .. 3e-3 and E
    falls by a tenth per update -- and there the gradient is 0.2 .. 0.6 off in relative terms (|g| <= 7e-5): the "finite U" case of
    the header, not a two-cycle.  Every row that passes moves by at most 1.3e-10.  So the premise is checked as test_reach_oracle.py
    checks it: update U + 1 moves no joint by more than 1e-10; the rows the rule admits and the premise does not are counted and
    printed with their worst figure, not compared."""
    ok, err, gn, moved = _envelope(name)
    if len(ok) == 0:
        print(f"[{name}] 0 rows meet the U against U+1 rule with no joint on a limit: nothing to compare")
        return
    share = err / (1e-4 * gn + 1e-9)
    fixed = moved <= 1e-10
    big = fixed & (gn > 1e-5)
    print(f"[{name}] {len(ok)} rows meet the rule, {int(fixed.sum())} of them at a fixed point ({int(big.sum())} with |g| > 1e-5); worst "
          f"err / (1e-4 |g| + 1e-9) on those = {share[fixed].max() if fixed.any() else 0.0:.2e}"
          + (f", worst relative error {np.max(err[big] / gn[big]):.2e}" if big.any() else "")
          + (f"; still moving: {int((~fixed).sum())} rows, joint move {moved[~fixed].min():.1e} .. {moved[~fixed].max():.1e}, worst share "
             f"{share[~fixed].max():.2e}" if (~fixed).any() else ""))
    assert (share[fixed] <= 1.0).all()
