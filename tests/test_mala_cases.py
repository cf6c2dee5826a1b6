"""The cases of tests/_mala_cases.py hold what they claim, and the reference alone stays inside every bound that
tests/test_gpu_mala_step.py puts on the kernels: oracle/ref_cpu/mala.py run in float32 against its own fp64 run, on every
case, with the decisive draws giving the same decisions in both precisions on all rows.  A later change of a case or of a
bound cannot outrun the reference silently.  No GPU."""
import numpy as np
import pytest
import torch

import _mala_cases as mc


def test_proposal_cases_contain_what_they_claim():
    sp = np.float32(mc.HP["switch_possibility"])
    for (B, D, n) in mc.PROPOSAL_SIZES:
        for clip in (False, True):
            c = mc.proposal_case(B, D, n, clip=clip, special=clip, seed=B + D + n)
            g = c["grad"]
            fin = np.isfinite(g) & (g != 0)
            assert np.isfinite(g[np.isfinite(g)].astype(np.float32) ** 2).all()
            assert (np.abs(g[fin]) >= 0.99e-3).all() and (np.abs(g[fin]) <= 1.01e3).all()
            if B * D >= 400:
                assert np.abs(g[fin]).min() < 1e-2 and np.abs(g[fin]).max() > 1e2 and (c["ema"] == 0).any()
            assert c["ema"].min() >= 0 and c["ema"].max() <= 100
            assert set(c["step"].tolist()) == set(mc.PROPOSE_STEPS[: B]) or B < len(mc.PROPOSE_STEPS)
            if B >= len(mc.PROPOSE_STEPS):  # rows on both sides of each period boundary
                k = set((c["step"] // mc.HP["stepsize_period"]).tolist())
                assert {0, 1, 2, 59, 60, 119} <= k
            u = c["u_switch"]
            off = np.abs(u.astype(np.float64) - float(sp))
            assert ((off >= 0.99e-3) | (u == sp)).all()
            if B * n >= 20:
                assert (u == 0).any() and (u == np.nextafter(np.float32(1), np.float32(0))).any() and (u == sp).any()
                o = mc.oracle_propose(c)
                assert np.array_equal(o["idx"][u == sp], c["idx"][u == sp]), "a draw equal to the probability must not switch"
                assert (o["idx"] != c["idx"]).any() and (o["idx"] == c["idx"]).any()
            if n > 64:
                o = mc.oracle_propose(c)
                sw = o["idx"] != c["idx"]
                assert sw[:, 64:].any(0).all() and (~sw[:, 64:]).any(0).all(), "a switched and a kept contact at every lane position >= 64"
            if clip:
                assert np.isnan(g).sum() == 1 and np.isposinf(g).sum() == 1 and np.isneginf(g).sum() == 1
                assert (g == 1e3).sum() == 1 and (g == -1e3).sum() == 1 and (g[:, c["planted"]["zero_col"]] == 0).all()
                if D > 64:
                    assert (c["planted"]["zero_col"] >= 64 or D == 65) and c["planted"]["cols"][0] >= 64
    # NaN-zeroed proposal rows: with the clip the NaN is removed first (optimizer.py:211-213), so the zeroed rows of the special
    # cases show with the clip off
    for (B, D, n) in mc.PROPOSAL_SIZES:
        c = mc.proposal_case(B, D, n, clip=False, special=True, seed=B + D + n)
        o = mc.oracle_propose(c)
        assert o["zeroed"].any() and (o["pose"][o["zeroed"]] == 0).all()
        assert o["zeroed"][c["planted"]["nan_row"]]
        if B >= 5:
            assert not o["zeroed"].all()


@pytest.mark.parametrize("B,D,n", mc.PROPOSAL_SIZES)
def test_float32_oracle_meets_the_proposal_bounds(B, D, n):
    worst = {}
    for clip, special in ((False, False), (True, True), (False, True)):
        c = mc.proposal_case(B, D, n, clip=clip, special=special, seed=B + D + n)
        o32 = mc.oracle_propose(c, torch.float32)
        for route in {mc.colsq_route(B, D), "inline" if (B <= 512 and D <= 64) else mc.colsq_route(B, D)}:
            fig = mc.check_proposal(c, o32, route, label=f"float32 oracle B={B} D={D} n={n} clip={clip} special={special}")
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0), v)
    print(f"B={B} D={D} n={n}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("n_obj,be,kind", mc.ZSCORE_CASES)
def test_float32_oracle_meets_the_z_bound(n_obj, be, kind):
    c = mc.proposal_case(n_obj * be, 25, 4, batch_each=be, seed=be + n_obj, energy=kind)
    o64 = mc.oracle_propose(c)
    if be == 1:
        assert np.isnan(o64["z"]).all()
    if kind == "equal":
        assert np.isnan(o64["z"][:be]).all() and (be == 1 or n_obj == 1 or np.isfinite(o64["z"][be:]).all())
    if kind == "cluster":
        e = c["energy"].reshape(-1, be).astype(np.float64)
        assert (e.std(1, ddof=1) < 1e-2).all() and (e > 9999).all()
    fig = mc.check_proposal(c, mc.oracle_propose(c, torch.float32), mc.colsq_route(c["B"], 25), label=f"float32 oracle z {n_obj}x{be} {kind}")
    print(f"n_obj={n_obj} batch_each={be} {kind}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))


@pytest.mark.parametrize("B", mc.ACCEPT_B)
@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("with_reset", [False, True])
def test_accept_cases_are_decisive_in_both_precisions(B, with_z, with_reset):
    c = mc.accept_case(B, 25, 4, 5, with_z, seed=B, with_reset=with_reset)
    a64, T64 = mc.oracle_accept(c)
    a32, T32 = mc.oracle_accept(c, torch.float32)
    assert np.array_equal(a64, a32), "decisive draws: the same decisions in float32 and fp64 on ALL rows"
    fig = mc.check_accept(c, a32.astype(np.uint8), T32.astype(np.float32), label=f"float32 oracle B={B}")
    print(f"B={B} z={with_z} reset={with_reset}: accepted {fig['accepted']} of {B}, temperature error {fig['T']:.3g}")
    cats = c["cats"]
    want = dict(up=True, tie=True, over=True, far=False, under=False, under0=False, new_nan=False, new_pinf=False, new_ninf=True,
                old_inf=True, u0=True, reset=with_reset or None)
    if with_z:
        want["z_nan"] = False
    for k, w in want.items():
        if w is not None and (cats == k).any():
            assert (a64[cats == k] == w).all(), k
    mid = np.nonzero(cats == "mid")[0]
    assert (a64[mid[mid % 2 == 0]]).all() and not (a64[mid[mid % 2 == 1]]).any()
    if B >= 17:
        assert a64.any() and not a64.all(), "both decisions occur"
        assert set(c["step"].tolist()) == set(mc.ACCEPT_STEPS)
        assert {0, 1, 199, 200} <= set((c["step"] // mc.HP["annealing_period"]).tolist())
        # what the special rows claim
        x = (c["energy_old"].astype(np.float64) - c["energy_new"]) / T64
        with np.errstate(all="ignore"):
            assert (np.exp(x[cats == "over"]).astype(np.float32) == np.inf).all(), "expf overflow"
            assert (np.exp(x[cats == "under"]).astype(np.float32) == 0).all() and (x[cats == "under"] < -110).all(), "expf underflow"
            p = np.exp(x)
        assert (c["u_accept"][cats == "u0"] == 0).all() and (c["u_accept"][cats == "under0"] == 0).all()
        if with_reset:
            rs = cats == "reset"
            assert (c["reset_mask"][rs] == 1).all() and (c["u_accept"][rs] > p[rs]).all() and c["reset_mask"].sum() == rs.sum()
        # the margin of every decisive row is DELTA, up to the rounding of u
        m = (np.abs(x) <= 30) & (p < 1) & (c["u_accept"] > 0)
        margin = np.abs(c["u_accept"][m] / p[m] - 1)
        assert m.sum() >= 4 and (np.abs(margin - mc.DELTA) < 1e-6).all()


def test_decisive_draws_on_the_shapes_of_the_merge_cases():
    for (D, n, nt) in mc.accept_shapes():
        c = mc.accept_case(17, D, n, nt, True, seed=D + n)
        assert c["terms_new"].shape == (nt, 17) and c["pose_new"].shape == (17, D) and c["idx_new"].shape == (17, n)
        assert not np.intersect1d(c["idx_new"], c["idx_old"]).size, "new and old indices must be told apart"
        a64, _ = mc.oracle_accept(c)
        a32, _ = mc.oracle_accept(c, torch.float32)
        assert np.array_equal(a64, a32) and a64.any() and not a64.all()
