"""Seeded cases of one MALA* step (propose, z-score, accept, merge), the oracle wrappers and the derived bounds, shared by
tests/test_mala_cases.py (CPU: the cases hold what they claim, the float32 oracle stays inside every bound) and
tests/test_gpu_mala_step.py (the kernels of csrc/loop_dev.h against the oracle).  TEST INFRASTRUCTURE, no GPU.

Every array is drawn in fp64 from np.random.RandomState(seed), rounded to fp32 and handed to both sides, so the oracle
(oracle/ref_cpu/mala.py, unchanged) sees exactly the fp32 inputs, in fp64.  The scalar hyper-parameters travel through the C
ABI as `float`; they are rounded the same way (HP below), so `1 - mu` or `decay ** k` start from the same numbers on both
sides.  Where inf or NaN is involved the expected pattern is that of the oracle run in float32, the precision the reference
itself runs in."""
import warnings

import numpy as np
import torch

from ref_cpu import mala as omala

U = 2.0 ** -24
DELTA = 1e-3  # distance of a decisive draw from the acceptance probability, relative
_r32 = lambda v: float(np.float32(v))
HP = dict(step_size=_r32(0.005), stepsize_period=50, decay=_r32(0.95), mu=_r32(0.98), switch_possibility=_r32(0.4),
          starting_temperature=18.0, annealing_period=30)
PROPOSE_STEPS = (0, 49, 50, 51, 99, 100, 2999, 3000, 5999)  # both sides of the period boundaries (stepsize_period = 50)
ACCEPT_STEPS = (29, 30, 31, 5999, 6000)                     # post-propose counters (annealing_period = 30)
N_CAND = 200


# ---- proposal -----------------------------------------------------------------------------------------------------------
def proposal_case(B, D, n, batch_each=None, clip=False, special=False, seed=0, energy="spread", n_cand=N_CAND):
    """-> dict of numpy inputs of gq_mala_propose.  Gradient magnitudes are log-uniform over 1e-3 .. 1e3 (columns differ by six
    decades, every square is far inside fp32 range), ema in [0, 100] with a few exact zeros, the step counters cycle through
    PROPOSE_STEPS.  special plants a NaN, +inf, -inf, +-1e3 (beyond the clip range of 100) in rows of their own and one
    all-zero column.  u_switch stays 1e-3 away from switch_possibility except for planted 0, nextafter(1, 0) and entries
    exactly equal to switch_possibility (which must not switch); with n > 64 every lane position >= 64 holds a switched and a
    kept contact in the first two rows.  energy: 'spread' (50 .. 80), 'cluster' (1e4 + 1e-2 rand) or 'equal' (the first object
    holds 64.0 in every row: all of its sums are exact in fp32, so std = 0 and z = 0 / 0 = NaN on every route)."""
    r = np.random.RandomState(seed)
    be = B if batch_each is None else batch_each
    assert B % be == 0
    grad = np.sign(r.rand(B, D) - 0.5) * 10.0 ** r.uniform(-3, 3, (B, D))
    ema = 100.0 * r.rand(B, D)
    ema[r.rand(B, D) < 0.05] = 0.0
    planted = {}
    if special:
        zc = D // 2  # the all-zero column: in the second pose slot of a lane where D > 65
        if D > 64:
            zc = 64 + (D - 64) // 2 if D > 65 else 63
        grad[:, zc] = 0.0
        ema[0, zc] = 0.0
        planted["zero_col"] = zc
        rows = [(k * max(B // 5, 1) + 1) % B for k in range(5)]  # B >= 5: five different rows
        cols = [(7 * k + 3) % D for k in range(5)]
        if D > 64:
            cols[0], cols[3] = 64, D - 1  # the NaN and an out-of-range value in the second slot
        cols = [c if c != zc else (c + 1) % D for c in cols]
        for (rw, c, v) in zip(rows, cols, (np.nan, np.inf, -np.inf, 1e3, -1e3)):
            grad[rw, c] = v
        planted.update(nan_row=rows[0], rows=rows, cols=cols)
    u = r.rand(B, n)
    sp = HP["switch_possibility"]
    near = np.abs(u - sp) < 1e-3
    u[near] = sp + np.where(u[near] < sp, -2e-3, 2e-3)
    flat = u.reshape(-1)
    for k, v in enumerate((0.0, float(np.nextafter(np.float32(1), np.float32(0))), sp, sp)):
        if flat.size > k + 2:
            flat[(k * 5 + 2) % flat.size] = v
    if n > 64 and B >= 2:
        u[0, 64:], u[1, 64:] = 0.1, 0.9
    idx = r.randint(0, n_cand, (B, n))
    new_idx = (idx + 1 + r.randint(0, n_cand - 1, (B, n))) % n_cand  # a switch always shows
    if energy == "cluster":
        e = 1e4 + 1e-2 * r.rand(B)
    else:
        e = 50.0 + 30.0 * r.rand(B)
        if energy == "equal":
            e[:be] = 64.0
    step = np.asarray(PROPOSE_STEPS, np.int64)[(np.arange(B) + seed) % len(PROPOSE_STEPS)]
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(B=B, D=D, n=n, batch_each=be, clip=bool(clip), special=bool(special), planted=planted,
                hand_pose=f(r.standard_normal((B, D))), grad=f(grad), ema=f(ema), step=step, idx=idx.astype(np.int64),
                u_switch=f(u), new_idx=new_idx.astype(np.int64), energy=f(e))


def oracle_propose(c, dtype=torch.float64):
    """oracle/ref_cpu/mala.py::propose + z_score on the case in `dtype` -> dict of numpy arrays (g2 = the column means)."""
    t = lambda k: torch.tensor(c[k]).to(dtype)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch: std() of a single row (batch_each = 1) has no degrees of freedom
        hp, idx2, ema, step, s = omala.propose(t("hand_pose"), t("grad"), t("ema"), torch.tensor(c["step"]), torch.tensor(c["idx"]),
                                               t("u_switch"), torch.tensor(c["new_idx"]), step_size=HP["step_size"],
                                               stepsize_period=HP["stepsize_period"], decay=HP["decay"], mu=HP["mu"],
                                               switch_possibility=HP["switch_possibility"], clip_grad=c["clip"])
        g = t("grad")
        if c["clip"]:
            g = g.clip(min=-100, max=100)
            g = torch.where(torch.isnan(g), torch.zeros_like(g), g)
        z = omala.z_score(t("energy"), c["batch_each"])
        stepv = s[:, None] * g / (torch.sqrt(ema) + 1e-6)
        zeroed = (t("hand_pose") - stepv).isnan().any(-1)  # optimizer.py:242-244
    return dict(pose=hp.numpy(), idx=idx2.numpy(), ema=ema.numpy(), step=step.numpy(), s=s.numpy(), z=z.numpy(),
                g2=(g**2).mean(0).numpy(), move=stepv.numpy(), zeroed=zeroed.numpy())


def colsq_route(B, D):
    """Which reduction gq_mala_propose takes for the column means: 'units' (B <= 512 and D <= 64) or 'mean256'."""
    return "units" if (B <= 512 and D <= 64) else "mean256"


def tol_mean(B, route):
    """Relative bound of a column mean of squares: all summands are non-negative, so the relative error of the sum is at most
    (longest chain of additions + 2) U; two more U for the square and the division."""
    chain = -(-B // 16) + 16 if route in ("units", "inline") else -(-B // 256) + 8
    return (chain + 4) * U


def rel(a, b):
    """|a - b| / |b| elementwise, 0 where both are 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))


def same_nonfinite(a, b):
    """NaN / +inf / -inf sit at the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


def check_proposal(c, got, route, label="", floor_of=None):
    """`got` (pose, idx, ema, step, s, z, g2 as numpy) against the fp64 oracle with the derived bounds; non-finite patterns
    against the float32 oracle.  floor_of: the float32 oracle's outputs when `got` is not that run itself.  -> the measured
    figures (s_ratio = error of s over the float32 oracle's error)."""
    o64 = oracle_propose(c)
    o32 = oracle_propose(c, torch.float32) if floor_of is None else floor_of
    B = c["B"]
    fig = {}
    # integers and flags: exact
    assert np.array_equal(got["idx"], o64["idx"]), f"{label}: idx_out"
    assert np.array_equal(got["step"], c["step"] + 1), f"{label}: step + 1"
    # column means
    tm = tol_mean(B, route)
    for k, tol in (("g2", tm), ("ema", tm + 4 * U)):
        assert same_nonfinite(got[k], o32[k]), f"{label}: non-finite pattern of {k}"
        fin = np.isfinite(o64[k]) & np.isfinite(got[k])
        e = rel(got[k], o64[k])[fin].max() if fin.any() else 0.0
        fig[k] = e
        assert e <= tol, f"{label}: {k} relative error {e:.3g} > {tol:.3g}"
    # step size: the larger of 4 x the float32 oracle's error on this case and 16 U
    floor_s = rel(o32["s"], o64["s"]).max()
    tol_s = max(4 * floor_s, 16 * U)
    e = rel(got["s"], o64["s"]).max()
    fig["s"], fig["s_floor"], fig["s_ratio"] = e, floor_s, (e / floor_s if floor_s > 0 else 0.0)
    assert e <= tol_s, f"{label}: s_out relative error {e:.3g} > {tol_s:.3g} (float32 oracle: {floor_s:.3g})"
    # pose: zeroed rows exactly zero, the rest inside |err| <= 4 U |pose| + |move| (tol_s + tol_ema / 2 + 8 U)
    z64 = o64["zeroed"]
    assert np.array_equal(z64, o32["zeroed"]), f"{label}: the float32 oracle zeroes other rows"
    fig["zeroed_rows"] = int(z64.sum())
    assert not (got["pose"][z64] != 0).any(), f"{label}: zeroed rows must be exactly zero"
    assert same_nonfinite(got["pose"], o32["pose"]), f"{label}: non-finite pattern of pose_out"
    live = ~z64
    with np.errstate(all="ignore"):
        allowed = 4 * U * np.abs(o64["pose"]) + np.abs(o64["move"]) * (tol_s + (tm + 4 * U) / 2 + 8 * U)
        err = np.abs(got["pose"].astype(np.float64) - o64["pose"])
    fin = live[:, None] & np.isfinite(o64["pose"]) & np.isfinite(allowed)
    bad = fin & (err > allowed)
    fig["pose_abs"] = err[fin].max() if fin.any() else 0.0
    fig["pose_over_allowed"] = (err[fin] / np.maximum(allowed[fin], 1e-300)).max() if fin.any() else 0.0
    assert not bad.any(), f"{label}: {bad.sum()} pose elements beyond the bound, worst {fig['pose_over_allowed']:.3g} x"
    # z-score: |err| <= 16 U (1 + |z|) max|e_obj| / sd_obj per row
    be = c["batch_each"]
    assert same_nonfinite(got["z"], o32["z"]), f"{label}: non-finite pattern of z"
    if be > 1:
        e64 = c["energy"].astype(np.float64).reshape(-1, be)
        sd = e64.std(1, ddof=1)
        with np.errstate(all="ignore"):
            zb = (16 * U * (1 + np.abs(o64["z"]).reshape(-1, be)) * np.abs(e64).max(1, keepdims=True) / sd[:, None]).reshape(-1)
        fin = np.isfinite(o64["z"]) & np.isfinite(zb)
        ez = np.abs(got["z"].astype(np.float64) - o64["z"])
        fig["z_abs"] = ez[fin].max() if fin.any() else 0.0
        fig["z_over_allowed"] = (ez[fin] / zb[fin]).max() if fin.any() else 0.0
        assert not (fin & (ez > zb)).any(), f"{label}: z beyond the cancellation bound, worst {fig['z_over_allowed']:.3g} x"
    return fig


# ---- accept -------------------------------------------------------------------------------------------------------------
# one category per row, cycled; rows 0 .. 16 hold each once.  x = (e_old - e_new) / T is the target exponent.
ACCEPT_CATS = ("mid", "mid", "up", "far", "over", "under", "under0", "mid", "mid", "tie", "new_nan", "new_pinf", "new_ninf",
               "old_inf", "z_nan", "u0", "reset")


def _oracle_T(e_old, step, z, dtype=torch.float64):
    t = lambda a: torch.tensor(np.asarray(a)).to(dtype)
    with np.errstate(all="ignore"):
        _, T = omala.accept(t(e_old), t(e_old), torch.tensor(np.asarray(step)), t(np.zeros(len(e_old))),
                            z=None if z is None else t(z), starting_temperature=HP["starting_temperature"], decay=HP["decay"],
                            annealing_period=HP["annealing_period"])
    return T.numpy().astype(np.float64)


def decisive_draws(e_old, e_new, step, z, seed=0):
    """Uniform draws (fp32) that put every row of the Metropolis test off the tie.

    With p = exp(x), x = (e_old - e_new) / T from the oracle in fp64: rows with |x| <= 30 and p < 1 get u = p (1 - DELTA) on
    even rows (the oracle accepts) and u = p (1 + DELTA) on odd rows (it rejects), DELTA = 1e-3.  An fp32 evaluation gets x
    with at most a few ulps of x plus the relative error of T (about 3e-6 from powf and erff), so p is off by at most
    30 * 4e-6 + 2 ulps = 1.2e-4 relative, an eighth of DELTA: no fp32 route may decide such a row differently.  Rows with
    p >= 1 get a random u in [0.01, 0.99] and must accept.  Every other row (x < -30: p < 1e-13, down to the underflow of expf below
    x = -104) gets a random u in [0.01, 0.99] and must reject.  Rows whose x is NaN (NaN energy or z) get a random u too: the
    comparison is false whatever u is.  No row is left to chance."""
    r = np.random.RandomState(seed)
    e_old, e_new = np.asarray(e_old, np.float64), np.asarray(e_new, np.float64)
    T = _oracle_T(e_old, step, z)
    with np.errstate(all="ignore"):
        x = (e_old - e_new) / T
        p = np.exp(x)
    B = len(e_old)
    u = r.uniform(0.01, 0.99, B)
    mid = (np.abs(x) <= 30) & (p < 1)
    rows = np.arange(B)
    u = np.where(mid, p * np.where(rows % 2 == 0, 1 - DELTA, 1 + DELTA), u)
    return np.ascontiguousarray(u, dtype=np.float32)


def accept_case(B, D, n, n_terms, with_z, seed=0, with_reset=True):
    """-> dict of numpy inputs of gq_mala_accept: the old state, the new state, the draws.  Row r is of category
    ACCEPT_CATS[r % 17] and carries the post-propose counter ACCEPT_STEPS[r % 5] (17 and 5 are coprime).  The energies are built
    from a target exponent x per category (e_new = e_old - x T in fp64, then rounded; decisive_draws works from the rounded
    values): mid -25 .. -0.01, up 0.01 .. 25, tie exactly 0, far -100 .. -35, over 200 .. 1000 (expf overflows), under -700 ..
    -120 (expf underflows to 0), under0 e_new = e_old + 1e5 with u = 0 (0 < 0 is false in fp64 as well), then the special
    rows: e_new NaN / +inf / -inf, e_old +inf, z NaN, u = 0 on a mid row (accepts), reset_mask on a row with u > p."""
    r = np.random.RandomState(seed)
    cats = np.array([ACCEPT_CATS[i % len(ACCEPT_CATS)] for i in range(B)])
    step = np.asarray(ACCEPT_STEPS, np.int64)[np.arange(B) % len(ACCEPT_STEPS)]
    e_old = np.float32(50.0 + 30.0 * r.rand(B)).astype(np.float64)
    z = np.float32(r.standard_normal(B)) if with_z else None
    if with_z:
        z[cats == "z_nan"] = np.nan
    T = _oracle_T(e_old, step, z)
    T = np.where(np.isfinite(T), T, 18.0)
    lo_hi = dict(mid=(-25, -0.01), up=(0.01, 25), tie=(0, 0), far=(-100, -35), over=(200, 1000), under=(-700, -120), under0=(0, 0),
                 new_nan=(0, 0), new_pinf=(0, 0), new_ninf=(0, 0), old_inf=(-5, 5), z_nan=(-5, 5), u0=(-25, -0.01), reset=(-25, -0.01))
    x = np.array([r.uniform(*lo_hi[c]) for c in cats])
    e_new = e_old - x * T
    e_new[cats == "under0"] = e_old[cats == "under0"] + 1e5
    e_new[cats == "new_nan"], e_new[cats == "new_pinf"], e_new[cats == "new_ninf"] = np.nan, np.inf, -np.inf
    e_old[cats == "old_inf"] = np.inf
    e_new = np.float32(e_new)
    e_old = np.float32(e_old)
    u = decisive_draws(e_old, e_new, step, z, seed + 1)
    u[(cats == "under0") | (cats == "u0")] = 0.0
    reset = np.zeros(B, np.uint8)
    if with_reset:
        rs = np.nonzero(cats == "reset")[0]
        reset[rs] = 1
        # the reset rows must be rows that the test itself rejects: u = p (1 + DELTA) whatever their parity
        if len(rs):
            with np.errstate(all="ignore"):
                p = np.exp((e_old[rs].astype(np.float64) - e_new[rs]) / _oracle_T(e_old, step, z)[rs])
            u[rs] = np.float32(p * (1 + DELTA))
    f = lambda *s: np.float32(r.standard_normal(s))
    return dict(B=B, D=D, n=n, n_terms=n_terms, cats=cats, step=step, energy_old=e_old, energy_new=e_new, z=z, u_accept=u,
                reset_mask=reset if with_reset else None,
                pose_old=f(B, D), pose_new=f(B, D), grad_old=f(B, D), grad_new=f(B, D),
                idx_old=r.randint(0, N_CAND, (B, n)).astype(np.int64), idx_new=r.randint(N_CAND, 2 * N_CAND, (B, n)).astype(np.int64),
                terms_old=f(n_terms, B), terms_new=f(n_terms, B))


def oracle_accept(c, dtype=torch.float64, e_new=None):
    """oracle/ref_cpu/mala.py::accept on the case in `dtype` -> (accept (B,) bool, temperature (B,) fp64), numpy."""
    t = lambda a: torch.tensor(np.asarray(a)).to(dtype)
    with np.errstate(all="ignore"):
        acc, T = omala.accept(t(c["energy_old"]), t(c["energy_new"] if e_new is None else e_new), torch.tensor(c["step"]),
                              t(c["u_accept"]), z=None if c["z"] is None else t(c["z"]),
                              reset_mask=None if c["reset_mask"] is None else torch.tensor(c["reset_mask"]).bool(),
                              starting_temperature=HP["starting_temperature"], decay=HP["decay"],
                              annealing_period=HP["annealing_period"])
    return acc.numpy(), T.numpy().astype(np.float64)


def check_accept(c, acc, temperature, label="", e_new=None):
    """Accept vector: exact against the fp64 oracle AND the float32 oracle, no row excluded.  Temperature: the larger of 4 x the
    float32 oracle's error on the case and 16 U, relative; NaN where the oracle's is.  -> figures (T_ratio)."""
    a64, T64 = oracle_accept(c, e_new=e_new)
    a32, T32 = oracle_accept(c, torch.float32, e_new=e_new)
    assert np.array_equal(a64, a32), f"{label}: the case is not decisive: float32 and fp64 oracle differ in rows {np.nonzero(a64 != a32)[0]}"
    acc = np.asarray(acc)
    assert set(np.unique(acc).tolist()) <= {0, 1}, f"{label}: accept flags {np.unique(acc)}"
    wrong = np.nonzero(acc.astype(bool) != a64)[0]
    assert wrong.size == 0, f"{label}: accept differs from the oracle in rows {wrong[:10]}"
    assert same_nonfinite(temperature, T32), f"{label}: non-finite pattern of the temperature"
    fin = np.isfinite(T64)
    floor = rel(T32, T64)[fin].max()
    e = rel(temperature, T64)[fin].max()
    tol = max(4 * floor, 16 * U)
    assert e <= tol, f"{label}: temperature relative error {e:.3g} > {tol:.3g} (float32 oracle: {floor:.3g})"
    return dict(T=e, T_floor=floor, T_ratio=(e / floor if floor > 0 else 0.0), accepted=int(a64.sum()), rows=len(a64))


def check_merge(c, acc, got, before=None, label="", new=None):
    """Accepted rows hold the bits of the new state, rejected rows those of the old state.  got: energy, pose, idx, grad, terms.
    new: the new state where it is not the case's (the fused tail computes energy, gradient and terms itself)."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a
    a = np.asarray(acc).astype(bool)
    new = new or dict(energy=c["energy_new"], pose=c["pose_new"], idx=c["idx_new"], grad=c["grad_new"], terms=c["terms_new"])
    old = dict(energy=c["energy_old"], pose=c["pose_old"], idx=c["idx_old"], grad=c["grad_old"], terms=c["terms_old"])
    for k in ("energy", "pose", "idx", "grad", "terms"):
        if k == "terms":
            if got[k].shape[0] == 0:
                continue
            want = np.where(a[None, :], bits(new[k]), bits(old[k]))
        else:
            m = a.reshape(-1, *([1] * (old[k].ndim - 1)))
            want = np.where(m, bits(new[k]), bits(old[k]))
        assert got[k].dtype == old[k].dtype and np.array_equal(bits(got[k]), want), f"{label}: merged {k}"


# ---- the case lists, shared by the CPU and the GPU test -------------------------------------------------------------------
# (B, D): every size at which the column means take another route or another trip count
MEAN_SIZES = [(1, 25), (15, 25), (16, 25), (17, 25), (512, 25), (513, 25), (1025, 25), (1, 73), (255, 73), (257, 73), (64, 11),
              (64, 64)]
# (B, D, n): the sizes above with four contacts, then contacts and pose dimensions around the second slot of a lane at B = 17
PROPOSAL_SIZES = [(B, D, 4) for B, D in MEAN_SIZES] + [(17, 25, n) for n in (1, 64, 65, 130)] + [(17, D, 4) for D in (10, 64, 65, 128)] + [
    (17, 128, 130)]
# (n_obj, batch_each, energy kind)
ZSCORE_CASES = [(n_obj, be, "spread") for be in (1, 2, 3, 63, 64, 65, 200) for n_obj in (1, 3)] + [
    (3, 65, "cluster"), (1, 200, "cluster"), (3, 3, "equal"), (3, 65, "equal"), (1, 200, "equal")]
ACCEPT_D, ACCEPT_N, ACCEPT_TERMS, ACCEPT_B = (10, 25, 64, 65, 73, 128), (1, 4, 64, 65, 130), (0, 5, 11, 64), (1, 17, 513)


def accept_shapes():
    """Every (D, n) pair once, n_terms cycling so that each value meets each D and each n."""
    out = []
    for i, D in enumerate(ACCEPT_D):
        for j, n in enumerate(ACCEPT_N):
            out.append((D, n, ACCEPT_TERMS[(i + j) % len(ACCEPT_TERMS)]))
    return out
