"""The contract of gq_init_select (include/graspqp_hip.h, "screened hull candidates") in numpy, and the cases shared by the host
test (tests/test_init_select_host.py) and the GPU test (tests/test_gpu_init_scene.py).

Points are lattice points k 2^-7 with integer k < 64: every coordinate difference, square and sum of three squares is a multiple
of 2^-14 below 2^-1, exact in float32 under any contraction, so an fp32 and an fp64 oracle agree (asserted by the host test).
Penalties are multiples of 1/8 with NaNs planted."""
import numpy as np


def select(points, penalty, K, tol=0.0, dtype=np.float64):
    """points (M,3), penalty (M) -> (sel (K) int32, n_feasible).  Phase 1: farthest-point sampling inside A = {penalty <= tol} from
    min A, a pick leaves A, first index on ties.  Phase 2: the candidates outside A by ascending (penalty, index), NaN last."""
    P = np.asarray(points, dtype=dtype)
    pen = np.asarray(penalty, dtype=np.float32)
    M = P.shape[0]
    with np.errstate(invalid="ignore"):
        feas = pen <= np.float32(tol)  # False for NaN, True for -0.0 at tol = 0
    nA = int(feas.sum())
    sel = []
    inA = feas.copy()
    d = np.full(M, np.inf, dtype=dtype)
    if nA:
        c = int(np.flatnonzero(feas)[0])
        for _ in range(min(K, nA)):
            sel.append(c)
            inA[c] = False
            if not inA.any():
                break
            d = np.minimum(d, ((P - P[c]) ** 2).sum(-1, dtype=dtype))
            c = int(np.argmax(np.where(inA, d, -1.0)))  # argmax: the first index among equals
    out = np.flatnonzero(~feas)
    key = np.where(np.isnan(pen[out]), np.inf, pen[out].astype(np.float64))
    rank = np.where(np.isnan(pen[out]), 1, 0)
    order = np.lexsort((out, key, rank))  # NaN after +inf, then penalty, then index
    sel.extend(int(i) for i in out[order][:K - len(sel)])
    assert len(sel) == K
    return np.asarray(sel, dtype=np.int32), nA


def select_all(points, penalty, K, tol=0.0, dtype=np.float64):
    """(n_obj,M,3), (n_obj,M) -> (sel (n_obj,K) int32, n_feasible (n_obj) int32)."""
    r = [select(p, q, K, tol, dtype) for p, q in zip(points, penalty)]
    return np.stack([s for s, _ in r]), np.asarray([n for _, n in r], dtype=np.int32)


def lattice(rng, M, distinct=True):
    """M lattice points k 2^-7, k in 0..63 per axis; ``distinct``: no two equal."""
    if distinct:
        flat = rng.choice(64 ** 3, size=M, replace=False)
    else:
        flat = rng.integers(0, 64 ** 3, size=M)
    k = np.stack([flat // 4096, (flat // 64) % 64, flat % 64], -1)
    return (k * 2.0 ** -7).astype(np.float32)


def penalties(rng, M, share, n_nan=3):
    """Feasible (exactly 0) with probability ``share``, otherwise a multiple of 1/8 in 1/8..4; ``n_nan`` NaNs among the infeasible."""
    pen = (rng.integers(1, 33, size=M) / 8.0).astype(np.float32)
    pen[rng.random(M) < share] = 0.0
    bad = np.flatnonzero(pen > 0)
    if len(bad):
        pen[rng.choice(bad, size=min(n_nan, len(bad)), replace=False)] = np.nan
    return pen


def random_cases():
    """(M, K, feasible share) of the issue: name -> dict(points (1,M,3), penalty (1,M), K, tol)."""
    out = {}
    for M, K, share in [(300, 40, 0.5), (300, 40, 0.05), (2100, 33, 0.3), (64, 64, 0.0), (1500, 70, 1.0)]:
        rng = np.random.default_rng(1000 * M + K)
        pen = penalties(rng, M, share)
        if (M, K, share) == (300, 40, 0.05):  # exactly 18 feasible: phase 2 fills 22
            pen[pen == 0] = 0.5
            pen[rng.choice(M, size=18, replace=False)] = 0.0
        out[f"M{M}_K{K}_share{share}"] = dict(points=lattice(rng, M)[None], penalty=pen[None], K=K, tol=0.0)
    return out


def hand_made_cases():
    out = {}
    rng = np.random.default_rng(7)
    M, K = 200, 24

    def base():
        return lattice(rng, M), np.full(M, 1.0, dtype=np.float32) + (rng.integers(0, 8, size=M) / 8.0).astype(np.float32)

    for name, n_feas in [("exactly_K_feasible", K), ("K_minus_1_feasible", K - 1)]:
        p, pen = base()
        pen[rng.choice(M, size=n_feas, replace=False)] = 0.0
        out[name] = dict(points=p[None], penalty=pen[None], K=K, tol=0.0)
    p, pen = base()
    pen[::3] = 0.0
    out["M_equals_K"] = dict(points=p[None, :50], penalty=pen[None, :50], K=50, tol=0.0)
    out["K_1"] = dict(points=p[None], penalty=pen[None], K=1, tol=0.0)
    pen1 = pen.copy()
    pen1[:] = 2.0
    pen1[5] = np.nan
    out["K_1_nothing_feasible"] = dict(points=p[None], penalty=pen1[None], K=1, tol=0.0)
    # duplicate points among the feasible: 30 feasible candidates on 6 distinct points, K = 12 picks stay distinct
    p, pen = base()
    feas = rng.choice(M, size=30, replace=False)
    pen[feas] = 0.0
    p[feas] = p[feas[:6]][np.arange(30) % 6]
    out["duplicate_points"] = dict(points=p[None], penalty=pen[None], K=12, tol=0.0)
    # +inf, NaN and -0.0 penalties: -0.0 is feasible, the fill order is finite < +inf < NaN
    p, pen = base()
    pen[:] = np.float32(np.inf)
    pen[[3, 50, 120]] = np.float32(-0.0)
    pen[[10, 11]] = 0.0
    pen[[7, 150]] = np.nan
    pen[[20, 90, 91]] = [0.75, 0.25, 0.25]
    out["inf_nan_negzero"] = dict(points=p[None], penalty=pen[None], K=M, tol=0.0)
    p, pen = base()
    pen[:] = (rng.integers(0, 9, size=M) / 8.0).astype(np.float32)  # 0, 1/8, 1/4 are feasible at tol = 0.25
    out["tol_0.25"] = dict(points=p[None], penalty=pen[None], K=90, tol=0.25)
    p, pen = base()
    pen[:] = 1.5
    pen[[4, 9]] = 0.0
    out["equal_penalties_by_index"] = dict(points=p[None], penalty=pen[None], K=20, tol=0.0)
    # three objects, three masks: most feasible, few feasible, none
    P3 = np.stack([lattice(rng, M) for _ in range(3)])
    pen3 = np.stack([penalties(rng, M, 0.7), penalties(rng, M, 0.04), penalties(rng, M, 0.0)])
    out["three_objects"] = dict(points=P3, penalty=pen3, K=K, tol=0.0)
    return out


def cases():
    c = random_cases()
    c.update(hand_made_cases())
    return c


# Ten points in units of 2^-7: nine on the x axis, index 8 at (8, 24, 0); penalties below, K = 6, tol = 0.
# A = {1, 2, 4, 6, 8} (index 8 is -0.0; 7 is NaN).  Squared distances in units of 2^-14:
#   t = 0: c = min A = 1 at (8,0,0).   d: 2 -> 1, 4 -> 64, 6 -> 576, 8 -> 576          -> 6 (the first of the two at 576)
#   t = 1: c = 6 at (32,0,0).          d: 2 -> 1, 4 -> 64, 8 -> min(576, 1152) = 576   -> 8
#   t = 2: c = 8 at (8,24,0).          d: 2 -> min(1, 577) = 1, 4 -> min(64, 640) = 64 -> 4
#   t = 3: c = 4 at (16,0,0).          d: 2 -> min(1, 49) = 1                          -> 2
#   t = 4: c = 2; A is empty: 5 feasible < K = 6, so one fill from {0: 0.5, 3: 0.25, 5: +inf, 7: NaN, 9: 0.25}
#   t = 5: the smallest (penalty, index) = (0.25, 3)
TEN_XY = np.array([[0, 0], [8, 0], [9, 0], [40, 0], [16, 0], [3, 0], [32, 0], [20, 0], [8, 24], [50, 0]])
TEN_PENALTY = np.array([0.5, 0.0, 0.0, 0.25, 0.0, np.inf, 0.0, np.nan, -0.0, 0.25], dtype=np.float32)
TEN_SEL, TEN_FEASIBLE = [1, 6, 8, 4, 2, 3], 5


def ten_point_case():
    p = np.zeros((10, 3), dtype=np.float32)
    p[:, :2] = TEN_XY * 2.0 ** -7
    return dict(points=p[None], penalty=TEN_PENALTY[None], K=6, tol=0.0)
