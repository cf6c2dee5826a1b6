"""The contract of gq_grasp_select / gq_grasp_distances (include/graspqp_hip.h, "grasp-set selection") in numpy, and the cases
shared by the host test (tests/test_select_body_host.py) and the GPU test (tests/test_gpu_select.py).

Layouts as in the header: Rg (B,9) row-major, link_T (B,L,12) = [A | b] row-major 3x4, t = hand_pose[:, :3], link moments (L,10) =
n, c (3), Cxx Cxy Cxz Cyy Cyz Czz of the centred second moment.  Everything here is fp64 unless a dtype is passed."""
import itertools

import numpy as np


def world(Rg, t, LT, dtype=np.float64):
    """W (B,L,3,4) = [Rg A | Rg b + t]"""
    R = np.asarray(Rg, dtype).reshape(-1, 1, 3, 3)
    T = np.asarray(LT, dtype).reshape(R.shape[0], -1, 3, 4)
    W = np.matmul(R, T)
    W[..., 3] += np.asarray(t, dtype)[:, None, :]
    return W.astype(dtype)


def moments(points, link, n_links):
    """(L,10) fp64 from the samples: a direct sum per link"""
    m = np.zeros((n_links, 10))
    points, link = np.asarray(points, np.float64), np.asarray(link)
    for l in range(n_links):
        p = points[link == l]
        if len(p) == 0:
            continue
        c = p.sum(0) / len(p)
        q = p - c
        C = np.einsum("si,sj->ij", q, q)
        m[l] = [len(p), *c, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]
    return m


def dist2_closed(W, mom, n_samples, batch_each, dtype=np.float64):
    """(n_obj,be,be) d^2 through the closed form, every operation in ``dtype`` (float32: the restatement whose distance from the
    fp64 value is the rounding noise of the formula)."""
    W = np.asarray(W, dtype)
    mom = np.asarray(mom, dtype)
    B, L = W.shape[:2]
    be = batch_each
    Wo = W.reshape(B // be, be, L, 3, 4)
    out = np.zeros((B // be, be, be), dtype)
    two = dtype(2)
    for l in range(L):
        n, c = mom[l, 0], mom[l, 1:4]
        if not n > 0:
            continue
        Cxx, Cxy, Cxz, Cyy, Cyz, Czz = mom[l, 4:]
        D = Wo[:, :, None, l] - Wo[:, None, :, l]  # (n_obj,be,be,3,4)
        x, y, z, b = D[..., 0], D[..., 1], D[..., 2], D[..., 3]
        v = x * c[0] + y * c[1] + z * c[2] + b
        quad = np.maximum(Cxx * x * x + Cyy * y * y + Czz * z * z + two * (Cxy * x * y + Cxz * x * z + Cyz * y * z), dtype(0))
        out += n * (v * v).sum(-1) + quad.sum(-1)
    return (out / dtype(n_samples)).astype(dtype)


def dist2_samples(Rg, t, LT, points, link, batch_each):
    """(n_obj,be,be) d^2 as the definition says: the mean over the samples of |x_w,i(s) - x_w,j(s)|^2, fp64"""
    W = world(Rg, t, LT)
    points, link = np.asarray(points, np.float64), np.asarray(link)
    Wl = W[:, link]  # (B,Ns,3,4)
    X = np.einsum("bsij,sj->bsi", Wl[..., :3], points) + Wl[..., 3]
    B, be = X.shape[0], batch_each
    Xo = X.reshape(B // be, be, -1, 3)
    out = np.zeros((B // be, be, be))
    for i in range(be):
        out[:, i, :] = ((Xo[:, i:i + 1] - Xo) ** 2).sum(-1).mean(-1)
    return out


def feasible(score, terms, tol):
    score = np.asarray(score, np.float64)
    ok = np.isfinite(score)
    for t, tl in enumerate(tol):
        if tl < np.inf:
            with np.errstate(invalid="ignore"):
                ok &= np.asarray(terms[t], np.float64) <= tl
    return ok


def _order_bits(score):
    u = np.asarray(score, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def select(d2, score, terms, tol, batch_each, K, radius2):
    """-> sel (n_obj,K) int32 global rows (-1: unused), n_selected, n_feasible, feasible (B) int32, and the list of the
    (object, row, pick) pairs the greedy run compared with radius2."""
    ok = feasible(score, terms, tol)
    B, be = len(ok), batch_each
    n_obj = B // be
    sel = np.full((n_obj, K), -1, np.int32)
    n_sel, n_feas = np.zeros(n_obj, np.int32), np.zeros(n_obj, np.int32)
    bits = _order_bits(score)
    compared = []
    for o in range(n_obj):
        alive = ok[o * be:(o + 1) * be].copy()
        n_feas[o] = alive.sum()
        key = (bits[o * be:(o + 1) * be] << np.uint64(32)) | np.arange(be, dtype=np.uint64)
        for it in range(K):
            if not alive.any():
                break
            rows = np.nonzero(alive)[0]
            pick = int(rows[np.argmin(key[rows])])
            sel[o, it] = o * be + pick
            n_sel[o] += 1
            alive[pick] = False
            if radius2 > 0:
                for r in np.nonzero(alive)[0]:
                    compared.append((o, int(r), pick))
                    if d2[o, r, pick] < radius2:
                        alive[r] = False
    return sel, n_sel, n_feas, ok.astype(np.int32), compared


# ---- cases whose fp32 arithmetic is exact ---------------------------------------------------------------------------------
def cube_rotations():
    """the 24 proper rotations of the cube, (24,3,3)"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    return np.stack(out)


ROT = cube_rotations()
EXACT_MOMENTS_N = (4, 0, 8, 2, 2)  # link 1 has no samples; Ns = 16


def exact_moments(rng, counts=EXACT_MOMENTS_N):
    """n from ``counts``, centroids multiples of 2^-7, C = G G' with G lower triangular in multiples of 2^-5"""
    m = np.zeros((len(counts), 10))
    for l, n in enumerate(counts):
        if n == 0:
            continue
        c = rng.integers(-8, 9, 3) / 128.0
        G = np.tril(rng.integers(-3, 4, (3, 3))) / 32.0
        C = G @ G.T
        m[l] = [n, *c, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]
    return m


def exact_rows(rng, n_obj, be, L, n_bases, jitter=3):
    """Rows around ``n_bases`` base poses per object: a cube rotation for the hand and for every link, translations and link offsets
    in multiples of 2^-7; a row is its base moved by up to ``jitter`` / 128 per axis, sometimes with one link turned."""
    B = n_obj * be
    Rg, t, LT = np.zeros((B, 9)), np.zeros((B, 3)), np.zeros((B, L, 12))
    for o in range(n_obj):
        bases = []
        for _ in range(n_bases):
            T = np.zeros((L, 3, 4))
            T[:, :, :3] = ROT[rng.integers(0, 24, L)]
            T[:, :, 3] = rng.integers(-32, 33, (L, 3)) / 128.0
            bases.append((ROT[rng.integers(0, 24)], rng.integers(-48, 49, 3) / 128.0, T))
        for r in range(be):
            R0, t0, T0 = bases[rng.integers(0, n_bases)]
            b = o * be + r
            T = T0.copy()
            if rng.random() < 0.2:
                T[rng.integers(0, L), :, :3] = ROT[rng.integers(0, 24)]
            Rg[b], t[b], LT[b] = R0.reshape(9), t0 + rng.integers(-jitter, jitter + 1, 3) / 128.0, T.reshape(L, 12)
    return Rg, t, LT


def _case(rng, n_obj, be, K, radius, n_bases=6, L=len(EXACT_MOMENTS_N), nT=2, tol=(0.0, np.inf), share=0.7, **kw):
    Rg, t, LT = exact_rows(rng, n_obj, be, L, n_bases)
    B = n_obj * be
    score = rng.integers(-64, 65, B) / 16.0
    terms = np.where(rng.random((nT, B)) < share, 0.0, rng.integers(1, 9, (nT, B)) / 16.0)
    c = dict(Rg=Rg, t=t, LT=LT, mom=exact_moments(rng), n_samples=16, batch_each=be, K=K, radius=radius, score=score,
             terms=terms, tol=list(tol))
    c.update(kw)
    return c


def cases():
    rng = np.random.default_rng(20)
    out = {}
    c = _case(rng, 3, 70, 8, 1 / 32)
    c["terms"][0, 70:140] = 0.25  # the second object has no feasible row
    c["terms"][0, 140:204] = 0.5  # the third has six
    out["three_objects_70"] = c
    out["rows_1100"] = _case(rng, 1, 1100, 24, 1 / 32, n_bases=40)
    out["radius_0"] = _case(rng, 2, 70, 12, 0.0)
    out["K_1"] = _case(rng, 2, 33, 1, 1 / 32)
    out["K_batch_each"] = _case(rng, 2, 33, 33, 1 / 64)
    # fewer distinct rows than K: four poses, every row an exact copy of one of them
    c = _case(rng, 1, 20, 8, 1 / 128, share=1.0)
    for b in range(20):
        for k in ("Rg", "t", "LT"):
            c[k][b] = c[k][b % 4]
    out["duplicates_radius_pos"] = c
    out["duplicates_radius_0"] = dict(c, radius=0.0)
    # rows 1 and 2 are row 0 moved by exactly the radius and by one step less: the first stays (strict), the second goes
    c = _case(rng, 1, 6, 6, 1 / 8, n_bases=1, share=1.0)
    for b in range(6):
        for k in ("Rg", "t", "LT"):
            c[k][b] = c[k][0]
    c["t"][1] = c["t"][0] + [1 / 8, 0, 0]
    c["t"][2] = c["t"][0] + [0, 15 / 128, 0]
    c["t"][3] = c["t"][0] + [0.5, 0, 0]
    c["t"][4] = c["t"][0] + [0.5, 1 / 8, 0]
    c["t"][5] = c["t"][0] + [0, 0, -0.5]
    c["score"] = np.asarray([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    out["pair_at_the_radius"] = c
    c = _case(rng, 1, 40, 10, 1 / 32, n_bases=12, share=1.0)
    c["score"][:] = 1.5  # equal scores: ascending row
    c["score"][[7, 21]] = -2.0
    out["equal_scores"] = c
    c = _case(rng, 1, 40, 40, 0.0, share=1.0)
    c["score"][[3, 17]] = np.nan
    c["score"][[4, 30]] = np.inf
    c["score"][5] = -np.inf
    c["score"][[6, 9]] = [-0.0, 0.0]
    c["terms"][0, 8] = np.nan   # under a gate: infeasible
    c["terms"][1, 10] = np.nan  # tol = +inf: not looked at
    c["terms"][1, 11] = np.inf
    out["nan_inf"] = c
    return out


def case_arrays(c):
    """the float32 arrays a case hands to the product: hand_pose (B,3), Rg, LT, mom, score, terms"""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return f(c["t"]), f(c["Rg"]), f(c["LT"]), f(c["mom"]), f(c["score"]), f(c["terms"])


def case_answer(c, dtype=np.float64):
    W = world(c["Rg"], c["t"], c["LT"], dtype)
    d2 = dist2_closed(W, c["mom"], c["n_samples"], c["batch_each"], dtype)
    r2 = dtype(c["radius"]) * dtype(c["radius"])
    return select(d2, c["score"], c["terms"], c["tol"], c["batch_each"], c["K"], r2)[:4], d2
