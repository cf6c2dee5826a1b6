"""fp64 oracle of gq_pen_bwd_body (csrc/pen_dev.h) and a builder of synthetic cases for it -- numpy only.

The backward of the hand-penetration query is a pure map of plain arrays: with x_h = R^T (s - t) the hand-frame position
of a surface point (Rg row-major, t = hand_pose[:, :3]), G = gvec and w the upstream gradient on dis,

    f_l       = - sum_{link = l} w G                 wrench[:, l, 0:3]
    m_l       = - sum_{link = l} w x_h x G           wrench[:, l, 3:6]   (about the hand origin)
    gRt[0:3]  =   sum w G
    gRt[3:12] =   sum w x_h (x) G                    row-major, K[a][b] = x_a G_b

over the points with w != 0 only (-0.0 does not contribute, NaN does).  Without w (the fused E_pen form) w = w_pen [dis > 0]
and e_pen = sum relu(dis).

Tolerance (derived, not tuned).  Beside every accumulator the oracle forms S = sum_i |addend_i| -- for the moments and K
with |x_h|_2 in place of the component of x_h, so that the rounding of x_h itself, which is relative to |s - t|, is covered.
The kernel adds the n addends of a round as 64 lane-strided chains (<= ceil(n / 64) additions each) and a 6-level tree, and
the rounds one after the other (<= r additions): the standard forward bound of that order is (ceil(n / 64) + 6 + r) u S with
u = 2^-24.  An addend carries at most 8 fp32 roundings (the subtraction s - t, the 3x3 transform, the product w G, the cross
or outer product).  Hence

    tol = (ceil(n_max / 64) + r + 14) 2^-24 S + 1e-30,     r = ceil(P / 1024) + 1,

with n_max the largest number of contributing points of any row of the case (a round takes up at least four 256-point
slices, so r bounds the number of rounds).  e_pen adds exact addends: thread-local chains of ceil(P / 256) additions, the
6-level tree, three additions across the wavefronts: tol = (ceil(P / 256) + 9) 2^-24 S + 1e-30."""
import math

import numpy as np

U = 2.0 ** -24
SENTINEL = 12345.0


def rounds(P):
    """r of the tolerance: an upper bound of the number of rounds of the point loop."""
    return -(-int(P) // 1024) + 1


def tol(S, n_max, P):
    """The derived tolerance of an accumulator with absolute sum S (module docstring)."""
    return (math.ceil(n_max / 64) + rounds(P) + 14) * U * np.asarray(S, np.float64) + 1e-30


def tol_e_pen(S, P):
    return (math.ceil(P / 256) + 9) * U * np.asarray(S, np.float64) + 1e-30


def oracle(surf, hand_pose, Rg, link, gvec, L, batch_each, w=None, dis=None, w_pen=None):
    """-> wrench (B,L,6), gRt (B,12), e_pen (B) or None, bound = {"wrench", "gRt", "e_pen" or None: tolerances of the same
    shapes, "n_max"}.  All inputs as the kernel reads them (fp32 arrays); the arithmetic is fp64."""
    surf, hp, G = (np.asarray(a, np.float64) for a in (surf, hand_pose, gvec))
    B, P = G.shape[:2]
    R = np.asarray(Rg, np.float64).reshape(B, 3, 3)
    link = np.asarray(link)
    e_pen = None
    if w is None:
        d = np.asarray(dis, np.float64)
        w = np.where(d > 0, float(w_pen), 0.0)
        e_pen = S_e = np.where(d > 0, d, 0.0).sum(1)  # relu as the kernel writes it: a NaN distance counts as 0
    w = np.asarray(w, np.float64)
    on = w != 0  # NaN != 0
    wrench, gRt = np.zeros((B, L, 6)), np.zeros((B, 12))
    S_w, S_g = np.zeros((B, L, 6)), np.zeros((B, 12))
    for b in range(B):
        i = np.nonzero(on[b])[0]
        if not i.size:
            continue
        x = (surf[b // batch_each, i] - hp[b, :3]) @ R[b]  # R^T (s - t)
        wG = w[b, i, None] * G[b, i]
        xn = np.linalg.norm(x, axis=1)
        f, m = -wG, -np.cross(x, wG)
        Sf, Sm = np.abs(wG), np.repeat((xn * np.linalg.norm(wG, axis=1))[:, None], 3, 1)
        li = link[b, i]
        assert li.min() >= 0 and li.max() < L, "link id out of range"
        np.add.at(wrench[b, :, 0:3], li, f)
        np.add.at(wrench[b, :, 3:6], li, m)
        np.add.at(S_w[b, :, 0:3], li, Sf)
        np.add.at(S_w[b, :, 3:6], li, Sm)
        gRt[b, 0:3] = wG.sum(0)
        gRt[b, 3:12] = (x[:, :, None] * wG[:, None, :]).sum(0).reshape(9)
        S_g[b, 0:3] = np.abs(wG).sum(0)
        S_g[b, 3:12] = (xn[:, None, None] * np.abs(wG)[:, None, :]).sum(0).repeat(3, 0).reshape(9)
    n_max = int(on.sum(1).max())
    bound = {"wrench": tol(S_w, n_max, P), "gRt": tol(S_g, n_max, P), "e_pen": None if e_pen is None else tol_e_pen(S_e, P),
             "n_max": n_max}
    return wrench, gRt, e_pen, bound


def make_case(B, P, L, n_obj=1, seed=0, density=0.5, fused=False, D=9):
    """A synthetic case, every array as the kernel reads it.  ``density``: the share of contributing points, one number or
    one per row.  fused = False: "w" ~ N(0,1) on that share and exactly 0 elsewhere ("dis" is None); fused = True: "dis" in
    (1e-4, 0.02) on that share and negative elsewhere -- in turn exactly 0.0, -1e30 (what the penetration-only query
    leaves) and a finite negative -- with "w" None.  At the other points link = 0 and gvec = 0: what the forward leaves
    there, because the ops layer zero-initialises."""
    assert B % n_obj == 0 and D >= 9
    rng = np.random.default_rng(seed)
    dens = np.broadcast_to(np.asarray(density, np.float64), (B,))
    surf = rng.uniform(-0.1, 0.1, (n_obj, P, 3)).astype(np.float32)
    t = rng.normal(size=(B, 3))
    t *= (0.1 * rng.uniform(0, 1, (B, 1)) / np.linalg.norm(t, axis=1, keepdims=True))
    hp = rng.normal(size=(B, D)).astype(np.float32)
    hp[:, :3] = t
    Rg = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].reshape(B, 9).astype(np.float32)
    on = rng.random((B, P)) < dens[:, None]  # density 1.0: every point, 0.0: none
    link = np.where(on, rng.integers(0, L, (B, P)), 0).astype(np.int32)
    g = rng.normal(size=(B, P, 3))
    g *= rng.uniform(0.5, 1.0, (B, P, 1)) / np.linalg.norm(g, axis=2, keepdims=True)
    gvec = np.where(on[..., None], g, 0.0).astype(np.float32)
    w = dis = None
    if fused:
        neg = np.stack([np.zeros((B, P)), np.full((B, P), -1e30), -rng.uniform(1e-4, 0.02, (B, P))])
        pick = (np.cumsum(~on, axis=1) - 1) % 3  # the k-th non-contributing point of a row takes kind k % 3
        dis = np.where(on, rng.uniform(1e-4, 0.02, (B, P)), np.take_along_axis(neg, pick[None], 0)[0]).astype(np.float32)
    else:
        w = np.where(on, rng.normal(size=(B, P)), 0.0).astype(np.float32)
        assert (w[on] != 0).all()
    return {"surf": surf, "hand_pose": hp, "Rg": Rg, "link": link, "gvec": gvec, "w": w, "dis": dis, "L": L,
            "batch_each": B // n_obj, "n_obj": n_obj, "B": B, "P": P}


def contributing(case):
    """(B,P) bool: the points the kernel takes up."""
    return case["w"] != 0 if case["w"] is not None else case["dis"] > 0


def slice_counts(case):
    """(B, ceil(P/256)) contributing points per 256-point slice."""
    on = contributing(case)
    B, P = on.shape
    pad = np.zeros((B, -(-P // 256) * 256), bool)
    pad[:, :P] = on
    return pad.reshape(B, -1, 256).sum(2)


def round_plan(counts, K, cap=1024):
    """The rounds the kernel takes for one row's per-slice counts: a list of (first slice, kfit, entries).  A round looks
    at K slices and takes up the longest prefix whose entries fit the list of ``cap`` (at least four always do)."""
    out, s = [], 0
    counts = list(counts)
    while s < len(counts):
        kfit = run = 0
        for k in range(K):
            c = counts[s + k] if s + k < len(counts) else 0
            if run + c > cap:
                break
            kfit, run = k + 1, run + c
        out.append((s, kfit, run))
        s += kfit
    return out


def oracle_of(case, w_pen=100.0):
    return oracle(case["surf"], case["hand_pose"], case["Rg"], case["link"], case["gvec"], case["L"], case["batch_each"],
                  w=case["w"], dis=case["dis"], w_pen=w_pen)


# ---- the kernel's constants and the cases of tests/test_gpu_pen_backward.py --------------------------------------------
def kernel_constants():
    """GQ_PENB_K, GQ_PENB_LIST (csrc/pen_dev.h) and the small K of the stand-alone launcher (csrc/sdf.hip), read from the
    sources: a case built for one value says so when the value changes, instead of passing without reaching its path."""
    import os
    import re

    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graspqp_amd", "csrc")
    pen, sdf = open(os.path.join(src, "pen_dev.h")).read(), open(os.path.join(src, "sdf.hip")).read()
    ks = sorted({int(k) for k in re.findall(r"gq_hand_pen_bwd_kernel<(\d+)>", sdf)})
    assert len(ks) == 1, "the launcher is expected to pick between one small K and GQ_PENB_K"
    return {"K": int(re.search(r"#define GQ_PENB_K (\d+)", pen).group(1)),
            "LIST": int(re.search(r"#define GQ_PENB_LIST (\d+)", pen).group(1)), "K_small": ks[0]}


def launcher_K(P, c):
    return c["K_small"] if P <= c["K_small"] * 256 else c["K"]


def plans(case, c):
    """Per row: the rounds of the stand-alone kernel the launcher picks for this case."""
    return [round_plan(row, launcher_K(case["P"], c), c["LIST"]) for row in slice_counts(case)]


def link_groups(L):
    """(wave tasks of the fold, whether the 12 global sums ride in the last link group, links in the last group)."""
    n = (L + 3) // 4
    last = L - 4 * (n - 1)
    return (n if last <= 2 else n + 1), last <= 2, last


RAGGED_P = (1, 255, 256, 257, 2500, 2560)
K16_P = (2561, 4096)
ROUNDS_P = (4097, 9000)
GROUP_L = (1, 2, 3, 4, 5, 12, 16, 17, 19, 20, 160)


def case_ragged(P, fused):
    return make_case(4, P, 14, seed=100 + P, density=[1.0, 0.5, 0.25, 0.5] if P == 1 else 0.3, fused=fused)


def case_k16(P, fused):
    return make_case(3, P, 14, seed=200 + P, density=0.2, fused=fused)


def force_on(case, b, p, link, value):
    """Make point p of row b contribute: weight (or distance) ``value``, the given link, a gradient of norm 0.75."""
    case["w" if case["w"] is not None else "dis"][b, p] = value
    case["link"][b, p] = link
    case["gvec"][b, p] = np.float32(0.75) * np.array([2.0, -1.0, 2.0], np.float32) / np.float32(3.0)
    return case


def case_rounds(P, fused):
    c = make_case(3, P, 14, seed=300 + P, density=0.1, fused=fused)
    for b in range(3):  # the last point always contributes: the ragged last round (of one point at P = 4097) is never empty
        force_on(c, b, P - 1, 13 - b, 0.01 if fused else -1.5)
    return c


def case_overflow(P, fused):
    return (make_case(3, 2500, 14, seed=400, density=[1.0, 0.45, 0.0], fused=fused) if P == 2500 else
            make_case(2, 9000, 14, seed=401, density=1.0, fused=fused))


def case_groups(L, fused):
    return make_case(3, 600, L, seed=500 + L, density=0.5, fused=fused)


def require_single_round(case, c, K):
    """One round that takes up every slice, in the K-instantiation asked for."""
    assert launcher_K(case["P"], c) == c[K], f"P = {case['P']} no longer takes the {K} kernel"
    for p, n in zip(plans(case, c), contributing(case).sum(1)):
        assert p == [(0, c[K], n)], f"not a single round: {p}"  # slices past P count as empty ones: kfit = K
    assert contributing(case).any()


def require_several_rounds(case, c):
    """More than one round, none of them cut short by the list: kfit == K until the slices run out."""
    K = launcher_K(case["P"], c)
    assert K == c["K"] and case["P"] > K * 256, "P must exceed one round of the large instantiation"
    for b, p in enumerate(plans(case, c)):
        assert len(p) >= 2, f"row {b}: one round only"
        assert all(kfit == K for _, kfit, _ in p), f"row {b}: the list cuts a round short: {p}"
        assert all(n > 0 for _, _, n in p), f"row {b}: a round without entries: {p}"
    assert case["P"] % (K * 256) != 0 and case["P"] % 256 != 0, "the last round and its last slice must be ragged"


def require_overflow_2500(case, c):
    p0, p1, p2 = plans(case, c)
    cnt = slice_counts(case)
    K = launcher_K(2500, c)
    assert K == c["K_small"] and c["LIST"] == 4 * 256, "row 0 is built for a list of exactly four full slices"
    assert cnt[0, : c["K_small"]].sum() >= c["LIST"] + 1, "row 0: >= 1025 contributing points among its first 2560"
    assert p0 == [(0, 4, 1024), (4, 4, 1024), (8, K, 2500 - 2048)], p0  # kfit = 4 exactly: four full slices fill the list
    # row 1: the first round stops at a slice that does not fit behind a partly filled list
    s, kfit, n = p1[0]
    assert kfit < K and n < c["LIST"] and n + cnt[1, kfit] > c["LIST"] and cnt[1, kfit] > 0, p1
    assert len(p1) >= 2 and sum(n for _, _, n in p1) == cnt[1].sum()
    assert cnt[2].sum() == 0 and p2 == [(0, K, 0)], "row 2 has no contributing point"


def require_overflow_9000(case, c):
    assert launcher_K(9000, c) == c["K"]
    for p in plans(case, c):
        assert all(kfit == 4 for _, kfit, _ in p[:-1]) and len(p) == -(-9000 // 1024), p  # every round cut short at four slices
        assert p[-1][2] == 9000 - 1024 * (len(p) - 1)


def require_groups(case, c):
    L = case["L"]
    tasks, ride, last = link_groups(L)
    want = {1: (1, True, 1), 2: (1, True, 2), 3: (2, False, 3), 4: (2, False, 4), 5: (2, True, 1), 12: (4, False, 4),
            16: (5, False, 4), 17: (5, True, 1), 19: (6, False, 3), 20: (6, False, 4), 160: (41, False, 4)}[L]
    assert (tasks, ride, last) == want
    on = contributing(case)
    assert (case["link"][on] == L - 1).any() and (case["link"][on] == 0).any(), "first and last link must be hit"
    if L <= 20:
        for b in range(case["B"]):
            assert set(case["link"][b][on[b]].tolist()) == set(range(L)), f"row {b}: a link without a point"
    assert len(plans(case, c)[0]) == 1
