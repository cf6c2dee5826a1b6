"""Pins tests/_pen_backward_oracle.py itself, without a GPU: the oracle's four formulas against torch fp64 autograd of the
energy they are the gradient of, the monotonicity of its derived tolerance, and the properties of the synthetic cases that
tests/test_gpu_pen_backward.py relies on to reach the kernel's paths (contributing counts per row and per 256-point
slice, round plans, link-group counts) -- stated on the builder's output, with the kernel's constants read from its source."""
import numpy as np
import pytest
import torch

import _pen_backward_oracle as pbo


def _small(seed, L=5, fused=False):
    return pbo.make_case(4, 37, L, n_obj=2, seed=seed, density=0.6, fused=fused)


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_gRt_is_the_gradient_of_the_energy_in_t_and_R():
    """E(t, R) = sum_i w_i G_i . R^T (s_i - t):  dE/dt = -R gsum,  dE/dR = R K."""
    c = _small(1)
    # dE/dR = R K needs R R^T = I: an fp64 orthonormal R here (the fp32 cast of the builder is orthonormal to 1e-7 only)
    c["Rg"] = np.linalg.qr(c["Rg"].astype(np.float64).reshape(-1, 3, 3))[0].reshape(-1, 9)
    _, gRt, _, _ = pbo.oracle_of(c)
    B = c["B"]
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    t = t64(c["hand_pose"][:, :3]).requires_grad_()
    R = t64(c["Rg"]).reshape(B, 3, 3).requires_grad_()
    s = t64(c["surf"]).repeat_interleave(c["batch_each"], 0)
    xh = torch.einsum("bka,bpk->bpa", R, s - t[:, None])  # R^T (s - t)
    E = (t64(c["w"])[..., None] * t64(c["gvec"]) * xh).sum()
    E.backward()
    Rn = R.detach().numpy()
    assert _rel(-np.einsum("bak,bk->ba", Rn, gRt[:, :3]), t.grad.numpy()) < 1e-12
    assert _rel(Rn @ gRt[:, 3:].reshape(B, 3, 3), R.grad.numpy()) < 1e-12


def test_wrench_is_the_gradient_in_a_rigid_motion_of_the_link():
    """dis of a point depends on where it lies in the frame of its link, so moving link l rigidly by (p, theta) about the
    hand origin moves its points by the inverse motion: E_l = sum_{link = l} w G . M^-1 x_h, and (f_l, m_l) = dE_l / d(p, theta)
    at the identity."""
    c = _small(2, L=3)
    wrench, _, _, _ = pbo.oracle_of(c)
    B, L = c["B"], c["L"]
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    R = t64(c["Rg"]).reshape(B, 3, 3)
    s = t64(c["surf"]).repeat_interleave(c["batch_each"], 0)
    xh = torch.einsum("bka,bpk->bpa", R, s - t64(c["hand_pose"][:, :3])[:, None])
    mot = torch.zeros(B, L, 6, dtype=torch.float64, requires_grad=True)
    th = mot[..., 3:]
    z = torch.zeros_like(th[..., 0])
    skew = torch.stack([z, -th[..., 2], th[..., 1], th[..., 2], z, -th[..., 0], -th[..., 1], th[..., 0], z], -1).reshape(B, L, 3, 3)
    M = torch.linalg.matrix_exp(skew)  # (B,L,3,3)
    li = torch.tensor(c["link"], dtype=torch.long)
    Mi = M[torch.arange(B)[:, None], li]    # (B,P,3,3)
    pi = mot[..., :3][torch.arange(B)[:, None], li]
    xm = torch.einsum("bpka,bpk->bpa", Mi, xh - pi)  # M^-1 x = M^T (x - p)
    E = (t64(c["w"])[..., None] * t64(c["gvec"]) * xm).sum()
    E.backward()
    assert _rel(wrench, mot.grad.numpy()) < 1e-12
    assert np.abs(wrench).min() > 0, "every link of the small case must carry points"


def test_fused_form_is_the_weighted_form_with_w_pen_on_the_penetrating_points():
    c = _small(3, fused=True)
    assert (c["dis"] == 0.0).any() and (c["dis"] == -1e30).any() and (c["dis"] > 0).any()
    wr, g, e, bd = pbo.oracle_of(c, w_pen=100.0)
    c2 = dict(c, w=np.where(c["dis"] > 0, np.float32(100.0), np.float32(0.0)), dis=None)
    wr2, g2, e2, bd2 = pbo.oracle_of(c2)
    assert e2 is None and bd2["e_pen"] is None
    assert np.array_equal(wr, wr2) and np.array_equal(g, g2) and np.array_equal(bd["wrench"], bd2["wrench"])
    assert _rel(e, np.maximum(c["dis"].astype(np.float64), 0).sum(1)) < 1e-15


def test_only_nonzero_weights_contribute():
    """w = +-0.0 never reaches the sums (a NaN gvec there stays out), w = NaN does, and only into what its point feeds."""
    c = _small(4, L=5)
    on = pbo.contributing(c)
    off = np.argwhere(~on)
    (b0, p0), (b1, p1) = off[0], off[1]
    c["w"][b1, p1] = -0.0
    c["gvec"][b0, p0] = c["gvec"][b1, p1] = np.nan
    wr, g, _, bd = pbo.oracle_of(c)
    assert np.isfinite(wr).all() and np.isfinite(g).all() and np.isfinite(bd["wrench"]).all()
    b, p = np.argwhere(on)[0]
    c["w"][b, p] = np.nan
    wr, g, _, _ = pbo.oracle_of(c)
    bad = np.zeros_like(wr, bool)
    bad[b, c["link"][b, p]] = True
    assert np.array_equal(np.isnan(wr), bad) and np.isnan(g[b]).all() and np.isfinite(np.delete(g, b, 0)).all()


def test_bound_is_monotone_in_the_count_and_in_the_inputs():
    S = np.array([0.0, 1e-3, 2.0])
    for P in (1, 2500, 9000):
        prev = None
        for n in (0, 1, 64, 65, 1024, 1025, 9000):
            t = pbo.tol(S, n, P)
            assert (t > 0).all() and (np.diff(t) > 0).all()  # in S
            assert prev is None or (t >= prev).all()         # in n_max
            prev = t
        assert (pbo.tol(S, 64, P + 1024) >= pbo.tol(S, 64, P)).all() and (pbo.tol_e_pen(S, P + 256) >= pbo.tol_e_pen(S, P)).all()
    # through the oracle: scaling the weights, the gradients or the lever arms scales S, more contributing points add to it
    c = _small(5)
    base = pbo.oracle_of(c)[3]
    for k, f in (("w", 2.0), ("gvec", 2.0)):
        bd = pbo.oracle_of(dict(c, **{k: c[k] * np.float32(f)}))[3]
        assert (bd["wrench"] >= base["wrench"]).all() and (bd["gRt"] >= base["gRt"]).all() and bd["gRt"].sum() > 1.9 * base["gRt"].sum()
    far = pbo.oracle_of(dict(c, surf=c["surf"] * np.float32(3.0)))[3]
    assert (far["gRt"][:, :3] == base["gRt"][:, :3]).all() and far["gRt"][:, 3:].sum() > base["gRt"][:, 3:].sum()
    w2 = c["w"].copy()
    w2[w2 == 0] = 0.5
    more = pbo.oracle_of(dict(c, w=w2, gvec=np.where(c["gvec"] == 0, np.float32(0.5), c["gvec"])))[3]
    assert more["n_max"] > base["n_max"] and (more["gRt"] > base["gRt"]).all()
    assert pbo.rounds(1) == 2 and pbo.rounds(1024) == 2 and pbo.rounds(1025) == 3 and pbo.rounds(9000) == 10


def test_builder_output_is_what_the_issue_of_the_kernel_reads():
    for fused in (False, True):
        c = pbo.make_case(6, 300, 14, n_obj=2, seed=9, density=0.5, fused=fused, D=25)
        on = pbo.contributing(c)
        assert c["batch_each"] == 3 and c["surf"].shape == (2, 300, 3) and c["hand_pose"].shape == (6, 25)
        assert all(c[k].dtype == np.float32 for k in ("surf", "hand_pose", "Rg", "gvec")) and c["link"].dtype == np.int32
        assert np.abs(c["surf"]).max() <= 0.1 and np.linalg.norm(c["hand_pose"][:, :3], axis=1).max() <= 0.1 + 1e-7
        R = c["Rg"].astype(np.float64).reshape(6, 3, 3)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
        n = np.linalg.norm(c["gvec"], axis=2)
        assert (n[on] >= 0.5 - 1e-6).all() and (n[on] <= 1 + 1e-6).all()
        assert (c["link"][~on] == 0).all() and (c["gvec"][~on] == 0).all() and c["link"].max() == 13
        assert 0.4 < on.mean() < 0.6
        if fused:
            assert c["w"] is None and (c["dis"][~on] <= 0).all()
            assert (c["dis"] == 0.0).any() and (c["dis"] == -1e30).any() and ((c["dis"] < 0) & (c["dis"] > -1)).any()
        else:
            assert c["dis"] is None and (c["w"][~on] == 0).all() and (c["w"] < 0).any() and (c["w"] > 0).any()
    a, b = pbo.make_case(2, 50, 3, seed=1, fused=False), pbo.make_case(2, 50, 3, seed=1, fused=True)
    assert all(np.array_equal(a[k], b[k]) for k in ("surf", "hand_pose", "Rg", "link", "gvec")), "both forms share one geometry"


def test_round_plan_follows_the_kernel():
    assert pbo.round_plan([256] * 10, 10) == [(0, 4, 1024), (4, 4, 1024), (8, 10, 512)]
    assert pbo.round_plan([200] * 10, 10) == [(0, 5, 1000), (5, 10, 1000)]
    assert pbo.round_plan([0] * 36, 16) == [(0, 16, 0), (16, 16, 0), (32, 16, 0)]
    assert pbo.round_plan([256, 256, 256, 255, 2], 10) == [(0, 4, 1023), (4, 10, 2)]  # one entry short of full: the slice of 2 waits


@pytest.mark.parametrize("fused", [False, True])
def test_tolerance_tells_one_wrong_entry_from_rounding(fused):
    """The errors the end-to-end 2e-3 gradient checks would hide -- one dropped list entry, one entry folded into the wrong
    link, one entry with a transposed K -- move some accumulator by more than 3 x its tolerance, even in the densest case
    (9000 contributing points in a row, where the tolerance is widest) and for an entry of median weight."""
    for case in (pbo.case_overflow(9000, fused), pbo.case_overflow(2500, fused), pbo.case_rounds(9000, fused)):
        wr, g, e, bd = pbo.oracle_of(case)
        on = pbo.contributing(case)[0]
        key = "dis" if fused else "w"
        mag = np.abs(case[key][0].astype(np.float64)) * np.linalg.norm(case["gvec"][0], axis=1)
        p = np.nonzero(on)[0][np.argsort(mag[on])[on.sum() // 2]]
        over = lambda a, b, t: float((np.abs(a - b) / t).max())
        dropped = dict(case, **{key: case[key].copy()})
        dropped[key][0, p] = 0.0
        wr2, g2, e2, _ = pbo.oracle_of(dropped)
        assert over(wr2, wr, bd["wrench"]) > 3 and over(g2, g, bd["gRt"]) > 3
        assert e is None or over(e2, e, bd["e_pen"]) > 3
        moved = dict(case, link=case["link"].copy())
        moved["link"][0, p] = (case["link"][0, p] + 1) % case["L"]
        wr3, g3, _, _ = pbo.oracle_of(moved)
        assert over(wr3, wr, bd["wrench"]) > 3 and np.array_equal(g3, g)
        # K transposed for that one entry: x (x) G -> G (x) x
        R = case["Rg"][0].astype(np.float64).reshape(3, 3)
        x = (case["surf"][0, p].astype(np.float64) - case["hand_pose"][0, :3]) @ R
        wG = (100.0 if fused else float(case["w"][0, p])) * case["gvec"][0, p].astype(np.float64)
        K1 = np.outer(x, wG)
        assert over(g[0, 3:] - K1.reshape(9) + K1.T.reshape(9), g[0, 3:], bd["gRt"][0, 3:]) > 3


# ---- the preconditions of the GPU cases, for both forms ---------------------------------------------------------------
@pytest.fixture(scope="module")
def consts():
    c = pbo.kernel_constants()
    assert c == {"K": 16, "LIST": 1024, "K_small": 10}, "the cases below were laid out for these values: revisit them"
    return c


@pytest.mark.parametrize("fused", [False, True])
def test_cases_reach_their_paths(consts, fused):
    for P in pbo.RAGGED_P:
        pbo.require_single_round(pbo.case_ragged(P, fused), consts, "K_small")
    assert max(pbo.RAGGED_P) == consts["K_small"] * 256 and min(pbo.K16_P) == consts["K_small"] * 256 + 1
    for P in pbo.K16_P:
        pbo.require_single_round(pbo.case_k16(P, fused), consts, "K")
    assert max(pbo.K16_P) == consts["K"] * 256 and min(pbo.ROUNDS_P) == consts["K"] * 256 + 1
    for P in pbo.ROUNDS_P:
        pbo.require_several_rounds(pbo.case_rounds(P, fused), consts)
    pbo.require_overflow_2500(pbo.case_overflow(2500, fused), consts)
    pbo.require_overflow_9000(pbo.case_overflow(9000, fused), consts)
    for L in pbo.GROUP_L:
        pbo.require_groups(pbo.case_groups(L, fused), consts)
    tasks = {L: pbo.link_groups(L)[0] for L in pbo.GROUP_L}
    assert sum(t > 4 for t in tasks.values()) >= 5 and tasks[160] > 8  # a wavefront folds two groups, and more than two
    assert {pbo.link_groups(L)[2] for L in pbo.GROUP_L} == {1, 2, 3, 4}
    assert not pbo.link_groups(16)[1] and not pbo.link_groups(19)[1] and not pbo.link_groups(20)[1]  # > 4 groups, sums do not ride
