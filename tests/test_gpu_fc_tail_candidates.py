"""The small-batch fc tail evaluates both candidate iterates before k* is known; the bits are the parent's.

gq_fc_tail_body (csrc/fcstep_dev.h, RPL > 0) runs the evaluation -- E_fc, the QP backward, the contact gradient -- on two
wavefronts while the block's other wavefronts replay the stop rule: wavefront 0 on the slot (the row's best iterate among
iterations 0 .. max_iter - 2), wavefront 1 on the last snapshot.  After the one barrier the wavefront that holds the row's
best iterate among 0..k* stores; when the rule stopped before the slot's iteration, wavefront 0 goes back to the
snapshot table, evaluates again and stores.  The arithmetic of an evaluation is the one the parent ran after k* was
known, so every output must be the parent's bit for bit.

tests/golden/fc_tail_parent_bits.npz (tools/make_golden_fc_tail.py, run with the parent's library) holds the contacts of the
eight rows of tests/test_gpu_fc_tail_slot.py and the parent's e_fc, val, svd, x, x_sum, g_cpts and n_iter of
gq_fc_tail_kernel<1, 4> at five settings:

  default   eps 5e-2: the rule stops at the last iteration or the one before -> rows commit from wavefront 1 (k* is the
            last iteration and it improved the row) or from wavefront 0
  huge      eps 1e30: k* = 0 -> every row whose slot holds a later iteration goes back to the table (wavefront 0, twice)
  mid       the mid-way eps of the slot test: rows served by the slot and rows that go back, in one launch
  zero      eps 0: no residual is small enough to stop the rule; it runs to the last iteration unless three iterations in a
            row improve no row
  one       max_iter = 1: there is no slot; only the last snapshot exists and wavefront 1 commits every row

Which wavefront commits a row follows from n_iter and the row's best iteration among all iterations and among all but the
last (the library's own box QP, as the slot test derives them); the cases together must take all three routes.  Every
output is pre-filled with a sentinel: a row that nobody stored keeps it, and a row stored by both wavefronts, or by
wavefront 0 before and after its second evaluation, would show as a mix that differs from the fixture."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _fc_tail_case as ftc  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fc_tail_parent_bits.npz")
MAX_ITER = 12
CASES = {"default": (5e-2, MAX_ITER), "huge": (1e30, MAX_ITER), "mid": (None, MAX_ITER), "zero": (0.0, MAX_ITER), "one": (5e-2, 1)}
_routes = {}


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return ops


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def best(gq, golden):
    """per-row best iteration among all iterations and among all but the last (the slot's), computed once"""
    F = ftc.run(gq, golden["in.pts"], golden["in.nrm"], golden["in.cog"], 5e-2, MAX_ITER)["F"]
    return ftc.best_iterations(gq, F, MAX_ITER), ftc.best_iterations(gq, F, MAX_ITER - 1)


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_are_the_parents_bits(gq, golden, best, case):
    eps, max_iter = CASES[case]
    eps = float(golden["in.eps_mid"]) if eps is None else eps
    B = golden["in.pts"].shape[0]
    assert B == 8
    out = ftc.run(gq, golden["in.pts"], golden["in.nrm"], golden["in.cog"], eps, max_iter)
    n_iter = int(out["n_iter"][0])
    assert n_iter == int(golden[f"{case}.n_iter"][0]), (n_iter, golden[f"{case}.n_iter"])
    ks, last = n_iter - 1, max_iter - 1
    if max_iter == 1:
        from_last, from_slot = np.ones(B, dtype=bool), np.zeros(B, dtype=bool)
    else:
        bi_all, bi_a = best
        from_last = (bi_all == last) if ks == last else np.zeros(B, dtype=bool)
        from_slot = ~from_last & (bi_a <= ks)
    redo = ~from_last & ~from_slot
    _routes[case] = (int(from_last.sum()), int(from_slot.sum()), int(redo.sum()))
    print(f"{case}: eps {eps:.3g} max_iter {max_iter} n_iter {n_iter}; rows committed by wavefront 1 (last snapshot) {_routes[case][0]}, "
          f"by wavefront 0 (slot) {_routes[case][1]}, by wavefront 0 after going back to the table {_routes[case][2]}")
    if case == "default":
        assert ks >= last - 1 and not redo.any()
    elif case == "huge":
        assert n_iter == 1 and redo.sum() == (best[1] > 0).sum() and redo.any()
    elif case == "mid":
        assert 2 <= ks <= MAX_ITER - 3 and redo.any() and from_slot.any()
    elif case == "one":
        assert n_iter == 1 and from_last.all()
    for k in ftc.OUTPUTS:
        got, ref = out[k], golden[f"{case}.{k}"]
        assert not (got == np.float32(ftc.SENTINEL)).any(), f"{case} {k}: the sentinel is left in {int((got == ftc.SENTINEL).sum())} places"
        if not ftc.same_bits(got, ref):
            rows = np.nonzero((got.reshape(B, -1) != ref.reshape(B, -1)).any(1))[0] if got.shape[0] == B else "-"
            raise AssertionError(f"{case} {k}: differs from the parent's bits in rows {rows}; max |diff| {np.abs(got - ref).max():.3g}")


def test_the_cases_take_all_three_routes(gq, golden, best):
    """wavefront 1 commits, wavefront 0 commits, wavefront 0 goes back to the table: each in at least one row of the cases"""
    for case in CASES:
        if case not in _routes:
            test_outputs_are_the_parents_bits(gq, golden, best, case)
    n_last, n_slot, n_redo = (sum(r[i] for r in _routes.values()) for i in range(3))
    assert n_last > 0 and n_slot > 0 and n_redo > 0, _routes
    assert sum(r[0] for c, r in _routes.items() if c != "one") > 0, "no row of a twelve-iteration case commits from wavefront 1"
