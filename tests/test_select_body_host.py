"""The grasp-set selection (gq_grasp_select: feasibility gate, ranking by score, greedy suppression of rows closer than the radius in
RMS hand-surface displacement) on the HOST: the bodies of graspqp_amd/csrc/select_dev.h behind tests/host_shim.h, compiled with
AddressSanitizer and UBSan and run as a program of its own (tests/select_host.cpp) that emulates a block of T threads serially.
``sel``, ``n_selected``, ``n_feasible``, ``feasible`` and (small cases) every d^2 must equal the numpy fp64 oracle
(tests/_select_oracle.py) EXACTLY, for T = 1, 64 and 1024.  The inputs make float32 arithmetic exact -- cube rotations, translations,
link offsets and centroids in multiples of 2^-7, second moments G G' with G in multiples of 2^-5, 16 samples, scores and terms in
multiples of 2^-4 -- so an fp32 and an fp64 oracle agree, asserted below, and equality is a fair demand.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _host_program
import _select_oracle as oracle

CASES = oracle.cases()


def write_case(path, c):
    hp, Rg, LT, mom, score, terms = oracle.case_arrays(c)
    B, L, nT = hp.shape[0], mom.shape[0], terms.shape[0]
    with open(path, "wb") as f:
        f.write(np.asarray([B // c["batch_each"], c["batch_each"], L, hp.shape[1], nT, c["K"], c["n_samples"]], np.int32).tobytes())
        f.write(np.asarray([c["radius"]] + list(c["tol"]), np.float32).tobytes())
        for a in (hp, Rg, LT, mom, score, terms):
            f.write(a.tobytes())


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    work = tmp_path_factory.mktemp("select")
    exe = _host_program.build("select_host", work)

    def go(case, T, matrix=False):
        path = str(work / "case.bin")
        write_case(path, case)
        lines = subprocess.check_output([exe, path, str(T)] + (["matrix"] if matrix else [])).decode().splitlines()
        n_obj = len(case["score"]) // case["batch_each"]
        rows = np.asarray([[int(v) for v in line.split()] for line in lines[:n_obj]], np.int32)
        feasible = np.asarray([int(v) for v in lines[n_obj].split()], np.int32)
        d2 = None
        if matrix:
            bits = np.asarray([[int(v, 16) for v in line.split()] for line in lines[n_obj + 1:]], np.uint32)
            d2 = bits.view(np.float32).reshape(n_obj, case["batch_each"], case["batch_each"])
        return rows[:, 2:], rows[:, 1], rows[:, 0], feasible, d2

    return go


@pytest.fixture(scope="module")
def answers():
    return {k: oracle.case_answer(c) for k, c in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_bodies_equal_the_oracle_for_every_block_size(run, answers, name):
    c = CASES[name]
    want, d2 = answers[name]
    w32, d32 = oracle.case_answer(c, np.float32)
    assert np.array_equal(d2, d32.astype(np.float64)), "the inputs must be exact in float32"
    assert all(np.array_equal(a, b) for a, b in zip(want, w32))
    small = c["batch_each"] <= 70
    for T in (1, 64, 1024):
        got = run(c, T, matrix=small and T == 64)
        for g, w, what in zip(got[:4], want, ("sel", "n_selected", "n_feasible", "feasible")):
            assert np.array_equal(g, w), (name, T, what)
        if got[4] is not None:
            assert np.array_equal(got[4].astype(np.float64), d2.transpose(0, 2, 1)), (name, "d^2")
            assert np.array_equal(got[4], got[4].transpose(0, 2, 1)) and not np.diagonal(got[4], axis1=1, axis2=2).any()


def test_the_closed_form_is_the_sum_over_the_samples():
    """the oracle's closed form against the definition on actual samples (fp64; the moments a direct sum over them)"""
    rng = np.random.default_rng(3)
    L, be = 5, 12
    link = np.sort(rng.integers(0, L, 60))
    link[link == 1] = 2  # a link without samples
    pts = rng.normal(0, 0.02, (60, 3))
    Rg, t, LT = oracle.exact_rows(rng, 2, be, L, 4)
    LT = LT + rng.normal(0, 0.01, LT.shape)
    mom = oracle.moments(pts, link, L)
    assert mom[1].tolist() == [0.0] * 10
    closed = oracle.dist2_closed(oracle.world(Rg, t, LT), mom, 60, be)
    direct = oracle.dist2_samples(Rg, t, LT, pts, link, be)
    assert np.abs(closed - direct).max() <= 1e-12 * max(1.0, direct.max())


def test_the_cases_cover_what_they_claim(answers):
    sel = {k: a[0][0] for k, a in answers.items()}
    nsel = {k: a[0][1] for k, a in answers.items()}
    nf = {k: a[0][2] for k, a in answers.items()}
    assert nf["three_objects_70"][1] == 0 and nsel["three_objects_70"][1] == 0 and (sel["three_objects_70"][1] == -1).all()
    assert 0 < nf["three_objects_70"][2] <= 6 and nsel["three_objects_70"][0] == 8
    assert (sel["three_objects_70"][2][sel["three_objects_70"][2] >= 0] >= 140).all()  # global rows
    assert nsel["rows_1100"][0] == 24 and sel["rows_1100"].max() >= 1024  # more rows than threads
    # suppression does something: the K lowest feasible scores are not the answer
    c = CASES["rows_1100"]
    ok = oracle.feasible(c["score"], c["terms"], c["tol"])
    lowest = sorted(np.nonzero(ok)[0], key=lambda r: (c["score"][r], r))[:24]
    assert sel["rows_1100"][0].tolist() != lowest
    c = CASES["radius_0"]
    ok = oracle.feasible(c["score"], c["terms"], c["tol"])
    assert sel["radius_0"][0].tolist() == sorted(np.nonzero(ok[:70])[0], key=lambda r: (c["score"][r], r))[:12]
    assert sel["K_1"].shape == (2, 1) and sel["K_batch_each"].shape == (2, 33)
    assert nsel["duplicates_radius_pos"][0] == 4 and nf["duplicates_radius_pos"][0] == 20  # one per distinct pose, fewer than K
    assert len({int(r) % 4 for r in sel["duplicates_radius_pos"][0][:4]}) == 4
    assert nsel["duplicates_radius_0"][0] == 8
    assert sel["pair_at_the_radius"][0].tolist() == [0, 1, 3, 4, 5, -1]  # d = radius stays, one step closer goes
    s = sel["equal_scores"][0]
    rest = [r for r in s[:nsel["equal_scores"][0]].tolist() if r not in (7, 21)]
    assert s[0] == 7 and len(rest) >= 6 and rest == sorted(rest)  # the smaller row wins among equal scores
    s = sel["nan_inf"][0]
    gone = {3, 17, 4, 30, 5, 8}  # NaN, +inf and -inf scores, a NaN term under a gate
    assert nf["nan_inf"][0] == 40 - len(gone) and not gone & set(s.tolist()) and {10, 11} <= set(s.tolist())
    assert s.tolist().index(6) < s.tolist().index(9)  # -0.0 sorts before +0.0 (order-preserving bits)
