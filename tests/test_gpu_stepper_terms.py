"""The stepper's optional terms on the GPU, as the table of graspqp_amd/stepper.py strings them together: the sequence of library
calls of one ``evaluate`` for the configurations of tests/_stepper_terms_case.py and for every term alone, and the bits of those
configurations against tests/golden/stepper_terms_parent_bits.npz, which the stepper recorded before the table existed
(tools/make_golden_stepper_terms.py).  The expected entry names and orders are written out here, not taken from the table.

8 rows (two objects, four each), 64 surface samples, a 100^3 wall, arm7: the smallest shapes at which an order or a pointer can
still be wrong."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _stepper_terms_case as stc  # noqa: E402

FIXED = ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints")
DECLARATION = ("E_prior", "E_wall", "E_scene", "E_approach", "E_pregrasp", "E_squeeze", "E_reach", "E_arm", "E_track", "E_lift")
# configuration -> (the term launches in launch order, the names that are on)
EXPECT = {
    "A": (["gq_tabletop_terms", "gq_scene_terms", "gq_approach_terms", "gq_pregrasp_terms", "gq_lift_terms", "gq_squeeze_terms",
           "gq_reach_terms", "gq_track_terms", "gq_arm_terms"], DECLARATION),
    "B": (["gq_clutter_terms", "gq_clutter_corridor_terms", "gq_squeeze_terms", "gq_reach_terms", "gq_arm_terms"],
          ("E_scene", "E_approach", "E_squeeze", "E_reach", "E_arm")),
    "C": (["gq_pregrasp_terms", "gq_lift_terms"], ("E_pregrasp", "E_lift")),
    "E_prior": (["gq_tabletop_terms"], ("E_prior", "E_wall")),
    "E_wall": (["gq_tabletop_terms"], ("E_prior", "E_wall")),
    "E_scene": (["gq_scene_terms"], ("E_scene",)),
    "E_approach": (["gq_approach_terms"], ("E_approach",)),
    "E_pregrasp": (["gq_pregrasp_terms"], ("E_pregrasp",)),
    "E_squeeze": (["gq_squeeze_terms"], ("E_squeeze",)),
    "E_reach": (["gq_reach_terms"], ("E_reach",)),
    "E_arm": (["gq_reach_terms", "gq_arm_terms"], ("E_reach", "E_arm")),
    "E_track": (["gq_reach_terms", "gq_track_terms"], ("E_reach", "E_track")),
    "E_lift": (["gq_lift_terms"], ("E_lift",)),
}
G_THETA_ARG = 12  # gq_fk_backward(hand, pose, idx, B, n, Rg, link_T, g_cpts, g_cnrm, g_sph, wrench, gRt, g_theta, ...)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C

    _C.lib()
    return _C


def _value(x):
    return getattr(x, "value", x)


def _trace(gq, monkeypatch, st):
    """The library calls of one ``evaluate``: [(entry name, arguments)]; every call still reaches the library."""
    real, calls = gq.call, []

    def recorder(name, *args):
        calls.append((name, args))
        return real(name, *args)

    hp, idx = stc.start()
    with monkeypatch.context() as m:
        m.setattr(gq, "call", recorder)
        st.evaluate(hp, idx)
    torch.cuda.synchronize()
    return calls


@pytest.fixture(scope="module")
def five_trace(gq):
    mp = pytest.MonkeyPatch()
    names = [name for name, _ in _trace(gq, mp, stc.stepper("five"))]
    assert names[0] == "gq_fk_forward" and names[-1] == "gq_fk_backward" and names.count("gq_fk_backward") == 1, names
    assert not any(n.endswith("_terms") or n.endswith("_total") for n in names), names
    return names


@pytest.mark.parametrize("case", list(EXPECT))
def test_launch_trace(gq, monkeypatch, five_trace, case):
    launches, on = EXPECT[case]
    st = stc.stepper(case)
    assert st.term_names == FIXED + on
    calls = _trace(gq, monkeypatch, st)
    names = [name for name, _ in calls]
    totals = (["gq_tabletop_total"] if "E_prior" in on else []) + ["gq_scene_total"] * len([k for k in on if k not in ("E_prior", "E_wall")])
    print(f"[{case}] {names}")
    assert names == five_trace[:-1] + launches + ["gq_fk_backward"] + totals
    w = st.w
    for (name, args), k in zip([c for c in calls if c[0] == "gq_scene_total"], [k for k in on if k not in ("E_prior", "E_wall")]):
        row = st.term_names.index(k)
        assert row == st.term_row(k)
        assert _value(args[0]) == st.total_new.data_ptr() and _value(args[1]) == st.terms_new[row].data_ptr(), k
        assert _value(args[2]) == float(w[k]) and _value(args[3]) == st.B, k
    for name, args in calls:
        if name == "gq_tabletop_total":
            assert [_value(a) for a in args[:6]] == [st.total_new.data_ptr(), st.terms_new[5].data_ptr(), float(w["E_prior"]),
                                                     st.terms_new[6].data_ptr(), float(w["E_wall"]), st.B]
        if name == "gq_fk_backward":
            g_theta = _value(args[G_THETA_ARG])
            if "E_pregrasp" in on or "E_squeeze" in on:
                assert g_theta == st.g_theta.data_ptr() and g_theta
            else:
                assert not g_theta


@pytest.fixture(scope="module")
def parent_bits():
    return np.load(os.path.join(stc.GOLDEN, "stepper_terms_parent_bits.npz"), allow_pickle=False)


def _assert_bits(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), f"{tag}: {int((got != want).sum())} of {got.size} values differ"


@pytest.mark.parametrize("case", stc.CASES)
def test_the_parents_bits_eager_and_captured(gq, parent_bits, case):
    """evaluate, reset + three steps and one step_reset give the bits of the stepper before the table; the three steps replayed
    from a captured graph give the bits of the eager ones."""
    out = stc.run(case)
    want = {k[len(case) + 1:]: parent_bits[k] for k in parent_bits.files if k.startswith(case + ".")}
    assert sorted(out) == sorted(want) and len(want) >= 2 + 5 + 2 * len(stc.STATE)
    for k in out:
        _assert_bits(np.ascontiguousarray(out[k]), np.ascontiguousarray(want[k]), f"{case}.{k}")
    assert out["steps.accept"].any() or out["reset.accept"].any()  # the chain moved
    captured = stc.three_steps(stc.stepper(case), captured=True)
    assert sorted(captured) == sorted(k for k in out if k.startswith("steps."))
    for k in captured:
        _assert_bits(np.ascontiguousarray(captured[k]), np.ascontiguousarray(out[k]), f"{case}.{k} captured vs eager")
