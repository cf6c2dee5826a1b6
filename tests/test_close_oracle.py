"""The finger-closing oracle (tests/_close_oracle.py) against facts computed by hand, and the guards and caps of the committed
cases (tests/_close_cases.py).  CPU only."""
import numpy as np
import pytest
import torch

import _close_cases as cc
import _close_oracle as co
import _scene_oracle as so
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec


@pytest.mark.parametrize("name", cc.HANDS)
def test_stop_masks_follow_the_tree(name):
    """bit l of mask a <=> some tree node between link l and the base (the link's own node included) is driven by joint a"""
    spec = get_hand_spec(name)
    J, JA, L = spec.n_nodes, spec.n_dofs, spec.n_links
    masks = ops.close_stop_masks_host(spec)
    assert masks.dtype == np.uint64 and masks.shape == (JA,)
    C = np.asarray(spec.coupling, np.float64).reshape(J, JA) if spec.is_coupled else np.eye(J)
    if not spec.is_coupled:
        assert J == JA
    for l in range(L):
        chain, j = [], int(spec.link_node[l])
        while j >= 0:
            chain.append(j)
            j = int(spec.node_parent[j])
        for a in range(JA):
            want = any(C[j, a] != 0 for j in chain)
            assert bool((int(masks[a]) >> l) & 1) == want, (name, l, a)
    fixed = [l for l in range(L) if int(spec.link_node[l]) < 0]
    assert all(not (int(m) >> l) & 1 for m in masks for l in fixed)  # a link on the base stops nothing
    if spec.is_coupled:  # every tree node that moves is driven by some actuated joint, and with it the links on it
        moving = [l for l in range(L) if int(spec.link_node[l]) >= 0]
        assert all(any((int(m) >> l) & 1 for m in masks) for l in moving)


def test_default_step_by_joint_kind():
    assert np.array_equal(ops.close_default_step(get_hand_spec("allegro")), np.full(16, 0.01, np.float32))
    assert np.array_equal(ops.close_default_step(get_hand_spec("panda")), np.full(1, 5e-4, np.float32))

    class Mixed:  # one actuated joint that drives a revolute and a prismatic node
        n_nodes, n_dofs, n_links, is_coupled = 2, 1, 1, True
        coupling, node_type = np.ones((2, 1)), np.array([1, 2])

    with pytest.raises(ValueError, match="revolute and prismatic"):
        ops.close_default_step(Mixed())


@pytest.mark.parametrize("name", cc.HANDS)
def test_free_motion_moves_the_fastest_joint_by_its_step(name):
    """no grid contact (the hand a metre outside the volume): after S steps the fastest joint has moved S x step, clamped at its
    limit, every other joint in proportion; nothing is touched or stopped"""
    spec = get_hand_spec(name)
    pts, lnk = cc.samples(name, 96)
    JA, S = spec.n_dofs, 7
    step = ops.close_default_step(spec)
    lo, hi = np.asarray(spec.joints_lower, np.float32).astype(np.float64), np.asarray(spec.joints_upper, np.float32).astype(np.float64)
    th0 = (0.5 * (lo + hi)).astype(np.float32)
    v = np.linspace(1.0, 0.25, JA).astype(np.float32) * cc.SENSE[name]
    hp = torch.cat([torch.tensor([1.0, 0.0, 0.0]), torch.tensor([1.0, 0, 0, 0, 1, 0]), torch.as_tensor(th0)])[None]
    ref = co.close(spec, pts, lnk, hp, torch.as_tensor(v)[None], (cc.fields()[0],), S, step, cc.TOUCH)
    assert (ref["touch_step"] < 0).all() and (ref["joint_stop"] < 0).all() and np.isinf(ref["phi"]).all()
    u = v.astype(np.float64) / step.astype(np.float64)
    delta = step.astype(np.float64) * u / np.abs(u).max()
    assert abs(delta[0]) == float(step[0])  # the fastest joint moves exactly its step
    want = np.clip(th0.astype(np.float64) + S * delta, lo, hi)
    np.testing.assert_allclose(ref["theta"][0], want, rtol=0, atol=1e-12)
    big = (0.2 * (hi - lo)).astype(np.float32)  # every joint a fifth of its range per step, all equally fast: on the limits after 3
    far = co.close(spec, pts, lnk, hp, torch.as_tensor(big * cc.SENSE[name])[None], (cc.fields()[0],), 4, big, cc.TOUCH)
    assert np.array_equal(far["theta"][0], hi if cc.SENSE[name] > 0 else lo)
    for bad in (np.zeros(JA, np.float32), np.full(JA, np.nan, np.float32), np.r_[np.inf, np.ones(JA - 1)].astype(np.float32)[:JA]):
        still = co.close(spec, pts, lnk, hp, torch.as_tensor(bad)[None], (cc.fields()[0],), 3, step, cc.TOUCH)
        assert np.array_equal(still["theta"][0], th0.astype(np.float64)), bad  # a zero or non-finite command does not move


@pytest.mark.parametrize("name,Ns,S", [(h, 512, 32) for h in cc.HANDS] + [("allegro", 96, 8)])
def test_a_touch_freezes_exactly_the_masked_joints(name, Ns, S):
    ref = cc.reference(name, Ns, S)
    ts, js, th, M, T = ref["touch_step"], ref["joint_stop"], ref["thetas"], ref["M"], ref["T"]
    masks = ref["masks"]  # (JA,L)
    B, L = ts.shape
    spec = get_hand_spec(name)
    lo_, hi_ = np.asarray(spec.joints_lower, np.float32).astype(np.float64), np.asarray(spec.joints_upper, np.float32).astype(np.float64)
    for b in range(B):
        for a in range(masks.shape[0]):
            mine = [ts[b, l] for l in range(L) if masks[a, l] and ts[b, l] >= 0]
            assert js[b, a] == (min(mine) if mine else -1), (b, a)  # stopped at the first touch of a link in its mask, else never
            if js[b, a] >= 0:
                assert (th[js[b, a]:, b, a] == th[js[b, a], b, a]).all(), (b, a)  # ... and it keeps its bits from then on
            else:  # a free joint takes its clamped step every time
                d = ref["delta"][b, a]
                want = th[:-1, b, a] if d == 0 else np.minimum(np.maximum(th[:-1, b, a] + d, lo_[a]), hi_[a])
                assert np.array_equal(th[1:, b, a], want), (b, a)
        for l in range(L):
            if ts[b, l] >= 0:
                s0 = ts[b, l]
                assert M[s0, b, l] <= cc.TOUCH and (M[:s0, b, l] > cc.TOUCH).all(), (b, l)
                assert (T[s0:, b, l] == T[s0, b, l]).all(), (b, l)  # a touched link's transform is the same at every later step
            else:
                assert (M[:, b, l] > cc.TOUCH).all(), (b, l)
    assert (ts >= 1).any() and (js >= 1).any() and (js < 0).any()


def test_guards_and_caps_hold_on_the_committed_cases():
    n_rows, n_und = 0, 0
    for name, Ns, S in cc.cases():
        ref = cc.reference(name, Ns, S)
        und = cc.assert_populated(name, ref, f"{name} Ns={Ns} S={S}")  # at most one row, no regime empty after the exclusion
        n_rows, n_und = n_rows + cc.B, n_und + int(und.sum())
        exact, nmask = cc.compare_masks(ref)
        has = ref["sample"] >= 0
        assert (has & ~exact).sum() <= 0.10 * has.size and (exact & ~nmask).sum() <= 0.10 * has.size, (name, Ns, S)
        hp, dirs, step = cc.inputs(name, Ns, S)
        assert hp.shape == (cc.B, 9 + get_hand_spec(name).n_dofs) and hp.dtype == torch.float32 and len(cc.fields()) == cc.B // cc.BE
        assert np.array_equal(step, ops.close_default_step(get_hand_spec(name)))
    assert n_und <= 0.05 * n_rows, (n_und, n_rows)
    radii = [float(-f.values.min()) for f in cc.fields()]  # the grids differ: the deepest node value is about minus the radius
    assert all(b - a > 0.003 for a, b in zip(radii, radii[1:])), radii
    assert cc.fields()[0].shape == (32, 32, 32) and float(cc.fields()[0].voxel) == np.float32(0.005)


def test_tie_goes_to_the_lowest_sample_index():
    ph = torch.tensor([[0.3, 0.1, 0.1, 0.2, float("inf"), 0.05, 0.05]], dtype=torch.float64)
    lnk = np.array([0, 0, 0, 0, 1, 2, 2])
    m, idx, second = co.link_minima(ph, lnk, 4)
    assert m[0].tolist() == [0.1, float("inf"), 0.05, float("inf")] and idx[0].tolist() == [1, -1, 5, -1]
    assert second[0, 0] == 0.1 and second[0, 2] == 0.05
