"""Finger closing on the GPU: gq_close_fingers (one block per row, S + 1 rounds in one launch) against tests/_close_oracle.py on the
cases of tests/_close_cases.py (8 rows = 4 objects x 2 rows, a stack of four sphere grids of different radii, every regime populated).

What is held to what, per case:
  * touch_step, joint_stop and sample: EXACT on the decidable rows (``_close_oracle.undecidable``; sample where the link's two
    smallest phi differ by more than NEAR).
  * theta, phi, point, normal: per row, error <= max(2 x the error of the oracle run in fp32 on that row, floor) and <= ceiling.  The
    floors and ceilings are the figures tests/test_gpu_scene.py and tests/test_gpu_pregrasp.py already use: phi 1e-6 (their atol) and
    1e-5 (their rtol, on a grid smaller than a metre); positions and joints 2e-6 (the atol of their pose comparison) and 1e-5; the
    grid gradient, here as a unit normal, 1e-4 (their norm-wise gradient bound) and 1e-3 (their bound for the stepper's sum).
  * single grid = stack of one, two runs, a row alone = the row among others: bit for bit.
  * a captured graph replayed on overwritten grid values = the eager launch on those values.
  * GraspStepper.close = ops.close_fingers on hand_pose; stepping on afterwards = a twin that never called it, bit for bit.
  * the sign of the default direction: one closing step lowers the fingertip links' smallest phi.
  * ops.hold_contacts on padded contacts against the fp64 hold reference on the unpadded ones."""
import os

import numpy as np
import pytest
import torch

import _close_cases as cc
import _close_oracle as co
import _hold_cases as hc
from graspqp_amd.hands import get_hand_spec

pytestmark = pytest.mark.gpu
FLOOR = dict(theta=2e-6, phi=1e-6, point=2e-6, normal=1e-4)
CEIL = dict(theta=1e-5, phi=1e-5, point=1e-5, normal=1e-3)
OUT = ("theta", "touch_step", "joint_stop", "phi", "sample", "point", "normal")


@pytest.fixture(scope="module")
def gq():
    import types

    import graspqp_amd.stepper as stepper
    from graspqp_amd import _C, ops

    assert torch.cuda.is_available()
    return types.SimpleNamespace(C=_C, ops=ops, stepper=stepper, hands={}, samples={})


def _hand(gq, name):
    if name not in gq.hands:
        gq.hands[name] = gq.ops.HandHandle(get_hand_spec(name))
    return gq.hands[name]


def _samples(gq, name, Ns):
    if (name, Ns) not in gq.samples:
        pts, lnk = cc.samples(name, Ns)
        sm = gq.ops.SurfaceSamples(get_hand_spec(name), pts, lnk)
        assert np.array_equal(sm.link.cpu().numpy(), lnk) and np.array_equal(sm.points.cpu().numpy(), pts)  # the oracle's order
        gq.samples[(name, Ns)] = sm
    return gq.samples[(name, Ns)]


def _stack(gq, grids=slice(None)):
    f = cc.fields()[grids]
    return gq.ops.SceneSDFSet(torch.stack([x.values for x in f]).cuda(), list(cc.G_ORIGIN), cc.G_H)


def _inputs(gq, name, Ns, S, rows=slice(None)):
    hp, dirs, step = cc.inputs(name, Ns, S)
    hp, dirs = hp[rows].cuda().contiguous(), dirs[rows].cuda().contiguous()
    Rg = gq.ops.fk_contacts(hp, torch.zeros(hp.shape[0], 1, dtype=torch.long, device="cuda"), _hand(gq, name))[0].contiguous()
    return hp, dirs, step, Rg


def _launch(gq, name, Ns, S, rows=slice(None), grid=None):
    hp, dirs, step, Rg = _inputs(gq, name, Ns, S, rows)
    if grid is None:
        first = (rows.start or 0) // cc.BE
        grid = _stack(gq, slice(first, first + hp.shape[0] // cc.BE))
    res = gq.ops.close_fingers(hp, _hand(gq, name), _samples(gq, name, Ns), Rg, grid, dirs, steps=S, step=step, touch=cc.TOUCH)
    torch.cuda.synchronize()
    assert torch.equal(res.touched, res.touch_step >= 0)
    return {k: getattr(res, k).cpu() for k in OUT}


def _row_err(a, b, mask=None):
    """per row: the largest |a - b| over the entries that count ((B,L) mask, or all); both infinite and equal counts as 0"""
    with np.errstate(invalid="ignore"):
        d = np.where(a == b, 0.0, np.abs(a - b))
    if mask is not None:
        d = np.where(mask.reshape(mask.shape + (1,) * (d.ndim - mask.ndim)), d, 0.0)
    return d.reshape(d.shape[0], -1).max(1)


@pytest.mark.parametrize("name,Ns,S", cc.cases())
def test_launch_matches_the_fp64_oracle(gq, name, Ns, S):
    tag = f"{name} Ns={Ns} S={S}"
    r64, r32 = cc.reference(name, Ns, S), cc.reference(name, Ns, S, torch.float32)
    und = cc.assert_populated(name, r64, tag)
    ok = ~und
    exact, nmask = cc.compare_masks(r64)
    out = {k: v.double().numpy() if v.is_floating_point() else v.numpy() for k, v in _launch(gq, name, Ns, S).items()}
    for k in ("touch_step", "joint_stop"):
        assert np.array_equal(out[k][ok], r64[k][ok]), (tag, k, out[k].tolist(), r64[k].tolist())
    assert np.array_equal(out["sample"][ok][exact[ok]], r64["sample"][ok][exact[ok]]), (tag, "sample")
    assert np.array_equal(out["sample"] < 0, r64["sample"] < 0) or und.any(), (tag, "links without a sample inside the volume")
    worst = {}
    for k, mask in (("theta", None), ("phi", None), ("point", exact), ("normal", nmask)):
        err, noise = _row_err(out[k], r64[k], mask)[ok], _row_err(r32[k], r64[k], mask)[ok]
        allow = np.minimum(np.maximum(2.0 * noise, FLOOR[k]), CEIL[k])
        worst[k] = (float(err.max()), float((err / allow).max()))
        print(f"[{tag}] {k}: worst error {err.max():.2e} (fp32 oracle {noise.max():.2e}), worst error / allowance {(err / allow).max():.3f}")
        assert (err <= np.maximum(2.0 * noise, FLOOR[k])).all(), (tag, k, "2 x fp32 noise", err.tolist(), noise.tolist())
        assert (err <= CEIL[k]).all(), (tag, k, "ceiling", err.tolist())
    assert np.isfinite(out["phi"][list(cc.CLOSING)]).any() and not np.isfinite(out["phi"][list(cc.OUTSIDE)]).any(), tag
    path = os.environ.get("GQ_CLOSE_ERRORS")  # a measuring run keeps the figures
    if path:
        with open(path, "a") as f:
            f.write(f"{tag}: " + ", ".join(f"{k} {e:.2e} ({r:.3f})" for k, (e, r) in worst.items()) + "\n")


@pytest.mark.parametrize("name,Ns,S", [("allegro", 512, 32), ("ability_hand", 96, 8), ("panda", 512, 8)])
def test_bitwise_reproducible_row_local_and_stack_of_one(gq, name, Ns, S):
    a, b = _launch(gq, name, Ns, S), _launch(gq, name, Ns, S)
    for k in OUT:
        assert torch.equal(a[k], b[k]), k
    for first in (0, 2):  # an object's two rows alone, on their grid alone: as a stack of one and as a single grid
        rows = slice(first, first + cc.BE)
        alone = _launch(gq, name, Ns, S, rows)
        single = _launch(gq, name, Ns, S, rows, gq.ops.SceneSDF(cc.fields()[first // cc.BE].values.cuda(), list(cc.G_ORIGIN), cc.G_H))
        for k in OUT:
            assert torch.equal(alone[k], a[k][rows]), (k, first)
            assert torch.equal(single[k], alone[k]), (k, first)
    # the other rows change (the joints of the objects' second rows are swapped among them, their commands negated): rows 0, 2, 4, 6 keep their bits
    hp, dirs, step, Rg = _inputs(gq, name, Ns, S)
    hp2, d2 = hp.clone(), dirs.clone()
    hp2[1::2, 9:] = hp[1::2, 9:].flip(0)
    d2[1::2] = -dirs[1::2]
    Rg2 = gq.ops.fk_contacts(hp2, torch.zeros(8, 1, dtype=torch.long, device="cuda"), _hand(gq, name))[0].contiguous()
    res = gq.ops.close_fingers(hp2, _hand(gq, name), _samples(gq, name, Ns), Rg2, _stack(gq), d2, steps=S, step=step, touch=cc.TOUCH)
    for k in OUT:
        assert torch.equal(getattr(res, k).cpu()[0::2], a[k][0::2]), k


def test_reading_another_rows_grid_would_fail(gq):
    """the radii differ so much that the stack in reversed order gives other touch steps: the per-row grid choice is tested at all"""
    name, Ns, S = "allegro", 512, 8
    hp, dirs, step, Rg = _inputs(gq, name, Ns, S)
    f = cc.fields()[::-1]
    rev = gq.ops.SceneSDFSet(torch.stack([x.values for x in f]).cuda(), list(cc.G_ORIGIN), cc.G_H)
    res = gq.ops.close_fingers(hp, _hand(gq, name), _samples(gq, name, Ns), Rg, rev, dirs, steps=S, step=step, touch=cc.TOUCH)
    assert not torch.equal(res.touch_step.cpu(), _launch(gq, name, Ns, S)["touch_step"])


def test_graph_replay_on_overwritten_grid_values(gq):
    name, Ns, S = "allegro", 512, 8
    ops, hand, sm = gq.ops, _hand(gq, name), _samples(gq, name, Ns)
    hp, dirs, step, Rg = _inputs(gq, name, Ns, S)
    values = torch.stack([x.values for x in cc.fields()]).cuda().contiguous()
    grid = ops.SceneSDFSet(values, list(cc.G_ORIGIN), cc.G_H)
    grids = ops._pregrasp_grids(grid.values, grid.origin, grid.voxel)
    step_dev, masks = torch.from_numpy(np.asarray(step, np.float32)).cuda(), ops.close_stop_masks(hand)
    out = ops._close_outputs(hp, hand.L)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        ops._close_call(hand, grids, sm.points, sm.link, hp, Rg, dirs, S, step_dev, cc.TOUCH, masks, *out)  # warm-up
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ops._close_call(hand, grids, sm.points, sm.link, hp, Rg, dirs, S, step_dev, cc.TOUCH, masks, *out)
    torch.cuda.synchronize()
    first = [t.clone() for t in out]
    values.copy_(values.flip(0))  # every row now reads a sphere of another radius
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    eager = ops.close_fingers(hp, hand, sm, Rg, grid, dirs, steps=S, step=step, touch=cc.TOUCH)
    torch.cuda.synchronize()
    for k, r, e in zip(OUT, replayed, eager):
        assert torch.equal(r, e), k
    assert not torch.equal(first[1], replayed[1])  # the new values were read


# ---- the stepper ----------------------------------------------------------------------------------------------------------------
STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")


def _sphere_stepper(gq, golden_dir, **kw):
    g = np.load(os.path.join(golden_dir, "mala_allegro_sphere_b8_n4.npz"), allow_pickle=False)
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    st = gq.stepper.GraspStepper(_hand(gq, "allegro"), gq.ops.MeshSet(fvs), torch.tensor(sps), be, 4, **kw)
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
    draws = lambda s: (f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept"))
    # the objects' own grid: one per object, 64^3 at 5 mm about the objects' common centre
    c = np.concatenate([f.reshape(-1, 3) for f in fvs]).mean(0)
    origin = [float(x) - 0.1575 for x in c]
    grid = gq.ops.SceneSDFSet(torch.stack([gq.ops.SceneSDF.from_meshes([fv], origin, (64, 64, 64), 0.005).values for fv in fvs]), origin,
                              0.005)
    return st, draws, grid


def test_stepper_close_reads_the_accepted_state_and_writes_nothing(gq, golden_dir):
    (st, draws, grid), (twin, _, _) = _sphere_stepper(gq, golden_dir), _sphere_stepper(gq, golden_dir)
    assert st.B == 8
    for s in (1,):
        st.step(draws=draws(s)), twin.step(draws=draws(s))
    v = torch.randn(st.B, st.J, generator=torch.Generator().manual_seed(3)).cuda()
    res = st.close(grid, direction=v, steps=8)
    Rg = gq.ops.fk_contacts(st.hand_pose, st.contact_idx, st.hand)[0].contiguous()
    want = gq.ops.close_fingers(st.hand_pose, st.hand, st.samples, Rg, grid, v, steps=8)
    for k in OUT + ("touched",):
        assert torch.equal(getattr(res, k), getattr(want, k)), k
    default = st.close(grid)  # the squeeze command, with E_squeeze off
    assert torch.isfinite(default.theta).all()
    for s in (2, 3):
        st.step(draws=draws(s)), twin.step(draws=draws(s))
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(st, k), getattr(twin, k)), k
    with pytest.raises(ValueError, match="n_grids"):
        st.close(gq.ops.SceneSDFSet(grid.values[:1].repeat(3, 1, 1, 1), grid.origin, grid.voxel))


def test_default_direction_closes(gq, golden_dir):
    """The sign of the default direction: on the objects' own grid, ONE closing step along it lowers the fingertip links' smallest
    phi (summed over the rows and fingertip links inside the volume, and for more of them than it raises)."""
    st, draws, grid = _sphere_stepper(gq, golden_dir)
    spec = st.hand.spec
    parents = set(int(p) for p in spec.node_parent)
    tips = [l for l, n in enumerate(spec.link_node) if int(n) >= 0 and int(n) not in parents]
    before = st.close(grid, direction=torch.zeros(st.B, st.J, device="cuda"), steps=1, touch=0.0).phi[:, tips]
    after = st.close(grid, steps=1, touch=0.0).phi[:, tips]
    both = torch.isfinite(before) & torch.isfinite(after)
    d = (after - before)[both].cpu().numpy()
    print(f"[default direction] fingertip links: {both.sum().item()} (row, link) pairs, mean change {d.mean():.3e} m, lowered {(d < 0).sum()}, "
          f"raised {(d > 0).sum()}")
    assert d.size >= st.B and d.mean() < 0 and (d < 0).sum() > (d > 0).sum()


def test_hold_contacts_on_padded_slots(gq):
    """ops.hold_contacts on CloseResult.contacts(n) with padded slots against the fp64 hold reference (tests/_hold_cases.loop /
    evaluate) on the UNPADDED contacts.  Allowance per row: 2 x the difference between the padded and the unpadded fp64 reference
    loops, floor 1e-6."""
    name, Ns, S, n, k = "allegro", 512, 32, 6, 4
    hp, dirs, step, Rg = _inputs(gq, name, Ns, S)
    res = gq.ops.close_fingers(hp, _hand(gq, name), _samples(gq, name, Ns), Rg, _stack(gq), dirs, steps=S, step=step, touch=cc.TOUCH)
    cp, nrm = res.contacts(n)
    count = res.touched.sum(1).cpu().numpy()
    assert (count < n).any() and (count >= 2).any() and cp.shape == (8, n, 3)
    assert float(nrm[torch.arange(n, device="cuda")[None] >= res.touched.sum(1, keepdim=True)].abs().max()) == 0.0
    loads = gq.ops.hold_loads(0.2)
    cog = torch.zeros(8, 3, device="cuda")
    e, resid, force = gq.ops.hold_contacts(cp, nrm, cog, loads, 2, hc.MU, hc.TW, k, hc.MAX_FORCE, hc.RIDGE, hc.T)
    torch.cuda.synchronize()
    w = torch.cat([loads[0, :3], hc.TW * loads[0, 3:]]).double()
    cp64, n64 = cp.cpu().double(), nrm.cpu().double()
    ref = {}
    for key, m_of in (("padded", lambda b: n), ("unpadded", lambda b: int(count[b]))):
        E, R = np.ones(8), np.ones(8)
        for b in range(8):
            m = m_of(b)
            if m == 0:
                continue
            F = hc.cone_matrix(cp64[b:b + 1, :m], n64[b:b + 1, :m], torch.zeros(1, 3, dtype=torch.float64), k)[0][0]
            x = hc.loop(F, w, hc.MAX_FORCE)
            r, V = hc.evaluate(F, w, x)
            E[b], R[b] = V / float(w @ w), float(r.norm()) / float(w.norm())
        ref[key] = (E, R)
    for i, (what, got) in enumerate((("E_hold", e), ("resid", resid[:, 0]))):
        allow = np.maximum(2.0 * np.abs(ref["padded"][i] - ref["unpadded"][i]), 1e-6)
        err = np.abs(got.cpu().double().numpy() - ref["unpadded"][i])
        print(f"[hold_contacts] {what}: worst error {err.max():.2e}, padded vs unpadded fp64 reference {np.abs(ref['padded'][i] - ref['unpadded'][i]).max():.2e}, "
              f"worst error / allowance {(err / allow).max():.3f}")
        assert (err <= allow).all(), (what, err.tolist(), allow.tolist())
    assert float(force[:, 0][torch.arange(n, device="cuda")[None] >= res.touched.sum(1, keepdim=True)].abs().max()) == 0.0  # a padded slot carries nothing
