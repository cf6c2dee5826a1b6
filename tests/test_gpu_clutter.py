"""GPU tests of the clutter scenes (include/graspqp_hip.h, "clutter scenes").

1. Grid selection is EXACT: every output of gq_clutter_terms / gq_clutter_corridor_terms / gq_clutter_query on row (point) b is
   compared bit for bit with the existing single-grid entry point called on that row with grid b // r.  No tolerance.
2. gq_clutter_compose against the fp64 oracle (tests/_clutter_oracle.py) at the project's bound for phi, rtol 1e-5 / atol 1e-6
   (DESIGN 14); the host build of the same body measured at most 2.1e-8 on these layouts (tests/test_clutter_body_host.py), so a
   wrong cell, pose order or excluded index is orders of magnitude outside it.  The random cases assert two guards on their INPUTS,
   computed by the oracle: no part-frame coordinate within 1e-4 cells of a volume's boundary planes, at least 10 % of the
   (node, part) pairs inside.
3. Through to the stepper, n_obj = 2: a SceneSDFSet of two identical grids against the one SceneSDF, bit for bit -- at 2 x 4 rows
   five eager iterations of which the third re-initialises two rows (step_reset), at 2 x 192 rows three replays of the captured
   graph (graph branches) against the single-grid stepper's replays; two different grids against the single-grid entry point per
   object, and the total against the class surface at 3e-4."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _clutter_oracle as co  # noqa: E402
import _scene_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402
from test_gpu_scene import Q_H, Q_ORIGIN, Q_SHAPE, _query_points  # noqa: E402  (the 257-point set of the single-grid query test)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def _hand(name):
    from graspqp_amd import ops

    return ops.HandHandle(get_hand_spec(name))


@functools.lru_cache(maxsize=None)
def _default_samples(name, n=512):
    return meshes.hand_surface_samples(get_hand_spec(name), n)


def _bits(a, b):
    """Bit for bit, NaNs included."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _set_of(gq, fields):
    f0 = fields[0]
    assert all(f.shape == f0.shape and np.array_equal(f.origin, f0.origin) and f.voxel == f0.voxel for f in fields)
    return gq.ops.SceneSDFSet(torch.stack([f.values for f in fields]).cuda(), [float(o) for o in f0.origin], float(f0.voxel))


# ---------------------------------------------------------------------------------------------------------------
# 1. grid selection, exact
# ---------------------------------------------------------------------------------------------------------------
T_SHAPE, T_H = (7, 6, 9), 0.04  # a box of 24 x 20 x 32 cm around the hands
MARGIN, DIST = 0.01, 0.10


@functools.lru_cache(maxsize=None)
def _three_fields():
    return tuple(so.random_field(T_SHAPE, co.centred(T_SHAPE, T_H), T_H, 40 + g) for g in range(3))


def _poses(spec, B, seed):
    gen = torch.Generator().manual_seed(seed)
    th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
    return torch.cat([0.05 * torch.randn(B, 3, generator=gen), torch.randn(B, 6, generator=gen), th], 1).float().cuda()


class _Launch:
    """The two fused launches through their C entry points, on a stack (ops.SceneSDFSet.grid_set) or on one grid."""

    def __init__(self, gq, hand, spec, samples, hp):
        self.gq, self.hand, self.spec, self.sm, self.hp = gq, hand, spec, samples, hp
        idx = torch.zeros(hp.shape[0], 1, dtype=torch.long, device="cuda")
        Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
        self.Rg, self.LT = Rg.contiguous(), LT.contiguous()

    def __call__(self, term, K, grid, rows, up=None, w=1.0, accumulate=0, bufs=None):
        n, L, sm = rows.stop - rows.start, self.hand.L, self.sm
        wrench, gRt = bufs or (torch.empty(n, L, 6, device="cuda"), torch.empty(n, 12, device="cuda"))
        e = torch.empty(n, device="cuda")
        hp, Rg, LT = self.hp[rows].contiguous(), self.Rg[rows].contiguous(), self.LT[rows].contiguous()
        up = None if up is None else up[rows].contiguous()
        if term == "scene":
            self.gq.ops._scene_call(grid, MARGIN, hp, sm.points, sm.link, L, Rg, LT, up, w, e, accumulate, wrench, gRt)
        else:
            self.gq.ops._approach_call(grid, MARGIN, DIST, K, hp, sm.points, sm.link, L, Rg, LT, self.spec.grasp_axis, up, w, e,
                                       accumulate, wrench, gRt)
        return e, wrench, gRt


@pytest.mark.parametrize("hand_name,Ns", [(h, n) for h in ("allegro", "panda") for n in (1, 63, 65, 512)])
def test_terms_select_the_grid_bit_for_bit(gq, hand_name, Ns):
    spec, hand = get_hand_spec(hand_name), _hand(hand_name)
    pts, lnk = _default_samples(hand_name)
    if Ns < 512:
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns
    fields = _three_fields()
    stack = _set_of(gq, fields)
    singles = [stack.scene(g) for g in range(3)]
    assert all(s.values.data_ptr() == stack.values[g].data_ptr() for g, s in enumerate(singles))  # shared memory
    gen = torch.Generator().manual_seed(3)
    seen_active = 0
    for r in (1, 3):
        B, L = 3 * r, hand.L
        run = _Launch(gq, hand, spec, samples, _poses(spec, B, 100 * r + Ns))
        up = torch.linspace(0.5, 3.0, B, device="cuda")
        pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12))]
        for term, K in (("scene", 0), ("corridor", 1), ("corridor", 4)):
            whole = slice(0, B)
            over = run(term, K, stack.grid_set, whole)
            acc = run(term, K, stack.grid_set, whole, up=up, w=0.0, accumulate=1, bufs=[p.clone() for p in pre])
            again = run(term, K, stack.grid_set, whole)
            torch.cuda.synchronize()
            active, differs = 0, 0
            for b in range(B):
                rows = slice(b, b + 1)
                one = run(term, K, singles[b // r].grid, rows)
                one_acc = run(term, K, singles[b // r].grid, rows, up=up, w=0.0, accumulate=1, bufs=[p[rows].clone() for p in pre])
                other = run(term, K, singles[(b // r + 1) % 3].grid, rows)
                torch.cuda.synchronize()
                for name, a, o in zip(("energy", "wrench", "gRt"), over, one):
                    assert _bits(a[rows], o), (term, K, r, b, name)
                for name, a, oa in zip(("wrench", "gRt"), acc[1:], one_acc[1:]):
                    assert _bits(a[rows], oa), (term, K, r, b, name, "accumulate")
                assert _bits(acc[0][rows], one[0])  # the energy is unweighted and overwritten
                active += int(one[0] > 0)
                differs += int(not _bits(one[0], other[0]))
            for a, b2 in zip(over, again):
                assert _bits(a, b2), (term, K, "run to run")
            # the case can fail: rows are active, and another grid gives other numbers (a single sample may miss the obstacles
            # in a combination; over the whole case it must not)
            assert active >= (1 if Ns > 1 else 0) and differs >= active - 1, (term, K, r, active, differs)
            seen_active += active
    assert seen_active >= 3, seen_active
    # G = 1: the single-grid launch on the whole batch
    run = _Launch(gq, hand, spec, samples, _poses(spec, 5, Ns))
    one_grid = _set_of(gq, fields[1:2])
    for term, K in (("scene", 0), ("corridor", 4)):
        for a, b in zip(run(term, K, one_grid.grid_set, slice(0, 5)), run(term, K, singles[1].grid, slice(0, 5))):
            assert _bits(a, b), (term, "G = 1")


def test_a_nan_row_leaves_the_other_rows_and_grids_alone(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, *_default_samples("allegro"))
    stack = _set_of(gq, _three_fields())
    hp = _poses(spec, 6, 17)
    bad = hp.clone()
    bad[2, 1] = float("nan")  # a row of grid 1
    run = _Launch(gq, hand, spec, samples, hp)
    for term, K in (("scene", 0), ("corridor", 4)):
        good = run(term, K, stack.grid_set, slice(0, 6))
        run.hp = bad
        got = run(term, K, stack.grid_set, slice(0, 6))
        run.hp = hp
        torch.cuda.synchronize()
        keep = torch.tensor([0, 1, 3, 4, 5], device="cuda")
        assert torch.isnan(got[0][2]) and torch.isfinite(good[0]).all() and (good[0] > 0).any()
        for a, b in zip(good, got):
            assert _bits(a[keep], b[keep]), term


def test_query_selects_the_grid_and_autograd(gq):
    fields = [so.random_field(Q_SHAPE, Q_ORIGIN, Q_H, 7 + g) for g in range(3)]
    stack = _set_of(gq, fields)
    x, kinds = _query_points()
    pts = torch.tensor(x, device="cuda")[None].repeat(3, 1, 1).contiguous()  # (G,257,3): the same points per grid
    phi, grad, inside = gq.ops._Eager.scene_distance_set(pts, stack.values, list(stack.origin), stack.voxel)
    torch.cuda.synchronize()
    assert phi.shape == (3, 257) and grad.shape == (3, 257, 3) and inside.shape == (3, 257)
    for g in range(3):
        one = stack.scene(g)
        p1, g1, i1 = gq.ops._Eager.scene_distance(pts[g], one.values, list(one.origin), one.voxel)
        assert _bits(phi[g], p1) and _bits(grad[g], g1) and torch.equal(inside[g], i1), g
    assert not _bits(phi[0], phi[1]) and int(inside[0].sum()) >= 100
    assert torch.isnan(phi[:, kinds["nonfinite"]]).all() and torch.isposinf(phi[:, kinds["outside"]]).all()
    # two points per grid of six: point i reads grid i // 2; and a leading dimension that G does not divide is refused
    six = pts[:, :2].reshape(6, 1, 3).contiguous()
    p6 = gq.ops.scene_distance(six, stack)
    assert _bits(p6.reshape(3, 2), phi[:, :2])
    with pytest.raises(ValueError, match="divisible"):
        gq.ops.scene_distance(pts[:, :1].reshape(3, 1, 3)[:2], stack)
    # autograd of the set-aware scene_distance: grad phi * upstream, zero outside the volume
    xg = pts.clone().requires_grad_()
    out = gq.ops.scene_distance(xg, stack)
    assert _bits(out.detach(), phi)
    up = torch.linspace(-1.0, 2.0, 3 * 257, device="cuda").reshape(3, 257)
    torch.where(torch.isfinite(out), out * up, torch.zeros_like(out)).sum().backward()
    torch.cuda.synchronize()
    fin = torch.isfinite(phi)
    want = grad * torch.where(fin, up, torch.zeros_like(up)).unsqueeze(-1)
    assert torch.equal(xg.grad[fin], want[fin]) and (xg.grad[torch.isposinf(phi)] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. compose against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------
def _compose(gq, out, tT, parts, pT, ex, base, far=co.FAR, stack=None):
    stack = stack or gq.ops.SceneSDFSet.empty(out.n_grids, [float(o) for o in out.origin], out.shape, float(out.voxel))
    stack.values.fill_(-7.0)  # every node must be written
    gq.ops.scene_compose(stack, tT.cuda(), [F.scene(gq) for F in parts], pT.cuda(), None if ex is None else ex.cuda(),
                         None if base is None else base.scene(gq), far)
    torch.cuda.synchronize()
    return stack


def _close(got, ref, tag):
    got, ref = got.cpu().numpy(), ref.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), tag
    ok = ~np.isnan(ref)
    print(f"[{tag}] max abs err {np.abs(got[ok] - ref[ok]).max():.3e} (max |phi| {np.abs(ref[ok]).max():.3e})")
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-5, atol=1e-6, err_msg=tag)


@pytest.mark.parametrize("with_base", [True, False])
@pytest.mark.parametrize("kind,seed", [("affine", co.SEEDS[0]), ("random", co.SEEDS[0]), ("random", co.SEEDS[1])])
def test_compose_matches_the_oracle(gq, kind, seed, with_base):
    out, tT, parts, pT, ex, base = co.layout(seed, kind)
    base = base if with_base else None
    ref, info = co.compose(out, tT, parts, pT, ex, base, co.FAR)
    print(f"[{kind} {seed} base={with_base}] guards: nearest boundary plane {info['edge']:.2e} cells, inside {info['inside']:.3f}")
    if kind == "random":
        assert info["edge"] >= co.EDGE and info["inside"] >= 0.10, info
    stack = _compose(gq, out, tT, parts, pT, ex, base)
    _close(stack.values, ref, f"{kind} {seed} base={with_base}")
    assert float((stack.values < co.FAR).float().mean()) >= 0.2  # the parts are seen
    again = _compose(gq, out, tT, parts, pT, ex, base)
    assert _bits(stack.values, again.values)  # run to run


def test_compose_beyond_one_tile_and_a_part_out_of_reach(gq):
    """(5,9,17) nodes: two tiles of 4 x 4 x 16 along x and z, three along y, none of them full.  A part far outside every target
    is left out by every block: the result is the composition without it, bit for bit."""
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "random", out_shape=co.OUT_SHAPE_TILES)
    ref, info = co.compose(out, tT, parts, pT, ex, base, co.FAR)
    assert info["edge"] >= co.EDGE and info["inside"] >= 0.10, info
    stack = _compose(gq, out, tT, parts, pT, ex, base)
    _close(stack.values, ref, "(5,9,17)")
    far_T = pT.clone()
    far_T[1, :, 3] = torch.tensor([0.5, -0.5, 0.5])
    moved = _compose(gq, out, tT, parts, far_T, ex, base)
    without = _compose(gq, out, tT, [parts[0], parts[2]], pT[[0, 2]], torch.tensor([0, -1, 1], dtype=torch.int32), base)
    assert _bits(moved.values, without.values) and not _bits(moved.values, stack.values)
    # no parts at all: the base alone; and exclude = None leaves no part out
    only_base = _compose(gq, out, tT, [], pT[:0], None, base)
    _close(only_base.values, co.compose(out, tT, [], pT[:0], None, base, co.FAR)[0], "base alone")
    everything = _compose(gq, out, tT, parts, pT, None, base)
    _close(everything.values, co.compose(out, tT, parts, pT, None, base, co.FAR)[0], "exclude = None")


def test_compose_nan_target_pose_and_nan_node(gq):
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "random")
    good = _compose(gq, out, tT, parts, pT, ex, base)
    T = tT.clone()
    T[1, 2, 3] = float("nan")
    got = _compose(gq, out, T, parts, pT, ex, base)
    assert torch.isnan(got.values[1]).all() and _bits(got.values[[0, 2]], good.values[[0, 2]])
    assert torch.isfinite(good.values).all()
    v = parts[1].values.clone()
    v[1, 2, 2] = float("nan")  # the min must not drop it
    poisoned = [parts[0], so.Field(parts[1].shape, parts[1].origin, parts[1].voxel, values=v), parts[2]]
    ref, _ = co.compose(out, tT, poisoned, pT, ex, base, co.FAR)
    got = _compose(gq, out, tT, poisoned, pT, ex, base)
    assert int(torch.isnan(ref).sum()) >= 10
    _close(got.values, ref, "NaN node")


def test_compose_in_a_captured_graph_follows_a_pose_update(gq):
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[1], "random")
    scenes, bs = [F.scene(gq) for F in parts], base.scene(gq)
    tTd, pTd, exd = tT.cuda().contiguous(), pT.cuda().contiguous(), ex.cuda()
    stack = gq.ops.SceneSDFSet.empty(out.n_grids, [float(o) for o in out.origin], out.shape, float(out.voxel))
    gq.ops.scene_compose(stack, tTd, scenes, pTd, exd, bs, co.FAR)  # warm-up outside the capture
    torch.cuda.synchronize()
    first = stack.values.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gq.ops.scene_compose(stack, tTd, scenes, pTd, exd, bs, co.FAR)
    stack.values.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(stack.values, first)
    new_pT = co.poses(len(parts), 777, 0.015)
    pTd.copy_(new_pT.cuda())  # in place: the replay reads the new poses
    exd.copy_(torch.tensor([1, 2, -1], dtype=torch.int32).cuda())
    graph.replay()
    torch.cuda.synchronize()
    fresh = _compose(gq, out, tT, parts, new_pT, torch.tensor([1, 2, -1], dtype=torch.int32), base)
    assert _bits(stack.values, fresh.values) and not _bits(stack.values, first)


def test_compose_refusals(gq):
    out, tT, parts, pT, ex, base = co.layout(co.SEEDS[0], "affine")
    stack = gq.ops.SceneSDFSet.empty(3, [0.0, 0.0, 0.0], (4, 4, 4), 0.01)
    scenes = [F.scene(gq) for F in parts]
    with pytest.raises(ValueError, match="far"):
        gq.ops.scene_compose(stack, tT.cuda(), scenes, pT.cuda(), None, None, float("inf"))
    with pytest.raises(ValueError, match="base"):
        gq.ops.scene_compose(stack, tT.cuda(), [], None, None, None, 0.02)
    with pytest.raises(ValueError, match="target_T"):
        gq.ops.scene_compose(stack, tT[:2].cuda(), scenes, pT.cuda(), None, None, 0.02)
    with pytest.raises(ValueError, match="part_T"):
        gq.ops.scene_compose(stack, tT.cuda(), scenes, pT[:2].cuda(), None, None, 0.02)
    with pytest.raises(ValueError, match="n_parts"):
        gq.ops.scene_compose(stack, tT.cuda(), scenes * 11, pT.repeat(11, 1, 1).cuda(), None, None, 0.02)
    with pytest.raises(ValueError, match="n_grids"):
        gq.ops.SceneSDFSet(torch.zeros(0, 2, 2, 2, device="cuda"), (0.0, 0.0, 0.0), 0.1)
    with pytest.raises(ValueError, match="nx"):
        gq.ops.SceneSDFSet(torch.zeros(2, 1, 2, 2, device="cuda"), (0.0, 0.0, 0.0), 0.1)
    v = torch.zeros(2, 3, 3, 3, device="cuda")
    assert gq.ops.SceneSDFSet(v, (0.0, 0.0, 0.0), 0.1).values.data_ptr() == v.data_ptr()  # used without a copy


# ---------------------------------------------------------------------------------------------------------------
# 3. through to the stepper: two objects
# ---------------------------------------------------------------------------------------------------------------
S_SHAPE, S_ORIGIN, S_H = (100, 100, 100), (-0.5013, -0.4987, -0.5021), 0.01
STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")
W_SCENE, W_BOTH = {"E_scene": 50.0}, {"E_scene": 50.0, "E_approach": 20.0}


@functools.lru_cache(maxsize=None)
def _wall(c=0.02):
    """A half-space through the workspace: a wall the hands of the fixtures reach into."""
    return so.affine(S_SHAPE, S_ORIGIN, S_H, c=c)


@functools.lru_cache(maxsize=None)
def _two_objects(be):
    spec = get_hand_spec("allegro")
    fv = meshes.icosphere(2, 0.05)
    sp = meshes.surface_points(fv, 256, oversample=4)
    B, n = 2 * be, 4
    gen = torch.Generator().manual_seed(B)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1) * 0.12
    hp = torch.cat([t, torch.randn(B, 6, generator=gen), torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=gen)], 1).cuda()
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda()
    draws = [(torch.rand(B, n, generator=gen).cuda(), torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda(),
              torch.rand(B, generator=gen).cuda()) for _ in range(5)]
    return fv, sp, n, hp, idx, draws


def _stepper(gq, be, sm, **kw):
    fv, sp, n, _, _, _ = _two_objects(be)
    surf = torch.tensor(np.stack([sp, sp]))
    return gq.stepper.GraspStepper(_hand("allegro"), gq.ops.MeshSet([fv, fv]), surf, be, n, surface_samples=sm, scene_margin=0.01,
                                   approach_distance=DIST, approach_stations=4, **kw)


def _sm(golden_dir):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    return ge["opt_surface_points"], ge["opt_surface_link"]


@pytest.mark.parametrize("weights", [W_SCENE, W_BOTH], ids=["scene", "scene+approach"])
@pytest.mark.parametrize("be,mode", [(4, "eager, step_reset"), (192, "graph branches")])
def test_identical_grids_equal_the_single_grid_stepper(gq, golden_dir, be, mode, weights):
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    B = 2 * be
    stack = _set_of(gq, [_wall(), _wall()])
    mask = torch.zeros(B, dtype=torch.bool)
    mask[[1, B - 2]] = True  # a row of each object
    out = []
    for scene in (_wall().scene(gq), stack):
        st = _stepper(gq, be, sm, weights=dict(weights), scene=scene)
        assert st.clutter == (scene is stack) and st.term_names[5:] == tuple(weights)
        st.reset(hp, idx)
        assert float(st.terms[5].max()) > 0
        if mode == "graph branches":
            st.capture()
            assert st.graph_mode == mode
            for d in draws[:3]:
                st.step(draws=d)
        else:
            for s, d in enumerate(draws):
                if s == 2:
                    st.step_reset(mask, hp.roll(3, 0), idx.roll(3, 0), draws=d)
                else:
                    st.step(draws=d)
        torch.cuda.synchronize()
        out.append([getattr(st, k).clone() for k in STATE] + [st.terms_new.clone(), st.total_new.clone()])
    for a, b, k in zip(out[0], out[1], STATE + ("terms_new", "total_new")):
        assert _bits(a.float(), b.float()) if a.is_floating_point() else torch.equal(a, b), k
    assert torch.isfinite(out[0][2]).all()


def test_different_grids_evaluate_per_object_and_the_class_surface(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    be = 4
    sm = _sm(golden_dir)
    fv, sp, n, hp, idx, _ = _two_objects(be)
    stack = _set_of(gq, [_wall(), _wall(-0.01)])  # the second object's wall stands 3 cm further in
    w = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0, **W_BOTH}
    st = _stepper(gq, be, sm, weights=dict(W_BOTH), scene=stack)
    terms, total, _ = st.evaluate(hp, idx)
    torch.cuda.synchronize()
    assert list(terms)[5:] == ["E_scene", "E_approach"]
    hand, L = _hand("allegro"), _hand("allegro").L
    samples = st.samples
    for g in range(2):
        rows = slice(g * be, (g + 1) * be)
        pose, Rg, LT = st.pose_new[rows].contiguous(), st.Rg[rows].contiguous(), st.link_T[rows].contiguous()
        e = torch.empty(be, device="cuda")
        gq.ops._scene_call(stack.scene(g).grid, 0.01, pose, samples.points, samples.link, L, Rg, LT, None, 0.0, e, 0, None, None)
        assert _bits(terms["E_scene"][rows], e) and (e > 0).any(), g
        gq.ops._approach_call(stack.scene(g).grid, 0.01, DIST, 4, pose, samples.points, samples.link, L, Rg, LT,
                              get_hand_spec("allegro").grasp_axis, None, 0.0, e, 0, None, None)
        assert _bits(terms["E_approach"][rows], e) and (e > 0).any(), g
        other = torch.empty(be, device="cuda")
        gq.ops._scene_call(stack.scene(1 - g).grid, 0.01, pose, samples.points, samples.link, L, Rg, LT, None, 0.0, other, 0, None, None)
        assert not _bits(terms["E_scene"][rows], other), g
    # the class surface with the same stack: the total at DESIGN 14's 3e-4, the two terms at the bound of the query
    hm = HandModel(get_hand_spec("allegro"), "cuda")
    hm.set_surface_points(samples.points.cpu().numpy(), samples.link.cpu().numpy())
    hm.set_scene(stack, 0.01)
    hm.set_approach(DIST, 4)
    om = ObjectModel(batch_size_each=be, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv, fv], surface_points_list=[sp, sp])
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=list(w), svd_gain=0.1)
    want = sum(w[k] * losses[k] for k in w).detach()
    rel = ((total - want).abs() / want.abs().clamp_min(1e-12)).cpu().numpy()
    print(f"[class surface] total rel err max {rel.max():.3e}")
    assert rel.max() < 3e-4
    for k in ("E_scene", "E_approach"):
        np.testing.assert_allclose(terms[k].cpu().numpy(), losses[k].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_zero_weight_with_a_set_is_the_stepper_without_a_scene(gq, golden_dir):
    be = 4
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    stack = _set_of(gq, [_wall(), _wall(-0.01)])
    fv, sp, n, _, _, _ = _two_objects(be)
    plain = gq.stepper.GraspStepper(_hand("allegro"), gq.ops.MeshSet([fv, fv]), torch.tensor(np.stack([sp, sp])), be, n)
    zero = _stepper(gq, be, sm, weights={"E_scene": 0.0, "E_approach": 0.0}, scene=stack)
    assert not zero.clutter and zero.scene is None and zero._fuse_loop and zero.term_names == plain.term_names and zero.samples is None
    for st in (plain, zero):
        st.reset(hp, idx)
        for d in draws[:3]:
            st.step(draws=d)
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(plain, k), getattr(zero, k)), k


def test_a_recompose_between_two_graph_replays(gq, golden_dir):
    """The stack is composed from one posed part (a tilted half-space on a 64^3 grid); the part moves 3 cm between two replays.
    The second replay equals a stepper built on a freshly composed stack, bit for bit, and its E_scene is the fp64 oracle's on the
    new composition (the hinge sum of DESIGN 14 at rtol 1e-5 / atol 1e-6), not on the old one."""
    be = 4
    sm = _sm(golden_dir)
    spec = get_hand_spec("allegro")
    _, _, _, hp, idx, draws = _two_objects(be)
    shape, h = (64, 64, 64), 0.0125
    part = so.affine(shape, co.centred(shape, h), h, c=0.02)
    out = co.Out(2, (60, 60, 60), co.centred((60, 60, 60), 0.0125), 0.0125)
    tT = co.poses(2, 31, 0.01)
    pT1 = co.poses(1, 32, 0.01)
    pT2 = pT1.clone()
    pT2[0, :, 3] += 0.03 * (pT1[0, :, :3] @ torch.tensor([0.36, -0.48, 0.8]))  # along the wall's normal, into the workspace
    far = 0.05
    pTd = pT1.cuda().contiguous()
    stack = gq.ops.SceneSDFSet.empty(2, [float(o) for o in out.origin], out.shape, 0.0125)
    compose = lambda: gq.ops.scene_compose(stack, tT.cuda(), [part.scene(gq)], pTd, None, None, far)
    compose()
    st = _stepper(gq, be, sm, weights=dict(W_SCENE), scene=stack)
    st.reset(hp, idx)
    st.capture()
    st.step(draws=draws[0])
    torch.cuda.synchronize()
    after_one = {k: getattr(st, k).clone() for k in STATE}
    pTd.copy_(pT2.cuda())  # a 12-float write ...
    compose()              # ... and one launch
    st.step(draws=draws[1])
    torch.cuda.synchronize()
    got = st.terms_new[5].clone()
    fresh = gq.ops.SceneSDFSet.empty(2, [float(o) for o in out.origin], out.shape, 0.0125)
    gq.ops.scene_compose(fresh, tT.cuda(), [part.scene(gq)], pT2.cuda(), None, None, far)
    ref = _stepper(gq, be, sm, weights=dict(W_SCENE), scene=fresh)
    ref.reset(hp, idx)
    for k in STATE:
        getattr(ref, k).copy_(after_one[k])
    ref.step(draws=draws[1])
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(st, k), getattr(ref, k)), k
    assert _bits(got, ref.terms_new[5])
    # the oracle: E_scene of the proposal on the fp64 composition, object by object
    pose = st.pose_new.double().cpu()
    for pT, same in ((pT2, True), (pT1, False)):
        phi, _ = co.compose(out, tT, [part], pT, None, None, far)
        e = np.concatenate([so.e_scene(spec, sm[0], sm[1], pose[g * be:(g + 1) * be],
                                       so.Field(out.shape, out.origin, out.voxel, values=phi[g].float()), 0.01)["E"] for g in range(2)])
        close = np.allclose(got.cpu().numpy(), e, rtol=1e-5, atol=1e-6)
        print(f"[recompose] part pose {'new' if same else 'old'}: max abs diff {np.abs(got.cpu().numpy() - e).max():.3e} (max E {e.max():.3e})")
        assert close == same and e.max() > 0


def test_stepper_and_class_surface_refusals(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    be = 4
    sm = _sm(golden_dir)
    fv, sp, n, hp, idx, _ = _two_objects(be)
    three = _set_of(gq, [_wall(), _wall(), _wall()])
    for weights in (W_SCENE, {"E_approach": 1.0}):
        with pytest.raises(ValueError, match="n_grids"):
            _stepper(gq, be, sm, weights=dict(weights), scene=three)
    hm = HandModel(get_hand_spec("allegro"), "cuda")
    hm.set_surface_points(*sm)
    hm.set_scene(three, 0.01)  # 8 rows, 3 grids
    om = ObjectModel(batch_size_each=be, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv, fv], surface_points_list=[sp, sp])
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    with pytest.raises(ValueError, match="divisible"):
        calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_scene"], svd_gain=0.1)
    with pytest.raises(ValueError, match="SceneSDFSet"):
        hm.set_scene(torch.zeros(2, 2, 2), 0.0)
