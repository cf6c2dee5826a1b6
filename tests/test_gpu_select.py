"""GPU tests of the grasp-set selection (include/graspqp_hip.h, "grasp-set selection"): ops.grasp_distances against the definition
summed over the actual samples in fp64, ops.grasp_select against the fp64 oracle of tests/_select_oracle.py, and
GraspStepper.select / export_poses(selection=...) on a stepper run next to a wall.

Sets: Allegro, 2 objects x 70 rows, the poses a short run from a seeded initialize() with one row copied onto another; and the
64-link chain of tests/_synthetic_hand.py (the most links SurfaceSamples accepts), 2 x 24 rows around eight base poses.

Distance bound, per pair: |d_hip - d_fp64| <= max(2 |d_np32 - d_fp64|, 1e-7 m) and <= 1e-5 m, where d_fp64 sums
|x_w,i(s) - x_w,j(s)|^2 over the samples in fp64 from the product's own Rg / link_T (FK is pinned elsewhere) and d_np32 is the
closed form restated in numpy float32: the noise-relative rule of tests/_parity.py with an absolute ceiling of 0.1 % of a 1 cm
radius.  The diagonal and the copied pair are exactly 0, the matrix exactly symmetric.

The selection must equal the oracle's exactly.  That is a fair demand because the test first asserts, on the CPU, that every pair
the oracle's greedy run compares has |d^2 / radius^2 - 1| > 1e-3 -- a condition on the inputs (seed and radius are chosen so that it
holds), four orders of magnitude above the error of d^2."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import init as oinit  # noqa: E402

import _fk_backward_case as fkb  # noqa: E402
import _scene_oracle as so  # noqa: E402
import _select_oracle as oracle  # noqa: E402
import _synthetic_hand as sh  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

N_OBJ = 2
RADIUS = {"allegro": 0.05, "chain64": 0.008}
K = 8


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, export, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper, "export": export})


@functools.lru_cache(maxsize=None)
def _object():
    fv = meshes.superquadric(40, 32, 16)
    return fv, oinit.convex_hull_faces(fv.reshape(-1, 3)), meshes.surface_points(fv, 300, oversample=4)


def _hulls():
    hull = _object()[1]
    fv = torch.tensor(np.concatenate([hull] * N_OBJ), dtype=torch.float32).cuda().contiguous()
    cdf = torch.tensor(np.concatenate([oinit.area_cdf(hull)] * N_OBJ), dtype=torch.float32).cuda().contiguous()
    off = torch.tensor(np.cumsum([0] + [len(hull)] * N_OBJ), dtype=torch.int32).cuda()
    return fv, cdf, off


def _stepper(gq, hand, be, weights=None, seed=11, **kw):
    fv, _, sp = _object()
    st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv] * N_OBJ), torch.tensor(np.stack([sp] * N_OBJ)), be, 4, weights=weights,
                                 seed=seed, **kw)
    st.set_hulls(_hulls())
    return st


@pytest.fixture(scope="module")
def allegro(gq):
    hand = gq.ops.HandHandle(get_hand_spec("allegro"))
    yield hand
    hand.close()


@pytest.fixture(scope="module")
def sets(gq, allegro, tmp_path_factory):
    """name -> dict(hp, Rg, LT device tensors, samples, be, copied = (row, row), score, terms): computed once, left unchanged"""
    out = {}
    # Allegro: a short run from a seeded initialize()
    be = 70
    st = _stepper(gq, allegro, be, seed=5)
    st.initialize()
    for _ in range(6):
        st.step()
    hp = st.hand_pose.clone()
    hp[9] = hp[5]
    hp[be + 30] = hp[be + 2]
    pts, lnk = meshes.hand_surface_samples(allegro.spec, 128)
    out["allegro"] = dict(hand=allegro, hp=hp, be=be, samples=gq.ops.SurfaceSamples(allegro, pts, lnk), copied=[(5, 9), (be + 2, be + 30)])
    # the 64-link chain: eight base poses, rows within millimetres of them
    spec = sh.build("chain64", tmp_path_factory.mktemp("synthetic_hands"))
    hand = gq.ops.HandHandle(spec)
    be = 24
    base = fkb.make_inputs(spec, 8, 4, 70, sh.joint_scale(spec))["hand_pose"]
    r = np.random.RandomState(3)
    rows = base[r.randint(0, 8, N_OBJ * be)].copy()
    rows[:, :3] += r.uniform(-0.004, 0.004, (N_OBJ * be, 3)).astype(np.float32)
    rows[:, 9:] += (0.02 * sh.joint_scale(spec) * r.standard_normal((N_OBJ * be, spec.n_dofs))).astype(np.float32)
    rows[7] = rows[3]
    link = r.randint(0, 64, 200)
    link[link == 17] = 18  # a link without samples
    link[:2] = [0, 63]
    pts = r.uniform(-0.01, 0.01, (200, 3)).astype(np.float32)
    out["chain64"] = dict(hand=hand, hp=torch.tensor(rows).cuda(), be=be, samples=gq.ops.SurfaceSamples(hand, pts, link), copied=[(3, 7)])
    for name, s in out.items():
        B = s["hp"].shape[0]
        idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
        s["Rg"], s["LT"] = (t.detach().contiguous() for t in gq.ops.fk_contacts(s["hp"], idx, s["hand"])[:2])
        g = np.random.default_rng(17)
        s["score"] = g.normal(0, 3, B).astype(np.float32)
        s["terms"] = np.where(g.random((2, B)) < 0.8, 0.0, g.random((2, B))).astype(np.float32)
        # the oracle's view: fp64 of the product's float32 arrays
        a = lambda t: t.cpu().numpy().astype(np.float64)
        s["np"] = dict(Rg=a(s["Rg"]), LT=a(s["LT"]), t=a(s["hp"][:, :3]), pts=a(s["samples"].points), link=s["samples"].link.cpu().numpy(),
                       mom=s["samples"].link_moments.cpu().numpy())
        n = s["np"]
        s["d2_fp64"] = oracle.dist2_samples(n["Rg"], n["t"], n["LT"], n["pts"], n["link"], s["be"])
    yield out
    out["chain64"]["hand"].close()


@pytest.mark.parametrize("name", ["allegro", "chain64"])
def test_distances_against_the_sum_over_the_samples(gq, sets, name):
    """Measured on the MI355X: see DESIGN section 22."""
    s, n = sets[name], sets[name]["np"]
    be = s["be"]
    d = gq.ops.grasp_distances(s["hp"], s["Rg"], s["LT"], s["samples"], be)
    assert d.shape == (N_OBJ, be, be) and d.dtype == torch.float32
    d = d.cpu().numpy()
    d64 = np.sqrt(s["d2_fp64"])
    W32 = oracle.world(n["Rg"], n["t"], n["LT"], np.float32)
    d32 = np.sqrt(oracle.dist2_closed(W32, n["mom"], s["samples"].Ns, be, np.float32)).astype(np.float64)
    err, floor = np.abs(d - d64), np.abs(d32 - d64)
    print(f"{name}: d in [{d64[d64 > 0].min():.3g}, {d64.max():.3g}] m; max |d_hip - d_fp64| = {err.max():.3g} m, "
          f"max |d_np32 - d_fp64| = {floor.max():.3g} m, worst err / max(2 floor, 1e-7) = {(err / np.maximum(2 * floor, 1e-7)).max():.3g}")
    assert np.all(err <= np.maximum(2 * floor, 1e-7)) and err.max() <= 1e-5
    assert not np.diagonal(d, axis1=1, axis2=2).any() and np.array_equal(d, d.transpose(0, 2, 1))
    for i, j in s["copied"]:
        o = i // be
        assert d[o, i % be, j % be] == 0.0 and d[o, j % be, i % be] == 0.0
    off = d64[~np.eye(be, dtype=bool)[None].repeat(N_OBJ, 0)]
    assert (off < 0.02).any() and (off > 0.05 if name == "allegro" else off > 0.02).any()  # near and far pairs both occur


def _variant(s, case):
    """score, terms, tol, radius of a selection case on a set"""
    be, score, terms = s["be"], s["score"].copy(), s["terms"].copy()
    radius = RADIUS["allegro" if be == 70 else "chain64"]
    if case == "gated":
        pass
    elif case == "none_and_few":
        terms[0, :be] = 0.5  # the first object has no feasible row
        terms[0, be:] = 0.5
        terms[:, be + 3:be + 8] = 0.0  # the second has five, fewer than K
    elif case == "radius_0":
        radius = 0.0
    return score, terms, [0.0, 0.0], radius


@pytest.mark.parametrize("case", ["gated", "none_and_few", "radius_0"])
@pytest.mark.parametrize("name", ["allegro", "chain64"])
def test_selection_equals_the_fp64_oracle(gq, sets, name, case):
    s, n = sets[name], sets[name]["np"]
    be = s["be"]
    score, terms, tol, radius = _variant(s, case)
    r2 = float(np.float32(radius)) ** 2
    want = oracle.select(s["d2_fp64"], score, terms, tol, be, K, r2)
    margins = [abs(s["d2_fp64"][o, r, p] / r2 - 1.0) for o, r, p in want[4]]
    print(f"{name}/{case}: n_feasible {want[2].tolist()}, n_selected {want[1].tolist()}, {len(margins)} pairs compared, "
          f"smallest |d^2/r^2 - 1| = {min(margins, default=np.inf):.3g}, suppressed {sum(s['d2_fp64'][o, r, p] < r2 for o, r, p in want[4])}")
    assert all(m > 1e-3 for m in margins), "a condition on the inputs: choose another seed or radius"
    if case == "gated":
        assert any(s["d2_fp64"][o, r, p] < r2 for o, r, p in want[4]) and want[1].min() >= 4  # suppression happens
    if case == "none_and_few":
        assert want[2].tolist() == [0, 5] and want[1][0] == 0 and 0 < want[1][1] <= 5
    dev = lambda a: torch.tensor(a).cuda()
    got = gq.ops.grasp_select(s["hp"], s["Rg"], s["LT"], s["samples"], be, dev(score), dev(terms), tol, K, radius)
    again = gq.ops.grasp_select(s["hp"], s["Rg"], s["LT"], s["samples"], be, dev(score), dev(terms), tol, K, radius)
    assert got.sel.dtype == torch.int32 and got.sel.shape == (N_OBJ, K) and got.feasible.shape == (N_OBJ * be,)
    for g, a, w, what in zip(got, again, want, ("sel", "n_selected", "n_feasible", "feasible")):
        assert np.array_equal(g.cpu().numpy(), w), (name, case, what, g.cpu().numpy(), w)
        assert torch.equal(g, a), "two calls give identical bits"
    if case == "radius_0":  # the K best feasible rows
        ok = oracle.feasible(score, terms, tol)
        for o in range(N_OBJ):
            rows = [r for r in np.argsort(score[o * be:(o + 1) * be], kind="stable") if ok[o * be + r]][:K]
            assert got.sel[o].cpu().tolist() == [o * be + int(r) for r in rows]


def test_graph_replay_reads_the_new_score(gq, sets):
    s = sets["allegro"]
    be, B = s["be"], s["hp"].shape[0]
    score, terms, tol, radius = _variant(s, "gated")
    sc, tm = torch.tensor(score).cuda(), torch.tensor(terms).cuda()
    call = lambda: gq.ops.grasp_select(s["hp"], s["Rg"], s["LT"], s["samples"], be, sc, tm, tol, K, radius)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    assert all(torch.equal(a, b) for a, b in zip(out, first))
    new = torch.tensor(np.random.default_rng(4).normal(0, 3, B).astype(np.float32)).cuda()
    sc.copy_(new)
    g.replay()
    eager = gq.ops.grasp_select(s["hp"], s["Rg"], s["LT"], s["samples"], be, new, tm, tol, K, radius)
    assert all(torch.equal(a, b) for a, b in zip(out, eager)) and not torch.equal(eager.sel, first.sel)


# ---- the stepper ------------------------------------------------------------------------------------------------------------
BE, ITERS = 64, 30
SHAPE, H = (80, 80, 80), 0.005
ORIGIN = (-0.5 * 79 * H,) * 3
WEIGHTS = {"E_scene": 50.0, "E_approach": 20.0}


def _wall_stepper(gq, hand, seed=11):
    wall = so.Field(SHAPE, ORIGIN, H, analytic=lambda x: 0.08 - x[..., 0]).scene(gq)  # free for x < 8 cm
    raw = meshes.hand_surface_samples(hand.spec, 128)
    st = _stepper(gq, hand, BE, WEIGHTS, seed=seed, scene=wall, scene_margin=0.005, approach_distance=0.10, approach_stations=4,
                  surface_samples=raw)
    st.initialize()
    return st


@pytest.fixture(scope="module")
def run(gq, allegro):
    st = _wall_stepper(gq, allegro)
    for _ in range(ITERS):
        st.step()
    return st


def test_stepper_select_properties(gq, run):
    st = run
    radius = 0.02
    sel = st.select(K, radius=radius)
    assert all(t.is_cuda for t in sel)
    i_s, i_a = st.term_names.index("E_scene"), st.term_names.index("E_approach")
    free = (st.terms[i_s] <= 0) & (st.terms[i_a] <= 0) & torch.isfinite(st.energy)
    print("n_feasible", sel.n_feasible.tolist(), "n_selected", sel.n_selected.tolist())
    assert torch.equal(sel.feasible.bool(), free) and sel.n_feasible.tolist() == free.view(N_OBJ, BE).sum(1).tolist()
    assert 0 < int(free.sum()) < N_OBJ * BE, "the wall must leave some rows feasible and some not"
    Rg, LT = st._select_fk
    d = gq.ops.grasp_distances(st.hand_pose, Rg, LT, st.samples, BE)
    for o in range(N_OBJ):
        n = int(sel.n_selected[o])
        rows = sel.sel[o, :n].long()
        assert n > 0 and (sel.sel[o, n:] == -1).all() and (rows // BE == o).all()
        assert free[rows].all()  # every selected row has its gated terms at or below the tolerance
        e = st.energy[rows]
        assert (e[1:] >= e[:-1]).all()  # the picks' scores ascend
        sub = d[o][rows % BE][:, rows % BE] + torch.eye(n, device="cuda")
        assert (sub >= radius).all(), "no two selected rows of an object are closer than the radius"
    # an explicit gate on E_pen on top: n_feasible follows
    i_p = st.term_names.index("E_pen")
    tol_pen = float(st.terms[i_p][free].median())
    gated = st.select(K, radius=radius, gates={"E_scene": 0.0, "E_approach": 0.0, "E_pen": tol_pen})
    want = (free & (st.terms[i_p] <= tol_pen)).view(N_OBJ, BE).sum(1)
    assert gated.n_feasible.tolist() == want.tolist() and int(want.sum()) < int(free.sum())
    # another score
    other = st.select(K, radius=0.0, score=-st.energy)
    assert (st.energy[other.sel[0, :int(other.n_selected[0])].long()].diff() <= 0).all()
    with pytest.raises(ValueError, match="unknown or switched-off"):
        st.select(K, gates={"E_pregrasp": 0.0})
    with pytest.raises(ValueError, match="score"):
        st.select(K, score=st.energy[:5])
    with pytest.raises(RuntimeError, match="grasp_select.*K"):
        st.select(BE + 1)


def test_export_writes_the_selection(gq, run, tmp_path):
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    st = run
    sel = st.select(K, radius=0.02)
    fv, _, sp = _object()
    names = ["objA", "objB"]
    hm = HandModel(st.hand.spec, "cuda")
    om = ObjectModel(batch_size_each=BE, num_samples=300)
    om.initialize_from_meshes([fv] * N_OBJ, names, surface_points_list=[sp] * N_OBJ)
    hm.set_parameters(st.hand_pose.clone(), st.contact_idx.clone())
    files = gq.export.export_poses(hm, st.energy, om, names, BE, str(tmp_path), "allegro", 4, "graspqp", selection=sel)
    plain = gq.export.snapshot_dicts(hm, st.energy, om, N_OBJ, BE)
    none = gq.export.snapshot_dicts(hm, st.energy, om, N_OBJ, BE, selection=None)
    jn = list(hm._actuated_joints_names)
    for a, f in enumerate(files):
        data = torch.load(f, weights_only=True)
        n = int(sel.n_selected[a])
        rows = sel.sel[a, :n].long().cpu()
        assert set(data) == set(plain[a]) | {"selected_rows", "n_feasible"}
        assert data["selected_rows"].dtype == torch.int64 and data["selected_rows"].tolist() == (rows - a * BE).tolist()
        assert data["n_feasible"] == int(sel.n_feasible[a])
        local = data["selected_rows"]
        assert torch.equal(data["values"], plain[a]["values"][local]) and torch.equal(data["values"], st.energy.cpu()[rows])
        assert torch.equal(data["contact_idx"], plain[a]["contact_idx"][local])
        assert torch.equal(data["parameters"]["root_pose"], plain[a]["parameters"]["root_pose"][local])
        for key in ("parameters", "grasp_velocities", "full_grasp_velocities", "grasp_velocities_off"):
            for nm in jn:
                assert torch.equal(data[key][nm], plain[a][key][nm][local]), (key, nm)
        # selection=None is the call without the argument
        assert set(none[a]) == set(plain[a])
        assert torch.equal(none[a]["values"], plain[a]["values"]) and torch.equal(none[a]["contact_idx"], plain[a]["contact_idx"])
        for key in ("parameters", "grasp_velocities", "full_grasp_velocities", "grasp_velocities_off"):
            assert all(torch.equal(none[a][key][k], plain[a][key][k]) for k in plain[a][key])
    # an object with nothing selected still gets its file, with zero-length tensors
    empty = gq.ops.GraspSelection(torch.full_like(sel.sel, -1), torch.zeros_like(sel.n_selected), torch.zeros_like(sel.n_feasible),
                                  torch.zeros_like(sel.feasible))
    files = gq.export.export_poses(hm, st.energy, om, names, BE, str(tmp_path), "allegro", 4, "graspqp", suffix="_empty", selection=empty)
    for f in files:
        data = torch.load(f, weights_only=True)
        assert os.path.exists(f) and data["values"].shape == (0,) and data["parameters"]["root_pose"].shape == (0, 7)
        assert data["contact_idx"].shape == (0, 4) and data["selected_rows"].shape == (0,) and data["n_feasible"] == 0


def test_selecting_leaves_the_chain_as_it_is(gq, allegro, run):
    """A stepper that selects half way is, bit for bit, the stepper that never does (`run`)."""
    st = _wall_stepper(gq, allegro)
    for _ in range(ITERS // 2):
        st.step()
    st.select(K, radius=0.02)
    for _ in range(ITERS - ITERS // 2):
        st.step()
    assert torch.equal(st.hand_pose, run.hand_pose) and torch.equal(st.contact_idx, run.contact_idx)
    assert torch.equal(st.energy, run.energy) and torch.equal(st.terms, run.terms)
