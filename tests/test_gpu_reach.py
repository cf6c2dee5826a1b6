"""E_reach on the GPU: gq_reach_terms through ops.reach_terms, GraspStepper and calculate_energy against the fp64 oracle of
tests/_reach_oracle.py, on the SETTLED rows of its seeded cases (the oracle's E at M and at 2M updates agree to 1e-3, or both are
below 1e-12): per row |E - E_64| <= 2e-3 E_64 + 1e-10 (the project's rtol for such terms; the atol is 100 x the fp32 resolution of a
1 m chain, squared), the hand_pose gradient norm-wise 1e-3 overall and 2e-3 on the translation part and on the rotation part.  Every
compared set holds a row with a clamped joint, one with E > 1e-3 and one with E < 1e-10 (``_reach_oracle.compared_set``).
B = 8 rows, 2 objects x 4 rows with a base each, an icosphere of 80 faces."""
import numpy as np
import pytest
import torch

import _reach_oracle as ro

pytestmark = pytest.mark.gpu

W_REACH = 1e4  # E_reach is of the order 1e-3 m^2: this weight puts it beside the other terms
B, BE, N_CONTACT = 8, 4, 4


@pytest.fixture(scope="module")
def gq():
    import types

    from graspqp_amd import _C, ops
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.stepper import GraspStepper

    assert torch.cuda.is_available()
    spec = get_hand_spec("allegro")
    return types.SimpleNamespace(C=_C, ops=ops, GraspStepper=GraspStepper, spec=spec, hand=ops.HandHandle(spec), arms={})


def _arm(gq, cs):
    key = (cs["name"], cs["arm"].n_seeds)
    if key not in gq.arms:
        gq.arms[key] = gq.ops.ArmHandle(cs["arm"])
    return gq.arms[key]


def _pose(gq, cs):
    """(B, 9 + J) float32: the case's root poses with the joints at mid-range, and seeded contact indices."""
    spec = gq.spec
    mid = 0.5 * (np.asarray(spec.joints_lower, np.float32) + np.asarray(spec.joints_upper, np.float32))
    hp = torch.cat([torch.from_numpy(cs["pose9"]), torch.from_numpy(mid)[None].expand(B, -1)], 1).contiguous()
    idx = torch.randint(spec.n_contact_candidates, (B, N_CONTACT), generator=torch.Generator().manual_seed(4))
    return hp, idx


def _op(gq, cs, base_T=None, up=None, **kw):
    ops = gq.ops
    hp, idx = _pose(gq, cs)
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    base = torch.from_numpy(cs["base_T"] if base_T is None else base_T).cuda()
    e, q, seed = ops.reach_terms(hpc, gq.hand, ix, Rg, LT, ws, _arm(gq, cs), base, BE, cs["axis"], cs["distance"], cs["stations"],
                                 return_q=True, **kw)
    (e * torch.as_tensor(cs["up"] if up is None else up, dtype=torch.float32).cuda()).sum().backward()
    return e.detach().cpu().numpy(), q.cpu().numpy(), seed.cpu().numpy(), hpc.grad.cpu().numpy()


@pytest.mark.parametrize("n_seeds,stations", [(1, 0), (4, 0), (1, 2), (4, 2)])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_op_matches_the_oracle(gq, name, n_seeds, stations):
    cs = ro.case(name, n_seeds, stations)
    tag = f"{name} S={n_seeds} K={stations}"
    E, q, seed, grad = _op(gq, cs)
    assert (grad[:, 9:] == 0).all()  # the hand's joints get no gradient from the arm
    ro.assert_close(E, grad, cs, tag)
    arm, ref, m = cs["arm"], cs["ref"], cs["settled"]
    # reach_q lies within the limits (float32 of them), and its FK in fp64 reproduces E to the same bound
    assert (q >= arm.lower.astype(np.float32)).all() and (q <= arm.upper.astype(np.float32)).all()
    base = ro._T44(cs["base_T"])[torch.arange(B) // BE]
    pose = torch.as_tensor(cs["pose9"], dtype=ro.F64)
    R = ro.gramschmidt(pose[:, 3:9])
    a = torch.as_tensor(cs["axis"], dtype=ro.F64)
    Efk = np.zeros(B)
    for k in range(stations + 1):
        d = cs["distance"] * k / stations if stations else 0.0
        Tee, _, _ = ro.fk(arm, torch.as_tensor(q[:, k], dtype=ro.F64), base)
        e = ro.error(Tee, pose[:, :3] - d * (R @ a), R, ro.RHO)
        Efk += (e * e).sum(-1).numpy() / (stations + 1)
    print(f"[{tag}] FK of reach_q: worst |E_fk - E| / (2e-3 E + 1e-10) = {np.max(np.abs(Efk - E) / (2e-3 * E + 1e-10)):.2e}")
    assert (np.abs(Efk - E) <= 2e-3 * E + 1e-10).all()
    # the winning seed, where the oracle's two best seeds differ by more than 1 %
    if n_seeds > 1:
        two = np.sort(ref["Eks"], -1)
        clear = m[:, None] & (two[:, :, 1] > 1.01 * two[:, :, 0] + 1e-12)
        print(f"[{tag}] {int(clear.sum())} settled stations with a clear winner")
        assert (seed[clear] == ref["seed"][clear]).all(), (seed, ref["seed"])
        assert clear.any() or name in ("gantry6", "chain8")  # these reach most targets from every seed: E of the order 1e-33
    else:
        assert (seed == 0).all()


def test_rows_follow_their_object_base(gq):
    """Two different bases for the two objects: row b reads base_T[b // batch_each]; swapping the bases swaps the values."""
    cs = ro.case("elbow6", 1, 0)
    assert not np.allclose(cs["base_T"][0], cs["base_T"][1])
    E, _, _, _ = _op(gq, cs)
    # the rows of object 0 under base 1 and the other way round, from the oracle
    swapped = cs["base_T"][::-1].copy()
    want = ro.reach(cs["arm"], cs["pose9"], swapped, BE)
    want2 = ro.reach(cs["arm"], cs["pose9"], swapped, BE, n_iter=2 * ro.M)
    st = ro.settled(want["E"], want2["E"])
    Es, _, _, _ = _op(gq, cs, base_T=swapped)
    assert st.sum() >= 2 and (np.abs(Es - want["E"])[st] <= 2e-3 * want["E"][st] + 1e-10).all()
    assert np.abs(Es - E).max() > 1e-4  # the base matters on these rows
    # the same rows and the same base in the other object slot give the same bits
    hp, idx = _pose(gq, cs)
    roll = lambda x: np.concatenate([x[BE:], x[:BE]])
    cs2 = dict(cs, pose9=roll(cs["pose9"]), up=roll(cs["up"]))
    E2, _, _, _ = _op(gq, cs2, base_T=swapped)
    assert np.array_equal(roll(E2), E)


def test_bad_parameters_return_the_error_status(gq):
    C, ops = gq.C, gq.ops
    cs = ro.case("short3", 1, 0)
    arm = _arm(gq, cs)
    hp, idx = _pose(gq, cs)
    z = lambda *s: torch.zeros(*s, device="cuda")
    lib = C.lib()
    import ctypes

    axis = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    hpc, Rg, base, e = hp.cuda(), z(B, 9), torch.from_numpy(cs["base_T"]).cuda(), z(B)

    def status(batch=B, n_obj=2, be=BE, D=0.1, K=0, M=24, lam=1e-4, rho=0.1):
        return lib.gq_reach_terms(arm.handle, C.f32(hpc), hpc.shape[1], C.f32(Rg), batch, C.f32(base), n_obj, be, axis, D, K, M, lam, rho,
                                  None, 1.0, C.f32(e), None, None, 0, None, C.stream_ptr())

    assert status(K=4) == 2 and b"n_stations" in lib.gq_last_error()
    assert status(K=2, D=0.0) == 2 and b"distance" in lib.gq_last_error()
    assert status(lam=0.0) == 2 and b"damping" in lib.gq_last_error()
    assert status(rho=float("nan")) == 2 and b"rot_scale" in lib.gq_last_error()
    assert status(M=-1) == 2 and b"n_iterations" in lib.gq_last_error()
    assert status(n_obj=3) == 2 and b"base_T" in lib.gq_last_error()
    torch.cuda.synchronize()


# ---- the stepper ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, cs, weights=None, **kw):
    from graspqp_amd.utils import meshes

    fv = meshes.icosphere(1, 0.05).astype(np.float32)  # 80 faces
    sp = torch.tensor(np.stack([meshes.surface_points(fv, 256, oversample=8).astype(np.float32)] * 2))
    return gq.GraspStepper(gq.hand, gq.ops.MeshSet([fv, fv]), sp, BE, N_CONTACT, weights=weights, **kw)


def _reach_kw(gq, cs):
    return dict(arm=_arm(gq, cs), arm_base=cs["base_T"], reach_distance=cs["distance"], reach_stations=cs["stations"])


def _scene(gq):
    z = -0.3 + 0.05 * torch.arange(13, dtype=torch.float32)
    return gq.ops.SceneSDF(z.view(1, 1, 13).expand(13, 13, 13).contiguous(), (-0.3, -0.3, -0.3), 0.05)


@pytest.mark.parametrize("mode", ["alone", "together"])
def test_evaluate_adds_the_weighted_oracle_term(gq, mode):
    """terms, total and gradient of the stepper with the weight = the stepper without it on the same (pose, idx), plus w x the
    oracle's term and gradient; g_theta and g_R are bitwise those of the run without the term."""
    cs = ro.case("arm7", 4, 2, axis=tuple(float(a) for a in gq.spec.grasp_axis))  # the stepper takes the hand's grasp axis
    hp, idx = _pose(gq, cs)
    base, kw = {}, {}
    if mode == "together":
        base = {"E_pregrasp": 30.0, "E_squeeze": 1000.0, "E_prior": 7.0}
        kw = dict(pregrasp_scene=_scene(gq), pregrasp_distance=0.08, pregrasp_stations=2)
    st0 = _stepper(gq, cs, weights=base or None, **kw)
    st1 = _stepper(gq, cs, weights=dict(base, E_reach=W_REACH), **kw, **_reach_kw(gq, cs))
    assert st1.term_names == st0.term_names + ("E_reach",) and not st1._fuse_loop
    t0, tot0, g0 = st0.evaluate(hp.cuda(), idx.cuda())
    t1, tot1, g1 = st1.evaluate(hp.cuda(), idx.cuda())
    for k in st0.term_names:
        assert torch.equal(t0[k], t1[k]), k
    if mode == "together":
        assert torch.equal(st0.g_theta, st1.g_theta) and torch.equal(st0.g_R, st1.g_R) and st0.g_theta.abs().max() > 0
    np.testing.assert_allclose(tot1.cpu().numpy(), (tot0 + W_REACH * t1["E_reach"]).cpu().numpy(), rtol=1e-6)
    cs1 = dict(cs, ref=ro.reach(cs["arm"], cs["pose9"], cs["base_T"], BE, cs["axis"], cs["distance"], cs["stations"]))  # up = 1
    ro.assert_close(t1["E_reach"].cpu().numpy(), ((g1 - g0) / W_REACH).cpu().numpy(), cs1, f"stepper {mode}")
    assert tuple(st1.reach_q.shape) == (B, 3, 7) and tuple(st1.reach_seed.shape) == (B, 3)


def _draws(st, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(st.B, st.n, device="cuda", generator=g),
            torch.randint(st.hand.spec.n_contact_candidates, (st.B, st.n), device="cuda", generator=g),
            torch.rand(st.B, device="cuda", generator=g))


def _state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st.hand_pose, st.contact_idx, st.grad, st.energy, st.ema, st.step_count, st.terms)]


def test_weight_zero_or_absent_changes_nothing(gq):
    cs = ro.case("elbow6", 4, 2)
    hp, idx = _pose(gq, cs)

    def five(st):
        st.reset(hp.cuda(), idx.cuda())
        for s in range(5):
            st.step(draws=_draws(st, 100 + s))
        return _state(st)

    want = five(_stepper(gq, cs))
    for kw in (dict(weights={"E_reach": 0.0}), dict(weights={"E_reach": 0.0}, **_reach_kw(gq, cs))):
        st = _stepper(gq, cs, **kw)
        assert st.term_names == ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints") and st.reach_q is None and st._fuse_loop
        assert all(torch.equal(a, b) for a, b in zip(five(st), want))


def test_captured_graph_replays_equal_eager_steps_and_runs_repeat(gq):
    cs = ro.case("elbow6", 4, 2)
    hp, idx = _pose(gq, cs)
    out = []
    for captured in (False, True, False):
        st = _stepper(gq, cs, weights={"E_reach": W_REACH}, **_reach_kw(gq, cs))
        st.reset(hp.cuda(), idx.cuda())
        if captured:
            st.capture()
        for s in range(5):
            st.step(draws=_draws(st, 200 + s))
        out.append(_state(st) + [st.reach_q.clone(), st.reach_seed.clone()])
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))  # a captured graph replays bit for bit against eager
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[2]))  # two runs are bitwise equal
    assert (out[0][5] == 5).all() and torch.isfinite(out[0][3]).all()


def test_select_gates_on_the_term(gq):
    cs = ro.case("elbow6", 1, 0)
    hp, idx = _pose(gq, cs)
    st = _stepper(gq, cs, weights={"E_reach": W_REACH}, **_reach_kw(gq, cs))
    st.reset(hp.cuda(), idx.cuda())
    e = st.terms[st.term_names.index("E_reach")].cpu()
    tol = 1e-6
    keep = e <= tol
    assert 0 < int(keep.sum()) < B
    sel = st.select(BE, radius=0.0, gates={"E_reach": tol})
    for o in range(2):
        rows = sel.sel[o][: int(sel.n_selected[o])].cpu().tolist()
        assert sorted(rows) == (torch.nonzero(keep[o * BE:(o + 1) * BE]).flatten() + o * BE).tolist()  # global row indices
    assert sel.feasible.cpu().tolist() == keep.int().tolist()
    assert int(st.select(BE, radius=0.0).n_selected.sum()) == B  # not gated by default
    with pytest.raises(ValueError, match="E_reach"):
        _stepper(gq, cs).select(BE, gates={"E_reach": tol})  # a gate on the switched-off term


def test_class_surface_term_is_the_op(gq):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF
    from graspqp_amd.utils import meshes

    cs = ro.case("gantry6", 4, 2, axis=tuple(float(a) for a in gq.spec.grasp_axis))  # calculate_energy takes the hand's grasp axis
    hp, idx = _pose(gq, cs)
    fv = meshes.icosphere(1, 0.05).astype(np.float32)
    sp = meshes.surface_points(fv, 64, oversample=8).astype(np.float32)
    hm = HandModel(gq.spec, "cuda")
    om = ObjectModel(batch_size_each=BE, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv, fv], surface_points_list=[sp, sp])
    hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
    hm.set_reach(cs["arm"], cs["base_T"], cs["distance"], cs["stations"])
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_reach"], svd_gain=0.1)
    up = torch.as_tensor(cs["up"], dtype=torch.float32).cuda()
    (g,) = torch.autograd.grad((losses["E_reach"] * up).sum(), hm.hand_pose)
    E, _, _, grad = _op(gq, cs)
    assert np.array_equal(losses["E_reach"].detach().cpu().numpy(), E) and np.array_equal(g.cpu().numpy(), grad)
    ro.assert_close(E, grad, cs, "class surface")
