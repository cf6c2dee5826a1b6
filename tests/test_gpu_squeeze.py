"""E_squeeze on the GPU: gq_squeeze_terms through ops.squeeze_terms and through GraspStepper, against the fp64 oracle
(ref_cpu.export.get_req_joint_velocities on OracleHand / OracleObject with autograd, tests/_squeeze_cases.py) at the project's
bounds for this quantity (tests/test_gpu_alt_energies.py): values rtol 2e-3 / atol 1e-9, theta rtol 2e-3 / atol 2e-5, gradients
norm-wise 1e-3 overall and 2e-3 per part.  Every input keeps clear of the term's two kinks and has contacts on both sides of the
clamp (``_squeeze_cases.assert_populated``).  B <= 8 rows, an icosphere of 80 faces."""
import numpy as np
import pytest
import torch

import _squeeze_cases as sq

pytestmark = pytest.mark.gpu

W_SQ = 1000.0  # E_squeeze is of the order 1e-4: this weight puts it beside the other terms
PRISMATIC = ("panda", "schunk2")


@pytest.fixture(scope="module")
def gq(tmp_path_factory):
    import types

    from graspqp_amd import _C, ops
    from graspqp_amd.stepper import GraspStepper

    assert torch.cuda.is_available()
    sq.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    return types.SimpleNamespace(C=_C, ops=ops, GraspStepper=GraspStepper, hands={})


def _hand(gq, name):
    if name not in gq.hands:
        gq.hands[name] = gq.ops.HandHandle(sq.spec_of(name))
    return gq.hands[name]


def _up(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) + 0.5


def _op(gq, name, hp, idx, up, tau=sq.TAU, lam=sq.LAM):
    ops, hand = gq.ops, _hand(gq, name)
    fv, _ = sq.sphere()
    ms = ops.MeshSet([fv])
    B, n = idx.shape
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, cp, _, _, ws = ops.fk_contacts(hpc, ix, hand)
    d2, sgn, nrm, cls = ops.sdf_meshset(cp.detach().reshape(-1, 3), ms, B * n)
    _, onrm = ops.signed_distance(d2, sgn, nrm)
    q = (d2.reshape(B, n), onrm.reshape(B, n, 3), cls.reshape(B, n, 3))
    e, th = ops.squeeze_terms(hpc, hand, ix, Rg, LT, ws, *q, cp, tau, lam, return_theta=True)
    (e * up.cuda()).sum().backward()
    state = (hand, ix, Rg.detach(), LT.detach(), ws, q, cp.detach())
    return e.detach().cpu().numpy(), th.cpu().numpy(), hpc.grad.cpu().numpy(), state


# 3n > JA (allegro n = 12), 3n = 3 < JA (n = 1: only the damping makes M regular), coupled hands (ability_hand, the dense coupling),
# all-prismatic hands, and the synthetic trees of tests/_synthetic_hand.py: chain64 alternates revolute and prismatic joints in one
# chain (every branch of the kinematic Hessian, JA = 64), comb43 is the deepest tree with branches
OP_CASES = [("allegro", 5), ("allegro", 12), ("allegro", 1), ("shadow_hand", 5), ("ability_hand", 5), ("panda", 3), ("schunk2", 3),
            ("comb43", 5), ("coupled12_dense", 5), ("chain64", 5)]


@pytest.mark.parametrize("name,n", OP_CASES)
def test_op_matches_the_oracle(gq, name, n):
    B = 6
    hp, idx = sq.inputs(name, B, n)
    up = _up(B)
    ref = sq.oracle(name, hp, idx, up)
    tag = f"{name} n={n}"
    sq.assert_populated(ref, sq.TAU, tag, name in PRISMATIC)
    E, th, grad, state = _op(gq, name, hp, idx, up)
    sq.assert_close(E, th, grad, ref, tag, name in PRISMATIC)
    if name in PRISMATIC:  # the contact Jacobian does not depend on prismatic joints: the launch's own joint gradient is exactly 0
        hand, ix, Rg, LT, ws, q, cp = state
        g_theta, g_R, g_cp = gq.ops._Eager.squeeze_terms_backward(hand.hid, ix, Rg, LT, ws, q[0], q[1], q[2], cp, sq.TAU, sq.LAM, up.cuda())
        assert (g_theta == 0).all() and g_R.abs().max() > 0 and g_cp.abs().max() > 0


def test_op_with_other_travel_and_damping(gq):
    B, n, tau, lam = 6, 5, 8e-3, 5e-3
    hp, idx = sq.inputs("allegro", B, n, tau)
    up = _up(B, 5)
    ref = sq.oracle("allegro", hp, idx, up, tau, lam)
    sq.assert_populated(ref, tau, "allegro tau=8e-3 lambda=5e-3")
    ref0 = sq.oracle("allegro", hp, idx, up)
    assert np.abs(ref["E"] - ref0["E"]).max() > 1e-2 * np.abs(ref0["E"]).max()  # the parameters matter on these inputs
    E, th, grad, _ = _op(gq, "allegro", hp, idx, up, tau, lam)
    sq.assert_close(E, th, grad, ref, "allegro tau=8e-3 lambda=5e-3")


def test_out_of_cap_shapes_and_bad_parameters_return_the_error_status(gq):
    C, ops, hand = gq.C, gq.ops, _hand(gq, "allegro")
    hp, idx = sq.inputs("allegro", 6, 5)
    B = 2
    Rg, LT, cp, _, _, ws = ops.fk_contacts(hp[:B].cuda(), idx[:B].cuda(), hand)
    # every call below is refused on the host, before any launch: the buffers are sized for the largest shape named all the same
    ix65 = torch.zeros(B, 65, dtype=torch.long, device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")
    lib = C.lib()

    def status(n, tau, lam, ws_bytes):
        return lib.gq_squeeze_terms(hand.handle, C.i64(ix65), B, n, C.f32(z(B, 65)), C.f32(z(B, 65, 3)), None, None, C.f32(Rg.reshape(B, 9)),
                                    C.f32(LT), C.ptr(ws), ws_bytes, tau, lam, None, 1.0, C.f32(z(B)), None, 0, None, None, None, None,
                                    C.stream_ptr())

    assert status(65, 5e-3, 1e-3, ws.numel()) == 2 and b"64" in lib.gq_last_error()
    assert status(0, 5e-3, 1e-3, ws.numel()) == 2
    assert status(5, 0.0, 1e-3, ws.numel()) == 2 and b"min_travel" in lib.gq_last_error()
    assert status(5, 5e-3, 0.0, ws.numel()) == 2 and b"damping" in lib.gq_last_error()
    assert status(5, 5e-3, float("nan"), ws.numel()) == 2
    assert status(5, 5e-3, 1e-3, 16) == 2 and b"workspace" in lib.gq_last_error()
    with pytest.raises(ValueError, match="64"):
        ops.squeeze_terms(hp[:B].cuda(), hand, ix65, Rg, LT, ws, z(B, 65), z(B, 65, 3), z(B, 65, 3), z(B, 65, 3))
    torch.cuda.synchronize()


# ---- the stepper ---------------------------------------------------------------------------------------------------------------
def _objects(gq, cloud=False):
    from graspqp_amd.utils import meshes

    fv, _ = sq.sphere()
    sp = torch.tensor(meshes.surface_points(fv, 512, oversample=8).astype(np.float32))[None]
    if not cloud:
        return gq.ops.MeshSet([fv]), sp
    pts = meshes.surface_points(fv, 2048, oversample=4).astype(np.float32)
    return gq.ops.PointCloudSet([pts], [pts / np.linalg.norm(pts, axis=1, keepdims=True)]), sp


def _stepper(gq, B, n, weights=None, cloud=False, **kw):
    objs, sp = _objects(gq, cloud)
    return gq.GraspStepper(_hand(gq, "allegro"), objs, sp, B, n, weights=weights, **kw)


def _scene(gq):
    """The half space below z = 0 as an obstacle: phi = z on a coarse grid (the opened hand reaches into it in some rows)."""
    z = -0.3 + 0.05 * torch.arange(13, dtype=torch.float32)
    return gq.ops.SceneSDF(z.view(1, 1, 13).expand(13, 13, 13).contiguous(), (-0.3, -0.3, -0.3), 0.05)


@pytest.mark.parametrize("mode", ["alone", "pregrasp", "prior", "fused"])
def test_evaluate_adds_the_weighted_oracle_term(gq, mode):
    """terms, total and gradient of the stepper with the weight = the stepper without it on the same (pose, idx), plus
    w x the oracle's term and gradient.  With E_pregrasp both launches write g_theta; with E_prior g_R is shared."""
    B, n = 6, 5
    hp, idx = sq.inputs("allegro", B, n)
    base, kw = {}, {}
    if mode == "pregrasp":
        base, kw = {"E_pregrasp": 30.0}, dict(pregrasp_scene=_scene(gq), pregrasp_distance=0.08, pregrasp_stations=2)
    if mode == "prior":
        base = {"E_prior": 7.0, "E_wall": 3.0}
    st0 = _stepper(gq, B, n, weights=base or None, **kw)
    st1 = _stepper(gq, B, n, weights=dict(base, E_squeeze=W_SQ), **kw)
    assert st1.term_names == st0.term_names + ("E_squeeze",)
    ref = sq.oracle("allegro", hp, idx, torch.ones(B))
    sq.assert_populated(ref, sq.TAU, f"stepper {mode}")
    if mode == "fused":  # the fused launches write the buffers the term reads
        for st in (st0, st1):
            st.pose_new.copy_(hp.cuda())
            st.idx_new.copy_(idx.cuda())
            st._evaluate(st.pose_new, st.idx_new, gq.C.stream_ptr(), fused=True)
        t0, tot0, g0 = dict(zip(st0.term_names, st0.terms_new.clone())), st0.total_new.clone(), st0.grad_new.clone()
        t1, tot1, g1 = dict(zip(st1.term_names, st1.terms_new.clone())), st1.total_new.clone(), st1.grad_new.clone()
    else:
        t0, tot0, g0 = st0.evaluate(hp.cuda(), idx.cuda())
        t1, tot1, g1 = st1.evaluate(hp.cuda(), idx.cuda())
    for k in st0.term_names:
        assert torch.equal(t0[k], t1[k]), k
    if mode == "pregrasp":
        assert (t0["E_pregrasp"] > 0).any() and st0.g_theta.abs().max() > 0  # the other writer of g_theta is not idle
    # the total: one fused multiply-add on top of the other terms' total
    np.testing.assert_allclose(tot1.cpu().numpy(), (tot0 + W_SQ * t1["E_squeeze"]).cpu().numpy(), rtol=1e-6)
    sq.assert_close(t1["E_squeeze"].cpu().numpy(), st1.squeeze_theta.cpu().numpy(), ((g1 - g0) / W_SQ).cpu().numpy(), ref,
                    f"stepper {mode}")


def test_evaluate_on_a_point_cloud(gq):
    """The same on a PointCloudSet.  The cloud's surfel distance is not the mesh's, so the oracle takes the query of the stepper's
    own buffers: the normals as constants, and the travel as sqrt(|p - closest|^2 + 1e-8) of the oracle hand's contact points with
    the closest points held (d dist_sq / dp = 2 (p - closest), the derivative every object query of the project has)."""
    from ref_cpu import export as oexp
    from ref_cpu import models as omodels

    B, n = 6, 5
    hp, idx = sq.inputs("allegro", B, n)
    st0, st1 = _stepper(gq, B, n, cloud=True), _stepper(gq, B, n, weights={"E_squeeze": W_SQ}, cloud=True)
    t0, tot0, g0 = st0.evaluate(hp.cuda(), idx.cuda())
    t1, tot1, g1 = st1.evaluate(hp.cuda(), idx.cuda())
    for k in st0.term_names:
        assert torch.equal(t0[k], t1[k]), k
    oh = omodels.OracleHand(sq.spec_of("allegro"), torch.float64)
    hp64 = hp.double().requires_grad_()
    oh.set_parameters(hp64, idx)
    closest, nrm = st1.closest.cpu().double(), st1.obj_normal.cpu().double()
    dist = torch.sqrt(((oh.contact_points - closest) ** 2).sum(-1) + 1e-8)
    np.testing.assert_allclose(dist.detach().numpy() ** 2 - 1e-8, st1.d2.cpu().numpy(), rtol=1e-3, atol=1e-9)  # the same query
    th, res = oexp.get_req_joint_velocities(oh, nrm * dist.unsqueeze(-1).clamp(min=sq.TAU), idx)
    E = res.mean(-1)
    (g,) = torch.autograd.grad(E.sum(), hp64)
    ref = dict(E=E.detach().numpy(), theta=th.detach().numpy(), grad=g.numpy(), dist=dist.detach())
    sq.assert_populated(ref, sq.TAU, "stepper cloud")
    np.testing.assert_allclose(tot1.cpu().numpy(), (tot0 + W_SQ * t1["E_squeeze"]).cpu().numpy(), rtol=1e-6)
    sq.assert_close(t1["E_squeeze"].cpu().numpy(), st1.squeeze_theta.cpu().numpy(), ((g1 - g0) / W_SQ).cpu().numpy(), ref, "stepper cloud")


def _draws(st, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B, n = st.B, st.n
    return (torch.rand(B, n, device="cuda", generator=g),
            torch.randint(st.hand.spec.n_contact_candidates, (B, n), device="cuda", generator=g), torch.rand(B, device="cuda", generator=g))


def _state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st.hand_pose, st.contact_idx, st.grad, st.energy, st.ema, st.step_count, st.terms)]


def _five_steps(st, hp, idx, reset_at=2):
    st.reset(hp.cuda(), idx.cuda())
    for s in range(5):
        if s == reset_at:
            mask = torch.zeros(st.B, dtype=torch.bool)
            mask[[1, st.B - 2]] = True
            st.step_reset(mask.cuda(), hp.cuda().roll(1, 0), idx.cuda().roll(1, 0), draws=_draws(st, 100 + s))
        else:
            st.step(draws=_draws(st, 100 + s))
    return _state(st)


def test_weight_zero_or_absent_changes_nothing(gq):
    B, n = 8, 4
    hp, idx = sq.inputs("allegro", B, n)
    want = _five_steps(_stepper(gq, B, n), hp, idx)
    for kw in (dict(weights={"E_squeeze": 0.0}), dict(weights={"E_squeeze": 0.0}, squeeze_min_travel=1e-2, squeeze_damping=1e-2)):
        st = _stepper(gq, B, n, **kw)
        assert st.term_names == ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints") and st.squeeze_theta is None and st._fuse_loop
        got = _five_steps(st, hp, idx)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("fork", [False, True])
def test_captured_graph_replays_equal_eager_steps(gq, fork):
    B, n = 8, 4
    hp, idx = sq.inputs("allegro", B, n)
    out = []
    for captured in (False, True):
        st = _stepper(gq, B, n, weights={"E_squeeze": W_SQ})
        st.reset(hp.cuda(), idx.cuda())
        if captured:
            st.capture(fork=fork, fused=not fork)
        for s in range(5):
            st.step(draws=_draws(st, 200 + s))
        out.append(_state(st) + [st.squeeze_theta.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert (out[0][5] == 5).all() and torch.isfinite(out[0][3]).all() and (out[0][6][-1] > 0).all()


def test_two_runs_from_one_seed_are_bit_identical(gq):
    B, n = 8, 4
    hp, idx = sq.inputs("allegro", B, n)
    out = []
    for _ in range(2):
        st = _stepper(gq, B, n, weights={"E_squeeze": W_SQ}, seed=11)
        st.reset(hp.cuda(), idx.cuda())
        for _ in range(5):
            st.step()
        out.append(_state(st) + [st.squeeze_theta.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_select_gates_on_the_term(gq):
    B, n = 8, 4
    hp, idx = sq.inputs("allegro", B, n)
    st = _stepper(gq, B, n, weights={"E_squeeze": W_SQ})
    st.reset(hp.cuda(), idx.cuda())
    e = st.terms[st.term_names.index("E_squeeze")].cpu()
    tol = float(e.sort().values[B // 2 - 1])  # half of the rows pass
    sel = st.select(B, radius=0.0, gates={"E_squeeze": tol})
    rows = sel.sel[0][: int(sel.n_selected[0])].cpu().tolist()
    assert sorted(rows) == sorted(torch.nonzero(e <= tol).flatten().tolist()) and 0 < len(rows) < B
    assert sel.feasible.cpu().tolist() == (e <= tol).int().tolist()
    assert int(st.select(B, radius=0.0).n_selected[0]) == B  # not gated by default
    with pytest.raises(ValueError, match="E_squeeze"):
        _stepper(gq, B, n).select(B, gates={"E_squeeze": tol})  # a gate on the switched-off term


def test_class_surface_term_is_the_op(gq):
    """calculate_energy(..., energy_names=[..., "E_squeeze"]) against the oracle, beside E_manipulativity's composed route."""
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    B, n = 6, 5
    hp, idx = sq.inputs("allegro", B, n)
    up = _up(B, 9)
    ref = sq.oracle("allegro", hp, idx, up)
    fv, sp = sq.sphere()
    hm = HandModel(sq.spec_of("allegro"), "cuda")
    om = ObjectModel(batch_size_each=B, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv], surface_points_list=[sp])
    hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    names = ["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_squeeze", "E_manipulativity"]
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=names, svd_gain=0.1)
    (g,) = torch.autograd.grad((losses["E_squeeze"] * up.cuda()).sum(), hm.hand_pose, retain_graph=True)
    sq.assert_close(losses["E_squeeze"].detach().cpu().numpy(), None, g.cpu().numpy(), ref, "class surface")
    np.testing.assert_allclose(losses["E_squeeze"].detach().cpu().numpy(), losses["E_manipulativity"].detach().cpu().numpy(), rtol=4e-3,
                               atol=2e-9)  # two routes, each within 2e-3 of the oracle
    hm.set_squeeze(8e-3, 5e-3)
    e2 = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_squeeze"], svd_gain=0.1)["E_squeeze"]
    np.testing.assert_allclose(e2.detach().cpu().numpy(), sq.oracle("allegro", hp, idx, up, 8e-3, 5e-3)["E"], rtol=2e-3, atol=1e-9)
