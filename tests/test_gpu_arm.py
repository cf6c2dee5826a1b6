"""E_arm on the GPU: gq_arm_terms through ops.arm_terms, GraspStepper and calculate_energy against the fp64 oracle of
tests/_arm_oracle.py.  reach_q is fed from the reach oracle, float32-exact.  Bounds: per row |E - E_64| <= 1e-5 m; per row with a
non-zero gradient the hand_pose gradient norm-wise within 1e-3 |g_64|.  They rest on the oracle's own float32 noise (float32
kinematics, points, field and columns, fp64 solve; tests/test_arm_oracle.py prints it): at most 1.3e-6 m and 1.1e-4 over all five
pools on the affine and the random field, under a quarter of the bounds.  The rows of a case meet the guards on the inputs
(|margin + r - phi| >= 2e-5 per sphere; on the random field every coordinate >= 1e-4 cells from a face).
B = 8 rows, 2 objects x 4 rows with a base each; grids of 24 x 24 x 20 nodes at 0.1 m."""
import ctypes

import numpy as np
import pytest
import torch

import _arm_oracle as ao
import _reach_oracle as ro
import _scene_oracle as so

pytestmark = pytest.mark.gpu

W_REACH, W_ARM = 1e4, 100.0  # E_arm is of the order 0.1 m: this weight puts it beside the other terms
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


def _arm(gq, arm):
    if id(arm) not in gq.arms:
        gq.arms[id(arm)] = (gq.ops.ArmHandle(arm), arm)  # the spec is kept: its id stays taken
    return gq.arms[id(arm)][0]


def _pose(gq, pose9):
    spec = gq.spec
    mid = 0.5 * (np.asarray(spec.joints_lower, np.float32) + np.asarray(spec.joints_upper, np.float32))
    hp = torch.cat([torch.from_numpy(np.asarray(pose9, np.float32)), torch.from_numpy(mid)[None].expand(B, -1)], 1).contiguous()
    idx = torch.randint(spec.n_contact_candidates, (B, N_CONTACT), generator=torch.Generator().manual_seed(4))
    return hp, idx


def _scene(gq, fields):
    if len(fields) == 1:
        return fields[0].scene(gq)
    f = fields[0]
    return gq.ops.SceneSDFSet(torch.stack([x.values for x in fields]).cuda(), [float(o) for o in f.origin], float(f.voxel))


def _op(gq, cs, fields=None, up=None, lam=ao.LAM_A):
    ops = gq.ops
    hp, idx = _pose(gq, cs["pose9"])
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    base = torch.from_numpy(cs["base_T"]).cuda()
    q = torch.from_numpy(cs["q"].astype(np.float32)).cuda()
    e = ops.arm_terms(hpc, gq.hand, ix, Rg, LT, ws, _arm(gq, cs["arm"]), base, BE, _scene(gq, fields or [cs["field"]]), cs["axis"], q,
                      cs["distance"], cs["stations"], ao.MARGIN, lam, ro.RHO)
    (e * torch.as_tensor(cs["up"] if up is None else up, dtype=torch.float32).cuda()).sum().backward()
    return e.detach().cpu().numpy(), hpc.grad.cpu().numpy()


@pytest.mark.parametrize("kind,spheres", [("affine", "link"), ("multilinear", "one"), ("random", "link"), ("random", "full")])
@pytest.mark.parametrize("stations", [0, 2])
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_op_matches_the_oracle(gq, name, stations, kind, spheres):
    cs = ao.case(name, stations, kind, spheres)
    tag = f"{name} K={stations} {kind} Ns={cs['arm'].n_spheres}"
    assert ao.guards(cs["res"], cs["arm"], ao.MARGIN, kind == "random")[0]
    if (kind, spheres) == ("affine", "link"):
        ao.assert_coverage(cs["res"], cs["arm"], tag)
    E, grad = _op(gq, cs)
    assert (grad[:, 9:] == 0).all()  # the hand's joints get no gradient from the arm
    ao.assert_close(E, grad, cs, tag)


def test_rows_pick_their_own_grid(gq):
    """A stack of two grids: row b reads grid b // 4; swapping the grids changes the result, and both orders match the oracle."""
    cs = ao.case("elbow6", 2, "affine")
    fa, fb = cs["field"], ao.field("random")
    out = []
    for fields in ([fa, fb], [fb, fa]):
        res = ao.arm_terms(cs["arm"], cs["q"], cs["pose9"], cs["base_T"], BE, fields, distance=cs["distance"], up=cs["up"])
        ok = ao.guard_rows(res, cs["arm"], ao.MARGIN, True)[0]
        E, grad = _op(gq, cs, fields)
        gn = np.linalg.norm(res["grad"], axis=-1)
        nz = ok & (gn > 0)
        rel = np.linalg.norm(grad[:, :9] - res["grad"], axis=-1)[nz] / gn[nz]
        print(f"[stack] rows compared {int(ok.sum())}; worst |dE| {np.abs(E - res['E'])[ok].max():.2e}; worst gradient rel err {rel.max():.2e}")
        assert ok.sum() >= 6 and (np.abs(E - res["E"])[ok] <= 1e-5).all() and (rel <= 1e-3).all()
        out.append(E)
    assert np.abs(out[0] - out[1]).max() > 1e-3
    # the single grid is the stack of one: the rows of object 0 are bitwise those of the stack whose grid 0 it is
    E1, g1 = _op(gq, cs, [fa])
    assert np.array_equal(E1[:BE], out[0][:BE])


def test_energy_is_the_sum_of_the_clutter_query_at_the_sphere_points(gq):
    """An arm whose kinematics are exact in float32 (prismatic joints, a revolute one at q = 0, dyadic numbers): the sphere points are
    known exactly, gq_clutter_query gives phi there, and e_arm is bit for bit the hinge sum in the documented order (spheres ascending,
    then stations ascending, then one multiplication by 1.0f / (K + 1))."""
    ops = gq.ops
    T = lambda x, y, z: ro.T((x, y, z))
    K = 2
    arm = ops.ArmSpec(["prismatic", "prismatic", "revolute", "prismatic"], np.stack([T(0.25, 0, 0.125), T(0, 0.5, 0), T(0.125, 0, 0.25), T(0, 0, 0.375)]),
                      [ro.X, ro.Y, ro.Z, ro.Z], [-1.0, -1.0, -1.0, -1.0], [1.0, 1.0, 1.0, 1.0])
    rng = np.random.default_rng(5)
    Ns = 37
    link = np.sort(rng.integers(0, 4, Ns))
    centre = rng.integers(-8, 9, (Ns, 3)) / 32.0
    radius = rng.integers(1, 5, Ns) / 64.0
    arm = arm.with_spheres(link, centre, radius)
    q = rng.integers(-16, 17, (B, K + 1, 4)) / 32.0
    q[:, :, 2] = 0.0
    base_T = np.stack([T(-0.5, 0.25, -0.125)[:3], T(0.125, -0.5, 0.0)[:3]]).astype(np.float32)
    fields = [ao.field("random", seed=1), ao.field("random", seed=2)]
    margin = np.float32(1.0 / 64.0)
    # the points, exactly: every joint frame is a pure translation
    x = np.zeros((B, K + 1, Ns, 3))
    for b in range(B):
        for k in range(K + 1):
            o, org = base_T[b // BE][:, 3].astype(np.float64), []
            for j in range(4):
                o = o + arm.joint_T[j][:, 3] + (q[b, k, j] * arm.joint_axis[j] if arm.joint_type[j] == 2 else 0.0)
                org.append(o)
            x[b, k] = np.array(org)[link] + centre
    x32 = x.astype(np.float32)
    assert (x32.astype(np.float64) == x).all()
    scene = _scene(gq, fields)
    flat = torch.from_numpy(x32.reshape(-1, 3)).cuda()
    phi, grad, inside = torch.empty(flat.shape[0], device="cuda"), torch.empty(flat.shape[0], 3, device="cuda"), \
        torch.empty(flat.shape[0], dtype=torch.uint8, device="cuda")
    ops._scene_query_call(scene.grid_set, flat, phi, grad, inside)
    phi, inside = phi.cpu().numpy().reshape(B, K + 1, Ns), inside.cpu().numpy().reshape(B, K + 1, Ns).astype(bool)
    assert inside.any() and (~inside).any()
    want = np.zeros(B, np.float32)
    for b in range(B):
        tot = np.float32(0.0)
        for k in range(K + 1):
            ek = np.float32(0.0)
            for s in range(Ns):
                h = (margin + np.float32(radius[s])) - phi[b, k, s] if inside[b, k, s] else np.float32(0.0)
                ek = np.float32(ek + (h if h > 0 else np.float32(0.0)))
            tot = np.float32(tot + ek)
        want[b] = tot * (np.float32(1.0) / np.float32(K + 1))
    cs = dict(arm=arm, pose9=np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32), (B, 1)), base_T=base_T, q=q, axis=ro.AXIS,
              distance=0.1, stations=K, up=np.ones(B))
    hp, idx = _pose(gq, cs["pose9"])
    hpc, ix = hp.cuda(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    e = ops.arm_terms(hpc, gq.hand, ix, Rg, LT, ws, _arm(gq, arm), torch.from_numpy(base_T).cuda(), BE, scene, ro.AXIS,
                      torch.from_numpy(q.astype(np.float32)).cuda(), 0.1, K, float(margin), ao.LAM_A, ro.RHO)
    got = e.cpu().numpy()
    print(f"[exact] e_arm {got}; hinge sum of the query {want}")
    assert (want > 0).sum() >= 4 and np.array_equal(got, want)


def test_bad_parameters_return_the_error_status(gq):
    C = gq.C
    cs = ao.case("short3", 0, "affine")
    arm = _arm(gq, cs["arm"])
    hp, _ = _pose(gq, cs["pose9"])
    z = lambda *s: torch.zeros(*s, device="cuda")
    lib = C.lib()
    axis = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    hpc, Rg, base, e, q = hp.cuda(), z(B, 9), torch.from_numpy(cs["base_T"]).cuda(), z(B), z(B, 4, 3)
    scene = cs["field"].scene(gq)
    grids = gq.ops._arm_scene_grids(scene)

    def status(batch=B, rpg=B, n_obj=2, be=BE, D=0.1, K=0, lam=1e-6, rho=0.1, margin=0.01, ns=None, rq=True, ax=axis):
        return lib.gq_arm_terms(arm.handle, ctypes.byref(grids), rpg, margin, lam, rho, C.i32(arm.sphere_link), C.f32(arm.sphere_centre),
                                C.f32(arm.sphere_radius), arm.Ns if ns is None else ns, C.f32(hpc), hpc.shape[1], C.f32(Rg), batch,
                                C.f32(base), n_obj, be, ax, D, K, C.f32(q) if rq else None, None, 1.0, C.f32(e), 0, None, C.stream_ptr())

    assert status() == 0
    for kw, word in ((dict(K=4), b"n_stations"), (dict(K=2, D=0.0), b"distance"), (dict(lam=0.0), b"damping"),
                     (dict(rho=float("nan")), b"rot_scale"), (dict(margin=-0.1), b"margin"), (dict(ns=0), b"n_spheres"),
                     (dict(ns=65), b"n_spheres"), (dict(n_obj=3), b"base_T"), (dict(rpg=4), b"grids"), (dict(rq=False), b"reach_q"),
                     (dict(ax=(ctypes.c_float * 3)(0.0, 0.0, 0.0)), b"grasp_axis")):
        assert status(**kw) == 2, kw
        msg = lib.gq_last_error()
        assert b"arm" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()


# ---- the stepper ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, weights=None, **kw):
    from graspqp_amd.utils import meshes

    fv = meshes.icosphere(1, 0.05).astype(np.float32)  # 80 faces
    sp = torch.tensor(np.stack([meshes.surface_points(fv, 256, oversample=8).astype(np.float32)] * 2))
    return gq.GraspStepper(gq.hand, gq.ops.MeshSet([fv, fv]), sp, BE, N_CONTACT, weights=weights, **kw)


def _case(gq, name="arm7", stations=2, kind="affine"):
    """The rows of a case with the HAND's grasp axis (the stepper and calculate_energy take it from the spec); the reach launch of the
    stepper finds its own reach_q, which at station 0 is the oracle's up to the float32 iteration"""
    return dict(ao.case(name, stations, kind), axis=tuple(float(a) for a in gq.spec.grasp_axis))


def _kw(gq, cs, scene=None):
    return dict(arm=_arm(gq, cs["arm"]), arm_base=cs["base_T"], reach_distance=cs["distance"], reach_stations=cs["stations"],
                arm_scene=cs["field"].scene(gq) if scene is None else scene, arm_margin=ao.MARGIN)


def _small_scene(gq):
    z = -0.3 + 0.05 * torch.arange(13, dtype=torch.float32)
    return gq.ops.SceneSDF(z.view(1, 1, 13).expand(13, 13, 13).contiguous(), (-0.3, -0.3, -0.3), 0.05)


@pytest.mark.parametrize("mode", ["alone", "together"])
def test_evaluate_adds_the_weighted_oracle_term(gq, mode):
    """terms, total and gradient of the stepper with the weight = the reach-only stepper on the same (pose, idx), plus w x the oracle's
    term and gradient at the reach_q the stepper holds; g_theta and g_R are bitwise those of the run without the term."""
    cs = _case(gq)
    hp, idx = _pose(gq, cs["pose9"])
    base, kw = {"E_reach": W_REACH}, {}
    if mode == "together":
        base = {"E_reach": W_REACH, "E_pregrasp": 30.0, "E_squeeze": 1000.0, "E_prior": 7.0}
        kw = dict(pregrasp_scene=_small_scene(gq), pregrasp_distance=0.08, pregrasp_stations=2)
    st0 = _stepper(gq, weights=base, **kw, **{k: v for k, v in _kw(gq, cs).items() if not k.startswith("arm_s") and k != "arm_margin"})
    st1 = _stepper(gq, weights=dict(base, E_arm=W_ARM), **kw, **_kw(gq, cs))
    assert st1.term_names == st0.term_names + ("E_arm",) and st0.term_names[-1] == "E_reach" and not st1._fuse_loop
    t0, tot0, g0 = st0.evaluate(hp.cuda(), idx.cuda())
    t1, tot1, g1 = st1.evaluate(hp.cuda(), idx.cuda())
    for k in st0.term_names:
        assert torch.equal(t0[k], t1[k]), k
    assert torch.equal(st0.reach_q, st1.reach_q)
    if mode == "together":
        assert torch.equal(st0.g_theta, st1.g_theta) and torch.equal(st0.g_R, st1.g_R) and st0.g_theta.abs().max() > 0
    np.testing.assert_allclose(tot1.cpu().numpy(), (tot0 + W_ARM * t1["E_arm"]).cpu().numpy(), rtol=1e-6)
    q = st1.reach_q.cpu().numpy().astype(np.float64)
    res = ao.arm_terms(cs["arm"], q, hp[:, :9].numpy(), cs["base_T"], BE, [cs["field"]], axis=cs["axis"], distance=cs["distance"])
    ok = ao.guard_rows(res, cs["arm"], ao.MARGIN)[0]
    E, dg = t1["E_arm"].cpu().numpy(), ((g1 - g0) / W_ARM).cpu().numpy()[:, :9]
    gn = np.linalg.norm(res["grad"], axis=-1)
    nz = ok & (gn > 0)
    # the difference of two float32 gradients of the whole energy: its rounding is relative to |g1|, not to the term's share
    noise = 4 * np.finfo(np.float32).eps * np.linalg.norm(g1.cpu().numpy()[:, :9], axis=-1) / W_ARM
    err = np.linalg.norm(dg - res["grad"], axis=-1)
    print(f"[stepper {mode}] rows {int(ok.sum())}, with a gradient {int(nz.sum())}; worst |dE| {np.abs(E - res['E'])[ok].max():.2e}; worst gradient "
          f"err / (1e-3 |g| + noise) {np.max(err[nz] / (1e-3 * gn[nz] + noise[nz])):.2e}")
    assert ok.sum() >= 6 and nz.sum() >= 2 and (res["E"][ok] > 0).any()
    assert (np.abs(E - res["E"])[ok] <= 1e-5).all()
    assert (err[nz] <= 1e-3 * gn[nz] + noise[nz]).all()


def test_stepper_fall_backs_and_what_follows_the_scene_check(gq):
    """arm_scene=None takes ``scene`` and arm_margin=None takes ``scene_margin``; after the scene argument come n_grids and
    ops.arm_check (the checks before it need no grid: tests/test_arm_surface.py)."""
    cs = _case(gq, "elbow6")
    kw = {k: v for k, v in _kw(gq, cs).items() if not k.startswith("arm_s") and k != "arm_margin"}
    w = {"E_reach": W_REACH, "E_arm": W_ARM}
    scene, other = cs["field"].scene(gq), _small_scene(gq)
    st = _stepper(gq, weights=w, scene=scene, arm_scene=None, scene_margin=0.03, arm_margin=0.01, **kw)
    assert st.arm_scene is scene and st.arm_margin == 0.01 and st.scene is None  # ``scene`` itself belongs to E_scene / E_approach
    st = _stepper(gq, weights=w, scene=scene, arm_scene=other, scene_margin=0.03, arm_margin=None, **kw)
    assert st.arm_scene is other and st.arm_margin == 0.03
    three = gq.ops.SceneSDFSet(torch.stack([cs["field"].values] * 3).cuda(), [float(o) for o in cs["field"].origin], float(cs["field"].voxel))
    with pytest.raises(ValueError, match="arm_scene has n_grids = 3, the stepper has n_obj = 2 objects"):
        _stepper(gq, weights=w, arm_scene=three, arm_margin=-1.0, **kw)  # the margin is wrong too: n_grids comes first
    with pytest.raises(ValueError, match="margin"):
        _stepper(gq, weights=w, arm_scene=scene, arm_margin=-1.0, **kw)


def _draws(st, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(st.B, st.n, device="cuda", generator=g),
            torch.randint(st.hand.spec.n_contact_candidates, (st.B, st.n), device="cuda", generator=g),
            torch.rand(st.B, device="cuda", generator=g))


def _state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st.hand_pose, st.contact_idx, st.grad, st.energy, st.ema, st.step_count, st.terms)]


def _five(st, hp, idx, seed=100):
    st.reset(hp.cuda(), idx.cuda())
    for s in range(5):
        st.step(draws=_draws(st, seed + s))
    return _state(st)


def test_weight_zero_or_absent_changes_nothing(gq):
    cs = _case(gq, "elbow6")
    hp, idx = _pose(gq, cs["pose9"])
    kw = _kw(gq, cs)
    reach_only = {k: v for k, v in kw.items() if not k.startswith("arm_s") and k != "arm_margin"}
    want = _five(_stepper(gq, weights={"E_reach": W_REACH}, **reach_only), hp, idx)
    for k2 in (dict(weights={"E_reach": W_REACH, "E_arm": 0.0}, **kw), dict(weights={"E_reach": W_REACH, "E_arm": 0.0}, **reach_only)):
        st = _stepper(gq, **k2)
        assert st.term_names[-1] == "E_reach" and not st.arm_mode and st.arm_scene is None
        assert all(torch.equal(a, b) for a, b in zip(_five(st, hp, idx), want))


def test_captured_graph_replays_equal_eager_steps_and_runs_repeat(gq):
    cs = _case(gq, "elbow6")
    hp, idx = _pose(gq, cs["pose9"])
    out = []
    for captured in (False, True, False):
        st = _stepper(gq, weights={"E_reach": W_REACH, "E_arm": W_ARM}, **_kw(gq, cs))
        st.reset(hp.cuda(), idx.cuda())
        if captured:
            st.capture()
        for s in range(5):
            st.step(draws=_draws(st, 200 + s))
        out.append(_state(st) + [st.reach_q.clone()])
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))  # a captured graph replays bit for bit against eager
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[2]))  # two runs are bitwise equal
    assert (out[0][5] == 5).all() and torch.isfinite(out[0][3]).all()


def test_select_gates_the_term_by_default(gq):
    cs = _case(gq, "elbow6", 0)
    hp, idx = _pose(gq, cs["pose9"])
    st = _stepper(gq, weights={"E_reach": W_REACH, "E_arm": W_ARM}, **_kw(gq, cs))
    st.reset(hp.cuda(), idx.cuda())
    e = st.terms[st.term_names.index("E_arm")].cpu()
    keep = e <= 0.0
    assert 0 < int(keep.sum()) < B
    sel = st.select(BE, radius=0.0)  # gates = None: E_arm <= 0 as the other obstacle terms, E_reach not gated
    assert sel.feasible.cpu().tolist() == keep.int().tolist()
    assert int(st.select(BE, radius=0.0, gates={}).n_selected.sum()) == B
    reach_only = {k: v for k, v in _kw(gq, cs).items() if not k.startswith("arm_s") and k != "arm_margin"}
    with pytest.raises(ValueError, match="E_arm"):
        _stepper(gq, weights={"E_reach": W_REACH}, **reach_only).select(BE, gates={"E_arm": 0.0})  # a gate on the switched-off term


def test_class_surface_term_is_the_op(gq):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF
    from graspqp_amd.utils import meshes

    ops = gq.ops
    cs = _case(gq, "gantry6", 2)
    hp, idx = _pose(gq, cs["pose9"])
    fv = meshes.icosphere(1, 0.05).astype(np.float32)
    sp = meshes.surface_points(fv, 64, oversample=8).astype(np.float32)
    hm = HandModel(gq.spec, "cuda")
    om = ObjectModel(batch_size_each=BE, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv, fv], surface_points_list=[sp, sp])
    hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
    hm.set_reach(cs["arm"], cs["base_T"], cs["distance"], cs["stations"])
    scene = cs["field"].scene(gq)
    hm.set_arm_scene(scene, ao.MARGIN)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_reach", "E_arm"],
                              svd_gain=0.1)
    up = torch.as_tensor(cs["up"], dtype=torch.float32).cuda()
    (g,) = torch.autograd.grad((losses["E_arm"] * up).sum(), hm.hand_pose)
    # the op, fed with the reach op's own reach_q
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    arm, base = hm.reach[0], torch.from_numpy(cs["base_T"]).cuda()
    _, q, _ = ops.reach_terms(hpc.detach(), gq.hand, ix, Rg, LT, ws, arm, base, BE, cs["axis"], cs["distance"], cs["stations"], return_q=True)
    e = ops.arm_terms(hpc, gq.hand, ix, Rg, LT, ws, arm, base, BE, scene, cs["axis"], q, cs["distance"], cs["stations"], ao.MARGIN)
    (e * up).sum().backward()
    assert torch.equal(losses["E_arm"].detach(), e.detach()) and torch.equal(g, hpc.grad)
    assert float(e.detach().max()) > 0 and float(hpc.grad.abs().max()) > 0
