"""E_track on the GPU: gq_track_terms through ops.track_terms, GraspStepper and calculate_energy against the fp64 oracle of
tests/_track_oracle.py, on the STABLE rows of its seeded cases (the oracle's own E and path do not move under a 1e-6 change of
q_start): per row |E - E_64| <= 2e-3 E_64 + 1e-10, the hand_pose gradient norm-wise 1e-3 overall and 2e-3 on the translation part
and on the rotation part (the reach term's bounds), track_q within 1e-3 and track_step within 2e-3 of the oracle's, track_q inside
the limits, and its FK in fp64 reproduces the kernel's mean and worst waypoint energy within the E bound.  Every compared set holds
a row with a clamped joint, one with E > 1e-3 and one with E < 1e-10 (``_track_oracle.compared_set``).  Eight-row cases, 2 objects x
4 rows with a base each, and the shapes where the lane mapping can go wrong.  The printed "share of the bound" lines are kept in
profiles/track_gpu_test_errors.txt."""
import ctypes

import numpy as np
import pytest
import torch

import _reach_oracle as ro
import _track_oracle as to

pytestmark = pytest.mark.gpu

W_REACH, W_TRACK, W_ARM = 1e4, 1e4, 100.0
BE, N_CONTACT = 4, 4


@pytest.fixture(scope="module")
def gq():
    import types

    from graspqp_amd import _C, ops
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.stepper import GraspStepper

    assert torch.cuda.is_available()
    spec = get_hand_spec("allegro")
    return types.SimpleNamespace(C=_C, ops=ops, GraspStepper=GraspStepper, spec=spec, hand=ops.HandHandle(spec), arms={})


def _arm(gq, spec, name):
    key = (name, spec.n_seeds, spec.n_spheres)
    if key not in gq.arms:
        gq.arms[key] = gq.ops.ArmHandle(spec)
    return gq.arms[key]


def _pose(gq, pose9):
    """(B, 9 + J) float32: the root poses with the hand's joints at mid-range, and seeded contact indices."""
    spec, B = gq.spec, len(pose9)
    mid = 0.5 * (np.asarray(spec.joints_lower, np.float32) + np.asarray(spec.joints_upper, np.float32))
    hp = torch.cat([torch.from_numpy(np.ascontiguousarray(pose9)), torch.from_numpy(mid)[None].expand(B, -1)], 1).contiguous()
    idx = torch.randint(spec.n_contact_candidates, (B, N_CONTACT), generator=torch.Generator().manual_seed(4))
    return hp, idx


def _op(gq, cs, rows=None, stations=0, q_start=None, up=None):
    """ops.track_terms on the rows ``rows`` of a case (None: all; the rows of ONE object when given) -> numpy E, q, worst, step,
    station_q, grad."""
    ops = gq.ops
    sel = np.arange(len(cs["pose9"])) if rows is None else np.asarray(rows)
    be = cs["batch_each"] if rows is None else len(sel)
    base = cs["base_T"] if rows is None else cs["base_T"][sel[0] // cs["batch_each"]][None]
    hp, idx = _pose(gq, cs["pose9"][sel])
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    qs = torch.from_numpy(cs["q_start"][sel]).cuda() if q_start is None else q_start
    e, q, worst, step, sq = ops.track_terms(hpc, gq.hand, ix, Rg, LT, ws, _arm(gq, cs["arm"], cs["name"]), torch.from_numpy(base).cuda(), be,
                                            cs["axis"], qs, cs["distance"], cs["T"], cs["U"], stations=stations, return_path=True)
    (e * torch.as_tensor(cs["up"][sel] if up is None else up, dtype=torch.float32).cuda()).sum().backward()
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    return n(e), n(q), n(worst), n(step), n(sq), hpc.grad.cpu().numpy()


def _check_path(cs, E, q, worst, tag):
    """track_q inside the float32 limits; its FK in fp64 reproduces the kernel's mean and worst waypoint energy within the E bound"""
    arm, T, B = cs["arm"], cs["T"], len(E)
    assert (q >= arm.lower.astype(np.float32)).all() and (q <= arm.upper.astype(np.float32)).all()
    base = ro._T44(cs["base_T"])[torch.arange(B) // cs["batch_each"]]
    pose = torch.as_tensor(cs["pose9"], dtype=ro.F64)
    R = ro.gramschmidt(pose[:, 3:9])
    a = torch.as_tensor(cs["axis"], dtype=ro.F64)
    Ei = np.zeros((B, T + 1))
    for i in range(T + 1):
        Tee, _, _ = ro.fk(arm, torch.as_tensor(q[:, i], dtype=ro.F64), base)
        e = ro.error(Tee, pose[:, :3] - cs["distance"] * (T - i) / T * (R @ a), R, ro.RHO)
        Ei[:, i] = (e * e).sum(-1).numpy()
    r1, r2 = np.abs(Ei.mean(-1) - E) / to.e_bound(E), np.abs(Ei.max(-1) - worst) / to.e_bound(worst)
    print(f"[{tag}] FK of track_q, share of the bound: mean {r1.max():.2e}, worst waypoint {r2.max():.2e}")
    assert r1.max() <= 1.0 and r2.max() <= 1.0


@pytest.mark.parametrize("T,U", to.SHAPES)
@pytest.mark.parametrize("n_seeds", to.SEEDS)
@pytest.mark.parametrize("name", ro.ARM_NAMES)
def test_op_matches_the_oracle(gq, name, n_seeds, T, U):
    cs = to.case(name, n_seeds, T, U)
    tag = f"{name} S={n_seeds} T={T} U={U}"
    E, q, worst, step, _, grad = _op(gq, cs)
    assert (grad[:, 9:] == 0).all()  # the hand's joints get no gradient from the arm
    to.assert_close(E, grad, q, step, cs, tag)
    _check_path(cs, E, q, worst, tag)


@pytest.mark.parametrize("name,n_seeds,B,be,T,U", [("short3", 1, 1, 1, 1, 1), ("chain8", 4, 13, 13, 64, 1), ("arm7", 4, 12, 3, 8, 3),
                                                   ("chain8", 1, 8, 4, 4, 2), ("short3", 4, 13, 13, 8, 3)])
def test_lane_mapping_shapes_and_rows_alone(gq, name, n_seeds, B, be, T, U):
    """B = 1, 8 and 13 (idle groups in the last wavefront), batch_each = 3 with alternating bases, N = 3 and N = 8, T = 1 with U = 1
    and T = 64 with U = 1: against the oracle, and every row of the batch is bitwise the same row evaluated alone."""
    cs = to.rows_case(name, n_seeds, B, be, T, U)
    tag = f"shape {name} B={B} be={be} T={T} U={U}"
    out = _op(gq, cs, stations=1)
    to.assert_close(out[0], out[5], out[1], out[3], cs, tag, kinds=False)
    _check_path(cs, out[0], out[1], out[2], tag)
    for b in range(B):
        alone = _op(gq, cs, rows=[b], stations=1)
        for x, y in zip(out, alone):
            assert np.array_equal(x[b:b + 1], y), (tag, b)


@pytest.mark.parametrize("K", [1, 2])
def test_station_q_is_the_waypoints_bits(gq, K):
    cs = to.case("arm7", 4, 8, 3)
    T = cs["T"]
    _, q, _, _, sq, _ = _op(gq, cs, stations=K)
    assert sq.shape == (8, K + 1, 7)
    for k in range(K + 1):
        assert np.array_equal(sq[:, k], q[:, T * (K - k) // K])
    assert np.array_equal(sq[:, 0], q[:, T]) and np.array_equal(sq[:, K], q[:, 0])  # station 0 is the grasp pose


def test_strided_q_start_view_equals_a_contiguous_copy(gq):
    cs = to.case("elbow6", 4, 4, 2)
    reach_q = torch.zeros(8, 3, 6).cuda()
    reach_q[:, 2] = torch.from_numpy(cs["q_start"]).cuda()
    reach_q[:, :2] = 7.0  # what a wrong stride would read
    view = reach_q[:, 2]
    assert not view.is_contiguous()
    a, b = _op(gq, cs, q_start=view), _op(gq, cs, q_start=view.contiguous())
    for x, y in zip(a, b):
        assert x is None or np.array_equal(x, y)
    to.assert_close(a[0], a[5], a[1], a[3], cs, "strided q_start")


def _raw(gq, cs):
    """The buffers of a direct gq_track_terms call on a case."""
    ops = gq.ops
    hp, idx = _pose(gq, cs["pose9"])
    hpc, ix = hp.cuda(), idx.cuda()
    Rg = ops.fk_contacts(hpc, ix, gq.hand)[0].contiguous()
    return hpc, Rg, torch.from_numpy(cs["base_T"]).cuda(), torch.from_numpy(cs["q_start"]).cuda(), _arm(gq, cs["arm"], cs["name"])


def test_accumulate_up_w_and_null_outputs(gq):
    ops = gq.ops
    cs = to.case("arm7", 1, 4, 2)
    hpc, Rg, base, qs, arm = _raw(gq, cs)
    B, T, N = 8, cs["T"], 7
    z = lambda *s: torch.zeros(*s, device="cuda")

    def call(up=None, w=1.0, e=None, q=None, worst=None, step=None, sq=None, acc=0, gRt=None, K=0):
        ops._track_call(arm, hpc, Rg, base, BE, cs["axis"], cs["distance"], T, cs["U"], ro.LAM, ro.RHO, qs, K, up, w, e, q, worst, step, sq,
                        acc, gRt)

    e, q, worst, step, g1 = z(B), z(B, T + 1, N), z(B), z(B), z(B, 12)
    call(e=e, q=q, worst=worst, step=step, gRt=g1)
    assert float(g1.abs().max()) > 0
    # accumulate = 1 adds to what is there, 0 overwrites it
    seed = torch.randn(B, 12, generator=torch.Generator().manual_seed(1)).cuda()
    g = seed.clone()
    call(acc=1, gRt=g)
    assert torch.equal(g, seed + g1)
    call(acc=0, gRt=g)
    assert torch.equal(g, g1)
    # up and w scale the gradient and leave the value alone: c = w up / (T+1), powers of two scale exactly
    up = torch.tensor([1.0, 2.0, 4.0, 0.5, 1.0, 2.0, 4.0, 0.5]).cuda()
    g2, e2 = z(B, 12), z(B)
    call(up=up, e=e2, gRt=g2)
    assert torch.equal(g2, g1 * up[:, None]) and torch.equal(e2, e)
    g3, g4 = z(B, 12), z(B, 12)
    call(w=2.0, gRt=g3)
    call(up=torch.full((B,), 2.0).cuda(), gRt=g4)
    assert torch.equal(g3, 2.0 * g1) and torch.equal(g3, g4)
    # every output alone, the others NULL: the same bits
    for kw, want in ((dict(e=z(B)), e), (dict(q=z(B, T + 1, N)), q), (dict(worst=z(B)), worst), (dict(step=z(B)), step)):
        call(**kw)
        assert torch.equal(next(iter(kw.values())), want), list(kw)
    sq = z(B, 2, N)
    call(sq=sq, K=1)
    assert torch.equal(sq[:, 0], q[:, T]) and torch.equal(sq[:, 1], q[:, 0])
    call()  # nothing at all to write
    torch.cuda.synchronize()


def test_bad_parameters_return_the_error_status(gq):
    C = gq.C
    cs = to.case("short3", 1, 4, 2)
    hpc, Rg, base, qs, arm = _raw(gq, cs)
    lib = C.lib()
    axis = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    B, N = 8, 3
    e, sq = torch.zeros(B, device="cuda"), torch.zeros(B, 4, N, device="cuda")

    def status(batch=B, n_obj=2, be=BE, D=0.1, T=4, U=2, lam=1e-4, rho=0.1, K=0, stride=N, start=True, station=False, ax=axis):
        return lib.gq_track_terms(arm.handle, C.f32(hpc), hpc.shape[1], C.f32(Rg), batch, C.f32(base), n_obj, be, ax, D, T, U, lam, rho,
                                  C.f32(qs) if start else None, stride, K, None, 1.0, C.f32(e), None, None, None,
                                  C.f32(sq) if station else None, 0, None, C.stream_ptr())

    assert status() == 0 and status(K=2, station=True) == 0 and status(K=3) == 0
    for kw, word in ((dict(T=0), b"n_waypoints"), (dict(T=65), b"n_waypoints"), (dict(U=0), b"n_updates"), (dict(U=17), b"n_updates"),
                     (dict(D=0.0), b"distance"), (dict(D=float("inf")), b"distance"), (dict(lam=0.0), b"damping"),
                     (dict(rho=float("nan")), b"rot_scale"), (dict(K=4), b"n_stations"), (dict(K=-1), b"n_stations"),
                     (dict(K=3, station=True), b"track_station_q"), (dict(K=0, station=True), b"track_station_q"),
                     (dict(n_obj=3), b"base_T"), (dict(batch=0), b"batch"), (dict(start=False), b"q_start"),
                     (dict(stride=N - 1), b"q_start_stride"), (dict(ax=(ctypes.c_float * 3)(0.0, 0.0, 0.0)), b"grasp_axis")):
        assert status(**kw) == 2, kw
        msg = lib.gq_last_error()
        assert b"track" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()


# ---- the stepper ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, weights=None, **kw):
    from graspqp_amd.utils import meshes

    fv = meshes.icosphere(1, 0.05).astype(np.float32)  # 80 faces
    sp = torch.tensor(np.stack([meshes.surface_points(fv, 256, oversample=8).astype(np.float32)] * 2))
    return gq.GraspStepper(gq.hand, gq.ops.MeshSet([fv, fv]), sp, BE, N_CONTACT, weights=weights, **kw)


def _case(gq, name="arm7", n_seeds=4, T=8, U=3):
    """The rows of a case with the HAND's grasp axis (the stepper and calculate_energy take it from the spec): the retreat line is
    another one than the pool's, so a test that compares with the oracle runs it again on the stepper's own start configuration"""
    return dict(to.case(name, n_seeds, T, U), axis=tuple(float(a) for a in gq.spec.grasp_axis))


def _kw(gq, cs):
    return dict(arm=_arm(gq, cs["arm"], cs["name"]), arm_base=cs["base_T"], reach_distance=cs["distance"], reach_stations=to.STATIONS,
                track_waypoints=cs["T"], track_updates=cs["U"])


def _scene(gq):
    z = 0.2 - (-0.6 + 0.05 * torch.arange(25, dtype=torch.float32))  # phi = 0.2 - z: a ceiling 0.2 m above the objects' origins
    return gq.ops.SceneSDF(z.view(1, 1, 25).expand(25, 25, 25).contiguous(), (-0.6, -0.6, -0.6), 0.05)


@pytest.mark.parametrize("mode", ["alone", "together"])
def test_evaluate_term_is_the_op_and_leaves_the_rest(gq, mode):
    """The stepper with the weight against the stepper without it on the same (pose, idx): every other term, g_theta and g_R are
    bitwise the same; the term's entry, track_q, track_step and track_worst are bitwise the launch on the stepper's own pose and
    reach_q[:, K]; the total gains w x the term, the gradient w x the oracle's."""
    ops = gq.ops
    cs = _case(gq)
    hp, idx = _pose(gq, cs["pose9"])
    base, kw = {"E_reach": W_REACH}, {}
    if mode == "together":
        base = {"E_reach": W_REACH, "E_pregrasp": 30.0, "E_squeeze": 1000.0, "E_prior": 7.0}
        kw = dict(pregrasp_scene=_scene(gq), pregrasp_distance=0.08, pregrasp_stations=2)
    st0 = _stepper(gq, weights=base, **kw, **_kw(gq, cs))
    st1 = _stepper(gq, weights=dict(base, E_track=W_TRACK), **kw, **_kw(gq, cs))
    assert st1.term_names == st0.term_names + ("E_track",) and st0.track_q is None and not st1._fuse_loop
    t0, tot0, g0 = st0.evaluate(hp.cuda(), idx.cuda())
    t1, tot1, g1 = st1.evaluate(hp.cuda(), idx.cuda())
    for k in st0.term_names:
        assert torch.equal(t0[k], t1[k]), k
    assert torch.equal(st0.reach_q, st1.reach_q)
    if mode == "together":
        assert torch.equal(st0.g_theta, st1.g_theta) and torch.equal(st0.g_R, st1.g_R) and st0.g_theta.abs().max() > 0
    np.testing.assert_allclose(tot1.cpu().numpy(), (tot0 + W_TRACK * t1["E_track"]).cpu().numpy(), rtol=1e-6)
    B, T, N, K = 8, cs["T"], 7, to.STATIONS
    z = lambda *s: torch.zeros(*s, device="cuda")
    e, q, worst, step = z(B), z(B, T + 1, N), z(B), z(B)
    ops._track_call(st1.arm, st1.pose_new, st1.Rg, st1.arm_base, BE, cs["axis"], cs["distance"], T, cs["U"], ro.LAM, ro.RHO,
                    st1.reach_q[:, K], K, None, 0.0, e, q, worst, step, None, 0, None)
    assert torch.equal(t1["E_track"], e) and torch.equal(st1.track_q, q)
    assert torch.equal(st1.track_worst, worst) and torch.equal(st1.track_step, step) and float(step.max()) > 0
    # against the oracle from the stepper's own start configuration (up = 1)
    qs = st1.reach_q[:, K].cpu().numpy()
    ref = to.track(cs["arm"], cs["pose9"], cs["base_T"], BE, qs, T, cs["U"], cs["axis"], cs["distance"])
    ok = to.stable(cs["arm"], cs["pose9"], cs["base_T"], BE, qs, T, cs["U"], ref, cs["axis"], cs["distance"])
    cs1 = dict(cs, ref=ref, stable=ok, q_start=qs)
    dg = ((g1 - g0) / W_TRACK).cpu().numpy()
    E = t1["E_track"].cpu().numpy()
    m = to.compared_set(cs1, f"stepper {mode}", kinds=False)
    assert m.sum() >= 6 and (np.abs(E - ref["E"])[m] <= to.e_bound(ref["E"])[m]).all()
    # the difference of two float32 gradients of the whole energy: its rounding is relative to |g1|, not to the term's share
    noise = 4 * np.finfo(np.float32).eps * np.linalg.norm(g1.cpu().numpy()[m][:, :9]) / W_TRACK
    err, gn = np.linalg.norm(dg[m][:, :9] - ref["grad"][m]), np.linalg.norm(ref["grad"][m])
    print(f"[stepper {mode}] gradient err / (1e-3 |g| + noise) = {err / (1e-3 * gn + noise):.2e}")
    assert err <= 1e-3 * gn + noise


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
    reach_only = {k: v for k, v in kw.items() if not k.startswith("track_")}
    want = _five(_stepper(gq, weights={"E_reach": W_REACH}, **reach_only), hp, idx)
    for k2 in (dict(weights={"E_reach": W_REACH, "E_track": 0.0}, **kw), dict(weights={"E_reach": W_REACH}, **kw)):
        st = _stepper(gq, **k2)
        assert st.term_names[-1] == "E_reach" and not st.track_mode and st.track_q is None
        assert all(torch.equal(a, b) for a, b in zip(_five(st, hp, idx), want))


def test_captured_graph_replays_equal_eager_steps_and_runs_repeat(gq):
    cs = _case(gq, "elbow6")
    hp, idx = _pose(gq, cs["pose9"])
    out = []
    for captured in (False, True, False):
        st = _stepper(gq, weights={"E_reach": W_REACH, "E_track": W_TRACK}, **_kw(gq, cs))
        st.reset(hp.cuda(), idx.cuda())
        if captured:
            st.capture()
        for s in range(5):
            st.step(draws=_draws(st, 200 + s))
        out.append(_state(st) + [st.reach_q.clone(), st.track_q.clone(), st.track_step.clone(), st.track_worst.clone()])
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))  # a captured graph replays bit for bit against eager
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[2]))  # two runs are bitwise equal
    assert (out[0][5] == 5).all() and torch.isfinite(out[0][3]).all()


def test_select_gates_on_the_term(gq):
    cs = _case(gq, "elbow6")
    hp, idx = _pose(gq, cs["pose9"])
    st = _stepper(gq, weights={"E_reach": W_REACH, "E_track": W_TRACK}, **_kw(gq, cs))
    st.reset(hp.cuda(), idx.cuda())
    e = st.terms[st.term_names.index("E_track")].cpu()
    tol = 1e-6
    keep = e <= tol
    assert 0 < int(keep.sum()) < 8
    sel = st.select(BE, radius=0.0, gates={"E_track": tol})
    assert sel.feasible.cpu().tolist() == keep.int().tolist()
    assert int(st.select(BE, radius=0.0).n_selected.sum()) == 8  # not gated by default
    reach_only = {k: v for k, v in _kw(gq, cs).items() if not k.startswith("track_")}
    with pytest.raises(ValueError, match="E_track"):
        _stepper(gq, weights={"E_reach": W_REACH}, **reach_only).select(BE, gates={"E_track": tol})  # a gate on the switched-off term


def test_arm_on_track_feeds_the_arm_term_the_path(gq):
    """arm_on_track=True: E_arm is bitwise ops.arm_terms at track_station_q, which is bitwise the waypoints of track_q; off, E_arm and
    everything before it are what they were."""
    ops = gq.ops
    cs = _case(gq, "arm7")
    spec = cs["arm"].with_link_spheres(0.05, 0.10)
    hp, idx = _pose(gq, cs["pose9"])
    scene = _scene(gq)
    kw = dict(_kw(gq, cs), arm=_arm(gq, spec, cs["name"]), arm_scene=scene, arm_margin=0.02)
    w = {"E_reach": W_REACH, "E_arm": W_ARM}
    st_ref = _stepper(gq, weights=w, **kw)
    st_off = _stepper(gq, weights=dict(w, E_track=W_TRACK), **kw)
    st_on = _stepper(gq, weights=dict(w, E_track=W_TRACK), arm_on_track=True, **kw)
    assert st_on.term_names[-2:] == ("E_arm", "E_track") and st_off.track_station_q is None
    tr, _, _ = st_ref.evaluate(hp.cuda(), idx.cuda())
    t0, _, _ = st_off.evaluate(hp.cuda(), idx.cuda())
    t1, _, _ = st_on.evaluate(hp.cuda(), idx.cuda())
    assert torch.equal(tr["E_arm"], t0["E_arm"]) and float(t0["E_arm"].max()) > 0  # off: unchanged
    assert torch.equal(t0["E_track"], t1["E_track"]) and torch.equal(st_off.track_q, st_on.track_q)
    T, K = cs["T"], to.STATIONS
    for k in range(K + 1):
        assert torch.equal(st_on.track_station_q[:, k], st_on.track_q[:, T * (K - k) // K])
    hpc, ix = hp.cuda(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    e = ops.arm_terms(hpc, gq.hand, ix, Rg, LT, ws, st_on.arm, st_on.arm_base, BE, scene, cs["axis"], st_on.track_station_q, cs["distance"], K,
                      0.02, 1e-6, ro.RHO)
    assert torch.equal(t1["E_arm"], e)
    assert not torch.equal(t1["E_arm"], t0["E_arm"])  # the path's configurations are not the reach term's on these rows
    with pytest.raises(ValueError, match="divide track_waypoints"):
        _stepper(gq, weights=dict(w, E_track=W_TRACK), arm_on_track=True, **dict(kw, track_waypoints=7))  # K = 2 does not divide 7


def test_class_surface_term_is_the_op(gq):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF
    from graspqp_amd.utils import meshes

    ops = gq.ops
    cs = _case(gq, "gantry6")
    hp, idx = _pose(gq, cs["pose9"])
    fv = meshes.icosphere(1, 0.05).astype(np.float32)
    sp = meshes.surface_points(fv, 64, oversample=8).astype(np.float32)
    hm = HandModel(gq.spec, "cuda")
    om = ObjectModel(batch_size_each=BE, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv, fv], surface_points_list=[sp, sp])
    hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
    hm.set_reach(cs["arm"], cs["base_T"], cs["distance"], to.STATIONS)
    hm.set_track(cs["T"], cs["U"])
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_reach", "E_track"],
                              svd_gain=0.1)
    up = torch.as_tensor(cs["up"], dtype=torch.float32).cuda()
    (g,) = torch.autograd.grad((losses["E_track"] * up).sum(), hm.hand_pose)
    # the op, fed with the reach op's own reach_q
    hpc, ix = hp.cuda().requires_grad_(), idx.cuda()
    Rg, LT, _, _, _, ws = ops.fk_contacts(hpc, ix, gq.hand)
    arm, base = hm.reach[0], torch.from_numpy(cs["base_T"]).cuda()
    _, q, _ = ops.reach_terms(hpc.detach(), gq.hand, ix, Rg, LT, ws, arm, base, BE, cs["axis"], cs["distance"], to.STATIONS, return_q=True)
    e = ops.track_terms(hpc, gq.hand, ix, Rg, LT, ws, arm, base, BE, cs["axis"], q[:, to.STATIONS], cs["distance"], cs["T"], cs["U"])
    (e * up).sum().backward()
    assert torch.equal(losses["E_track"].detach(), e.detach()) and torch.equal(g, hpc.grad)
    assert float(hpc.grad.abs().max()) > 0
