"""The surface of the payload-holding term: ops.hold_loads / ops.hold_check values and refusals, the class-surface energy name, the
stepper's verb, the export keys and the selection gate.  The first half needs no GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import _hold_cases as hc
import _squeeze_cases as sq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


# ---- no GPU ---------------------------------------------------------------------------------------------------------------------
def test_hold_loads_values():
    from graspqp_amd import ops

    w = ops.hold_loads(2.0)
    assert w.shape == (1, 6) and w.dtype == torch.float32 and not w.is_cuda
    np.testing.assert_allclose(w.numpy(), [[0, 0, -19.62, 0, 0, 0]], atol=1e-6)
    w = ops.hold_loads(2.0, up=(0, 3, 0), accelerations=((0, 0, 0), (1, 0, 0)), com_offset=(0.1, 0, 0), g=10.0)  # up is normalised
    np.testing.assert_allclose(w.numpy(), [[0, -20, 0, 0, 0, -2.0], [-2, -20, 0, 0, 0, -2.0]], atol=1e-6)
    w = ops.hold_loads([1.0, 3.0], accelerations=((0, 0, 2.0),), com_offset=[(0, 0, 0), (0, 0.5, 0)])
    assert w.shape == (2, 1, 6)
    np.testing.assert_allclose(w[:, 0].numpy(), [[0, 0, -11.81, 0, 0, 0], [0, 0, -35.43, -17.715, 0, 0]], rtol=1e-6, atol=1e-6)
    for bad in (dict(mass=0.0), dict(mass=float("nan")), dict(mass=1.0, up=(0, 0, 0)), dict(mass=1.0, accelerations=[(0, 0, 0)] * 9),
                dict(mass=1.0, accelerations=(0, 0, 0)), dict(mass=[1.0, 2.0], com_offset=[(0, 0, 0)] * 3), dict(mass=1.0, g=0.0)):
        with pytest.raises(ValueError, match="hold_loads"):
            ops.hold_loads(**bad)


def test_hold_check_refusals():
    from graspqp_amd import ops

    lw = ops.hold_loads(1.0, accelerations=hc.ACC[:3])
    out = ops.hold_check(None, 5, 4, lw, 4.0)
    assert out.shape == (1, 3, 6) and out.dtype == torch.float32
    assert ops.hold_check(None, 5, 4, lw[None].expand(2, 3, 6), 4.0, n_obj=2).shape == (2, 3, 6)
    torque_only = torch.tensor([[0, 0, 0, 0, 0, 1.0]])
    assert ops.hold_check(None, 5, 4, torque_only, 4.0).shape == (1, 1, 6)
    zero, nan = lw.clone(), lw.clone()
    zero[1] = 0
    nan[2, 4] = float("nan")
    for kw in (dict(loads=zero), dict(loads=nan), dict(loads=lw[:, :5]), dict(loads=torch.zeros(9, 6) + 1), dict(max_force=0.0),
               dict(max_force=float("inf")), dict(ridge=0.0), dict(iterations=0), dict(iterations=65), dict(friction=0.0), dict(friction=1.2),
               dict(n_contact=65), dict(n_contact=33), dict(n_cone_vecs=2), dict(loads=torque_only, torque_weight=0.0),
               dict(torque_limits=[1.0, -1.0]), dict(loads=lw[None].expand(3, 3, 6), n_obj=2)):
        args = dict(hand=None, n_contact=5, n_cone_vecs=4, loads=lw, max_force=4.0)
        args.update(kw)
        with pytest.raises(ValueError, match="hold_terms"):
            ops.hold_check(**args)


def test_the_energy_name_needs_set_hold():
    from graspqp_amd.core import energy

    with pytest.raises(ValueError, match="set_hold"):
        energy._extra_terms({}, types.SimpleNamespace(), ["E_hold"], None, None)


def test_the_stepper_table_is_untouched():
    from graspqp_amd import stepper

    assert "E_hold" not in stepper.TERMS and "E_hold" not in stepper.LAUNCH_ORDER
    with pytest.raises(ValueError):
        stepper.merge_weights({"E_hold": 1.0})


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "hold_terms") and hasattr(ns, "hold_terms_backward")
    stand_in = type("H", (), {"J": 11})()  # what the fake kernel reads of a hand: its actuated joints
    hid = ops._register_handle(stand_in)
    Bn, n, k, L = 6, 5, 8, 3
    with FakeTensorMode():
        e = lambda *s, **kw: torch.empty(*s, device="cuda", **kw)
        args = (hid, e(Bn, n, dtype=torch.int64), e(Bn, 3, 3), e(Bn, 4, 3, 4), e(64, dtype=torch.uint8), e(Bn, n, 3), e(Bn, n, 3), e(Bn, 3),
                e(2, L, 6), 3, 0.5, 5.0, k, 4.0, 1e-4, 16)
        out = ns.hold_terms(*args, None)
        assert [tuple(t.shape) for t in out] == [(Bn,), (Bn, L), (Bn, L, n * k), (Bn, L, n, 3), (Bn, L, 11), (0,)]
        assert ns.hold_terms(*args, e(11))[5].shape == (Bn,)
        assert ns.hold_terms_backward(*args[5:], e(Bn)).shape == (Bn, n, 3)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_new_kernel_resources():
    """The new kernels (one and two column slots): up to 8 wavefronts per block, no scratch, no vector spills."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    new = {key: v for key, v in kernel_resources(LIB).items() if "hold" in key}
    assert len(new) == 2, sorted(new)
    for key, r in new.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (key, r)
        assert r["max_threads"] == 512 and r["vgpr"] + r["agpr"] <= 256, (key, r)  # 8 wavefronts of a block fit one CU


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gq(tmp_path_factory):
    from graspqp_amd import _C, ops
    from graspqp_amd.stepper import GraspStepper

    assert torch.cuda.is_available()
    sq.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    return types.SimpleNamespace(C=_C, ops=ops, GraspStepper=GraspStepper, hand=ops.HandHandle(sq.spec_of("allegro")))


LOADS = dict(mass=0.3, accelerations=hc.ACC[:3])
MAX_FORCE = 5.0


def _op_on(gq, hp, idx, objs, cog, fc, lim=None):
    """ops.hold_terms on the state (hp, idx), composed from the public ops."""
    ops = gq.ops
    Bn, n = idx.shape
    Rg, LT, cp, _, _, ws = ops.fk_contacts(hp, idx, gq.hand)
    d2, sgn, nrm, _ = ops.sdf_meshset(cp.detach().reshape(-1, 3), objs, Bn * n)
    _, onrm = ops.signed_distance(d2, sgn, nrm)
    return ops.hold_terms(hp, gq.hand, idx, Rg, LT, ws, onrm.reshape(Bn, n, 3), cp, cog, ops.hold_loads(**LOADS), Bn, fc["friction"],
                          fc["torque_weight"], fc["n_cone_vecs"], MAX_FORCE, torque_limits=lim, return_details=True)


def _stepper(gq, Bn, n, **kw):
    from graspqp_amd.utils import meshes

    fv, _ = sq.sphere()
    sp = torch.tensor(meshes.surface_points(fv, 512, oversample=8).astype(np.float32))[None]
    return gq.GraspStepper(gq.hand, gq.ops.MeshSet([fv]), sp, Bn, n, **kw)


def _draws(st, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(st.B, st.n, device="cuda", generator=g),
            torch.randint(st.hand.spec.n_contact_candidates, (st.B, st.n), device="cuda", generator=g), torch.rand(st.B, device="cuda", generator=g))


def _state(st):
    torch.cuda.synchronize()
    return [t.clone() for t in (st.hand_pose, st.contact_idx, st.grad, st.energy, st.ema, st.step_count, st.terms)]


@pytest.mark.gpu
def test_stepper_hold_is_the_op_and_leaves_the_chain_alone(gq):
    Bn, n = 8, 4
    hp, idx = sq.inputs("allegro", Bn, n)
    lim = torch.full((gq.hand.J,), 0.5)
    out = []
    for call in (False, True):
        st = _stepper(gq, Bn, n)
        st.reset(hp.cuda(), idx.cuda())
        for s in range(3):
            st.step(draws=_draws(st, 300 + s))
        if call:
            res = st.hold(gq.ops.hold_loads(**LOADS), MAX_FORCE, torque_limits=lim)
            want = _op_on(gq, st.hand_pose.clone(), st.contact_idx.clone(), st.objs, st.cog, st.fc, lim)
            for a, b in zip(res, want):
                assert torch.equal(a, b)
            assert res.e.shape == (Bn,) and res.resid.shape == (Bn, 3) and res.force.shape == (Bn, 3, n, 3) and res.effort.shape == (Bn,)
            assert torch.isfinite(res.e).all() and (res.e > 0).all() and (res.e <= 1.0 + 1e-6).all() and (res.effort > 0).all()
        for s in range(3):
            st.step(draws=_draws(st, 400 + s))
        out.append(_state(st))
    assert all(torch.equal(a, b) for a, b in zip(*out))  # the bits of a stepper that never called hold()
    with pytest.raises(ValueError, match="GraspStepper.hold"):
        st.hold(gq.ops.hold_loads(**LOADS), 0.0)


@pytest.mark.gpu
def test_select_gates_on_the_residual(gq):
    Bn, n = 8, 4
    hp, idx = sq.inputs("allegro", Bn, n)
    st = _stepper(gq, Bn, n)
    st.reset(hp.cuda(), idx.cuda())
    h = st.hold(gq.ops.hold_loads(**LOADS), MAX_FORCE)
    worst = h.resid.amax(1).cpu()
    tol = float(worst.sort().values[Bn // 2 - 1])  # half of the rows pass
    sel = st.select(Bn, radius=0.0, score=torch.where(h.resid.amax(1) <= tol, st.energy, torch.inf))
    rows = sel.sel[0][: int(sel.n_selected[0])].cpu().tolist()
    assert sorted(rows) == sorted(torch.nonzero(worst <= tol).flatten().tolist()) and 0 < len(rows) < Bn
    assert all(float(worst[r]) <= tol for r in rows)


@pytest.mark.gpu
def test_class_surface_term_is_the_op_and_export_takes_the_result(gq):
    from graspqp_amd import export
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    Bn, n = 6, 5
    hp, idx = sq.inputs("allegro", Bn, n)
    fv, sp = sq.sphere()
    hm = HandModel(sq.spec_of("allegro"), "cuda")
    om = ObjectModel(batch_size_each=Bn, num_samples=sp.shape[0])
    om.initialize_from_meshes([fv], surface_points_list=[sp])
    hm.set_parameters(hp.cuda().requires_grad_(), idx.cuda())
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.4, "max_limit": 20.0, "n_cone_vecs": 8})
    names = ["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_hold"]
    with pytest.raises(ValueError, match="set_hold"):
        calculate_energy(hm, om, energy_fnc=fn, energy_names=names, svd_gain=0.1)
    hm.set_hold(gq.ops.hold_loads(**LOADS), MAX_FORCE)
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=names, svd_gain=0.1)
    fc = fn.fc_config(svd_gain=0.1)
    want = _op_on(types.SimpleNamespace(ops=gq.ops, hand=hm._hand), hm.hand_pose.detach(), idx.cuda(), om._meshset, om.cog, fc)
    # the energy function and the ops reach the same contact normals by different launches: the same numbers, not pinned to the bit
    torch.testing.assert_close(losses["E_hold"].detach(), want.e, rtol=1e-4, atol=1e-6)
    assert (want.e > 0).all()
    (g,) = torch.autograd.grad(losses["E_hold"].sum(), hm.hand_pose, retain_graph=True)
    assert g.shape == hp.shape and torch.isfinite(g).all() and g[:, :3].abs().max() > 0  # through the contact points to the pose
    # export: two more keys with the argument, the dict as it was without
    energy = sum(losses[k] for k in names[:5]).detach()
    plain = export.snapshot_dicts(hm, energy, om, 1, Bn)
    held = export.snapshot_dicts(hm, energy, om, 1, Bn, hold=want)
    assert set(held[0]) - set(plain[0]) == {"hold_force", "hold_torque"}
    assert held[0]["hold_force"].shape == (Bn, 3, n, 3) and held[0]["hold_torque"].shape == (Bn, 3, hm.n_dofs)
    assert torch.equal(held[0]["hold_force"], want.force.cpu())
    with pytest.raises(ValueError, match="hold"):
        export.snapshot_dicts(hm, energy, om, 1, Bn, hold=gq.ops.HoldResult(*(t[:2] if t is not None else None for t in want)))
