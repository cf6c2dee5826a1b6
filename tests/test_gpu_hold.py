"""E_hold on the GPU: gq_hold_terms (one block per row, one wavefront per load) against tests/_hold_cases.py.

What is held to what, per case of 8 rows (4 objects x 2 rows; every regime of the box QP occurs, ``assert_populated``):
  * the fp64 run of the SAME loop at the same T = 16: E, resid, force, torque, g_contact_pts.  Per row, kernel error <= 2 x the error
    of that loop run in fp32 on the CPU for the row, with a floor of 1e-4 and an absolute ceiling of 5e-3 (tests/_parity.py).  E and
    resid are dimensionless shares in [0, 1] and take the figures as they are; forces take them times the row's largest load |w|
    (N), torques times |w| x 0.3 m (the span of a hand).  Gradients norm-wise per row: error <= 2 x max(the fp32 loop's error of the
    row, its worst over the case's rows), and <= 5e-3 of max(|g|, 1e-3).  No row is left out.
  * the exact optimum (scipy BVLS, fp64): E within 1e-3 absolute.  This documents the envelope approximation, not parity.
  * reproducibility and isolation: two launches bitwise equal, rows 0..3 alone = inside the 8, L = 1 with load l = slice l of L = 8.
  * autograd of ops.hold_terms = g_contact_pts of the raw launch.

Measured on an MI355X (45 cases; the launch's loop runs in fp64): worst errors against the fp64 loop E 1.6e-7, resid 1.1e-7, force
3.1e-6 N, torque 3.2e-6 N m, gradient 1.4e-7 (9.9e-7 relative); worst error over allowance 0.002, 0.001, 0.001, 0.005; E within
1.6e-7 of the BVLS optimum.  What is left is the fp32 rounding of the inputs' products and of the outputs."""
import numpy as np
import pytest
import torch

import _hold_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gq():
    import types

    from graspqp_amd import _C, ops

    assert torch.cuda.is_available()
    return types.SimpleNamespace(C=_C, ops=ops, hands={})


def _hand(gq, name):
    if name not in gq.hands:
        gq.hands[name] = gq.ops.HandHandle(hc.spec_of(name))
    return gq.hands[name]


def _launch(gq, name, n, k, loads, rows=slice(None), up=None, limits=None, iters=hc.T):
    """The raw launch with every output -> dict of CPU tensors.  ``loads`` (n_obj,L,6) CPU; rows: which of the 8 rows run."""
    ops, hand = gq.ops, _hand(gq, name)
    hp, idx, cp, nrm, cog = (t[rows].cuda().contiguous() for t in hc.inputs(name, n))
    Bn, L = hp.shape[0], loads.shape[1]
    Rg, LT, _, _, _, ws = ops.fk_contacts(hp, idx, hand)
    z = lambda *s: torch.full(s, float("nan"), device="cuda")
    out = dict(e=z(Bn), resid=z(Bn, L), x=z(Bn, L, n * k), force=z(Bn, L, n, 3), torque=z(Bn, L, hand.J), g=z(Bn, n, 3))
    if limits is not None:
        out["effort"] = z(Bn)
    first = (rows.start or 0) // hc.BE
    lw = ops.hold_check(hand, n, k, loads, hc.MAX_FORCE, hc.RIDGE, iters, hc.MU, hc.TW)[first:first + Bn // hc.BE]
    ops._hold_call(hand, idx, Rg.contiguous(), LT.contiguous(), ws, nrm, cp, cog, lw.cuda().contiguous(), hc.BE, k, hc.MU, hc.TW,
                   hc.MAX_FORCE, hc.RIDGE, iters, limits, up, 1.0, out["e"], out["resid"], out["x"], out["force"], out["torque"],
                   out.get("effort"), 0, out["g"])
    torch.cuda.synchronize()
    return {key: v.cpu() for key, v in out.items()}


def _bounded(err, noise, scale, what, tag):
    """Per row: err <= max(2 noise, 1e-4 scale) and err <= 5e-3 scale; prints the worst ratio to the allowance."""
    allow = np.minimum(np.maximum(2.0 * noise, 1e-4 * scale), 5e-3 * scale)
    ratio = err / allow
    print(f"[{tag}] {what}: worst error {err.max():.2e} (fp32 loop {noise.max():.2e}), worst error / allowance {ratio.max():.3f}")
    assert (err <= np.maximum(2.0 * noise, 1e-4 * scale)).all(), (tag, what, "2 x fp32 noise", err.tolist(), noise.tolist())
    assert (err <= 5e-3 * scale).all(), (tag, what, "ceiling", err.tolist())
    return float(ratio.max())


@pytest.mark.parametrize("L", hc.LOADS)
@pytest.mark.parametrize("n,k", hc.NK)
@pytest.mark.parametrize("name", hc.HANDS)
def test_launch_matches_the_fp64_loop(gq, name, n, k, L):
    tag = f"{name} n={n} k={k} L={L}"
    r64 = hc.reference(name, n, k, L, torch.float64, with_exact=True)
    r32 = hc.reference(name, n, k, L, torch.float32)
    hc.assert_populated(r64, n, tag)
    assert np.abs(r64["E"] - r64["E_exact"]).max() < 1e-6, tag  # the fp64 loop itself has converged at T = 16 on these cases
    out = {key: v.double().numpy() for key, v in _launch(gq, name, n, k, hc.loads(L)).items()}
    rows = lambda a: a.reshape(hc.B, -1)
    wmax = r64["wnorm"].max(1)
    _bounded(np.abs(out["e"] - r64["E"]), np.abs(r32["E"] - r64["E"]), np.ones(hc.B), "E", tag)
    _bounded(np.abs(out["resid"] - r64["resid"]).max(1), np.abs(r32["resid"] - r64["resid"]).max(1), np.ones(hc.B), "resid", tag)
    _bounded(np.abs(rows(out["force"] - r64["force"])).max(1), np.abs(rows(r32["force"] - r64["force"])).max(1), wmax, "force", tag)
    _bounded(np.abs(rows(out["torque"] - r64["torque"])).max(1), np.abs(rows(r32["torque"] - r64["torque"])).max(1), 0.3 * wmax, "torque",
             tag)
    ge, gn = np.linalg.norm(rows(out["g"] - r64["g"]), axis=1), np.linalg.norm(rows(r32["g"] - r64["g"]), axis=1)
    gs = np.maximum(np.linalg.norm(rows(r64["g"]), axis=1), 1e-3)
    print(f"[{tag}] g: worst error {ge.max():.2e} (fp32 loop {gn.max():.2e}), worst relative {np.max(ge / gs):.2e}")
    assert (ge <= 2.0 * np.maximum(gn, gn.max())).all(), (tag, "g", ge.tolist(), gn.tolist())
    assert (ge <= 5e-3 * gs).all(), (tag, "g ceiling", (ge / gs).tolist())
    # the envelope approximation: E at the iterate against E at the exact optimum
    print(f"[{tag}] |E - E(BVLS)| max {np.abs(out['e'] - r64['E_exact']).max():.2e}")
    assert np.abs(out["e"] - r64["E_exact"]).max() <= 1e-3, tag
    zero = r64["resid"].min(1) > 0.999  # nothing held: no gradient
    assert np.abs(rows(out["g"])[zero]).max() < 1e-3 and np.abs(out["e"][zero] - 1).max() < 1e-3, tag


@pytest.mark.parametrize("name,n,k", [("allegro", 3, 4), ("ability_hand", 12, 8), ("panda", 5, 8)])
def test_bitwise_reproducible_and_row_local(gq, name, n, k):
    lw = hc.loads(8)
    a, b = _launch(gq, name, n, k, lw), _launch(gq, name, n, k, lw)
    for key in a:
        assert torch.equal(a[key], b[key]) and torch.isfinite(a[key]).all(), key
    half = _launch(gq, name, n, k, lw, rows=slice(0, 4))  # rows 0..3 alone
    for key in a:
        assert torch.equal(half[key], a[key][:4]), key
    for l in (0, 3, 7):  # one load alone = its slice of the eight
        one = _launch(gq, name, n, k, lw[:, l:l + 1].contiguous())
        for key in ("x", "force", "torque", "resid"):
            assert torch.equal(one[key][:, 0], a[key][:, l]), (key, l)


def test_effort_is_the_largest_torque_over_its_limit(gq):
    name, n, k, L = "ability_hand", 5, 8, 3
    hand = _hand(gq, name)
    lim = (0.2 + torch.rand(hand.J, generator=torch.Generator().manual_seed(3))).cuda()
    out = _launch(gq, name, n, k, hc.loads(L), limits=lim)
    want = (out["torque"].abs() / lim.cpu()).amax((1, 2))
    torch.testing.assert_close(out["effort"], want, rtol=1e-6, atol=0.0)
    assert (want > 0).all()


def test_other_iteration_counts_follow_the_same_loop(gq):
    """T = 3 (far from converged) and T = 20: the launch still tracks the fp64 loop at the same T, so the count is honoured."""
    name, n, k, L = "allegro", 12, 4, 3
    e16 = hc.reference(name, n, k, L)["E"]
    for iters in (3, 20):
        ref = hc.reference(name, n, k, L, torch.float64, iters)
        out = _launch(gq, name, n, k, hc.loads(L), iters=iters)
        err = np.abs(out["e"].double().numpy() - ref["E"]).max()
        print(f"[T={iters}] E err {err:.2e}, |E_T - E_16| {np.abs(ref['E'] - e16).max():.2e}")
        assert err <= 1e-3
    assert np.abs(hc.reference(name, n, k, L, torch.float64, 3)["E"] - e16).max() > 1e-2  # T = 3 is another answer: the count matters


def test_autograd_is_the_raw_launch(gq):
    ops = gq.ops
    name, n, k, L = "ability_hand", 5, 8, 3
    hand = _hand(gq, name)
    hp, idx, cp, nrm, cog = (t.cuda() for t in hc.inputs(name, n))
    up = (torch.rand(hc.B, generator=torch.Generator().manual_seed(5)) + 0.5).cuda()
    raw = _launch(gq, name, n, k, hc.loads(L), up=up)
    Rg, LT, _, _, _, ws = ops.fk_contacts(hp, idx, hand)
    cpg = cp.clone().requires_grad_()
    res = ops.hold_terms(hp, hand, idx, Rg, LT, ws, nrm, cpg, cog[::hc.BE].contiguous(), hc.loads(L), hc.BE, hc.MU, hc.TW, k, hc.MAX_FORCE,
                         return_details=True)
    assert res.effort is None and not res.torque.requires_grad and not res.force.requires_grad and res.e.requires_grad
    (g,) = torch.autograd.grad((res.e * up).sum(), cpg)
    assert torch.equal(g.cpu(), raw["g"]) and g.abs().max() > 0
    for key, val in (("e", res.e), ("resid", res.resid), ("x", res.x), ("force", res.force), ("torque", res.torque)):
        assert torch.equal(val.detach().cpu(), raw[key]), key
    old = ops.use_dispatcher(True)  # the registered op and its registered backward give the same bits
    try:
        cpd = cp.clone().requires_grad_()
        e2 = ops.hold_terms(hp, hand, idx, Rg, LT, ws, nrm, cpd, cog, hc.loads(L), hc.BE, hc.MU, hc.TW, k, hc.MAX_FORCE)
        (g2,) = torch.autograd.grad((e2 * up).sum(), cpd)
    finally:
        ops.use_dispatcher(old)
    assert torch.equal(g2, g) and torch.equal(e2.detach(), res.e.detach())


def test_bad_shapes_and_parameters_return_the_error_status(gq):
    C, ops = gq.C, gq.ops
    lib = C.lib()
    z = lambda *s: torch.zeros(*s, device="cuda")
    Bn = 2
    lw = ops.hold_loads(1.0, accelerations=hc.ACC)  # (8,6)
    lwd = lw.cuda()
    host = lambda t: t.contiguous().data_ptr()

    def status(n=5, k=4, L=3, iters=16, max_force=4.0, ridge=1e-4, mu=0.5, loads=lw, sets=1, each=Bn):
        # every call is refused on the host, before any launch: the buffers are sized for the largest shape named all the same
        return lib.gq_hold_terms(None, None, Bn, n, k, C.f32(z(Bn, 65, 3)), C.f32(z(Bn, 65, 3)), C.f32(z(Bn, 3)), None, None, None, 0,
                                 C.f32(lwd), host(loads), sets, L, each, mu, 5.0, max_force, ridge, iters, None, None, 1.0, C.f32(z(Bn)),
                                 None, None, None, None, None, 0, None, C.stream_ptr())

    assert status(n=65) == 2 and b"contacts" in lib.gq_last_error()
    assert status(n=0) == 2
    assert status(n=33, k=4) == 2 and b"128" in lib.gq_last_error()
    assert status(k=2) == 2
    assert status(L=0) == 2 and status(L=9) == 2 and b"loads" in lib.gq_last_error()
    assert status(iters=0) == 2 and status(iters=65) == 2 and b"iterations" in lib.gq_last_error()
    assert status(max_force=0.0) == 2 and b"max_force" in lib.gq_last_error()
    assert status(max_force=float("inf")) == 2
    assert status(ridge=0.0) == 2 and b"ridge" in lib.gq_last_error()
    assert status(ridge=float("nan")) == 2
    assert status(mu=0.0) == 2 and status(mu=1.5) == 2
    bad = lw.clone()
    bad[1] = 0.0
    assert status(loads=bad) == 2 and b"load 1" in lib.gq_last_error()
    bad[1, 0] = float("nan")
    assert status(loads=bad) == 2
    assert status(each=1) == 2 and b"cover" in lib.gq_last_error()
    assert lib.gq_hold_terms(None, None, Bn, 5, 4, C.f32(z(Bn, 5, 3)), C.f32(z(Bn, 5, 3)), C.f32(z(Bn, 3)), None, None, None, 0, C.f32(lwd),
                             host(lw), 1, 3, Bn, 0.5, 5.0, 4.0, 1e-4, 16, None, None, 1.0, None, None, None, None, C.f32(z(Bn, 3, 16)), None,
                             0, None, C.stream_ptr()) == 2 and b"torque" in lib.gq_last_error()  # a torque output without the hand
    torch.cuda.synchronize()
