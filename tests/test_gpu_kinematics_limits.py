"""The kinematics kernels at the limits gq_hand_create declares (J <= 64 tree joints, L <= 64 links, S <= 256 spheres, 64 sphere
groups, 320 FK-backward items), on the synthetic hands of tests/_synthetic_hand.py against the fp64 oracle (oracle/ref_cpu):
the self-penetration scan on given centres, FK forward and backward (block kernel and, beyond 512 rows, the one-wavefront
kernel), the explicit Jacobians, and the refusals of sizes beyond the limits.

Tolerances are the ones the shipped hands are held to (forward 2e-6 / 3e-6, backward 1e-4 on the norm and rtol 2e-3 / atol
2e-4, Jacobians 2e-6, E_spen rtol 1e-4 / atol 1e-7).  Only the 64-deep chain accumulates more fp32 round-off than those were
meant for: there the same oracle is run in float32 on the same inputs, its error against its fp64 self is the noise floor,
and the kernel is allowed the larger of the fixed tolerance and 4 x that floor (2 x: two independent fp32 evaluations can sit
on opposite sides of the truth; 2 x: another association order and fused multiply-adds).  star63 holds the fixed tolerances
and does not use the floor."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ref_cpu import export as oexp  # noqa: E402
from ref_cpu import kin as okin  # noqa: E402
from ref_cpu import models as omodels  # noqa: E402

import _fk_backward_case as fkb  # noqa: E402
import _synthetic_hand as sh  # noqa: E402


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C})


@pytest.fixture(scope="module")
def hands(gq, tmp_path_factory):
    """name -> (spec, HandHandle), built on first use and kept for the module; layout(sizes, ...) the same for the flat hands."""
    root = tmp_path_factory.mktemp("synthetic_hands")
    cache = {}

    class Hands:
        def __call__(self, name):
            if name not in cache:
                spec = sh.build(name, root)
                cache[name] = (spec, gq.ops.HandHandle(spec))
            return cache[name]

        def layout(self, sizes, **kw):
            key = (tuple(sizes), tuple(sorted((k, str(v)) for k, v in kw.items())))
            if key not in cache:
                spec = sh.layout(root, sizes, **kw)
                cache[key] = (spec, gq.ops.HandHandle(spec))
            return cache[key]

    yield Hands()
    for _, hand in cache.values():
        hand.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the self-penetration scan on given centres
# ---------------------------------------------------------------------------------------------------------------------------
# group sizes, half-width of the box of centres (m)
LAYOUTS = {"ng2": ([1, 1], 0.012), "ng17": ([1] * 17, 0.05), "ng18_s70": ([3] * 6 + [5] * 8 + [1] * 3 + [9], 0.07),
           "ng33_s130": ([4] * 32 + [2], 0.09), "ng64_s256": ([4] * 64, 0.12)}
SPEN_SEED = 5
SPEN_ROWS = 8


def spen_scene(sizes, half_width, seed=SPEN_SEED, B=SPEN_ROWS):
    """World centres (B,S,3) float32, uniform in the box; the radii come with the layout hand (uniform in [5 mm, 15 mm])."""
    return np.random.RandomState(seed + 1).uniform(-half_width, half_width, (B, sum(sizes), 3)).astype(np.float32)


def spen_facts(spec, centers):
    """What the scene exercises, from the fp64 view of the float32 centres and radii alone: per row and scanned group the best
    pair, its penetration, its margin over the runner-up and the distance of its centres; per sphere the number of groups
    whose gradient lands on it."""
    c = np.asarray(centers, np.float64)
    rad = np.asarray(spec.sphere, np.float64)[:, 3]
    link = np.asarray(spec.sphere_link)
    B, S = c.shape[:2]
    starts = [s for s in range(S) if s == 0 or link[s] != link[s - 1]] + [S]
    ng = len(starts) - 2
    best, gap, dist = np.zeros((B, ng)), np.full((B, ng), np.inf), np.zeros((B, ng))
    hits = np.zeros((B, S), dtype=int)
    for r in range(B):
        for gi, (a0, a1) in enumerate(zip(starts[:-2], starts[1:-1])):
            dd = np.linalg.norm(c[r, a0:a1, None] - c[r, None, a1:] + 1e-13, axis=-1)
            pen = dd - (rad[a0:a1, None] + rad[None, a1:])
            flat = np.sort(pen.ravel())
            a, b = np.unravel_index(np.argmin(pen), pen.shape)
            best[r, gi], dist[r, gi] = flat[0], dd[a, b]
            if len(flat) > 1:
                gap[r, gi] = flat[1] - flat[0]
            if flat[0] < 0:
                hits[r, a0 + a] += 1
                hits[r, a1 + b] += 1
    return dict(best=best, gap=gap, dist=dist, hits=hits, ng=ng)


def assert_spen_preconditions(spec, centers, label):
    """The scene must reach the paths it is there for, and its argmin pairs must be unambiguous in fp32 (distance round-off is
    about 1e-8 m) -- asserted on the oracle's view alone, before the kernel is looked at."""
    f = spen_facts(spec, centers)
    NG, S = f["ng"] + 1, spec.n_spheres
    pen = f["best"] < 0
    print(f"{label}: penetrating groups per row {pen.sum(1).tolist()}, min gap {f['gap'].min():.3g}, min |pen| {np.abs(f['best']).min():.3g}, "
          f"min |a-b| {f['dist'].min():.3g}, max contributions on one sphere {f['hits'].max()}")
    assert pen.any(1).all(), "every row must have penetrating groups"
    if NG >= 18:
        assert pen[:, 16:].any(), "a penetrating group in the second pass of the scan"
    if NG == 64:
        assert pen[:, 48:].any(), "a penetrating group in the fourth pass of the scan"
    if S > 64:
        assert f["hits"][:, 64:].any(), "a sphere beyond the first stride must receive a gradient"
    if S > 2:
        assert f["hits"].max() >= 2, "a sphere must receive contributions from two groups"
    assert f["gap"].min() >= 1e-5 and np.abs(f["best"]).min() >= 1e-5 and f["dist"].min() >= 1e-3
    return f


def _oracle_spen(spec, centers):
    c = torch.tensor(np.asarray(centers, np.float64)).requires_grad_()
    e = okin.self_penetration(spec, c)
    e.sum().backward()
    return e.detach().numpy(), c.grad.numpy()


def _device_spen(gq, hand, centers):
    c = torch.tensor(centers).cuda().requires_grad_()
    e = gq.ops.self_pen(c, hand)
    e.sum().backward()
    return e.detach().cpu().numpy(), c.grad.cpu().numpy()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_self_pen_scan_on_given_centres(gq, hands, name):
    """ops.self_pen against okin.self_penetration in fp64 and its autograd gradient, every row, group and element.  Gradient
    tolerance 1e-4 absolute: a contribution is a unit vector (a-b)/|a-b|; coordinate round-off of about 2e-8 m over |a-b| >=
    1e-3 m is 2e-5 per component, times 5 for up to three contributions on a sphere (one sphere of the NG = 64 scene takes
    four: 8e-5).  Measured on the MI355X: gradient max abs 6.7e-8 .. 1.5e-7, e_spen max rel 3.8e-8 .. 8.9e-8 over the five
    layouts; the scenes' smallest margin over the runner-up is 1.7e-5 m, smallest |pen| 1.8e-5 m, smallest |a-b| 2.1e-3 m."""
    sizes, hw = LAYOUTS[name]
    spec, hand = hands.layout(sizes, seed=SPEN_SEED)
    centers = spen_scene(sizes, hw)
    assert_spen_preconditions(spec, centers, name)
    eo, go = _oracle_spen(spec, centers)
    e, g = _device_spen(gq, hand, centers)
    print(f"{name}: e_spen max rel {np.abs(e - eo).max() / eo.max():.3g}, gradient max abs {np.abs(g - go).max():.3g}")
    np.testing.assert_allclose(e, eo, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(g, go, rtol=0, atol=1e-4)


def test_self_pen_exact_tie_goes_to_the_first_pair(gq, hands):
    """Two pairs of one group with the same penetration to the bit (coordinates on a 2^-10 m grid, equal radii): the energy is
    the oracle's, and the gradient goes to the first minimal pair in (a, b) order -- the documented rule of the scan's key."""
    spec, hand = hands.layout([2, 2], seed=3, radii=[0.005] * 4)
    u = sh.GRID
    base = np.array([[0, 0, 0], [0, 64, 0], [8, 0, 0], [8, 64, 0]], np.float64) * u  # (a0, a1 | b0, b1): a0-b0 and a1-b1 tie
    shift = np.arange(SPEN_ROWS)[:, None, None] * np.array([16, -8, 4], np.float64)[None, None] * u
    centers = (base[None] + shift).astype(np.float32)
    assert np.array_equal(centers.astype(np.float64), base[None] + shift), "the scene must be exact in float32"
    d = centers[:, :2, None].astype(np.float64) - centers[:, None, 2:]
    assert (np.linalg.norm(d[:, 0, 0], axis=-1) == np.linalg.norm(d[:, 1, 1], axis=-1)).all()
    eo, _ = _oracle_spen(spec, centers)
    assert (eo > 2e-3).all()
    e, g = _device_spen(gq, hand, centers)
    np.testing.assert_allclose(e, eo, rtol=1e-4, atol=1e-7)
    want = np.zeros_like(g)
    want[:, 0, 0], want[:, 2, 0] = 1.0, -1.0  # dE/da = -(a-b)/|a-b| with a - b = (-8u, 0, 0); dE/db = the opposite
    np.testing.assert_allclose(g, want, rtol=0, atol=1e-6)


def test_self_pen_without_spheres_is_zero(gq, hands):
    spec, hand = hands("nospheres")
    e = gq.ops.self_pen(torch.zeros(5, 0, 3, device="cuda"), hand)
    assert e.shape == (5,) and e.dtype == torch.float32 and not e.any()


def test_self_pen_fused_forms_on_star63(gq, hands):
    """S = 65, NG = 18: the scan inside gq_fk_forward and inside gq_spheres_self_pen (centres from the kinematics) and
    gq_self_pen_forward on the centres they produced run one device body -- same e_spen and centre gradients, bit for bit."""
    spec, hand = hands("star63")
    B, n, w_spen = 6, 4, 10.0
    inp = fkb.make_inputs(spec, B, n, 61, sh.joint_scale(spec))
    hp, idx = torch.tensor(inp["hand_pose"]).cuda(), torch.tensor(inp["idx"]).cuda()
    C, f32 = gq.C.call, gq.C.f32
    S, L = spec.n_spheres, spec.n_links
    new = lambda *s, v=-1.0: torch.full(s, v, device="cuda")
    Rg, LT, cp, cn = new(B, 9), new(B, L, 12), new(B, n, 3), new(B, n, 3)
    sc0, e0, g0 = new(B, S, 3), new(B, v=-3.0), new(B, S, 3, v=-3.0)
    ws, nb = hand.fk_ws(B, hp.device)
    C("gq_fk_forward", hand.handle, f32(hp), gq.C.i64(idx), B, n, f32(Rg), f32(LT), f32(cp), f32(cn), f32(sc0), w_spen, f32(e0),
      f32(g0), None, None, gq.C.ptr(ws), nb, gq.C.stream_ptr())
    sc1, e1, g1 = new(B, S, 3), new(B), new(B, S, 3)
    C("gq_spheres_self_pen", hand.handle, f32(hp), hp.shape[1], f32(Rg), f32(LT), B, w_spen, f32(sc1), f32(e1), f32(g1),
      gq.C.stream_ptr())
    e2, g2 = new(B, v=-2.0), new(B, S, 3, v=-2.0)
    C("gq_self_pen_forward", hand.handle, f32(sc1), B, w_spen, f32(e2), f32(g2), gq.C.stream_ptr())
    torch.cuda.synchronize()
    f = spen_facts(spec, sc1.cpu().numpy())
    pen = f["best"] < 0
    print("star63 fused: penetrating groups per row", pen.sum(1).tolist(), "in the second pass", int(pen[:, 16:].sum()),
          "on spheres >= 64", int(f["hits"][:, 64:].sum()))
    assert pen.any(1).all() and pen[:, 16:].any() and f["hits"][:, 64:].any(), "the scene must reach the second pass and stride"
    assert torch.equal(sc0, sc1)
    assert torch.equal(e0, e1) and torch.equal(g0, g1)
    assert torch.equal(e2, e1) and torch.equal(g2, g1)
    eo = okin.self_penetration(spec, sc1.cpu().double()).numpy()
    np.testing.assert_allclose(e1.cpu().numpy(), eo, rtol=1e-4, atol=1e-7)
    # the class surface (grad_scale 1; the scale is on the gradient alone)
    np.testing.assert_array_equal(gq.ops.self_pen(sc1, hand).cpu().numpy(), e1.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# 2. FK forward and backward
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle_forward(spec, hp, idx, weights, dtype):
    oh = omodels.OracleHand(spec, dtype)
    hpo = torch.tensor(hp, dtype=dtype).requires_grad_()
    oh.set_parameters(hpo, torch.tensor(idx))
    sph = okin.sphere_centers_world(spec, oh.current_status, oh.global_rotation, oh.global_translation)
    w1, w2, w3, w4 = (w.to(dtype) for w in weights)
    ((oh.contact_points * w1).sum() + (oh.contact_normals * w2).sum() + (sph * w3).sum() + (oh.global_rotation * w4).sum()).backward()
    a = lambda t: t.detach().double().numpy()
    return dict(Rg=a(oh.global_rotation), LT=a(oh.current_status)[:, :, :3, :], cp=a(oh.contact_points), cn=a(oh.contact_normals),
                sc=a(sph), grad=a(oh.hand_pose.grad))


FORWARD_TOL = dict(Rg=2e-6, LT=3e-6, cp=3e-6, cn=3e-6, sc=3e-6)


@pytest.mark.parametrize("name", sh.TOPOLOGIES)
def test_fk_contacts_forward_backward_on_synthetic_hands(gq, hands, name):
    """The body of test_gpu_parity.py::test_fk_contacts_forward_backward on every topology, B = 4, n = 12.  chain64 takes the
    fp32-oracle floor (module docstring).  Measured on the MI355X for chain64, max abs error of the kernel / of the fp32
    oracle: Rg 1.5e-7 / 7.9e-8, link_T 6.5e-7 / 6.4e-7, contact points 6.7e-8 / 6.4e-8, normals 4.6e-7 / 5.7e-7, sphere
    centres 7.4e-8 / 8.5e-8; gradient norm-wise 2.4e-7 / 3.7e-7, max abs 8.6e-6 / 1.4e-5.  The kernel sits at the floor and
    4 x the floor stays below the fixed tolerances: the chain holds them as they are.  star63: link_T 1.9e-7, gradient
    7.5e-8 norm-wise with the fixed tolerances."""
    spec, hand = hands(name)
    B, n = 4, 12
    inp = fkb.make_inputs(spec, B, n, 70, sh.joint_scale(spec))
    hp, idx = inp["hand_pose"], inp["idx"]
    g = torch.Generator().manual_seed(9)
    S = spec.n_spheres
    weights = [torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B, n, 3), (B, n, 3), (B, S, 3), (B, 3, 3))]
    o = _oracle_forward(spec, hp, idx, weights, torch.float64)
    floor = {k: 0.0 for k in o}
    if name == "chain64":
        o32 = _oracle_forward(spec, hp, idx, weights, torch.float32)
        floor = {k: float(np.abs(o32[k] - o[k]).max()) if o[k].size else 0.0 for k in o}
        floor["grad_norm"] = float(np.linalg.norm(o32["grad"] - o["grad"]) / np.linalg.norm(o["grad"]))
    hpg = torch.tensor(hp).cuda().requires_grad_()
    Rg, LT, cp, cn, sc, _ = gq.ops.fk_contacts(hpg, torch.tensor(idx).cuda(), hand)
    assert sc.shape == (B, S, 3)
    got = dict(Rg=Rg, LT=LT, cp=cp, cn=cn, sc=sc)
    for k, tol in FORWARD_TOL.items():
        v = got[k].detach().cpu().numpy()
        err = float(np.abs(v - o[k]).max()) if v.size else 0.0
        print(f"{name} {k}: kernel max abs {err:.3g}, fp32 oracle floor {floor[k]:.3g}")
        np.testing.assert_allclose(v, o[k], rtol=0, atol=max(tol, 4 * floor[k]))
    w1, w2, w3, w4 = (w.float().cuda() for w in weights)
    ((cp * w1).sum() + (cn * w2).sum() + (sc * w3).sum() + (Rg * w4).sum()).backward()
    go, gg = o["grad"], hpg.grad.cpu().numpy()
    nrm = np.linalg.norm(gg - go) / np.linalg.norm(go)
    print(f"{name} backward: kernel norm-wise {nrm:.3g}, max abs {np.abs(gg - go).max():.3g}; fp32 oracle floor "
          f"{floor.get('grad_norm', 0.0):.3g}, {floor['grad']:.3g}")
    assert nrm < max(1e-4, 4 * floor.get("grad_norm", 0.0))
    assert (np.abs(gg - go) <= np.maximum(2e-4 + 2e-3 * np.abs(go), 4 * floor["grad"])).all()


# (topology, contacts, the gradient inputs handed over, fp32-oracle floor)
_NO_SPHERES = tuple(k for k in fkb.GRAD_INPUTS if k != "g_spheres")
BACKWARD_CASES = {"chain64": (64, fkb.GRAD_INPUTS, True), "star63": (12, fkb.GRAD_INPUTS, False),
                  "comb43": (12, fkb.GRAD_INPUTS, False), "coupled12": (12, fkb.GRAD_INPUTS, False),
                  "coupled12_dense": (12, fkb.GRAD_INPUTS, False), "nospheres": (12, _NO_SPHERES, False)}


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_fk_backward_on_synthetic_hands(gq, hands, name):
    """The seven-input check of test_gpu_fk_backward_block.py with the energy and accept tail (fkb.check), B = 4.  chain64 with
    n = 64: n + S = 320 items exactly, five passes of the item loop, and the fp32-oracle floor.  Measured on the MI355X for
    chain64: kernel 2.3e-7 norm-wise, 1.8e-5 max abs (gradients up to 73); fp32 oracle 2.3e-7 and 2.2e-5 -- at the floor, and
    inside the fixed tolerances.  star63 (6.9e-8 norm-wise, 1.4e-6 max abs) and the others hold the fixed tolerances; the
    floor rule is not applied to them."""
    spec, hand = hands(name)
    n, present, floor = BACKWARD_CASES[name]
    if name == "chain64":
        assert n + spec.n_spheres == 320
    _, out, _ = fkb.check(gq.C, spec, hand, 4, n, 80, present=present, tail=True, joint_scale=sh.joint_scale(spec), fp32_floor=floor)
    assert 0 < out["accept"].sum() < 4, "the accept step must go both ways"
    acc = out["accept"].astype(bool)
    np.testing.assert_array_equal(out["grad"][acc], out["grad_pose"][acc])  # the merged state is the new gradient, D up to 73


@pytest.mark.parametrize("name", ["chain64", "star63"])
def test_fk_backward_wave_kernel_bits_equal_the_block_kernel(gq, hands, name):
    """More than 512 rows go to gq_fk_backward_wave_kernel (lane j = node j, all 64 lanes live here).  "Same bits either way":
    the B = 4 inputs tiled to 516 rows give, row for row, the bits of the four-wavefront block kernel."""
    spec, hand = hands(name)
    n = 64 if name == "chain64" else 12
    inp = fkb.make_inputs(spec, 4, n, 90, sh.joint_scale(spec))
    inp.update(fkb.forward_state(gq.C, hand, inp))
    ref = fkb.run_backward(gq.C, hand, inp)
    reps = 129
    tile = lambda k, v: np.tile(v, (1, reps)) if k == "terms_old" else np.tile(v, (reps,) + (1,) * (v.ndim - 1))
    out = fkb.run_backward(gq.C, hand, {k: tile(k, v) for k, v in inp.items()})
    assert out["grad_pose"].shape[0] == 516 > 512
    assert np.isfinite(ref["grad_pose"]).all() and 0 < ref["accept"].sum() < 4
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k in ("grad_pose", "e_dis", "e_joints", "total", "accept"):
        want = np.tile(ref[k], (reps,) + (1,) * (ref[k].ndim - 1))
        assert out[k].dtype == want.dtype and np.array_equal(bits(out[k]), bits(want)), f"{name}: {k} differs between the kernels"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. explicit Jacobians
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain64", "star63", "coupled12"])
def test_explicit_jacobians_on_synthetic_hands(gq, hands, name):
    """test_gpu_export.py::test_explicit_jacobians on the synthetic hands, B = 3, n = 12: link and contact Jacobians against the
    oracle's analytic form, the contact form against autograd through the oracle FK, and against the FK backward (the
    transposed form).  2e-6 absolute and 1e-4 on the norm; chain64 takes the fp32-oracle floor.  Measured on the MI355X for
    chain64: link and contact Jacobian 5.6e-7 max abs (fp32 oracle 5.2e-7 / 4.6e-7), against the FK backward 7.9e-8 norm-wise
    (fp32 oracle 2.1e-7), contact Jacobian backward 3.6e-7 norm-wise (fp32 oracle 3.3e-7): inside the fixed tolerances.
    star63: 1.4e-7 / 9.7e-8 / 4.6e-8 / 9.6e-8 with the fixed tolerances."""
    spec, hand = hands(name)
    B, n = 3, 12
    inp = fkb.make_inputs(spec, B, n, 95, sh.joint_scale(spec))
    hp, idx = torch.tensor(inp["hand_pose"]), torch.tensor(inp["idx"])
    th = hp[:, 9:].double()
    Jl_o, Jc_o = oexp.link_jacobian(spec, th), oexp.contact_jacobian(spec, th, idx)
    w = torch.randn(B, n, 3, generator=torch.Generator().manual_seed(7))
    R = okin.special_gramschmidt(hp[:, 3:9].double())
    wh = (R.transpose(1, 2).unsqueeze(1) @ w.double().unsqueeze(-1)).squeeze(-1)  # R^T w
    cross = lambda Jc: torch.einsum("bnkj,bnk->bj", Jc.double(), wh)
    fl = fc = fx = 0.0
    if name == "chain64":
        Jc32 = oexp.contact_jacobian(spec, th.float(), idx)
        fl = float((oexp.link_jacobian(spec, th.float()).double() - Jl_o).abs().max())
        fc = float((Jc32.double() - Jc_o).abs().max())
        fx = float((cross(Jc32) - cross(Jc_o)).norm() / cross(Jc_o).norm())
    hpg = hp.cuda().requires_grad_()
    Rg, LT, cp, _, _, ws = gq.ops.fk_contacts(hpg, idx.cuda(), hand)
    Jl = gq.ops.link_jacobian(hand, LT, ws)
    Jc = gq.ops.contact_jacobian(hand, idx.cuda(), LT, ws)
    assert Jl.shape == (B, spec.n_links, 6, spec.n_dofs) and Jc.shape == (B, n, 3, spec.n_dofs)
    el, ec = float((Jl.cpu().double() - Jl_o).abs().max()), float((Jc.cpu().double() - Jc_o).abs().max())
    print(f"{name}: link Jacobian max abs {el:.3g} (fp32 oracle floor {fl:.3g}), contact Jacobian {ec:.3g} (floor {fc:.3g})")
    np.testing.assert_allclose(Jl.cpu().numpy(), Jl_o.numpy(), rtol=0, atol=max(2e-6, 4 * fl))
    np.testing.assert_allclose(Jc.cpu().numpy(), Jc_o.numpy(), rtol=0, atol=max(2e-6, 4 * fc))
    Ja = torch.autograd.functional.jacobian(lambda t: oexp.contact_points_hand_frame(spec, t, idx).sum(0), th)  # rows are independent
    np.testing.assert_allclose(Jc.cpu().numpy(), Ja.permute(2, 0, 1, 3).numpy(), rtol=0, atol=max(2e-6, 4 * fc))
    (cp * w.cuda()).sum().backward()
    g_explicit, g_bwd = cross(Jc.cpu()), hpg.grad[:, 9:].cpu().double()
    ex = float((g_explicit - g_bwd).norm() / g_bwd.norm())
    print(f"{name}: explicit Jacobian against the FK backward, norm-wise {ex:.3g} (fp32 oracle floor {fx:.3g})")
    assert ex <= max(1e-4, 4 * fx)
    assert float((g_bwd - cross(Jc_o)).norm() / cross(Jc_o).norm()) <= max(1e-4, 4 * fx)
    # the closed-form kinematic Hessian (gq_contact_jacobian_backward, the same J / L exposure): d sum(G . Jc) / d theta for a
    # random G against autograd through the oracle's analytic Jacobian.  1e-4 on the norm, the bound of the FK backward: both
    # are fp32 sums of triple products of unit axes and lever arms along the path of a contact
    G = torch.randn(B, n, 3, spec.n_dofs, generator=torch.Generator().manual_seed(8))

    def hessian_product(dtype):
        t = th.to(dtype).clone().requires_grad_()
        (oexp.contact_jacobian(spec, t, idx) * G.to(dtype)).sum().backward()
        return t.grad.double()

    gh_o = hessian_product(torch.float64)
    fh = float((hessian_product(torch.float32) - gh_o).norm() / gh_o.norm()) if name == "chain64" else 0.0
    g_th = torch.full((B, spec.n_dofs), float("nan"), device="cuda")
    C = gq.C
    C.call("gq_contact_jacobian_backward", hand.handle, C.i64(idx.cuda()), B, n, C.f32(LT.detach().contiguous()), C.f32(G.cuda()),
           C.f32(g_th), C.ptr(ws), ws.numel(), C.stream_ptr())
    eh = float((g_th.cpu().double() - gh_o).norm() / gh_o.norm())
    print(f"{name}: contact Jacobian backward, norm-wise {eh:.3g} (fp32 oracle floor {fh:.3g})")
    assert gh_o.norm() > 0 and eh <= max(1e-4, 4 * fh)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. refusals: ordinary error returns of the host-side argument checks, nothing is launched
# ---------------------------------------------------------------------------------------------------------------------------
def _tables(J=3, L=3, C=4, S=4):
    """Valid tables of a small chain, sized as asked (the checks under test look at sizes and orderings only)."""
    eye = np.tile(np.eye(4, dtype=np.float32)[:3][None], (max(J, L), 1, 1))
    return dict(n_dofs=J, n_links=L, n_cand=C, n_spheres=S, node_parent=np.arange(-1, J - 1, dtype=np.int32),
                node_type=np.ones(J, np.int32), node_pre=eye[:J].copy(), node_axis=np.tile(np.float32([0, 0, 1]), (J, 1)),
                link_node=np.clip(np.arange(L) - 1, -1, J - 1).astype(np.int32), link_offset=eye[:L].copy(),
                cand_pos=np.zeros((C, 3), np.float32), cand_nrm=np.tile(np.float32([0, 0, 1]), (C, 1)),
                cand_link=np.sort(np.arange(C) % L).astype(np.int32), sphere=np.full((S, 4), 0.01, np.float32),
                sphere_link=np.sort(np.arange(S) % L).astype(np.int32), joints_lower=np.full(J, -1, np.float32),
                joints_upper=np.full(J, 1, np.float32), n_actuated=0, coupling=None, coupling_offset=None)


def _try_create(gq, t):
    """gq_hand_create on the tables, the ctypes route of ops.HandHandle -> (status, message, handle value)."""
    d, keep = gq.C.HandDesc(), []
    for k, v in t.items():
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            keep.append(v)
            setattr(d, k, v.ctypes.data_as(ctypes.c_void_p))
        else:
            setattr(d, k, v)
    lib, h = gq.C.lib(), ctypes.c_void_p(0)
    rc = lib.gq_hand_create(ctypes.byref(d), ctypes.byref(h))
    msg = lib.gq_last_error() if rc else b""
    if rc == 0:
        lib.gq_hand_destroy(h)
    return rc, (msg or b"").decode(), h.value


def _decreasing_sphere_link(t):
    t["sphere_link"][-1] = 0


def _parent_not_before(t):
    t["node_parent"][1] = 1


def _cand_link_out_of_range(t):
    t["cand_link"][-1] = t["n_links"]


def _actuated_without_matrix(t):
    t["n_actuated"] = 2


REFUSALS = {"65 tree joints": (dict(J=65), None, "bad sizes J=65"), "65 links": (dict(L=65), None, "bad sizes J=3 L=65"),
            "257 spheres": (dict(S=257), None, "S=257"),
            "sphere_link decreases": ({}, _decreasing_sphere_link, "sphere_link must be sorted"),
            "node_parent[j] >= j": ({}, _parent_not_before, "node_parent must be topologically sorted"),
            "cand_link out of range": ({}, _cand_link_out_of_range, "cand_link out of range"),
            "n_actuated without coupling": ({}, _actuated_without_matrix, "n_actuated without a coupling matrix")}


def test_hand_create_accepts_the_valid_tables(gq):
    assert _try_create(gq, _tables())[0] == 0
    assert _try_create(gq, _tables(J=64, L=64, S=256))[0] == 0, "the declared limits themselves are accepted"


@pytest.mark.parametrize("case", list(REFUSALS))
def test_hand_create_refuses(gq, case):
    sizes, spoil, message = REFUSALS[case]
    t = _tables(**sizes)
    if spoil:
        spoil(t)
    rc, msg, handle = _try_create(gq, t)
    assert rc != 0 and message in msg and not handle, (rc, msg, handle)


def test_fk_backward_refuses_more_than_320_items(gq, hands):
    """chain64 with n = 65: n + S = 321.  The launcher refuses before it launches; grad_pose keeps its NaN sentinel."""
    spec, hand = hands("chain64")
    B, n = 2, 65
    hp, idx = torch.zeros(B, 9 + spec.n_dofs, device="cuda"), torch.zeros(B, n, dtype=torch.int64, device="cuda")
    Rg, LT, g = torch.zeros(B, 9, device="cuda"), torch.zeros(B, spec.n_links, 12, device="cuda"), torch.zeros(B, n, 3, device="cuda")
    gp = torch.full((B, 9 + spec.n_dofs), float("nan"), device="cuda")
    ws, nb = hand.fk_ws(B, hp.device)
    C = gq.C
    with pytest.raises(RuntimeError, match="n_contact \\+ n_spheres = 321 exceeds 320"):
        C.call("gq_fk_backward", hand.handle, C.f32(hp), C.i64(idx), B, n, C.f32(Rg), C.f32(LT), C.f32(g), None, None, None, None,
               None, None, C.f32(gp), None, None, C.ptr(ws), nb, C.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(gp).all()
