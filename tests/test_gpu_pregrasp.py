"""GPU tests of the pre-grasp term (E_pregrasp: the OPENED hand along the approach corridor, the grasp pose included): the fused
launch (opened kinematics, stations and joint gradient in one kernel) against the contract written in torch fp64
(tests/_pregrasp_oracle.py) at the shapes, station counts, openings and tree shapes at which the kernel can go wrong; its joint
columns against the composed route of existing launches; closed forms; the C entry's upstream / accumulate / reproducibility /
NaN / stack rules; and the stepper's pre-grasp mode (evaluation, iterations against the class surface, hipGraph replay, grids
overwritten in place).

Bounds: values rtol 1e-5 / atol 1e-6, gradients norm-wise 1e-4 over the whole (B, D) gradient, energies against
the class surface 3e-4.  Guards, caps and the seeded search: tests/_pregrasp_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _pregrasp_cases as pc  # noqa: E402
import _pregrasp_oracle as po  # noqa: E402
import _scene_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gq(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    pc.set_synthetic_root(tmp_path_factory.mktemp("synthetic_hands"))
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


@functools.lru_cache(maxsize=None)
def _hand(name):
    from graspqp_amd import ops

    return ops.HandHandle(pc.spec_of(name))


def _q(name):
    return torch.tensor(pc.open_joints(pc.spec_of(name))).cuda()


def _state(gq, hand, hp32):
    hpg = hp32.clone().cuda().requires_grad_()
    idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
    return hpg, idx, Rg, LT, ws


def _op(gq, hand, samples, hp32, scene, axis, D, K, opening, margin, open_joints=None, scale=3.0):
    """The op on the GPU: (E_pregrasp, d (scale E_pregrasp) / d hand_pose) as numpy."""
    hpg, idx, Rg, LT, ws = _state(gq, hand, hp32)
    e = gq.ops.pregrasp_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, axis, D, K, opening, open_joints, margin)
    (scale * e).sum().backward()
    torch.cuda.synchronize()
    return e.detach().cpu().numpy(), hpg.grad.cpu().numpy()


def _composed(gq, hand, samples, hp32, q, scene, axis, D, K, opening, margin, scale=3.0):
    """The composed route of existing launches on the same inputs: fk_contacts at the opened pose, scene_terms (station 0) +
    approach_terms (stations 1..K) there with autograd, the chain rule by (1 - alpha) through the opened pose."""
    hpg = hp32.clone().cuda().requires_grad_()
    opened = torch.cat([hpg[:, :9], (1.0 - opening) * hpg[:, 9:] + opening * q[None]], 1)
    idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(opened.detach(), idx, hand)
    e = gq.ops.scene_terms(opened, hand, samples, idx, Rg, LT, ws, scene, margin)
    if K > 0:
        e = e + K * gq.ops.approach_terms(opened, hand, samples, idx, Rg, LT, ws, scene, axis, D, K, margin)
    e = e * (1.0 / (K + 1))
    (scale * e).sum().backward()
    torch.cuda.synchronize()
    return e.detach().cpu().numpy(), hpg.grad.cpu().numpy()


def _assert_matches(got, ref, tag, factor=1.0, cols=None):
    e, g = got
    re_, rg = ref
    whole = np.linalg.norm(rg)
    if cols is not None:
        g, rg = g[:, cols], rg[:, cols]
    gerr = np.linalg.norm(g - rg) / max(whole, 1e-300)
    print(f"[{tag}] E_pregrasp max abs err {np.abs(e - re_).max():.3e} (max {np.abs(re_).max():.3e}, max rel "
          f"{(np.abs(e - re_) / np.maximum(np.abs(re_), 1e-30)).max():.3e}), grad err / whole gradient norm {gerr:.3e}")
    np.testing.assert_allclose(e, re_, rtol=factor * 1e-5, atol=factor * 1e-6, err_msg=f"{tag} E_pregrasp")
    assert np.linalg.norm(g - rg) <= factor * 1e-4 * whole, tag


def _case(gq, row):
    name, Ns, B, K, kind, opening, margin = row
    spec, hand = pc.spec_of(name), _hand(name)
    pts, lnk = pc.samples(name, Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns == len(pts)
    pc.assert_caps(Ns, B, K, kind)
    D = pc.corridor(K)
    hp, ref = pc.guarded(name, Ns, B, K, D, kind, opening, margin)
    tag = f"{name} Ns={Ns} B={B} K={K} D={D} {kind} opening={opening} margin={margin}"
    pc.assert_guards(ref, margin, tag, Ns, B, K, kind == "random", opening)
    return spec, hand, samples, D, hp, ref, tag


ALL = pc.TABLE + pc.TABLE_SYNTHETIC
IDS = ["-".join(str(v) for v in row) for row in ALL]


# ---------------------------------------------------------------------------------------------------------------
# 1. the op against the oracle: shapes, station counts, openings, tree shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ALL, ids=IDS)
def test_op_matches_the_oracle(gq, row):
    name, Ns, B, K, kind, opening, margin = row
    spec, hand, samples, D, hp, ref, tag = _case(gq, row)
    scene = pc.field(kind).scene(gq)
    got = _op(gq, hand, samples, hp, scene, spec.grasp_axis, D, K, opening, margin)
    _assert_matches(got, (ref["E"], ref["grad"]), tag)
    if opening == 1.0:  # the opened hand no longer depends on the joints
        assert (got[1][:, 9:] == 0).all() and (ref["grad"][:, 9:] == 0).all()
    else:
        assert np.abs(got[1][:, 9:]).max() > 0
    if opening == 0.0:  # the opened hand is the hand: station 0 is E_scene, stations 1..K are E_approach, on the same grid
        hpg, idx, Rg, LT, ws = _state(gq, hand, hp)
        es = gq.ops.scene_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, margin)
        ea = gq.ops.approach_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, spec.grasp_axis, D, K, margin)
        e = (es + K * ea) * (1.0 / (K + 1))
        (3.0 * e).sum().backward()
        torch.cuda.synchronize()
        # both sides round on their own: 2 x the bounds
        _assert_matches(got, (e.detach().cpu().numpy(), hpg.grad.cpu().numpy()), tag + " vs scene_terms + approach_terms", factor=2.0)


BIG_B, BIG_K, BIG_OPENING, BIG_MARGIN = 3, 2, 0.5, 0.01  # more than 512 samples: 577 = 10 chunks, 1100 = 18


def _tail_active(ref):
    """Samples at indices >= 512 (a wavefront's later chunks) with an active station."""
    return int(ref["active"][:, :, 512:].any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def _big_samples(Ns):
    pts, lnk = meshes.hand_surface_samples(get_hand_spec("allegro"), Ns)
    assert len(pts) == Ns and (np.diff(lnk) >= 0).all()  # they come by link: the order of the launch
    return pts, lnk


def _big_guarded(pts, lnk):
    """The seeded guard loop of ``pc.guarded`` on the multilinear field for samples of one's own, with 5 active samples beyond
    index 511."""
    spec = pc.spec_of("allegro")
    for seed in range(100 * BIG_B + len(pts), 100 * BIG_B + len(pts) + 200):
        hp = pc.pose(spec, BIG_B, seed)
        ref = po.e_pregrasp(spec, pts, lnk, hp.double(), pc.open_joints(spec), BIG_OPENING, pc.field("multilinear"), BIG_MARGIN,
                            pc.corridor(BIG_K), BIG_K)
        if pc.conditions(ref, BIG_MARGIN, len(pts), BIG_B, False, BIG_OPENING) and _tail_active(ref) >= 5:
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


@pytest.mark.parametrize("Ns", [577, 1100])
def test_more_than_512_samples_match_the_oracle(gq, Ns):
    """A wavefront's second and third trip through the chunk loop, K = 2 (three stations), opening 0.5.  The oracle has 195
    samples at indices >= 512 with an active station at Ns = 577 (every one of the 3 x 65) and 1204 at Ns = 1100; all station points
    lie inside the volume."""
    spec, hand = pc.spec_of("allegro"), _hand("allegro")
    pts, lnk = _big_samples(Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns and np.array_equal(samples.link.cpu().numpy(), lnk)
    hp, ref = _big_guarded(pts, lnk)
    D = pc.corridor(BIG_K)
    tag = f"allegro Ns={Ns} B={BIG_B} K={BIG_K} D={D} multilinear opening={BIG_OPENING} margin={BIG_MARGIN}"
    pc.assert_guards(ref, BIG_MARGIN, tag, Ns, BIG_B, BIG_K, False, BIG_OPENING)
    print(f"[{tag}] samples at indices >= 512 with an active station: {_tail_active(ref)}")
    assert _tail_active(ref) >= 5 and ref["inside"].all()
    got = _op(gq, hand, samples, hp, pc.field("multilinear").scene(gq), spec.grasp_axis, D, BIG_K, BIG_OPENING, BIG_MARGIN)
    _assert_matches(got, (ref["E"], ref["grad"]), tag)


def test_second_chunk_run_to_run_and_sample_order(gq):
    """Ns = 577 through the C entry: bitwise run to run; the samples by link against the same samples shuffled, within the
    bounds of ``_assert_matches`` (the order of the samples moves the last bits only)."""
    spec, hand = pc.spec_of("allegro"), _hand("allegro")
    pts, lnk = _big_samples(577)
    hp, ref = _big_guarded(pts, lnk)
    scene = pc.field("multilinear").scene(gq)
    grids = gq.ops._pregrasp_grids(scene.values, scene.origin, scene.voxel)
    B, D, q = BIG_B, pc.corridor(BIG_K), _q("allegro")
    hp = hp.cuda()
    Rg = gq.ops.fk_contacts(hp, torch.zeros(B, 1, dtype=torch.long, device="cuda"), hand)[0].contiguous()

    def run(p, l):
        p, l = torch.tensor(p).cuda(), torch.tensor(l.astype(np.int32)).cuda()
        g_theta, gRt, e = torch.empty(B, spec.n_dofs, device="cuda"), torch.empty(B, 12, device="cuda"), torch.empty(B, device="cuda")
        gq.ops._pregrasp_call(hand, grids, BIG_MARGIN, D, BIG_K, BIG_OPENING, q, hp, p, l, Rg, spec.grasp_axis, None, 1.5, e, 0,
                              g_theta, gRt)
        torch.cuda.synchronize()
        return g_theta, gRt, e

    by_link, again = run(pts, lnk), run(pts, lnk)
    for a, b in zip(by_link, again):
        assert torch.equal(a, b)
    np.testing.assert_allclose(by_link[2].cpu().numpy(), ref["E"], rtol=1e-5, atol=1e-6)
    assert by_link[0].abs().max() > 0 and by_link[1].abs().max() > 0
    perm = np.random.default_rng(577).permutation(577)
    assert not (np.diff(lnk[perm]) >= 0).all()
    shuffled = run(pts[perm], lnk[perm])
    grad = lambda r: np.concatenate([r[0].cpu().numpy(), r[1].cpu().numpy()], 1)
    _assert_matches((shuffled[2].cpu().numpy(), grad(shuffled)), (by_link[2].cpu().numpy(), grad(by_link)), "Ns=577 shuffled vs by link")


# ---------------------------------------------------------------------------------------------------------------
# 2. the joint columns alone: the fused launch against the composed route of existing launches
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ALL, ids=IDS)
def test_joint_columns_are_as_good_as_the_composed_route(gq, row):
    """Both routes are held to the fp64 oracle on the joint columns.  The fused launch's error may be at most twice the composed
    route's own (one more rounding order of the same fp32 sums: the margin of tests/_parity.py), plus a floor of 1e-6 of the whole
    gradient's norm."""
    name, Ns, B, K, kind, opening, margin = row
    spec, hand, samples, D, hp, ref, tag = _case(gq, row)
    scene = pc.field(kind).scene(gq)
    _, g_fused = _op(gq, hand, samples, hp, scene, spec.grasp_axis, D, K, opening, margin)
    _, g_comp = _composed(gq, hand, samples, hp, _q(name), scene, spec.grasp_axis, D, K, opening, margin)
    whole = np.linalg.norm(ref["grad"])
    err_fused = np.linalg.norm(g_fused[:, 9:] - ref["grad"][:, 9:])
    err_comp = np.linalg.norm(g_comp[:, 9:] - ref["grad"][:, 9:])
    print(f"[{tag}] joint columns vs oracle: fused {err_fused:.3e}, composed route {err_comp:.3e} (whole gradient norm {whole:.3e}, "
          f"joint columns {np.linalg.norm(ref['grad'][:, 9:]):.3e})")
    assert err_fused <= 2.0 * err_comp + 1e-6 * whole, tag


# ---------------------------------------------------------------------------------------------------------------
# 3. closed forms
# ---------------------------------------------------------------------------------------------------------------
def test_affine_field_closed_form(gq):
    """phi(x_w^k) = phi(x_w) - d_k n . (R a) at the opened hand."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, K, D, opening, margin = 128, 3, 4, 0.08, 0.5, 0.01
    pts, lnk = pc.samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp, ref = pc.guarded("allegro", Ns, B, K, D, "affine", opening, margin)
    F = pc.field("affine")
    pc.assert_guards(ref, margin, "affine", Ns, B, K, False, opening)
    assert ref["inside"].all()
    q = pc.open_joints(spec)
    at_pose = so.e_scene(spec, pts, lnk, po.opened_pose(hp.double(), q, opening), F, margin)  # phi at the opened, unshifted samples
    assert at_pose["inside"].all()
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(B, 1, dtype=torch.long))
    slope = (oh.global_rotation @ oh.grasp_axis).numpy() @ np.array([0.36, -0.48, 0.8])  # (B): n . (R a)
    closed = sum(np.maximum(margin - (at_pose["phi"] - (D * k / K) * slope[:, None]), 0.0).sum(-1) for k in range(K + 1)) / (K + 1)
    np.testing.assert_allclose(ref["E"], closed, rtol=1e-9, atol=1e-12)  # the oracle agrees with the closed form
    got = _op(gq, hand, samples, hp, F.scene(gq), spec.grasp_axis, D, K, opening, margin)
    _assert_matches(got, (closed, ref["grad"]), "affine closed form")


def test_no_station_equals_scene_terms_at_the_opened_pose(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, D, opening, margin = 512, 3, 0.08, 0.25, 0.01
    pts, lnk = pc.samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp, ref = pc.guarded("allegro", Ns, B, 0, D, "multilinear", opening, margin)
    pc.assert_guards(ref, margin, "K=0", Ns, B, 0, False, opening)
    scene = pc.field("multilinear").scene(gq)
    got = _op(gq, hand, samples, hp, scene, spec.grasp_axis, D, 0, opening, margin)
    opened = po.opened_pose(hp.double(), pc.open_joints(spec), opening).float()
    hpg, idx, Rg, LT, ws = _state(gq, hand, opened)
    es = gq.ops.scene_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, margin)
    (3.0 * es).sum().backward()
    torch.cuda.synchronize()
    g = hpg.grad.cpu().numpy().copy()
    g[:, 9:] *= 1.0 - opening  # the chain rule through the opened pose
    _assert_matches(got, (es.detach().cpu().numpy(), g), "K=0 vs scene_terms at the opened pose", factor=2.0)
    _assert_matches(got, (ref["E"], ref["grad"]), "K=0 vs oracle")


def test_last_stations_outside_the_volume(gq):
    """A 30^3 grid of 1 cm around the hand, a corridor of 40 cm in 4 steps: the opened hand leaves the volume on its way."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, K, D, opening, margin = 64, 1, 4, 0.40, 0.5, 0.01
    pts, lnk = pc.samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    F = so.random_field((30, 30, 30), (-0.15137, -0.14291, -0.15173), 0.01, 5)
    q = pc.open_joints(spec)
    for seed in range(200):
        hp = pc.pose(spec, B, seed, spread=0.02)
        ref = po.e_pregrasp(spec, pts, lnk, hp.double(), q, opening, F, margin, D, K)
        face, near = po.guards(ref, margin)
        ins = ref["inside"].sum(axis=(0, 2))
        if face >= po.FACE and near >= po.NEAR and ins[0] >= 10 and ins[-1] == 0 and ref["active"].sum() >= 5 and pc.joint_share(ref) >= 5e-3:
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    print(f"[leaving] points inside per station {ins.tolist()}, active per station {ref['active'].sum(axis=(0, 2)).tolist()}")
    assert B * Ns * (K + 1) <= 512 and face >= po.FACE and near >= po.NEAR
    # an independent test of the box: the points outside contribute exactly nothing
    lo = np.asarray(F.origin, dtype=np.float64)
    hi = lo + float(F.voxel) * (np.array(F.shape) - 1)
    assert np.array_equal(((ref["x"] >= lo) & (ref["x"] <= hi)).all(-1), ref["inside"])
    assert not ref["active"][:, -1].any() and ref["active"][:, 0].any()
    _assert_matches(_op(gq, hand, samples, hp, F.scene(gq), spec.grasp_axis, D, K, opening, margin), (ref["E"], ref["grad"]), "leaving")


def test_everything_outside_the_volume(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = pc.samples("allegro", 512)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp = pc.pose(spec, 3, 1)
    hp[:, 0] += 10.0
    e, g = _op(gq, hand, samples, hp, pc.field("random").scene(gq), spec.grasp_axis, 0.08, 4, 0.5, 0.01)
    assert (e == 0).all() and (g == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. the C entry itself
# ---------------------------------------------------------------------------------------------------------------
def _entry(gq, name="allegro", Ns=128, B=6, K=3, opening=0.5, margin=0.01, kind="multilinear"):
    spec, hand = pc.spec_of(name), _hand(name)
    pts, lnk = pc.samples(name, Ns)
    keep = lnk != 3  # a link without samples, Ns not a multiple of 64
    samples = gq.ops.SurfaceSamples(hand, pts[keep], lnk[keep])
    assert 64 < samples.Ns < 128
    D, F, q = pc.corridor(K), pc.field(kind), pc.open_joints(spec)
    for seed in range(700, 900):
        hp = pc.pose(spec, B, seed)
        ref = po.e_pregrasp(spec, pts[keep], lnk[keep], hp.double(), q, opening, F, margin, D, K)
        if pc.conditions(ref, margin, samples.Ns, B, False, opening):
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    hp = hp.cuda()
    Rg = gq.ops.fk_contacts(hp, torch.zeros(B, 1, dtype=torch.long, device="cuda"), hand)[0].contiguous()
    J = spec.n_dofs

    def run(grids, up, w, accumulate, bufs=None, pose=hp, want=(True, True, True), rows=slice(None)):
        pose, R = pose[rows].contiguous(), Rg[rows].contiguous()
        n = pose.shape[0]
        g_theta, gRt = bufs or (torch.empty(n, J, device="cuda"), torch.empty(n, 12, device="cuda"))
        e = torch.empty(n, device="cuda")
        gq.ops._pregrasp_call(hand, grids, margin, D, K, opening, torch.tensor(q).cuda(), pose, samples.points, samples.link, R,
                              spec.grasp_axis, up, w, e if want[0] else None, accumulate, g_theta if want[1] else None,
                              gRt if want[2] else None)  # raises if the launch returns an error
        torch.cuda.synchronize()
        return g_theta, gRt, e

    return spec, hand, samples, F, ref, hp, run


def test_upstream_vectors_accumulate_bits_null_outputs_and_reproducibility(gq):
    spec, hand, samples, F, ref, hp, run = _entry(gq)
    B = hp.shape[0]
    scene = F.scene(gq)
    grids = gq.ops._pregrasp_grids(scene.values, scene.origin, scene.voxel)
    one = run(grids, None, 1.0, 0)
    again = run(grids, None, 1.0, 0)
    for a, b in zip(one, again):
        assert torch.equal(a, b)  # run to run
    np.testing.assert_allclose(one[2].cpu().numpy(), ref["E"], rtol=1e-5, atol=1e-6)
    assert one[0].abs().max() > 0 and one[1].abs().max() > 0
    # a non-uniform upstream per row == the per-row scaled result (up * 1/(K+1) rounds once more than the scalar)
    uw = torch.linspace(0.5, 3.0, B, device="cuda")
    vec = run(grids, uw, 0.0, 0)
    for got, unit in ((vec[0], one[0]), (vec[1], one[1])):
        want = unit * uw.view(B, 1)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=6 * EPS32, atol=6 * EPS32 * float(want.abs().max()))
    assert torch.equal(vec[2], one[2])  # the energy is unweighted
    # accumulate: bit 0 adds to gRt, bit 1 to g_theta -- pre-fill + the overwriting launch's value, bit for bit
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in (tuple(one[0].shape), (B, 12))]
    for acc_bits in (1, 2, 3):
        acc = run(grids, uw, 0.0, acc_bits, [p.clone() for p in pre])
        assert torch.equal(acc[0], pre[0] + vec[0] if acc_bits & 2 else vec[0]), acc_bits
        assert torch.equal(acc[1], pre[1] + vec[1] if acc_bits & 1 else vec[1]), acc_bits
        assert torch.equal(acc[2], vec[2])  # the energy is a value: overwritten
    # NULL outputs: each of the three alone gives the bits of the full launch, the others untouched
    for k in range(3):
        want = [i == k for i in range(3)]
        bufs = [torch.full_like(one[0], 7.0), torch.full_like(one[1], 7.0)]
        out = run(grids, None, 1.0, 0, bufs, want=want)
        if k == 0:
            assert torch.equal(out[2], one[2]) and (bufs[0] == 7.0).all() and (bufs[1] == 7.0).all()
        if k == 1:
            assert torch.equal(out[0], one[0]) and (bufs[1] == 7.0).all()
        if k == 2:
            assert torch.equal(out[1], one[1]) and (bufs[0] == 7.0).all()


def test_nan_row_leaves_the_other_rows_untouched(gq):
    spec, hand, samples, F, ref, hp, run = _entry(gq, B=4)
    scene = F.scene(gq)
    grids = gq.ops._pregrasp_grids(scene.values, scene.origin, scene.voxel)
    good = run(grids, None, 1.0, 0)
    node = next(int(spec.link_node[int(l)]) for l in samples.link.tolist() if int(spec.link_node[int(l)]) >= 0)
    for col in (1, 9 + node):  # a NaN translation; a NaN joint that carries a sampled link (allegro: actuated joint = tree node)
        bad = hp.clone()
        bad[2, col] = float("nan")
        out = run(grids, None, 1.0, 0, pose=bad)
        keep = torch.tensor([0, 1, 3], device="cuda")
        assert torch.isnan(out[2][2]) and torch.isnan(out[1][2]).all() and torch.isnan(out[0][2]).any(), col
        assert torch.isfinite(good[2]).all() and (good[2] > 0).all()
        for a, b in zip(good, out):
            assert torch.equal(a[keep], b[keep]), col


def test_stack_of_grids_equals_single_grid_launches(gq):
    """A stack of 3 grids with rows_per_grid 2: bit for bit three single-grid launches on the row pairs."""
    spec, hand, samples, F, ref, hp, run = _entry(gq, B=6)
    fields = [F, so.multilinear(pc.G_SHAPE, pc.G_ORIGIN, pc.G_H, c=(-0.03, 0.4, -0.35, 0.7, 0.6, -0.5, 0.3, 1.2)),
              pc.field("random")]
    stack = gq.ops.SceneSDFSet(torch.stack([f.values for f in fields]).cuda(), [float(o) for o in F.origin], float(F.voxel))
    both = run(gq.ops._pregrasp_grids(stack.values, stack.origin, stack.voxel), None, 2.0, 0)
    seen = []
    for g, f in enumerate(fields):
        sc = f.scene(gq)
        single = run(gq.ops._pregrasp_grids(sc.values, sc.origin, sc.voxel), None, 2.0, 0, rows=slice(2 * g, 2 * g + 2))
        for a, b in zip(both, single):
            assert torch.equal(a[2 * g:2 * g + 2], b), g
        seen.append(single[2].clone())
    assert not torch.equal(seen[0], seen[1]) and (seen[2] > 0).all()  # the grids differ and every one is met
    # ... and through the op, with autograd
    idx = torch.zeros(6, 1, dtype=torch.long, device="cuda")
    hpg = hp.clone().requires_grad_()
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
    e = gq.ops.pregrasp_terms(hpg, hand, samples, idx, Rg, LT, ws, stack, spec.grasp_axis, pc.corridor(3), 3, 0.5, None, 0.01)
    assert torch.equal(e, both[2])
    e.sum().backward()
    assert torch.isfinite(hpg.grad).all() and hpg.grad[:, 9:].abs().max() > 0
    with pytest.raises(ValueError, match="pregrasp"):
        gq.ops.pregrasp_terms(hpg[:4], hand, samples, idx[:4], Rg[:4], LT[:4], ws, stack, spec.grasp_axis, 0.08, 3, 0.5, None, 0.01)


# ---------------------------------------------------------------------------------------------------------------
# 5. the stepper
# ---------------------------------------------------------------------------------------------------------------
S_SHAPE, S_ORIGIN, S_H = (100, 100, 100), (-0.5013, -0.4987, -0.5021), 0.01
PG = dict(pregrasp_distance=0.10, pregrasp_stations=4, pregrasp_opening=0.5)
AP = dict(approach_distance=0.10, approach_stations=4)
STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")
TT = {"E_prior": 2.0, "E_wall": 3.0}
BASE_NAMES = ["E_dis", "E_fc", "E_pen", "E_spen", "E_joints"]


@functools.lru_cache(maxsize=None)
def _wall(c=0.02):
    """A half-space through the workspace: a wall the hands of the fixtures reach into (that of tests/test_gpu_scene.py)."""
    return so.affine(S_SHAPE, S_ORIGIN, S_H, c=c)


def _stepper(gq, g, n_contact, hand=None, **kw):
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    return gq.stepper.GraspStepper(hand or _hand("allegro"), gq.ops.MeshSet(fvs), torch.tensor(sps), be, n_contact, **kw)


def _class_surface(gq, g, hp, idx, sm, scene, margin, pregrasp=None, corridor=None):
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    hm = HandModel(get_hand_spec("allegro"), "cuda")
    hm.set_surface_points(*sm)
    if scene is not None:
        hm.set_scene(scene, margin)
    if corridor is not None:
        hm.set_approach(*corridor)
    if pregrasp is not None:
        hm.set_pregrasp(**pregrasp)
    be, n_obj = int(g["batch_size_each"]), int(g["n_obj"])
    om = ObjectModel(batch_size_each=be, num_samples=g["obj0_surface_points"].shape[0])
    om.initialize_from_meshes([g[f"obj{i}_face_verts"] for i in range(n_obj)],
                              surface_points_list=[g[f"obj{i}_surface_points"] for i in range(n_obj)])
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    return hm, om


@pytest.mark.parametrize("tabletop,scene_on", [(False, False), (True, False), (False, True), (True, True)])
def test_zero_weight_is_the_stepper_without_the_term(gq, golden_dir, tabletop, scene_on):
    g = _load(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    w = dict(TT) if tabletop else {}
    base = dict(surface_samples=sm) if tabletop or scene_on else {}
    if scene_on:
        w["E_scene"] = 50.0
        base.update(scene=_wall().scene(gq), scene_margin=0.01)
    with_term = dict(base, weights=dict(w, E_pregrasp=0.0), pregrasp_distance=0.07, pregrasp_stations=5, pregrasp_margin=0.02,
                     pregrasp_opening=0.3, pregrasp_scene=_wall(-0.01).scene(gq), pregrasp_joints=[0.1] * 16)
    sts = [_stepper(gq, g, 4, **dict(base, weights=w or None)), _stepper(gq, g, 4, **with_term)]
    assert not sts[1].pregrasp_mode and sts[1].term_names == sts[0].term_names and "E_pregrasp" not in sts[1].term_names
    assert sts[1]._fuse_loop == sts[0]._fuse_loop == (not (tabletop or scene_on)) and sts[1].terms.shape == sts[0].terms.shape
    assert (sts[1].samples is None) == (sts[0].samples is None) and (sts[1].scene is None) == (not scene_on)
    for st in sts:
        st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
        for s in (1, 2, 3):
            st.step(draws=(f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")))
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(sts[0], k), getattr(sts[1], k)), k


@pytest.mark.parametrize("tabletop,scene_on,approach_on", [(False, False, False), (False, True, True), (True, True, False)])
def test_stepper_evaluate_in_pregrasp_mode(gq, golden_dir, tabletop, scene_on, approach_on):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    sm = (g["opt_surface_points"], g["opt_surface_link"])
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    idx = torch.tensor(g["contact_idx"]).cuda()
    F = _wall()
    scene, margin, w = F.scene(gq), 0.01, 20.0
    w0 = dict(TT) if tabletop else {}
    if scene_on:
        w0["E_scene"] = 50.0
    if approach_on:
        w0["E_approach"] = 10.0
    base = dict(surface_samples=sm, scene=scene, scene_margin=0.005, **AP)
    st0 = _stepper(gq, g, 4, **dict(base, weights=w0 or None))
    st1 = _stepper(gq, g, 4, **dict(base, weights=dict(w0, E_pregrasp=w), pregrasp_margin=margin, **PG))
    names = (BASE_NAMES + (["E_prior", "E_wall"] if tabletop else []) + (["E_scene"] if scene_on else []) +
             (["E_approach"] if approach_on else []) + ["E_pregrasp"])
    assert st1.pregrasp_mode and not st1._fuse_loop and st1.terms.shape == (len(names), hp.shape[0])
    assert st1.scene_mode == scene_on and st1.tabletop == tabletop and st1.approach_mode == approach_on and st1.pregrasp_margin == margin
    t0, tot0, g0 = st0.evaluate(hp, idx)
    t1, tot1, g1 = st1.evaluate(hp, idx)
    t1b, tot1b, g1b = st1.evaluate(hp, idx)  # g_theta is overwritten, not accumulated: a second evaluation gives the same bits
    torch.cuda.synchronize()
    assert torch.equal(g1, g1b) and torch.equal(tot1, tot1b)
    assert list(t1) == names and list(t0) == names[:-1] and st1.term_names[-1] == "E_pregrasp"
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    samples = gq.ops.SurfaceSamples(hand, *sm)
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    ep = gq.ops.pregrasp_terms(hp, hand, samples, idx, Rg, LT, ws, scene, spec.grasp_axis, PG["pregrasp_distance"],
                               PG["pregrasp_stations"], PG["pregrasp_opening"], None, margin)
    assert torch.equal(t1["E_pregrasp"], ep) and (ep > 0).any()
    d_tot = (tot1.double() - tot0.double()).cpu().numpy()
    want = (w * ep.double()).cpu().numpy()
    rel = np.abs(d_tot - want) / np.abs(tot1.double().cpu().numpy())
    print(f"[evaluate tabletop={tabletop} scene={scene_on} approach={approach_on}] total - parts rel err max {rel.max():.3e}")
    assert rel.max() <= 3e-4
    ref = po.e_pregrasp(spec, sm[0], sm[1], hp.double().cpu(), pc.open_joints(spec), PG["pregrasp_opening"], F, margin,
                        PG["pregrasp_distance"], PG["pregrasp_stations"], scale=w)
    assert po.guards(ref, margin)[1] >= po.NEAR and np.abs(ref["grad"][:, 9:]).max() > 0
    want_g = g0.double().cpu().numpy() + ref["grad"]
    gerr = np.linalg.norm(g1.double().cpu().numpy() - want_g) / np.linalg.norm(want_g)
    jerr = np.linalg.norm((g1 - g0).double().cpu().numpy()[:, 9:] - ref["grad"][:, 9:]) / np.linalg.norm(ref["grad"])
    print(f"[evaluate tabletop={tabletop} scene={scene_on} approach={approach_on}] grad vs sum of parts rel err {gerr:.3e}, joint "
          f"columns of the difference vs oracle {jerr:.3e}")
    assert gerr <= 1e-3  # the bound of tests/test_gpu_scene.py::test_stepper_evaluate_in_scene_mode for the same sum
    # the joint columns the launch hands to the FK backward as g_theta: the fused launch's own 1e-4, plus the rounding of the
    # difference of two fp32 gradients that each carry every term (a few eps of the whole gradient per summand)
    jabs = np.linalg.norm((g1 - g0).double().cpu().numpy()[:, 9:] - ref["grad"][:, 9:])
    assert jabs <= 1e-4 * np.linalg.norm(ref["grad"]) + 16 * EPS32 * float(g1.norm()), (jabs, np.linalg.norm(ref["grad"]))


def test_fused_launch_equals_the_class_surface(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    sm = (samples.points.cpu().numpy(), samples.link.cpu().numpy())
    scene, margin, D, K, opening = _wall().scene(gq), 0.01, 0.10, 4, 0.5
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    idx = torch.tensor(g["contact_idx"]).cuda()
    e_op, g_op = _op(gq, hand, samples, hp.cpu(), scene, spec.grasp_axis, D, K, opening, margin, scale=1.0)
    hm, om = _class_surface(gq, g, hp, idx, sm, scene, margin, dict(distance=D, stations=K, opening=opening))
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=BASE_NAMES + ["E_pregrasp"], svd_gain=0.1)
    e_cls = losses["E_pregrasp"].detach().cpu().numpy()
    assert (e_cls > 0).any()
    print(f"[fused vs class surface] E_pregrasp max abs diff {np.abs(e_op - e_cls).max():.3e} (max {e_cls.max():.3e})")
    np.testing.assert_allclose(e_op, e_cls, rtol=1e-5, atol=1e-6)
    losses["E_pregrasp"].sum().backward()
    g_cls = hm.hand_pose.grad.cpu().numpy()
    gerr = np.linalg.norm(g_cls - g_op) / np.linalg.norm(g_op)
    print(f"[class surface vs pregrasp_terms] grad rel diff {gerr:.3e}")
    assert gerr <= 1e-4 and np.abs(g_cls[:, 9:]).max() > 0


def test_pregrasp_iterations_match_the_class_surface(gq, golden_dir):
    """Five iterations (the third one re-initialises two rows), teacher-forced from the class-surface state: the loop of
    tests/test_gpu_approach.py::test_approach_iterations_match_the_class_surface with the pre-grasp term on top."""
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.optimizer import MalaStar
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    C = gq.C
    g = _load(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    samples = gq.ops.SurfaceSamples(_hand("allegro"), ge["opt_surface_points"], ge["opt_surface_link"])
    sm = (samples.points.cpu().numpy(), samples.link.cpu().numpy())
    be, n_obj = int(g["batch_size_each"]), int(g["n_obj"])
    B = be * n_obj
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    scene, margin = _wall().scene(gq), 0.01
    extra = {"E_scene": 50.0, "E_approach": 20.0, "E_pregrasp": 30.0}
    w = dict({"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}, **extra)
    st = _stepper(gq, g, 4, weights=extra, surface_samples=sm, scene=scene, scene_margin=margin, **AP, **PG)
    assert st.term_names[-3:] == ("E_scene", "E_approach", "E_pregrasp") and st.pregrasp_margin == margin
    hm, om = _class_surface(gq, g, f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda(), sm, scene, margin,
                            dict(distance=PG["pregrasp_distance"], stations=PG["pregrasp_stations"], opening=PG["pregrasp_opening"]),
                            (AP["approach_distance"], AP["approach_stations"]))
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})

    def total():
        losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=list(w), svd_gain=0.1)
        return sum(w[k] * losses[k] for k in w), losses

    opt = MalaStar(hm, switch_possibility=0.4, device="cuda", batch_size=be)
    energy, _ = total()
    energy.sum().backward()
    opt.zero_grad()
    energy = energy.detach().clone()
    st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
    np.testing.assert_allclose(st.energy.cpu().numpy(), energy.cpu().numpy(), rtol=3e-4)
    mask = torch.zeros(B, dtype=torch.bool)
    mask[[1, B - 2]] = True
    new_pose = f32("hand_pose0").roll(3, 0)
    new_idx = torch.tensor(g["contact_idx0"]).cuda().roll(3, 0)
    assert int(g["n_steps"]) >= 5
    for s in range(1, 6):
        grad = hm.hand_pose.grad
        st.hand_pose.copy_(hm.hand_pose.detach())
        st.contact_idx.copy_(hm.contact_point_indices)
        st.grad.copy_(torch.zeros_like(st.grad) if grad is None else grad)
        st.energy.copy_(energy)
        st.ema.copy_(opt.ema_grad_hand_pose)
        st.step_count.copy_(opt.step)
        terms_before = st.terms.clone()
        u_sw, n_ix = f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda()
        opt.try_step(draws=(u_sw, n_ix))
        eb = energy.view(-1, be)
        z = ((eb - eb.mean(-1, keepdim=True)) / eb.std(-1, keepdim=True)).view(-1)
        rm = None
        if s == 3:
            rm = mask.cuda()
            hm.set_parameters(new_pose.clone().requires_grad_(), new_idx, env_mask=rm)
            opt.reset_envs(rm)
        opt.zero_grad()
        new_energy, losses = total()
        new_energy.sum().backward()
        T = torch.empty(B, device="cuda")
        hpd, gd, ixd = hm.hand_pose.detach().contiguous(), hm.hand_pose.grad.contiguous(), hm.contact_point_indices.contiguous()
        ne, u0, zc = new_energy.detach().contiguous(), torch.zeros(B, device="cuda"), z.contiguous()
        g_new_cls = gd.clone()  # the gradient at the proposed pose, before the accept step merges
        e_t, p_t, i_t, g_t, a_t = energy.clone(), hpd.clone(), ixd.clone(), gd.clone(), torch.empty(B, dtype=torch.uint8, device="cuda")
        C.call("gq_mala_accept", C.f32(ne), C.f32(u0), C.f32(zc), C.u8(None), C.i64(opt.step), C.f32(hpd), C.i64(ixd), C.f32(gd), B,
               hpd.shape[1], 4, opt.starting_temperature, opt.temperature_decay, opt.annealing_period, C.f32(e_t), C.f32(p_t),
               C.i64(i_t), C.f32(g_t), C.u8(a_t), C.f32(T), 0, None, None, C.stream_ptr())
        p = torch.exp((energy - new_energy.detach()) / T)
        cands = [f32(f"s{s}_u_accept")] + [torch.rand(B, generator=torch.Generator().manual_seed(1000 * s + k)).cuda() for k in range(8)]
        u_ac = next(u for u in cands if bool(((u - p).abs() >= 1e-3).all()))
        with torch.no_grad():
            accept, T_cls = opt.accept_step(energy, new_energy, rm, z, 1.0, u_accept=u_ac)
        assert torch.allclose(T_cls, T)
        if s == 3:
            st.step_reset(mask, new_pose, new_idx, draws=(u_sw, n_ix, u_ac))
        else:
            st.step(draws=(u_sw, n_ix, u_ac))
        torch.cuda.synchronize()
        rel = ((st.total_new - new_energy.detach()).abs() / new_energy.detach().abs().clamp_min(1e-12)).cpu().numpy()
        print(f"[iteration {s}] total_new rel err max {rel.max():.3e}, E_pregrasp max {float(st.terms_new[7].max()):.4f}, "
              f"min margin {float((u_ac - p).abs().min()):.3e}, accepted {int(accept.sum())}/{B}")
        assert rel.max() < 3e-4, rel
        assert float(st.terms_new[7].max()) > 0, "no station point of the opened hand inside the wall in this iteration"
        for i, k in ((5, "E_scene"), (6, "E_approach"), (7, "E_pregrasp")):
            np.testing.assert_allclose(st.terms_new[i].cpu().numpy(), losses[k].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
        gerr = float((st.grad_new - g_new_cls).norm() / g_new_cls.norm())
        print(f"[iteration {s}] gradient of the total vs class surface rel diff {gerr:.3e}")
        assert gerr <= 1e-3
        assert st.accept.bool().tolist() == accept.tolist()
        if s == 3:
            assert accept[mask.cuda()].all()
        acc = st.accept.bool()
        assert torch.equal(st.terms[7][acc], st.terms_new[7][acc])
        assert torch.equal(st.terms[7][~acc], terms_before[7][~acc])
        np.testing.assert_allclose(st.energy.cpu().numpy(), energy.cpu().numpy(), rtol=3e-4)
        np.testing.assert_allclose(st.hand_pose.cpu().numpy(), hm.hand_pose.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
        assert torch.equal(st.contact_idx, hm.contact_point_indices)


def _graph_scene(B, n_obj=1):
    spec = get_hand_spec("allegro")
    fv = meshes.icosphere(2, 0.05)
    sp = torch.tensor(meshes.surface_points(fv, 256, oversample=4))[None].repeat(n_obj, 1, 1)
    n = 4
    gen = torch.Generator().manual_seed(B)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1) * 0.12
    hp = torch.cat([t, torch.randn(B, 6, generator=gen), torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=gen)], 1).cuda()
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda()
    draws = [(torch.rand(B, n, generator=gen).cuda(), torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda(),
              torch.rand(B, generator=gen).cuda()) for _ in range(3)]
    return fv, sp, n, hp, idx, draws


@pytest.mark.parametrize("B,mode,w_scene,w_approach,energy_type,optimizer",
                         [(8, "one grid", 50.0, 20.0, "graspqp", "mala_star"), (384, "graph branches", 50.0, 20.0, "graspqp", "mala_star"),
                          (8, "one grid", 0.0, 0.0, "graspqp", "mala_star"), (384, "graph branches", 0.0, 0.0, "graspqp", "mala_star"),
                          (8, "one grid", 50.0, 0.0, "dexgrasp", "dexgraspnet")])
def test_graph_replay_equals_eager_steps(gq, golden_dir, B, mode, w_scene, w_approach, energy_type, optimizer):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    weights = {"E_scene": w_scene, "E_approach": w_approach, "E_pregrasp": 30.0}
    out = []
    for graph in (False, True):
        st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights=weights, surface_samples=sm,
                                     scene=_wall().scene(gq), scene_margin=0.01, energy_type=energy_type, optimizer=optimizer, **AP, **PG)
        st.reset(hp, idx)
        assert st.term_names[-1] == "E_pregrasp" and float(st.terms[-1].max()) > 0
        assert len(st.term_names) == 6 + (w_scene > 0) + (w_approach > 0)
        if graph:
            st.capture()
            assert st.graph_mode == mode
        for d in draws:
            st.step(draws=d)
        torch.cuda.synchronize()
        out.append([getattr(st, k).clone() for k in STATE])
    for a, b, k in zip(out[0], out[1], STATE):
        assert torch.equal(a, b), k
    assert torch.isfinite(out[0][2]).all()


def test_cloud_object_and_run(gq, golden_dir):
    """An object given as an oriented point cloud, and ``run`` from the captured graph, in pre-grasp mode."""
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    B = 8
    fv, sp, n, hp, idx, _ = _graph_scene(B)
    pts = sp[0].numpy().astype(np.float32)
    nrm = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    st = gq.stepper.GraspStepper(hand, gq.ops.PointCloudSet([pts], [nrm]), sp, B, n, weights={"E_pregrasp": 30.0},
                                 surface_samples=sm, scene=_wall().scene(gq), scene_margin=0.01, **PG)
    assert st.cloud and st.pregrasp_mode and not st.scene_mode and not st.approach_mode and st.term_names[-1] == "E_pregrasp"
    st.reset(hp, idx)
    assert float(st.terms[-1].max()) > 0
    st.capture()
    st.run(6, reset_epochs=None)
    torch.cuda.synchronize()
    assert torch.isfinite(st.energy).all() and torch.isfinite(st.terms).all() and torch.isfinite(st.hand_pose).all()


def test_stack_and_own_scene_in_the_stepper(gq, golden_dir):
    """Two objects, a SceneSDFSet with one grid each as ``pregrasp_scene`` while ``scene`` (E_scene) is another grid: every row's
    E_pregrasp and gradient share are bit for bit those of a stepper whose pregrasp_scene is that object's grid alone."""
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    be = 4
    fv, sp, n, hp, idx, _ = _graph_scene(2 * be, n_obj=2)
    fields = [_wall(), _wall(-0.01)]
    other = _wall(0.05).scene(gq)  # the grid of E_scene: a third wall
    stack = gq.ops.SceneSDFSet(torch.stack([f.values for f in fields]).cuda(), [float(o) for o in fields[0].origin], float(fields[0].voxel))
    kw = dict(weights={"E_scene": 50.0, "E_pregrasp": 30.0}, surface_samples=sm, scene=other, scene_margin=0.01, **PG)
    st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv, fv]), sp, be, n, pregrasp_scene=stack, **kw)
    assert st.pregrasp_scene is stack and st.scene is other and not st.clutter
    t, tot, grad = st.evaluate(hp, idx)
    torch.cuda.synchronize()
    for gi, f in enumerate(fields):
        one = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv, fv]), sp, be, n, pregrasp_scene=f.scene(gq), **kw)
        t1, tot1, grad1 = one.evaluate(hp, idx)
        torch.cuda.synchronize()
        rows = slice(gi * be, (gi + 1) * be)
        for k in t:
            assert torch.equal(t[k][rows], t1[k][rows]), (gi, k)
        assert torch.equal(tot[rows], tot1[rows]) and torch.equal(grad[rows], grad1[rows]), gi
    # pregrasp_scene = None takes ``scene``
    same = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv, fv]), sp, be, n, **kw)
    assert same.pregrasp_scene is other
    t2 = same.evaluate(hp, idx)[0]
    assert not torch.equal(t2["E_pregrasp"], t["E_pregrasp"]) and torch.equal(t2["E_scene"], t["E_scene"])
    with pytest.raises(ValueError, match="n_grids"):
        gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp[:1], 2 * be, n, pregrasp_scene=stack, **kw)


def test_grid_overwritten_in_place_between_graph_replays(gq, golden_dir):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    B = 8
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    F1, F2 = _wall(), _wall(-0.01)  # the wall moves 3 cm
    mk = lambda scene: gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights={"E_pregrasp": 30.0},
                                               surface_samples=sm, pregrasp_scene=scene, pregrasp_margin=0.01, **PG)
    moving = F1.scene(gq)
    ptr = moving.values.data_ptr()
    st = mk(moving)
    st.reset(hp, idx)
    st.capture()
    st.step(draws=draws[0])
    torch.cuda.synchronize()
    after_one = {k: getattr(st, k).clone() for k in STATE}
    moving.values.copy_(F2.values.cuda())  # in place: the captured graph reads the new numbers
    assert moving.values.data_ptr() == ptr
    st.step(draws=draws[1])
    torch.cuda.synchronize()
    results = []
    for F in (F2, F1):  # a stepper built on the new values / on the old ones, continued from the same state
        ref = mk(F.scene(gq))
        ref.reset(hp, idx)
        for k in STATE:
            getattr(ref, k).copy_(after_one[k])
        ref.step(draws=draws[1])
        torch.cuda.synchronize()
        results.append(ref)
    for k in STATE:
        assert torch.equal(getattr(st, k), getattr(results[0], k)), k
    assert not torch.equal(st.terms_new[-1], results[1].terms_new[-1]), "moving the wall changed nothing"


def test_refusals(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    scene = _wall().scene(gq)
    with pytest.raises(ValueError, match="E_pregrasp"):
        _stepper(gq, g, 4, weights={"E_pregrasp": 1.0})  # no grid
    with pytest.raises(ValueError, match="E_pregrasp"):
        _stepper(gq, g, 4, weights={"E_pregrasp": -1.0}, scene=scene)
    for kw, word in ((dict(pregrasp_distance=0.0), "pregrasp_distance"), (dict(pregrasp_distance=float("nan")), "pregrasp_distance"),
                     (dict(pregrasp_stations=-1), "pregrasp_stations"), (dict(pregrasp_stations=33), "pregrasp_stations"),
                     (dict(pregrasp_stations=2.5), "pregrasp_stations"), (dict(pregrasp_margin=-0.01), "pregrasp_margin"),
                     (dict(pregrasp_opening=-0.1), "pregrasp_opening"), (dict(pregrasp_opening=1.5), "pregrasp_opening"),
                     (dict(pregrasp_opening=float("nan")), "pregrasp_opening"), (dict(pregrasp_joints=[0.0] * 3), "pregrasp_joints"),
                     (dict(approach_distance=-1.0), "pregrasp_distance"), (dict(approach_stations=40), "pregrasp_stations")):
        with pytest.raises(ValueError, match=word):
            _stepper(gq, g, 4, weights={"E_pregrasp": 1.0}, scene=scene, **kw)
    for K in (0, 32):  # the limits are accepted; the grid may come as pregrasp_scene alone
        st = _stepper(gq, g, 4, weights={"E_pregrasp": 1.0}, pregrasp_scene=scene, pregrasp_stations=K, pregrasp_opening=float(K > 0))
        assert st.pregrasp_stations == K and st.scene is None and st.pregrasp_distance == 0.10
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    sm = (g["opt_surface_points"], g["opt_surface_link"])
    hm, om = _class_surface(gq, g, hp, torch.tensor(g["contact_idx"]).cuda(), sm, None, 0.0)
    with pytest.raises(ValueError, match="set_scene"):
        hm.set_pregrasp(0.1, 4)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    with pytest.raises(ValueError, match="E_pregrasp"):
        calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_pregrasp"], svd_gain=0.1)
    for args, kw, word in (((0.0, 4), {}, "distance"), ((0.1, -1), {}, "stations"), ((0.1, 33), {}, "stations"), ((0.1, 4), dict(margin=-1.0), "margin"),
                           ((0.1, 4), dict(opening=2.0), "opening"), ((0.1, 4), dict(open_joints=[0.0]), "open_joints"),
                           ((0.1, 4), dict(scene="grid"), "scene")):
        with pytest.raises(ValueError, match=word):
            hm.set_pregrasp(*args, scene=kw.pop("scene", scene), **kw)
    hm.set_pregrasp(0.1, 0, scene=scene)  # a grid of its own, no set_scene: the margin is 0
    e = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_pregrasp"], svd_gain=0.1)["E_pregrasp"]
    assert e.shape == (hp.shape[0],) and torch.isfinite(e).all()
    # the op's own refusals come from gq_pregrasp_check
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, *sm)
    idx = torch.zeros(hp.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    for axis, D, K, opening, word in (((0.0, 0.0, 1.0), 0.1, 33, 0.5, "n_stations"), ((0.0, 0.0, 1.0), -0.1, 4, 0.5, "distance"),
                                      ((0.0, 0.0, 0.0), 0.1, 4, 0.5, "grasp_axis"), ((0.0, 0.0, 1.0), 0.1, 4, 1.5, "opening")):
        with pytest.raises(ValueError, match=f"pregrasp.*{word}"):
            gq.ops.pregrasp_terms(hp, hand, samples, idx, Rg, LT, ws, scene, axis, D, K, opening)
    with pytest.raises(ValueError, match="open_joints"):
        gq.ops.pregrasp_terms(hp, hand, samples, idx, Rg, LT, ws, scene, (0.0, 0.0, 1.0), 0.1, 4, 0.5, open_joints=[0.0, 1.0])
    with pytest.raises(ValueError, match="margin"):
        gq.ops.pregrasp_terms(hp, hand, samples, idx, Rg, LT, ws, scene, (0.0, 0.0, 1.0), 0.1, 4, 0.5, margin=-1.0)
