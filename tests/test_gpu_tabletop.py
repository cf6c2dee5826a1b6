"""GPU tests of the tabletop terms (E_prior / E_wall, reference core/energy.py:68-78) as the stepper runs them: the op and
its gradient against the reference-made fixtures and the fp64 oracle, the shapes at which the kernel can go wrong, the
stepper's seven-term evaluation, its iterations against the class surface and its hipGraph replay.

Bounds: values rtol 1e-5 / atol 1e-6 and gradients norm-wise 1e-4 are the ones the class-surface test of the same
quantities holds (tests/test_gpu_alt_energies.py); a new energy against the class surface 3e-4 is the bound of
test_mala_iterations_match_reference_optimizer."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402
from ref_cpu import energy as oenergy  # noqa: E402
from ref_cpu import models as omodels  # noqa: E402

from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
NEAR = 2e-5  # a sample closer to the plane than this is too close to ask an fp32 kernel for the oracle's side


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


def _oracle(spec, pts, lnk, hp64, a=2.0, b=3.0, table_z=0.0):
    """fp64: (E_prior, E_wall, d (a E_prior + b E_wall) / d hand_pose, heights of the samples above the plane)."""
    oh = omodels.OracleHand(spec, torch.float64)
    oh.surface_points, oh.surface_link = np.asarray(pts, dtype=np.float64), np.asarray(lnk)
    hp = hp64.clone()
    hp[:, 2] -= table_z  # the oracle's plane is z = 0
    hp.requires_grad_()
    oh.set_parameters(hp, torch.zeros(hp.shape[0], 1, dtype=torch.long))
    t = oenergy.optional_terms(oh)
    h = oh.get_surface_points()[..., 2].detach()
    (a * t["E_prior"] + b * t["E_wall"]).sum().backward()
    return t["E_prior"].detach().numpy(), t["E_wall"].detach().numpy(), oh.hand_pose.grad.numpy(), h.numpy()


def _op(gq, hand, samples, hp32, a=2.0, b=3.0, table_z=0.0):
    """The op on the GPU: (E_prior, E_wall, d (a E_prior + b E_wall) / d hand_pose) as numpy."""
    hpg = hp32.clone().cuda().requires_grad_()
    idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
    ep, ew = gq.ops.tabletop_terms(hpg, hand, samples, idx, Rg, LT, ws, hand.spec.grasp_axis, table_z)
    (a * ep + b * ew).sum().backward()
    torch.cuda.synchronize()
    return ep.detach().cpu().numpy(), ew.detach().cpu().numpy(), hpg.grad.cpu().numpy()


def _assert_matches(got, ref, tag):
    ep, ew, g = got
    rp, rw, rg = ref
    print(f"[{tag}] E_prior max abs err {np.abs(ep - rp).max():.3e}, E_wall max abs err {np.abs(ew - rw).max():.3e} "
          f"(max {np.abs(rw).max():.3e}), grad rel err {np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-300):.3e}")
    np.testing.assert_allclose(ep, rp, rtol=1e-5, atol=1e-6, err_msg=f"{tag} E_prior")
    np.testing.assert_allclose(ew, rw, rtol=1e-5, atol=1e-6, err_msg=f"{tag} E_wall")
    assert np.linalg.norm(g - rg) <= 1e-4 * np.linalg.norm(rg), tag


# ---------------------------------------------------------------------------------------------------------------
# 1. the op against the reference-made fixtures
# ---------------------------------------------------------------------------------------------------------------
def test_op_matches_the_reference_fixture_sphere(gq, golden_dir):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    hp32 = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    _assert_matches(_op(gq, hand, samples, hp32), (g["opt_E_prior"], g["opt_E_wall"], g["opt_grad"]), "sphere fixture")
    for dz, lo, hi in ((0.0, 44, 64), (0.1, 21, 50), (0.15, 7, 34)):
        hp = hp32.clone()
        hp[:, 2] += dz
        rp, rw, rg, h = _oracle(spec, g["opt_surface_points"], g["opt_surface_link"], hp.double())
        below = (h < 0).sum(-1)
        assert np.abs(h).min() >= 3e-4 and below.min() >= lo and below.max() <= hi, (dz, below, np.abs(h).min())
        _assert_matches(_op(gq, hand, samples, hp), (rp, rw, rg), f"sphere dz={dz}")


def test_op_matches_the_reference_fixture_sq(gq, golden_dir):
    g = _load(golden_dir, "energy_allegro_sq_b6_n12.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    hp32 = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    ep, ew, _ = _op(gq, hand, samples, hp32)
    print(f"[sq fixture] E_prior max abs err {np.abs(ep - g['opt_E_prior']).max():.3e}, E_wall max abs err "
          f"{np.abs(ew - g['opt_E_wall']).max():.3e}")
    np.testing.assert_allclose(ep, g["opt_E_prior"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ew, g["opt_E_wall"], rtol=1e-5, atol=1e-6)
    # the gradient: at translations shifted upwards (the unshifted pose has a sample 5e-6 m from the plane)
    for dz, lo, hi in ((0.05, 30, 61), (0.1, 10, 48), (0.3, 0, 0)):
        hp = hp32.clone()
        hp[:, 2] += dz
        rp, rw, rg, h = _oracle(spec, g["opt_surface_points"], g["opt_surface_link"], hp.double())
        below = (h < 0).sum(-1)
        assert np.abs(h).min() > 6e-5 and below.min() >= lo and below.max() <= hi, (dz, below, np.abs(h).min())
        got = _op(gq, hand, samples, hp)
        _assert_matches(got, (rp, rw, rg), f"sq dz={dz}")
        if hi == 0:  # nothing below the plane: E_wall and its gradient are exactly zero
            assert (got[1] == 0).all()
            gw = _op(gq, hand, samples, hp, a=0.0, b=3.0)[2]
            assert (gw == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. shapes where the kernel can go wrong
# ---------------------------------------------------------------------------------------------------------------
def _straddling_pose(spec, B, pts, lnk, seed0):
    """Seeded pose whose samples lie on both sides of the plane in every row (for more than one sample) and none within
    NEAR of it; the next seed is drawn otherwise.  -> (pose float32, oracle results at that float32 pose)."""
    for seed in range(seed0, seed0 + 50):
        gen = torch.Generator().manual_seed(seed)
        t = torch.cat([0.1 * torch.randn(B, 2, generator=gen), 0.02 * torch.randn(B, 1, generator=gen)], 1)
        th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
        hp = torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).float()
        rp, rw, rg, h = _oracle(spec, pts, lnk, hp.double())
        if np.abs(h).min() < NEAR:
            continue
        below = (h < 0).sum(-1)
        if len(pts) > 1 and (below.min() == 0 or below.max() == len(pts)):
            continue
        return hp, (rp, rw, rg)
    raise AssertionError("no seeded pose leaves samples on both sides of the plane")


@pytest.mark.parametrize("hand_name,Ns", [("allegro", 1), ("allegro", 63), ("allegro", 65), ("allegro", 512), ("panda", 512),
                                          ("schunk2", 512)])
def test_op_shapes_match_the_oracle(gq, hand_name, Ns):
    spec, hand = get_hand_spec(hand_name), _hand(hand_name)
    pts, lnk = _default_samples(hand_name)
    if Ns < 512:  # a seeded subset, in shuffled order (the terms do not depend on the order of the samples)
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns and (np.diff(samples.link.cpu().numpy()) >= 0).all()
    if Ns == 512:
        assert len(np.unique(lnk)) <= spec.n_links
    for B in (1, 7):
        hp, ref = _straddling_pose(spec, B, pts, lnk, 100 * B + Ns)
        _assert_matches(_op(gq, hand, samples, hp), ref, f"{hand_name} Ns={Ns} B={B}")


BIG_B, BIG_TABLE_Z = 3, 0.05  # more than 512 samples: 577 = 10 chunks (wavefront 1's second chunk holds one sample), 1100 = 18


def _big_pose(spec, pts, lnk):
    """The seeded loop of ``_straddling_pose`` with the plane at BIG_TABLE_Z, and at least 5 samples beyond index 511 below it.
    -> (pose float32, oracle results, heights over the plane)."""
    for seed in range(100 * BIG_B + len(pts), 100 * BIG_B + len(pts) + 50):
        gen = torch.Generator().manual_seed(seed)
        t = torch.cat([0.1 * torch.randn(BIG_B, 2, generator=gen), 0.02 * torch.randn(BIG_B, 1, generator=gen)], 1)
        th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(BIG_B, spec.n_dofs, generator=gen)
        hp = torch.cat([t, torch.randn(BIG_B, 6, generator=gen), th], 1).float()
        rp, rw, rg, h = _oracle(spec, pts, lnk, hp.double(), table_z=BIG_TABLE_Z)
        below = (h < 0).sum(-1)
        if np.abs(h).min() >= NEAR and below.min() > 0 and below.max() < len(pts) and (h[:, 512:] < 0).sum() >= 5:
            return hp, (rp, rw, rg), h
    raise AssertionError("no seeded pose leaves samples on both sides of the plane")


def _without_link_3(n):
    """``n`` samples of the allegro hand of which none rides on link 3: those of ``_default_samples(n)`` topped up from 2 n."""
    (p1, l1), (p2, l2) = _default_samples("allegro", n), _default_samples("allegro", 2 * n)
    pts, lnk = np.concatenate([p1[l1 != 3], p2[l2 != 3]])[:n], np.concatenate([l1[l1 != 3], l2[l2 != 3]])[:n]
    assert len(pts) == n
    return pts, lnk


@pytest.mark.parametrize("Ns", [577, 1100])
def test_more_than_512_samples_match_the_oracle(gq, Ns):
    """A wavefront's second and third trip through the chunk loop: allegro, B = 3, the plane at z = 0.05 so that samples beyond
    index 511 lie below it (asserted: at least 5; the oracle has 191 of them at Ns = 577 and 1069 at Ns = 1100)."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _default_samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns and np.array_equal(samples.link.cpu().numpy(), lnk)  # they come by link: the order of the launch
    hp, ref, h = _big_pose(spec, pts, lnk)
    tail = int((h[:, 512:] < 0).sum())
    print(f"[allegro Ns={Ns} B={BIG_B}] samples below the plane {int((h < 0).sum())}, of them at indices >= 512: {tail}")
    assert tail >= 5 and np.abs(h).min() >= NEAR
    _assert_matches(_op(gq, hand, samples, hp, table_z=BIG_TABLE_Z), ref, f"allegro Ns={Ns} B={BIG_B} table_z={BIG_TABLE_Z}")


def test_second_chunk_run_to_run_sample_order_and_a_link_without_samples(gq):
    """Ns = 577 through the C entry: bitwise run to run; the samples by link against the same samples shuffled, within the
    bounds of ``_assert_matches`` (the order of the samples moves the last bits only); a link without samples."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _without_link_3(577)
    hp, ref, h = _big_pose(spec, pts, lnk)
    B, L = BIG_B, hand.L
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
    axis = [float(a) for a in spec.grasp_axis]

    def run(p, l, accumulate=0, bufs=None):
        p, l = torch.tensor(p).cuda(), torch.tensor(l.astype(np.int32)).cuda()
        wrench, gRt, gR = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"), torch.empty(B, 9, device="cuda"))
        ew, ep = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        gq.ops._tabletop_call(hp, p, l, L, Rg.contiguous(), LT.contiguous(), axis, BIG_TABLE_Z, None, 1.5, None, 0.5, ew, ep,
                              accumulate, wrench, gRt, gR)
        torch.cuda.synchronize()
        return wrench, gRt, gR, ew, ep

    order = np.argsort(lnk, kind="stable")
    by_link, again = run(pts[order], lnk[order]), run(pts[order], lnk[order])
    for a, b in zip(by_link, again):
        assert torch.equal(a, b)
    np.testing.assert_allclose(by_link[3].cpu().numpy(), ref[1], rtol=1e-5, atol=1e-6)
    perm = np.random.default_rng(577).permutation(577)
    assert not (np.diff(lnk[perm]) >= 0).all()
    shuffled = run(pts[perm], lnk[perm])
    grad = lambda r: np.concatenate([r[0].cpu().numpy().reshape(B, -1), r[1].cpu().numpy(), r[2].cpu().numpy()], 1)
    _assert_matches((shuffled[4].cpu().numpy(), shuffled[3].cpu().numpy(), grad(shuffled)),
                    (by_link[4].cpu().numpy(), by_link[3].cpu().numpy(), grad(by_link)), "Ns=577 shuffled vs by link")
    for r in (by_link, shuffled):
        assert (r[0][:, 3] == 0).all() and r[0].abs().max() > 0  # the link without samples: zero wrench
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12), (B, 9))]
    acc = run(pts[order], lnk[order], 1, [p.clone() for p in pre])
    for a, p, v in zip(acc[:3], pre, by_link[:3]):
        assert torch.equal(a, p + v)
    assert torch.equal(acc[0][:, 3], pre[0][:, 3])  # left alone


# ---------------------------------------------------------------------------------------------------------------
# 3. table_z
# ---------------------------------------------------------------------------------------------------------------
def test_raising_the_plane_equals_lowering_the_hand(gq, golden_dir):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    hp[:, 2] += 0.1
    for dz in (0.03, -0.02):
        lowered = hp.clone()
        lowered[:, 2] -= dz
        h = _oracle(spec, g["opt_surface_points"], g["opt_surface_link"], lowered.double())[3]
        assert np.abs(h).min() >= NEAR and (h < 0).any() and (h > 0).any()
        # rtol 1e-5 alone is asked of E_wall: a height carries ~3 roundings of terms of size <= 0.2 m (7e-8 m), so the sums
        # of the two forms can differ by 7e-8 m per sample below; that is inside 1e-5 of the sum where the mean depth of the
        # samples below is at least 7 mm, which every row of this pose has several times over
        depth = np.where(h < 0, -h, 0.0).sum(-1) / np.maximum((h < 0).sum(-1), 1)
        assert ((h < 0).sum(-1) > 0).all() and depth.min() >= 7e-3, depth
        a = _op(gq, hand, samples, hp, table_z=dz)
        b = _op(gq, hand, samples, lowered, table_z=0.0)
        assert (a[1] > 0).any()
        print(f"[table_z={dz}] E_wall rel diff max {np.abs(a[1] - b[1]).max() / np.abs(b[1]).min():.3e}, "
              f"grad abs diff max {np.abs(a[2] - b[2]).max():.3e}")
        for x, y, name in zip(a, b, ("E_prior", "E_wall", "grad")):  # the gradient sees the same samples below
            np.testing.assert_allclose(x, y, rtol=1e-5, atol=0.0, err_msg=name)


# ---------------------------------------------------------------------------------------------------------------
# 4. per-row upstream, accumulate, reproducibility (the C entry itself)
# ---------------------------------------------------------------------------------------------------------------
def test_upstream_vectors_accumulate_and_reproducibility(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _default_samples("allegro")
    pts, lnk = pts[lnk != 3], lnk[lnk != 3]  # a link without samples
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    B, L = 7, hand.L
    hp, _ = _straddling_pose(spec, B, pts, lnk, 7)
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
    axis = [float(a) for a in spec.grasp_axis]

    def run(up_wall, w_wall, up_prior, w_prior, accumulate, bufs=None):
        wrench, gRt, gR = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"), torch.empty(B, 9, device="cuda"))
        ew, ep = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        gq.ops._tabletop_call(hp, samples.points, samples.link, L, Rg.contiguous(), LT.contiguous(), axis, 0.0, up_wall, w_wall,
                              up_prior, w_prior, ew, ep, accumulate, wrench, gRt, gR)
        torch.cuda.synchronize()
        return wrench, gRt, gR, ew, ep

    one = run(None, 1.0, None, 1.0, 0)
    again = run(None, 1.0, None, 1.0, 0)
    for a, b in zip(one, again):
        assert torch.equal(a, b)
    assert (one[0][:, 3] == 0).all() and one[0].abs().max() > 0  # the link without samples: zero wrench
    # a non-uniform upstream per row == the per-row scaled result (two roundings apart; m = S x g_h cancels, hence the floor)
    uw, up = torch.linspace(0.5, 3.0, B, device="cuda"), torch.linspace(-1.0, 2.0, B, device="cuda")
    vec = run(uw, 0.0, up, 0.0, 0)
    for got, unit, u in ((vec[0], one[0], uw.view(B, 1, 1)), (vec[1], one[1], uw.view(B, 1)), (vec[2], one[2], up.view(B, 1))):
        want = unit * u
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=4 * EPS32, atol=4 * EPS32 * float(want.abs().max()))
    assert torch.equal(vec[3], one[3]) and torch.equal(vec[4], one[4])  # the energies are unweighted
    # scalar weights: the same idiom
    sca = run(None, 2.5, None, 0.75, 0)
    np.testing.assert_allclose(sca[0].cpu().numpy(), (2.5 * one[0]).cpu().numpy(), rtol=4 * EPS32, atol=4 * EPS32 * float(one[0].abs().max()) * 2.5)
    np.testing.assert_allclose(sca[2].cpu().numpy(), (0.75 * one[2]).cpu().numpy(), rtol=4 * EPS32)
    # accumulate = 1 on pre-filled buffers == pre-fill + the accumulate = 0 result, bit for bit
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12), (B, 9))]
    acc = run(uw, 0.0, up, 0.0, 1, [p.clone() for p in pre])
    for a, p, v in zip(acc[:3], pre, vec[:3]):
        assert torch.equal(a, p + v)
    assert torch.equal(acc[0][:, 3], pre[0][:, 3])  # left alone


# ---------------------------------------------------------------------------------------------------------------
# 5. / 6. the stepper's evaluation
# ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, g, n_contact, hand=None, **kw):
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    return gq.stepper.GraspStepper(hand or _hand("allegro"), gq.ops.MeshSet(fvs), torch.tensor(sps), be, n_contact, **kw)


@pytest.mark.parametrize("tag,n,energy_type", [("allegro_sphere_b4_n4", 4, "graspqp"), ("allegro_sq_b6_n12", 12, "graspqp"),
                                               ("allegro_sphere_b4_n4", 4, "dexgrasp")])
def test_stepper_evaluate_in_tabletop_mode(gq, golden_dir, tag, n, energy_type):
    g = _load(golden_dir, f"energy_{tag}.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    sm = (g["opt_surface_points"], g["opt_surface_link"])
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    idx = torch.tensor(g["contact_idx"]).cuda()
    st0 = _stepper(gq, g, n, energy_type=energy_type)
    st1 = _stepper(gq, g, n, energy_type=energy_type, weights={"E_prior": 2.0, "E_wall": 3.0}, surface_samples=sm)
    assert st1.tabletop and not st1._fuse_loop and st1.terms.shape == (7, hp.shape[0])
    t0, tot0, g0 = st0.evaluate(hp, idx)
    t1, tot1, g1 = st1.evaluate(hp, idx)
    torch.cuda.synchronize()
    assert list(t1) == ["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_prior", "E_wall"] and list(t0) == list(t1)[:5]
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    samples = gq.ops.SurfaceSamples(hand, *sm)
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    ep, ew = gq.ops.tabletop_terms(hp, hand, samples, idx, Rg, LT, ws, spec.grasp_axis)
    assert torch.equal(t1["E_prior"], ep) and torch.equal(t1["E_wall"], ew)
    d_tot = (tot1.double() - tot0.double()).cpu().numpy()
    want = (2.0 * ep.double() + 3.0 * ew.double()).cpu().numpy()
    print(f"[{tag} {energy_type}] total diff max err {np.abs(d_tot - want).max():.3e}, bound {4 * EPS32 * float(tot1.abs().min()):.3e}")
    assert (np.abs(d_tot - want) <= 4 * EPS32 * tot1.abs().cpu().numpy()).all()
    rg = _oracle(spec, sm[0], sm[1], hp.double().cpu())[2]
    dg = (g1.double() - g0.double()).cpu().numpy()
    err, bound = np.linalg.norm(dg - rg), 1e-4 * np.linalg.norm(rg) + 4 * EPS32 * float(g0.double().norm())
    print(f"[{tag} {energy_type}] grad diff err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_zero_weights_are_the_default_stepper(gq, golden_dir):
    g = _load(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    sts = [_stepper(gq, g, 4), _stepper(gq, g, 4, weights={"E_wall": 0.0, "E_prior": 0.0})]
    B = sts[0].B
    assert sts[1].terms.shape == (5, B) and sts[1]._fuse_loop and not sts[1].tabletop and sts[1].samples is None
    for st in sts:
        st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
        for s in (1, 2, 3):
            st.step(draws=(f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")))
    torch.cuda.synchronize()
    for k in ("hand_pose", "contact_idx", "energy", "grad", "terms"):
        assert torch.equal(getattr(sts[0], k), getattr(sts[1], k)), k
    with pytest.raises(ValueError, match="E_manipulativity"):
        _stepper(gq, g, 4, weights={"E_manipulativity": 1.0})


# ---------------------------------------------------------------------------------------------------------------
# 7. iterations against the class surface
# ---------------------------------------------------------------------------------------------------------------
def test_tabletop_iterations_match_the_class_surface(gq, golden_dir):
    """Five iterations (the third one re-initialises two rows), teacher-forced from the class-surface state: the loop of
    test_mala_class_surface / test_stepper_reset_iteration_matches_class_surface with both tabletop terms."""
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.core.optimizer import MalaStar
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    C = gq.C
    g = _load(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    be, n_obj = int(g["batch_size_each"]), int(g["n_obj"])
    B = be * n_obj
    spec = get_hand_spec("allegro")
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    w = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0, "E_prior": 2.0, "E_wall": 3.0}
    st = _stepper(gq, g, 4, weights={"E_prior": 2.0, "E_wall": 3.0}, surface_samples=sm)
    hm = HandModel(spec, "cuda")
    hm.set_surface_points(*sm)
    om = ObjectModel(batch_size_each=be, num_samples=g["obj0_surface_points"].shape[0])
    om.initialize_from_meshes([g[f"obj{i}_face_verts"] for i in range(n_obj)],
                              surface_points_list=[g[f"obj{i}_surface_points"] for i in range(n_obj)])
    hm.set_parameters(f32("hand_pose0").requires_grad_(), torch.tensor(g["contact_idx0"]).cuda())
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
        # teacher forcing: the stepper starts the iteration from the class surface's accepted state
        grad = hm.hand_pose.grad
        st.hand_pose.copy_(hm.hand_pose.detach())
        st.contact_idx.copy_(hm.contact_point_indices)
        st.grad.copy_(torch.zeros_like(st.grad) if grad is None else grad)
        st.energy.copy_(energy)
        st.ema.copy_(opt.ema_grad_hand_pose)
        st.step_count.copy_(opt.step)
        terms_before = st.terms.clone()
        u_sw, n_ix = f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda()
        # --- class surface
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
        # the temperature of this accept step (it does not depend on the draw), from a throw-away call on copies
        T = torch.empty(B, device="cuda")
        hpd, gd, ixd = hm.hand_pose.detach().contiguous(), hm.hand_pose.grad.contiguous(), hm.contact_point_indices.contiguous()
        ne, u0, zc = new_energy.detach().contiguous(), torch.zeros(B, device="cuda"), z.contiguous()
        e_t, p_t, i_t, g_t, a_t = energy.clone(), hpd.clone(), ixd.clone(), gd.clone(), torch.empty(B, dtype=torch.uint8, device="cuda")
        C.call("gq_mala_accept", C.f32(ne), C.f32(u0), C.f32(zc), C.u8(None), C.i64(opt.step), C.f32(hpd), C.i64(ixd), C.f32(gd), B,
               hpd.shape[1], 4, opt.starting_temperature, opt.temperature_decay, opt.annealing_period, C.f32(e_t), C.f32(p_t),
               C.i64(i_t), C.f32(g_t), C.u8(a_t), C.f32(T), 0, None, None, C.stream_ptr())
        p = torch.exp((energy - new_energy.detach()) / T)
        # injected accept draws: the fixture's, or seeded ones if a row's Metropolis margin is below 1e-3 (no row is excluded)
        cands = [f32(f"s{s}_u_accept")] + [torch.rand(B, generator=torch.Generator().manual_seed(1000 * s + k)).cuda() for k in range(8)]
        u_ac = next(u for u in cands if bool(((u - p).abs() >= 1e-3).all()))
        with torch.no_grad():
            accept, T_cls = opt.accept_step(energy, new_energy, rm, z, 1.0, u_accept=u_ac)
        assert torch.allclose(T_cls, T)
        # --- stepper
        if s == 3:
            st.step_reset(mask, new_pose, new_idx, draws=(u_sw, n_ix, u_ac))
        else:
            st.step(draws=(u_sw, n_ix, u_ac))
        torch.cuda.synchronize()
        rel = ((st.total_new - new_energy.detach()).abs() / new_energy.detach().abs().clamp_min(1e-12)).cpu().numpy()
        print(f"[iteration {s}] total_new rel err max {rel.max():.3e}, E_wall max {float(st.terms_new[6].max()):.4f}, "
              f"min margin {float((u_ac - p).abs().min()):.3e}, accepted {int(accept.sum())}/{B}")
        assert rel.max() < 3e-4, rel
        assert float(st.terms_new[6].max()) > 0, "no sample below the plane in this iteration"
        np.testing.assert_allclose(st.terms_new[5].cpu().numpy(), losses["E_prior"].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(st.terms_new[6].cpu().numpy(), losses["E_wall"].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
        assert st.accept.bool().tolist() == accept.tolist()
        if s == 3:
            assert accept[mask.cuda()].all()
        acc = st.accept.bool()
        assert torch.equal(st.terms[5:7][:, acc], st.terms_new[5:7][:, acc])
        assert torch.equal(st.terms[5:7][:, ~acc], terms_before[5:7][:, ~acc])
        np.testing.assert_allclose(st.energy.cpu().numpy(), energy.cpu().numpy(), rtol=3e-4)
        np.testing.assert_allclose(st.hand_pose.cpu().numpy(), hm.hand_pose.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
        assert torch.equal(st.contact_idx, hm.contact_point_indices)


# ---------------------------------------------------------------------------------------------------------------
# 8. hipGraph replay
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,mode,optimizer", [(8, "one grid", "mala_star"), (384, "graph branches", "mala_star"),
                                              (8, "one grid", "dexgraspnet")])
def test_graph_replay_equals_eager_steps(gq, golden_dir, B, mode, optimizer):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    fv = meshes.icosphere(2, 0.05)
    sp = torch.tensor(meshes.surface_points(fv, 256, oversample=4))[None]
    n = 4
    gen = torch.Generator().manual_seed(B)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1) * 0.12
    hp = torch.cat([t, torch.randn(B, 6, generator=gen), torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=gen)], 1).cuda()
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda()
    draws = [(torch.rand(B, n, generator=gen).cuda(), torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda(),
              torch.rand(B, generator=gen).cuda()) for _ in range(3)]
    out = []
    for graph in (False, True):
        st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights={"E_prior": 2.0, "E_wall": 3.0},
                                     surface_samples=sm, optimizer=optimizer)
        st.reset(hp, idx)
        assert float(st.terms[6].max()) > 0
        if graph:
            st.capture()
            assert st.graph_mode == mode
        for d in draws:
            st.step(draws=d)
        torch.cuda.synchronize()
        out.append([getattr(st, k).clone() for k in ("hand_pose", "contact_idx", "energy", "grad", "terms", "accept")])
    for a, b, k in zip(out[0], out[1], ("hand_pose", "contact_idx", "energy", "grad", "terms", "accept")):
        assert torch.equal(a, b), k
    assert torch.isfinite(out[0][2]).all()


# ---------------------------------------------------------------------------------------------------------------
# the registered ops
# ---------------------------------------------------------------------------------------------------------------
def test_registered_ops_opcheck_and_dispatcher_route(gq, golden_dir):
    """torch.library.opcheck on the two ops (schema, fake kernels consistent with the real ones; their gradient is wired by
    ops.tabletop_terms, as for hand_pen), and the dispatcher route gives the bits of the eager route."""
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    B = hp.shape[0]
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
    axis = [float(a) for a in hand.spec.grasp_axis]
    ns = torch.ops.graspqp_amd
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(ns.tabletop_terms, (hp, samples.points, samples.link, hand.L, Rg, LT, axis, 0.0), test_utils=utils)
    up = torch.linspace(0.5, 2.0, B, device="cuda")
    torch.library.opcheck(ns.tabletop_terms_backward, (hp, samples.points, samples.link, hand.L, Rg, LT, axis, 0.0, up, up),
                          test_utils=utils)
    eager = _op(gq, hand, samples, hp.cpu())
    old = gq.ops.use_dispatcher(True)
    try:
        routed = _op(gq, hand, samples, hp.cpu())
    finally:
        gq.ops.use_dispatcher(old)
    for a, b in zip(eager, routed):
        assert np.array_equal(a, b)
