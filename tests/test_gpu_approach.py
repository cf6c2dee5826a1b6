"""GPU tests of the approach term (E_approach: the scene grid along the hand's approach corridor): the fused launch against the
contract written in torch fp64 (tests/_approach_oracle.py) at the shapes and station counts at which the kernel can go wrong,
against closed forms and the existing scene / tabletop launches, the C entry's accumulate / upstream / reproducibility rules,
and the stepper's approach mode (evaluation, iterations against the class surface, hipGraph replay, obstacles moved in place).

Bounds: values rtol 1e-5 / atol 1e-6, gradients norm-wise 1e-4, energies against the class surface 3e-4.

Guards: conditions on the INPUTS, computed by the fp64 oracle over all B Ns K station points and asserted -- on the random field
no coordinate within 1e-4 cells of a cell face, on every field no |phi - margin| < 2e-5.  Poses come from a deterministic seeded
search (at most 200 seeds) that also asks for at least 5 active points (or Ns B if smaller) and one active point at every
station."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _approach_oracle as ao  # noqa: E402
import _scene_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
G_SHAPE, G_ORIGIN, G_H = (100, 96, 104), (-0.5, -0.48, -0.52), 0.01


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
def _samples(name, Ns):
    """``hand_surface_samples(spec, 512)``, or a seeded subset of it in shuffled order."""
    pts, lnk = meshes.hand_surface_samples(get_hand_spec(name), 512)
    if Ns < 512:
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    return pts, lnk


@functools.lru_cache(maxsize=None)
def _field(kind, shape=G_SHAPE, origin=G_ORIGIN, voxel=G_H, seed=11):
    if kind == "affine":
        return so.affine(shape, origin, voxel)
    if kind == "multilinear":
        return so.multilinear(shape, origin, voxel)
    if kind == "random":
        return so.random_field(shape, origin, voxel, seed)
    raise KeyError(kind)


def _pose(spec, B, seed, spread=0.1):
    """The pose generator of test_gpu_scene._guarded_pose."""
    gen = torch.Generator().manual_seed(seed)
    t = spread * torch.randn(B, 3, generator=gen)
    th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
    return torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).float()


def _conditions(ref, margin, Ns, B, cells):
    face, near = ao.guards(ref, margin)
    act = ref["active"]
    return ((face >= ao.FACE or not cells) and near >= ao.NEAR and act.sum() >= min(5, Ns * B) and
            bool(act.any(axis=(0, 2)).all()))


@functools.lru_cache(maxsize=None)
def _guarded(hand_name, Ns, B, K, D, kind, margin, seed0=None, extra=None):
    """Seeded float32 pose whose B Ns K station points pass the conditions of the module docstring, and the oracle's results at
    it (computed once, shared)."""
    spec = get_hand_spec(hand_name)
    pts, lnk = _samples(hand_name, Ns)
    F = _field(kind)
    seed0 = 100 * B + Ns if seed0 is None else seed0
    for seed in range(seed0, seed0 + 200):
        hp = _pose(spec, B, seed)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), F, margin, D, K)
        if _conditions(ref, margin, Ns, B, kind == "random") and (extra is None or extra(ref)):
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


def _assert_guards(ref, margin, tag, Ns, B, K, cells):
    face, near = ao.guards(ref, margin)
    act = ref["active"]
    print(f"[{tag}] guards over {act.size} points: nearest cell face {face:.2e} cells, nearest |phi - margin| {near:.2e} m, active "
          f"per station {act.sum(axis=(0, 2)).tolist()}")
    assert act.size == B * Ns * K
    if cells:
        assert face >= ao.FACE, (tag, face)
    assert near >= ao.NEAR, (tag, near)
    assert act.sum() >= min(5, Ns * B) and act.any(axis=(0, 2)).all(), tag


def _state(gq, hand, hp32):
    hpg = hp32.clone().cuda().requires_grad_()
    idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
    return hpg, idx, Rg, LT, ws


def _op(gq, hand, samples, hp32, scene, axis, D, K, margin, scale=3.0):
    """The op on the GPU: (E_approach, d (scale E_approach) / d hand_pose) as numpy."""
    hpg, idx, Rg, LT, ws = _state(gq, hand, hp32)
    e = gq.ops.approach_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, axis, D, K, margin)
    (scale * e).sum().backward()
    torch.cuda.synchronize()
    return e.detach().cpu().numpy(), hpg.grad.cpu().numpy()


def _assert_matches(got, ref, tag, factor=1.0, cols=None):
    e, g = got
    re_, rg = ref
    if cols is not None:
        g, rg = g[:, cols], rg[:, cols]
    gerr = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-300)
    print(f"[{tag}] E_approach max abs err {np.abs(e - re_).max():.3e} (max {np.abs(re_).max():.3e}, max rel "
          f"{(np.abs(e - re_) / np.maximum(np.abs(re_), 1e-30)).max():.3e}), grad rel err {gerr:.3e}")
    np.testing.assert_allclose(e, re_, rtol=factor * 1e-5, atol=factor * 1e-6, err_msg=f"{tag} E_approach")
    assert np.linalg.norm(g - rg) <= factor * 1e-4 * np.linalg.norm(rg), tag


# ---------------------------------------------------------------------------------------------------------------
# 1. the op against the oracle: shapes and station counts
# ---------------------------------------------------------------------------------------------------------------
TABLE = [("allegro", 1, 1, 4, 0.08, "random", 0.0), ("allegro", 63, 1, 4, 0.08, "random", 0.0),
         ("allegro", 65, 1, 4, 0.08, "random", 0.0), ("allegro", 128, 1, 4, 0.08, "random", 0.01),
         ("allegro", 512, 1, 1, 0.08, "random", 0.0), ("allegro", 512, 3, 2, 0.08, "multilinear", 0.01),
         ("allegro", 65, 7, 8, 0.10, "multilinear", 0.01), ("panda", 512, 2, 3, 0.08, "multilinear", 0.01),
         ("schunk2", 512, 2, 3, 0.08, "multilinear", 0.01), ("allegro", 512, 1, 32, 0.10, "multilinear", 0.0)]


@pytest.mark.parametrize("hand_name,Ns,B,K,D,kind,margin", TABLE)
def test_op_matches_the_oracle(gq, hand_name, Ns, B, K, D, kind, margin):
    spec, hand = get_hand_spec(hand_name), _hand(hand_name)
    pts, lnk = _samples(hand_name, Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns
    # the caps on the inputs: 512 points on the random field, 4 096 on the smooth ones, K = 32 on its own as the limit
    assert B * Ns * K <= (512 if kind == "random" else 4096) or (K == 32 and B == 1)
    hp, ref = _guarded(hand_name, Ns, B, K, D, kind, margin)
    tag = f"{hand_name} Ns={Ns} B={B} K={K} D={D} {kind} margin={margin}"
    _assert_guards(ref, margin, tag, Ns, B, K, kind == "random")
    _assert_matches(_op(gq, hand, samples, hp, _field(kind).scene(gq), spec.grasp_axis, D, K, margin), (ref["E"], ref["grad"]), tag)


BIG_B, BIG_K, BIG_D, BIG_MARGIN = 3, 3, 0.08, 0.01  # more than 512 samples: 577 = 10 chunks, 1100 = 18


def _tail_active(ref):
    """Samples at indices >= 512 (a wavefront's later chunks) with an active station."""
    return int(ref["active"][:, :, 512:].any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def _big_samples(Ns):
    pts, lnk = meshes.hand_surface_samples(get_hand_spec("allegro"), Ns)
    assert len(pts) == Ns and (np.diff(lnk) >= 0).all()  # they come by link: the order of the launch
    return pts, lnk


def _big_guarded(pts, lnk):
    """The seeded guard loop on the multilinear field for samples of one's own, with 5 active samples beyond index 511."""
    spec = get_hand_spec("allegro")
    for seed in range(100 * BIG_B + len(pts), 100 * BIG_B + len(pts) + 200):
        hp = _pose(spec, BIG_B, seed)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), _field("multilinear"), BIG_MARGIN, BIG_D, BIG_K)
        if _conditions(ref, BIG_MARGIN, len(pts), BIG_B, False) and _tail_active(ref) >= 5:
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


@pytest.mark.parametrize("Ns", [577, 1100])
def test_more_than_512_samples_match_the_oracle(gq, Ns):
    """A wavefront's second and third trip through the chunk loop, K = 3.  The oracle has 195 samples at indices >= 512 with an
    active station at Ns = 577 (every one of the 3 x 65) and 1183 at Ns = 1100; all station points lie inside the volume."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _big_samples(Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns and np.array_equal(samples.link.cpu().numpy(), lnk)
    hp, ref = _big_guarded(pts, lnk)
    tag = f"allegro Ns={Ns} B={BIG_B} K={BIG_K} D={BIG_D} multilinear margin={BIG_MARGIN}"
    _assert_guards(ref, BIG_MARGIN, tag, Ns, BIG_B, BIG_K, False)
    print(f"[{tag}] samples at indices >= 512 with an active station: {_tail_active(ref)}")
    assert _tail_active(ref) >= 5 and ref["inside"].all()
    got = _op(gq, hand, samples, hp, _field("multilinear").scene(gq), spec.grasp_axis, BIG_D, BIG_K, BIG_MARGIN)
    _assert_matches(got, (ref["E"], ref["grad"]), tag)


def test_second_chunk_run_to_run_sample_order_and_a_link_without_samples(gq):
    """Ns = 577 through the C entry: bitwise run to run; the samples by link against the same samples shuffled, within the
    bounds of ``_assert_matches`` (the order of the samples moves the last bits only); a link without samples."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    (p1, l1), (p2, l2) = _big_samples(577), _big_samples(1100)
    pts = np.concatenate([p1[l1 != 3], p2[l2 != 3]])[:577]  # 577 samples, none on link 3
    lnk = np.concatenate([l1[l1 != 3], l2[l2 != 3]])[:577]
    assert len(pts) == 577
    scene = _field("multilinear").scene(gq)
    hp, ref = _big_guarded(pts, lnk)
    B, L = BIG_B, hand.L
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)

    def run(p, l, accumulate=0, bufs=None):
        p, l = torch.tensor(p).cuda(), torch.tensor(l.astype(np.int32)).cuda()
        wrench, gRt = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"))
        e = torch.empty(B, device="cuda")
        gq.ops._approach_call(scene.grid, BIG_MARGIN, BIG_D, BIG_K, hp, p, l, L, Rg.contiguous(), LT.contiguous(), spec.grasp_axis,
                              None, 1.5, e, accumulate, wrench, gRt)
        torch.cuda.synchronize()
        return wrench, gRt, e

    order = np.argsort(lnk, kind="stable")
    by_link, again = run(pts[order], lnk[order]), run(pts[order], lnk[order])
    for a, b in zip(by_link, again):
        assert torch.equal(a, b)
    np.testing.assert_allclose(by_link[2].cpu().numpy(), ref["E"], rtol=1e-5, atol=1e-6)
    perm = np.random.default_rng(577).permutation(577)
    assert not (np.diff(lnk[perm]) >= 0).all()
    shuffled = run(pts[perm], lnk[perm])
    grad = lambda r: np.concatenate([r[0].cpu().numpy().reshape(B, -1), r[1].cpu().numpy()], 1)
    _assert_matches((shuffled[2].cpu().numpy(), grad(shuffled)), (by_link[2].cpu().numpy(), grad(by_link)), "Ns=577 shuffled vs by link")
    for r in (by_link, shuffled):
        assert (r[0][:, 3] == 0).all() and r[0].abs().max() > 0  # the link without samples: zero wrench
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12))]
    acc = run(pts[order], lnk[order], 1, [p.clone() for p in pre])
    for a, p, v in zip(acc[:2], pre, by_link[:2]):
        assert torch.equal(a, p + v)
    assert torch.equal(acc[0][:, 3], pre[0][:, 3])  # left alone


# ---------------------------------------------------------------------------------------------------------------
# 2. affine field: the closed form phi(x_w) - d_k n . (R a)
# ---------------------------------------------------------------------------------------------------------------
def test_affine_field_closed_form(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, K, D, margin = 128, 3, 4, 0.08, 0.01
    pts, lnk = _samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp, ref = _guarded("allegro", Ns, B, K, D, "affine", margin)
    F = _field("affine")
    _assert_guards(ref, margin, "affine", Ns, B, K, False)
    assert ref["inside"].all()
    at_pose = so.e_scene(spec, pts, lnk, hp.double(), F, margin)  # phi at the unshifted samples
    assert at_pose["inside"].all()
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(B, 1, dtype=torch.long))
    n = np.array([0.36, -0.48, 0.8])
    slope = (oh.global_rotation @ oh.grasp_axis).numpy() @ n  # (B): n . (R a)
    closed = sum(np.maximum(margin - (at_pose["phi"] - (D * k / K) * slope[:, None]), 0.0).sum(-1) for k in range(1, K + 1)) / K
    np.testing.assert_allclose(ref["E"], closed, rtol=1e-9, atol=1e-12)  # the oracle agrees with the closed form
    got = _op(gq, hand, samples, hp, F.scene(gq), spec.grasp_axis, D, K, margin)
    _assert_matches(got, (closed, ref["grad"]), "affine closed form")


# ---------------------------------------------------------------------------------------------------------------
# 3. K = 1 is the scene launch at the retreated pose
# ---------------------------------------------------------------------------------------------------------------
def test_one_station_equals_scene_terms_at_the_retreated_pose(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, D, margin = 512, 3, 0.08, 0.01
    pts, lnk = _samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp, ref = _guarded("allegro", Ns, B, 1, D, "multilinear", margin)
    _assert_guards(ref, margin, "K=1", Ns, B, 1, False)
    scene = _field("multilinear").scene(gq)
    got = _op(gq, hand, samples, hp, scene, spec.grasp_axis, D, 1, margin)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(B, 1, dtype=torch.long))
    hp2 = hp.clone()
    hp2[:, :3] = (hp[:, :3].double() - D * (oh.global_rotation @ oh.grasp_axis)).float()
    hpg, idx, Rg, LT, ws = _state(gq, hand, hp2)
    es = gq.ops.scene_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, margin)
    (3.0 * es).sum().backward()
    torch.cuda.synchronize()
    want = (es.detach().cpu().numpy(), hpg.grad.cpu().numpy())
    # both sides round on their own: 2 x the bounds; the rot6d columns differ by the derivative of the shift
    _assert_matches(got, want, "K=1 vs scene_terms d/dt", factor=2.0, cols=slice(0, 3))
    _assert_matches(got, want, "K=1 vs scene_terms d/dtheta", factor=2.0, cols=slice(9, None))
    _assert_matches(got, (ref["E"], ref["grad"]), "K=1 vs oracle")


# ---------------------------------------------------------------------------------------------------------------
# 4. a plane as the field: the mean over the stations of E_wall at the retreated poses
# ---------------------------------------------------------------------------------------------------------------
def test_plane_field_equals_the_mean_tabletop_wall(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, K, D, table_z = 512, 2, 3, 0.08, 0.03
    pts, lnk = _samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    F = so.plane(G_SHAPE, G_ORIGIN, G_H, table_z)
    for seed in range(300, 500):
        hp = _pose(spec, B, seed)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), F, 0.0, D, K)
        if _conditions(ref, 0.0, Ns, B, False) and ref["inside"].all():
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    _assert_guards(ref, 0.0, "plane", Ns, B, K, False)
    e, _ = _op(gq, hand, samples, hp, F.scene(gq), spec.grasp_axis, D, K, 0.0)
    oh = so.hand_oracle(spec, pts, lnk)
    oh.set_parameters(hp.double(), torch.zeros(B, 1, dtype=torch.long))
    back = oh.global_rotation @ oh.grasp_axis
    walls = []
    for k in range(1, K + 1):
        hpk = hp.clone()
        hpk[:, :3] = (hp[:, :3].double() - (D * k / K) * back).float()
        hpg, idx, Rg, LT, ws = _state(gq, hand, hpk)
        _, ew = gq.ops.tabletop_terms(hpg, hand, samples, idx, Rg, LT, ws, spec.grasp_axis, table_z)
        walls.append(ew.detach().double().cpu().numpy())
    want = sum(walls) / K
    print(f"[plane] E_approach vs mean E_wall max abs diff {np.abs(e - want).max():.3e} (max {want.max():.3e})")
    assert (want > 0).all()
    np.testing.assert_allclose(e, want, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(e, ref["E"], rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------
# 5. stations leaving the volume
# ---------------------------------------------------------------------------------------------------------------
def test_last_stations_outside_the_volume(gq):
    """A 30^3 grid of 1 cm around the hand, a corridor of 40 cm in 4 stations: the hand leaves the volume on its way."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    Ns, B, K, D, margin = 64, 1, 4, 0.40, 0.01
    pts, lnk = _samples("allegro", Ns)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    F = so.random_field((30, 30, 30), (-0.15137, -0.14291, -0.15173), 0.01, 5)
    for seed in range(200):
        hp = _pose(spec, B, seed, spread=0.02)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), F, margin, D, K)
        face, near = ao.guards(ref, margin)
        ins = ref["inside"].sum(axis=(0, 2))
        if face >= ao.FACE and near >= ao.NEAR and ins[0] >= 10 and ins[-1] == 0 and ref["active"].sum() >= 5:
            break
    else:
        raise AssertionError("no seeded pose passes the guards")
    print(f"[leaving] points inside per station {ins.tolist()}, active per station {ref['active'].sum(axis=(0, 2)).tolist()}")
    assert B * Ns * K <= 512 and face >= ao.FACE and near >= ao.NEAR
    # an independent test of the box: the points outside contribute exactly nothing
    lo = np.asarray(F.origin, dtype=np.float64)
    hi = lo + float(F.voxel) * (np.array(F.shape) - 1)
    assert np.array_equal(((ref["x"] >= lo) & (ref["x"] <= hi)).all(-1), ref["inside"])
    assert not ref["active"][:, -1].any() and ref["active"][:, 0].any()
    _assert_matches(_op(gq, hand, samples, hp, F.scene(gq), spec.grasp_axis, D, K, margin), (ref["E"], ref["grad"]), "leaving")


def test_everything_outside_the_volume(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _samples("allegro", 512)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp = _pose(spec, 3, 1)
    hp[:, 0] += 10.0
    e, g = _op(gq, hand, samples, hp, _field("random").scene(gq), spec.grasp_axis, 0.08, 4, 0.01)
    assert (e == 0).all() and (g == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. per-row upstream, accumulate, reproducibility, NaN (the C entry itself)
# ---------------------------------------------------------------------------------------------------------------
def _without_link_3(Ns):
    pts, lnk = _samples("allegro", Ns)
    return pts[lnk != 3], lnk[lnk != 3]


def _guarded_no_link_3(B, K, D, margin):
    spec = get_hand_spec("allegro")
    pts, lnk = _without_link_3(128)
    for seed in range(700, 900):
        hp = _pose(spec, B, seed)
        ref = ao.e_approach(spec, pts, lnk, hp.double(), _field("multilinear"), margin, D, K)
        if _conditions(ref, margin, len(pts), B, False):
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


def test_upstream_vectors_accumulate_and_reproducibility(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _without_link_3(128)  # a link without samples, Ns not a multiple of 64
    assert 64 < len(pts) < 128
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    B, L, K, D, margin = 7, hand.L, 4, 0.08, 0.01
    scene = _field("multilinear").scene(gq)
    hp, ref = _guarded_no_link_3(B, K, D, margin)
    assert B * len(pts) * K <= 4096
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)

    def run(up, w, accumulate, bufs=None):
        wrench, gRt = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"))
        e = torch.empty(B, device="cuda")
        gq.ops._approach_call(scene.grid, margin, D, K, hp, samples.points, samples.link, L, Rg.contiguous(), LT.contiguous(),
                              spec.grasp_axis, up, w, e, accumulate, wrench, gRt)
        torch.cuda.synchronize()
        return wrench, gRt, e

    one = run(None, 1.0, 0)
    again = run(None, 1.0, 0)
    for a, b in zip(one, again):
        assert torch.equal(a, b)
    assert (one[0][:, 3] == 0).all() and one[0].abs().max() > 0  # the link without samples: zero wrench
    np.testing.assert_allclose(one[2].cpu().numpy(), ref["E"], rtol=1e-5, atol=1e-6)
    # gsum = -sum_l f_l
    np.testing.assert_allclose(one[1][:, :3].cpu().numpy(), -one[0][:, :, :3].sum(1).cpu().numpy(), rtol=1e-5,
                               atol=4 * EPS32 * float(one[0].abs().max()) * L)
    # a non-uniform upstream per row == the per-row scaled result (up * (1/K) rounds once more than the scalar)
    uw = torch.linspace(0.5, 3.0, B, device="cuda")
    vec = run(uw, 0.0, 0)
    for got, unit, u in ((vec[0], one[0], uw.view(B, 1, 1)), (vec[1], one[1], uw.view(B, 1))):
        want = unit * u
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=6 * EPS32, atol=6 * EPS32 * float(want.abs().max()))
    assert torch.equal(vec[2], one[2])  # the energy is unweighted
    # accumulate = 1 on pre-filled buffers == pre-fill + the accumulate = 0 result, bit for bit
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12))]
    acc = run(uw, 0.0, 1, [p.clone() for p in pre])
    for a, p, v in zip(acc[:2], pre, vec[:2]):
        assert torch.equal(a, p + v)
    assert torch.equal(acc[0][:, 3], pre[0][:, 3])  # left alone


def test_nan_translation_gives_a_nan_row_and_leaves_the_others(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _samples("allegro", 512)
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    scene = _field("random").scene(gq)
    hp = _pose(spec, 4, 2, spread=0.05).cuda()
    B, L = hp.shape[0], hand.L
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
    bad = hp.clone()
    bad[2, 1] = float("nan")
    out = []
    for pose in (hp, bad):
        e, wrench, gRt = torch.empty(B, device="cuda"), torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda")
        gq.ops._approach_call(scene.grid, 0.0, 0.08, 3, pose, samples.points, samples.link, L, Rg.contiguous(), LT.contiguous(),
                              spec.grasp_axis, None, 1.0, e, 0, wrench, gRt)  # raises if the launch returns an error
        torch.cuda.synchronize()
        out.append((e, wrench, gRt))
    keep = torch.tensor([0, 1, 3], device="cuda")
    assert torch.isnan(out[1][0][2]) and torch.isnan(out[1][2][2]).all()
    assert torch.isfinite(out[0][0]).all() and (out[0][0] > 0).all()
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a[keep], b[keep])


# ---------------------------------------------------------------------------------------------------------------
# 7. the fused launch against the class-surface composition
# ---------------------------------------------------------------------------------------------------------------
S_SHAPE, S_ORIGIN, S_H = (100, 100, 100), (-0.5013, -0.4987, -0.5021), 0.01
AP = dict(approach_distance=0.10, approach_stations=4)


@functools.lru_cache(maxsize=None)
def _wall(c=0.02):
    """A half-space through the workspace: a wall the hands of the fixtures reach into (that of tests/test_gpu_scene.py)."""
    return so.affine(S_SHAPE, S_ORIGIN, S_H, c=c)


def _class_surface(gq, g, hp, idx, sm, scene, margin, corridor=None):
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    hm = HandModel(get_hand_spec("allegro"), "cuda")
    hm.set_surface_points(*sm)
    if scene is not None:
        hm.set_scene(scene, margin)
    if corridor is not None:
        hm.set_approach(*corridor)
    be, n_obj = int(g["batch_size_each"]), int(g["n_obj"])
    om = ObjectModel(batch_size_each=be, num_samples=g["obj0_surface_points"].shape[0])
    om.initialize_from_meshes([g[f"obj{i}_face_verts"] for i in range(n_obj)],
                              surface_points_list=[g[f"obj{i}_surface_points"] for i in range(n_obj)])
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    return hm, om


def test_fused_launch_equals_the_class_surface(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    sm = (samples.points.cpu().numpy(), samples.link.cpu().numpy())
    scene, margin, D, K = _wall().scene(gq), 0.01, 0.10, 4
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    idx = torch.tensor(g["contact_idx"]).cuda()
    e_op, g_op = _op(gq, hand, samples, hp.cpu(), scene, spec.grasp_axis, D, K, margin, scale=1.0)
    hm, om = _class_surface(gq, g, hp, idx, sm, scene, margin, (D, K))
    assert hm.approach == (D, K, None) and hm.scene_margin == margin  # margin=None follows the scene's
    ref = ao.e_approach(spec, sm[0], sm[1], hp.double().cpu(), _wall(), margin, D, K)
    near = ao.guards(ref, margin)[1]
    print(f"[fused vs class surface] guard over {ref['active'].size} points: nearest |phi - margin| {near:.2e} m")
    assert near >= ao.NEAR and ref["active"].any(axis=(0, 2)).all()
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_approach"],
                              svd_gain=0.1)
    e_cls = losses["E_approach"].detach().cpu().numpy()
    assert (e_cls > 0).any()
    print(f"[fused vs class surface] E_approach max abs diff {np.abs(e_op - e_cls).max():.3e} (max {e_cls.max():.3e})")
    np.testing.assert_allclose(e_op, e_cls, rtol=1e-5, atol=1e-6)
    losses["E_approach"].sum().backward()
    g_cls = hm.hand_pose.grad.cpu().numpy()
    gerr = np.linalg.norm(g_cls - g_op) / np.linalg.norm(g_op)
    print(f"[class surface vs approach_terms] grad rel diff {gerr:.3e}")
    assert gerr <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# 8. the stepper
# ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, g, n_contact, hand=None, **kw):
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    return gq.stepper.GraspStepper(hand or _hand("allegro"), gq.ops.MeshSet(fvs), torch.tensor(sps), be, n_contact, **kw)


STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")
TT = {"E_prior": 2.0, "E_wall": 3.0}


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
    with_term = dict(base, weights=dict(w, E_approach=0.0), approach_distance=0.07, approach_stations=5, approach_margin=0.02)
    if not scene_on:
        with_term.update(scene=_wall().scene(gq))
    sts = [_stepper(gq, g, 4, **dict(base, weights=w or None)), _stepper(gq, g, 4, **with_term)]
    assert not sts[1].approach_mode and sts[1].term_names == sts[0].term_names and "E_approach" not in sts[1].term_names
    assert sts[1]._fuse_loop == sts[0]._fuse_loop == (not (tabletop or scene_on)) and sts[1].terms.shape == sts[0].terms.shape
    assert (sts[1].samples is None) == (sts[0].samples is None) and (sts[1].scene is None) == (not scene_on)
    for st in sts:
        st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
        for s in (1, 2, 3):
            st.step(draws=(f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")))
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(sts[0], k), getattr(sts[1], k)), k


@pytest.mark.parametrize("tabletop,scene_on", [(False, False), (False, True), (True, True)])
def test_stepper_evaluate_in_approach_mode(gq, golden_dir, tabletop, scene_on):
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
    base = dict(surface_samples=sm, scene=scene, scene_margin=0.005)
    st0 = _stepper(gq, g, 4, **dict(base, weights=w0 or None))
    st1 = _stepper(gq, g, 4, **dict(base, weights=dict(w0, E_approach=w), approach_margin=margin, **AP))
    names = (["E_dis", "E_fc", "E_pen", "E_spen", "E_joints"] + (["E_prior", "E_wall"] if tabletop else []) +
             (["E_scene"] if scene_on else []) + ["E_approach"])
    assert st1.approach_mode and not st1._fuse_loop and st1.terms.shape == (len(names), hp.shape[0])
    assert st1.scene_mode == scene_on and st1.tabletop == tabletop and st1.approach_margin == margin
    t0, tot0, g0 = st0.evaluate(hp, idx)
    t1, tot1, g1 = st1.evaluate(hp, idx)
    torch.cuda.synchronize()
    assert list(t1) == names and list(t0) == names[:-1] and st1.term_names[-1] == "E_approach"
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    samples = gq.ops.SurfaceSamples(hand, *sm)
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    ea = gq.ops.approach_terms(hp, hand, samples, idx, Rg, LT, ws, scene, spec.grasp_axis, AP["approach_distance"],
                               AP["approach_stations"], margin)
    assert torch.equal(t1["E_approach"], ea) and (ea > 0).any()
    d_tot = (tot1.double() - tot0.double()).cpu().numpy()
    want = (w * ea.double()).cpu().numpy()
    rel = np.abs(d_tot - want) / np.abs(tot1.double().cpu().numpy())
    print(f"[evaluate tabletop={tabletop} scene={scene_on}] total - parts rel err max {rel.max():.3e}")
    assert rel.max() <= 3e-4
    ref = ao.e_approach(spec, sm[0], sm[1], hp.double().cpu(), F, margin, AP["approach_distance"], AP["approach_stations"], scale=w)
    assert ao.guards(ref, margin)[1] >= ao.NEAR
    want_g = g0.double().cpu().numpy() + ref["grad"]
    gerr = np.linalg.norm(g1.double().cpu().numpy() - want_g) / np.linalg.norm(want_g)
    print(f"[evaluate tabletop={tabletop} scene={scene_on}] grad vs sum of parts rel err {gerr:.3e}")
    assert gerr <= 1e-3  # the bound of tests/test_gpu_scene.py::test_stepper_evaluate_in_scene_mode for the same sum


def test_approach_iterations_match_the_class_surface(gq, golden_dir):
    """Five iterations (the third one re-initialises two rows), teacher-forced from the class-surface state: the loop of
    tests/test_gpu_scene.py::test_scene_iterations_match_the_class_surface with the scene and the approach term."""
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
    w = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0, "E_scene": 50.0, "E_approach": 20.0}
    st = _stepper(gq, g, 4, weights={"E_scene": 50.0, "E_approach": 20.0}, surface_samples=sm, scene=scene, scene_margin=margin, **AP)
    assert st.term_names[-2:] == ("E_scene", "E_approach") and st.approach_margin == margin
    hm, om = _class_surface(gq, g, f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda(), sm, scene, margin,
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
        print(f"[iteration {s}] total_new rel err max {rel.max():.3e}, E_approach max {float(st.terms_new[6].max()):.4f}, "
              f"min margin {float((u_ac - p).abs().min()):.3e}, accepted {int(accept.sum())}/{B}")
        assert rel.max() < 3e-4, rel
        assert float(st.terms_new[6].max()) > 0, "no station point inside the wall in this iteration"
        for i, k in ((5, "E_scene"), (6, "E_approach")):
            np.testing.assert_allclose(st.terms_new[i].cpu().numpy(), losses[k].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
        assert st.accept.bool().tolist() == accept.tolist()
        if s == 3:
            assert accept[mask.cuda()].all()
        acc = st.accept.bool()
        assert torch.equal(st.terms[6][acc], st.terms_new[6][acc])
        assert torch.equal(st.terms[6][~acc], terms_before[6][~acc])
        np.testing.assert_allclose(st.energy.cpu().numpy(), energy.cpu().numpy(), rtol=3e-4)
        np.testing.assert_allclose(st.hand_pose.cpu().numpy(), hm.hand_pose.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
        assert torch.equal(st.contact_idx, hm.contact_point_indices)


def _graph_scene(B):
    spec = get_hand_spec("allegro")
    fv = meshes.icosphere(2, 0.05)
    sp = torch.tensor(meshes.surface_points(fv, 256, oversample=4))[None]
    n = 4
    gen = torch.Generator().manual_seed(B)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen), dim=-1) * 0.12
    hp = torch.cat([t, torch.randn(B, 6, generator=gen), torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(B, spec.n_dofs, generator=gen)], 1).cuda()
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda()
    draws = [(torch.rand(B, n, generator=gen).cuda(), torch.randint(spec.n_contact_candidates, (B, n), generator=gen).cuda(),
              torch.rand(B, generator=gen).cuda()) for _ in range(3)]
    return fv, sp, n, hp, idx, draws


@pytest.mark.parametrize("B,mode,w_scene,energy_type,optimizer",
                         [(8, "one grid", 50.0, "graspqp", "mala_star"), (384, "graph branches", 50.0, "graspqp", "mala_star"),
                          (8, "one grid", 0.0, "graspqp", "mala_star"), (8, "one grid", 50.0, "dexgrasp", "dexgraspnet")])
def test_graph_replay_equals_eager_steps(gq, golden_dir, B, mode, w_scene, energy_type, optimizer):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    weights = {"E_scene": w_scene, "E_approach": 20.0}
    out = []
    for graph in (False, True):
        st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights=weights, surface_samples=sm,
                                     scene=_wall().scene(gq), scene_margin=0.01, energy_type=energy_type, optimizer=optimizer, **AP)
        st.reset(hp, idx)
        assert st.term_names[-1] == "E_approach" and float(st.terms[-1].max()) > 0
        assert st.scene_mode == (w_scene > 0) and len(st.term_names) == (7 if w_scene > 0 else 6)
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
    """An object given as an oriented point cloud, and ``run`` with a reset iteration, in approach mode."""
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    B = 8
    fv, sp, n, hp, idx, _ = _graph_scene(B)
    pts = sp[0].numpy().astype(np.float32)
    nrm = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    st = gq.stepper.GraspStepper(hand, gq.ops.PointCloudSet([pts], [nrm]), sp, B, n, weights={"E_approach": 20.0},
                                 surface_samples=sm, scene=_wall().scene(gq), scene_margin=0.01, **AP)
    assert st.cloud and st.approach_mode and not st.scene_mode and st.term_names[-1] == "E_approach"
    st.reset(hp, idx)
    assert float(st.terms[-1].max()) > 0
    st.capture()
    st.run(6, reset_epochs=None)
    torch.cuda.synchronize()
    assert torch.isfinite(st.energy).all() and torch.isfinite(st.terms).all() and torch.isfinite(st.hand_pose).all()


def test_obstacles_moved_in_place_between_graph_replays(gq, golden_dir):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    B = 8
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    F1, F2 = _wall(), _wall(-0.01)  # the wall moves 3 cm
    mk = lambda scene: gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights={"E_approach": 20.0},
                                               surface_samples=sm, scene=scene, scene_margin=0.01, **AP)
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
    with pytest.raises(ValueError, match="E_approach"):
        _stepper(gq, g, 4, weights={"E_approach": 1.0})  # no scene
    with pytest.raises(ValueError, match="E_approach"):
        _stepper(gq, g, 4, weights={"E_approach": -1.0}, scene=scene)
    for kw, word in ((dict(approach_distance=0.0), "approach_distance"), (dict(approach_distance=float("nan")), "approach_distance"),
                     (dict(approach_stations=0), "approach_stations"), (dict(approach_stations=33), "approach_stations"),
                     (dict(approach_stations=2.5), "approach_stations"), (dict(approach_margin=-0.01), "approach_margin")):
        with pytest.raises(ValueError, match=word):
            _stepper(gq, g, 4, weights={"E_approach": 1.0}, scene=scene, **kw)
    _stepper(gq, g, 4, weights={"E_approach": 1.0}, scene=scene, approach_stations=32)  # the limits are accepted
    _stepper(gq, g, 4, weights={"E_approach": 1.0}, scene=scene, approach_stations=1)
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    sm = (g["opt_surface_points"], g["opt_surface_link"])
    hm, om = _class_surface(gq, g, hp, torch.tensor(g["contact_idx"]).cuda(), sm, None, 0.0)
    with pytest.raises(ValueError, match="set_scene"):
        hm.set_approach(0.1, 4)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    with pytest.raises(ValueError, match="E_approach"):
        calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_approach"], svd_gain=0.1)
    hm.set_scene(scene, 0.01)
    with pytest.raises(ValueError, match="E_approach"):  # a scene, but no corridor
        calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_approach"], svd_gain=0.1)
    for args, word in (((0.0, 4), "distance"), ((0.1, 0), "stations"), ((0.1, 33), "stations"), ((0.1, 4, -1.0), "margin")):
        with pytest.raises(ValueError, match=word):
            hm.set_approach(*args)
    # the op's own refusals come from gq_approach_check
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, *sm)
    idx = torch.zeros(hp.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    for axis, D, K, word in (((0.0, 0.0, 1.0), 0.1, 33, "n_stations"), ((0.0, 0.0, 1.0), -0.1, 4, "distance"),
                             ((0.0, 0.0, 0.0), 0.1, 4, "grasp_axis")):
        with pytest.raises(ValueError, match=f"approach.*{word}"):
            gq.ops.approach_terms(hp, hand, samples, idx, Rg, LT, ws, scene, axis, D, K, 0.0)
