"""GPU tests of the scene term (E_scene on a signed-distance grid of the surroundings): the query and the fused launch against
the contract written in torch fp64 (tests/_scene_oracle.py), the shapes at which the kernel can go wrong, the C entry's
accumulate / upstream / reproducibility rules, the set-up constructors, and the stepper's scene mode (evaluation, iterations
against the class surface, hipGraph replay, obstacles moved in place).

Bounds: values rtol 1e-5 / atol 1e-6 and gradients norm-wise 1e-4 (those of tests/test_gpu_tabletop.py); a new energy against
the class surface 3e-4 (test_mala_iterations_match_reference_optimizer); the SDF bound of DESIGN 3 for the constructors.

Test fields: (a) affine and (b) global multilinear are reproduced exactly by every cell, so their oracle is the analytic formula;
(c) random node values are the only kind that exposes a wrong cell, and their cases assert two guards on the INPUTS, computed by
the fp64 oracle: no sample coordinate within 1e-4 cells of a cell face, no sample with |phi - margin| < 2e-5."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401
from ref_cpu import sdf as osdf  # noqa: E402

import _scene_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)
ORIGIN, H = (-0.40137, -0.40291, -0.40173), 0.01  # the inputs the face guard was checked with (7.8e-4 cells at the closest)
DZ = (0.0, 0.1, 0.15)


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


@functools.lru_cache(maxsize=None)
def _field(kind, shape=(80, 80, 80), origin=ORIGIN, voxel=H, seed=5):
    if kind == "affine":
        return so.affine(shape, origin, voxel)
    if kind == "multilinear":
        return so.multilinear(shape, origin, voxel)
    if kind == "random":
        return so.random_field(shape, origin, voxel, seed)
    raise KeyError(kind)


def _op(gq, hand, samples, hp32, scene, margin, scale=3.0):
    """The op on the GPU: (E_scene, d (scale E_scene) / d hand_pose) as numpy."""
    hpg = hp32.clone().cuda().requires_grad_()
    idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
    e = gq.ops.scene_terms(hpg, hand, samples, idx, Rg, LT, ws, scene, margin)
    (scale * e).sum().backward()
    torch.cuda.synchronize()
    return e.detach().cpu().numpy(), hpg.grad.cpu().numpy()


def _assert_matches(got, ref, tag):
    e, g = got
    re_, rg = ref
    gerr = np.linalg.norm(g - rg) / max(np.linalg.norm(rg), 1e-300)
    print(f"[{tag}] E_scene max abs err {np.abs(e - re_).max():.3e} (max {np.abs(re_).max():.3e}, max rel "
          f"{(np.abs(e - re_) / np.maximum(np.abs(re_), 1e-30)).max():.3e}), grad rel err {gerr:.3e}")
    np.testing.assert_allclose(e, re_, rtol=1e-5, atol=1e-6, err_msg=f"{tag} E_scene")
    assert np.linalg.norm(g - rg) <= 1e-4 * np.linalg.norm(rg), tag


def _assert_guards(res, margin, tag, min_active=5):
    face, near = so.guards(res, margin)
    n_act = int(res["active"].sum())
    print(f"[{tag}] guards: nearest cell face {face:.2e} cells, nearest |phi - margin| {near:.2e} m, active samples {n_act}")
    assert face >= so.FACE and near >= so.NEAR, (tag, face, near)
    assert n_act >= min_active, (tag, n_act)


# ---------------------------------------------------------------------------------------------------------------
# 1. the query: scene_distance on a (5,4,3) grid
# ---------------------------------------------------------------------------------------------------------------
Q_SHAPE, Q_ORIGIN, Q_H = (5, 4, 3), (-0.25, -0.25, -0.125), 0.125  # node positions and u at the nodes are exact in float32


def _query_points():
    """257 points: 240 seeded ones in and around the volume, then the special ones.  -> (points float32, indices by kind)."""
    rng = np.random.default_rng(3)
    lo, hi = np.array(Q_ORIGIN), np.array(Q_ORIGIN) + Q_H * (np.array(Q_SHAPE) - 1)
    x = rng.uniform(lo - 0.05, hi + 0.05, (257, 3)).astype(np.float32)
    f32 = np.float32
    nodes = [(1, 2, 1), (0, 0, 0), (4, 3, 2), (3, 0, 2)]  # on nodes, the first and the last one among them
    for k, ijk in enumerate(nodes):
        x[240 + k] = lo + Q_H * np.array(ijk)
    x[244] = (hi[0], -0.1, 0.03)  # on the last node plane of each axis: u = n - 1, inside
    x[245] = (0.1, hi[1], -0.06)
    x[246] = (-0.2, 0.05, hi[2])
    x[247] = (np.nextafter(f32(hi[0]), f32(np.inf)), -0.1, 0.03)  # one ulp beyond it: outside
    x[248] = (0.1, np.nextafter(f32(hi[1]), f32(np.inf)), -0.06)
    x[249] = (-0.2, 0.05, np.nextafter(f32(hi[2]), f32(np.inf)))
    x[250] = (np.nextafter(f32(lo[0]), f32(-np.inf)), 0.0, 0.0)  # one ulp before the first plane: outside
    x[251] = (100.0, 0.0, 0.0)  # far outside
    x[252] = (0.0, -1e30, 0.0)
    x[253] = (0.0, 0.0, 3e38)
    x[254] = (0.0, np.nan, 0.0)
    x[255] = (np.inf, 0.0, 0.0)
    x[256] = (0.0, 0.0, -np.inf)
    kinds = dict(random=np.arange(240), inside=np.arange(240, 247), outside=np.arange(247, 254), nonfinite=np.arange(254, 257))
    return x, kinds


@pytest.mark.parametrize("kind", ["affine", "multilinear", "random"])
def test_scene_distance_matches_the_oracle(gq, kind):
    F = _field(kind, Q_SHAPE, Q_ORIGIN, Q_H, 7)
    scene = F.scene(gq)
    x, kinds = _query_points()
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref = so.phi(F, x64)
    ins_ref, _, _, u = so.locate(F, x64.detach())
    fin = torch.isfinite(ref)
    ref[fin].sum().backward()
    rphi, rgrad, ins_ref = ref.detach().numpy(), x64.grad.numpy(), ins_ref.numpy()
    # the special points are where they should be, and the seeded ones stay clear of the cell faces (a guard on the inputs)
    assert ins_ref[kinds["inside"]].all() and not ins_ref[kinds["outside"]].any() and not ins_ref[kinds["nonfinite"]].any()
    assert 100 <= ins_ref[kinds["random"]].sum() <= 230
    ur = u.numpy()[kinds["random"]]
    assert np.abs(ur - np.round(ur)).min() >= so.FACE
    xg = torch.tensor(x, device="cuda", requires_grad=True)
    phi, grad, inside = gq.ops._Eager.scene_distance(xg.detach(), scene.values, list(scene.origin), scene.voxel)
    phi2 = gq.ops.scene_distance(xg, scene)
    up = torch.linspace(-1.0, 2.0, len(x), device="cuda")
    torch.where(torch.isfinite(phi2), phi2 * up, torch.zeros_like(phi2)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(phi, phi2.detach()) or (torch.equal(torch.isnan(phi), torch.isnan(phi2)) and
                                                torch.equal(phi[~torch.isnan(phi)], phi2.detach()[~torch.isnan(phi)]))
    p, g, ins = phi.cpu().numpy(), grad.cpu().numpy(), inside.cpu().numpy().astype(bool)
    assert np.array_equal(ins, ins_ref)
    gerr = np.linalg.norm(g[ins] - rgrad[ins]) / np.linalg.norm(rgrad[ins])
    print(f"[query {kind}] {int(ins.sum())} inside; phi max abs err {np.abs(p[ins] - rphi[ins]).max():.3e} (max |phi| "
          f"{np.abs(rphi[ins]).max():.3e}), grad rel err {gerr:.3e}")
    np.testing.assert_allclose(p[ins], rphi[ins], rtol=1e-5, atol=1e-6)
    assert gerr <= 1e-4
    out = np.concatenate([kinds["outside"], kinds["random"][~ins_ref[kinds["random"]]]])
    assert np.isposinf(p[out]).all() and (g[out] == 0).all() and not ins[out].any()
    assert np.isnan(p[kinds["nonfinite"]]).all() and not ins[kinds["nonfinite"]].any()
    # the last node plane takes the last cell with weight 1: phi is the node's own value on a node
    nodes = kinds["inside"][:4]
    ijk = np.round((x[nodes] - np.array(Q_ORIGIN)) / Q_H).astype(int)
    np.testing.assert_allclose(p[nodes], F.values.numpy()[ijk[:, 0], ijk[:, 1], ijk[:, 2]], rtol=0, atol=1e-7)
    # autograd through the op: grad * upstream, zero outside the volume
    gx = xg.grad
    want = grad * torch.where(torch.isfinite(phi), up, torch.zeros_like(up)).unsqueeze(-1)
    keep = torch.tensor(ins | np.isin(np.arange(len(x)), out), device="cuda")
    assert torch.equal(gx[keep], want[keep])
    assert (gx[torch.tensor(out, device="cuda")] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. scene_terms against the oracle on the sphere fixture
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["affine", "multilinear", "random"])
def test_scene_terms_match_the_oracle(gq, golden_dir, kind):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = g["opt_surface_points"], g["opt_surface_link"]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp32 = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    F = _field(kind, (62, 64, 80) if kind == "random" else (80, 80, 80))
    scene = F.scene(gq)
    for dz in DZ:
        hp = hp32.clone()
        hp[:, 2] += dz
        for margin in (0.0, 0.01):
            tag = f"{kind} dz={dz} margin={margin}"
            ref = so.e_scene(spec, pts, lnk, hp.double(), F, margin)
            assert ref["inside"].all()
            _assert_guards(ref, margin, tag)
            _assert_matches(_op(gq, hand, samples, hp, scene, margin), (ref["E"], ref["grad"]), tag)


# ---------------------------------------------------------------------------------------------------------------
# 3. a plane as the field: E_scene is E_wall
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_z", [0.0, 0.03])
def test_plane_field_equals_the_tabletop_wall(gq, golden_dir, table_z):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = g["opt_surface_points"], g["opt_surface_link"]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp32 = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    F = so.plane((80, 80, 80), ORIGIN, H, table_z)
    scene = F.scene(gq)
    for dz in DZ:
        hp = hp32.clone()
        hp[:, 2] += dz
        ref = so.e_scene(spec, pts, lnk, hp.double(), F, 0.0)
        _assert_guards(ref, 0.0, f"plane {table_z} dz={dz}")
        assert ref["inside"].all() and np.abs(ref["phi"]).min() >= (3e-4 if table_z == 0.0 else so.NEAR)
        e, ge = _op(gq, hand, samples, hp, scene, 0.0)
        hpg = hp.clone().cuda().requires_grad_()
        idx = torch.zeros(hpg.shape[0], 1, dtype=torch.long, device="cuda")
        Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hpg.detach(), idx, hand)
        _, ew = gq.ops.tabletop_terms(hpg, hand, samples, idx, Rg, LT, ws, spec.grasp_axis, table_z)
        (3.0 * ew).sum().backward()
        torch.cuda.synchronize()
        _assert_matches((e, ge), (ew.detach().cpu().numpy(), hpg.grad.cpu().numpy()), f"plane {table_z} dz={dz} vs E_wall")
        _assert_matches((e, ge), (ref["E"], ref["grad"]), f"plane {table_z} dz={dz} vs oracle")


# ---------------------------------------------------------------------------------------------------------------
# 4. shapes where the kernel can go wrong
# ---------------------------------------------------------------------------------------------------------------
def _guarded_pose(spec, B, pts, lnk, F, margin, seed0, min_active, spread=0.1, cells=True):
    """Seeded pose whose samples pass the guards (the cell-face one only if ``cells``: on a field every cell reproduces the
    cell cannot matter) and of which at least ``min_active`` are active; the next seed is drawn otherwise.  -> (pose float32, oracle results at that float32 pose)."""
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        t = spread * torch.randn(B, 3, generator=gen)
        th = torch.tensor(spec.default_state)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=gen)
        hp = torch.cat([t, torch.randn(B, 6, generator=gen), th], 1).float()
        ref = so.e_scene(spec, pts, lnk, hp.double(), F, margin)
        face, near = so.guards(ref, margin)
        if (face >= so.FACE or not cells) and near >= so.NEAR and ref["active"].sum() >= min_active:
            return hp, ref
    raise AssertionError("no seeded pose passes the guards")


@pytest.mark.parametrize("hand_name,Ns", [("allegro", 1), ("allegro", 63), ("allegro", 65), ("allegro", 512), ("panda", 512),
                                          ("schunk2", 512)])
def test_op_shapes_match_the_oracle(gq, hand_name, Ns):
    spec, hand = get_hand_spec(hand_name), _hand(hand_name)
    pts, lnk = _default_samples(hand_name)
    if Ns < 512:  # a seeded subset, in shuffled order (the term does not depend on the order of the samples)
        pick = np.random.default_rng(Ns).permutation(512)[:Ns]
        pts, lnk = pts[pick], lnk[pick]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns
    # one row on the random field (the cell matters), seven on the multilinear one (it does not: of 3 584 samples some always lie
    # within 1e-4 cells of a face, so no seeded pose would pass the random field's guard; the hinge guard holds for both)
    for B, kind, margin in ((1, "random", 0.0), (7, "multilinear", 0.01)):
        F = _field(kind, (100, 96, 104), (-0.5, -0.48, -0.52), 0.01, 11)
        scene = F.scene(gq)
        hp, ref = _guarded_pose(spec, B, pts, lnk, F, margin, 100 * B + Ns, min(5, Ns * B), cells=kind == "random")
        tag = f"{hand_name} Ns={Ns} B={B} {kind}"
        if kind == "random":
            _assert_guards(ref, margin, tag, min(5, Ns * B))
        assert so.guards(ref, margin)[1] >= so.NEAR and ref["active"].sum() >= min(5, Ns * B)
        _assert_matches(_op(gq, hand, samples, hp, scene, margin), (ref["E"], ref["grad"]), tag)


BIG_B, BIG_MARGIN = 3, 0.01  # more than 512 samples: 577 = 10 chunks (wavefront 1's second chunk holds one sample), 1100 = 18


@functools.lru_cache(maxsize=None)
def _big_case(Ns):
    """allegro, ``hand_surface_samples(spec, Ns)`` (they come by link, the order of the launch), B = 3 on the multilinear field; the
    first pose of the seeded guard loop, and the oracle's results at it."""
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, Ns)
    assert len(pts) == Ns and (np.diff(lnk) >= 0).all()
    F = _field("multilinear", (100, 96, 104), (-0.5, -0.48, -0.52), 0.01)
    hp, ref = _guarded_pose(spec, BIG_B, pts, lnk, F, BIG_MARGIN, 100 * BIG_B + Ns, 5, cells=False)
    return spec, pts, lnk, F, hp, ref


@pytest.mark.parametrize("Ns", [577, 1100])
def test_more_than_512_samples_match_the_oracle(gq, Ns):
    """A wavefront's second and third trip through the chunk loop.  The oracle has 195 active samples at indices >= 512 at
    Ns = 577 (every one of the 3 x 65) and 1189 at Ns = 1100; all samples lie inside the volume."""
    spec, pts, lnk, F, hp, ref = _big_case(Ns)
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    assert samples.Ns == Ns and np.array_equal(samples.link.cpu().numpy(), lnk)
    tag = f"allegro Ns={Ns} B={BIG_B} multilinear"
    tail = int(ref["active"][:, 512:].sum())
    print(f"[{tag}] active samples at indices >= 512: {tail}")
    assert tail >= 5 and ref["inside"].all()
    assert so.guards(ref, BIG_MARGIN)[1] >= so.NEAR
    _assert_matches(_op(gq, hand, samples, hp, F.scene(gq), BIG_MARGIN), (ref["E"], ref["grad"]), tag)


def _big_without_link_3():
    """577 samples of which none rides on link 3: the 577 of ``_big_case`` without that link's, topped up from the 1100."""
    (_, p1, l1, _, _, _), (_, p2, l2, _, _, _) = _big_case(577), _big_case(1100)
    k1, k2 = l1 != 3, l2 != 3
    pts, lnk = np.concatenate([p1[k1], p2[k2]])[:577], np.concatenate([l1[k1], l2[k2]])[:577]
    assert len(pts) == 577 and (lnk != 3).all()
    return pts, lnk


def test_second_chunk_run_to_run_sample_order_and_a_link_without_samples(gq):
    """Ns = 577 through the C entry: bitwise run to run; the samples by link against the same samples shuffled, within the
    bounds of ``_assert_matches`` (the order of the samples moves the last bits only); a link without samples."""
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _big_without_link_3()
    F = _big_case(577)[3]
    scene = F.scene(gq)
    hp, ref = _guarded_pose(spec, BIG_B, pts, lnk, F, BIG_MARGIN, 100 * BIG_B + 577, 5, cells=False)
    assert ref["active"][:, 512:].sum() >= 5
    B, L = BIG_B, hand.L
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)

    def run(p, l, accumulate=0, bufs=None):
        p, l = torch.tensor(p).cuda(), torch.tensor(l.astype(np.int32)).cuda()
        wrench, gRt = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"))
        e = torch.empty(B, device="cuda")
        gq.ops._scene_call(scene.grid, BIG_MARGIN, hp, p, l, L, Rg.contiguous(), LT.contiguous(), None, 1.5, e, accumulate, wrench, gRt)
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


@pytest.mark.parametrize("case", ["one cell", "30^3", "entirely outside"])
def test_hand_partly_or_entirely_outside_the_volume(gq, golden_dir, case):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = g["opt_surface_points"], g["opt_surface_link"]
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32)
    if case == "one cell":  # a (2,2,2) grid: one cell of 10 cm through the hand
        F = so.random_field((2, 2, 2), (-0.11754, -0.0486, -0.10234), 0.15, 2)
    else:
        F = _field("random", (30, 30, 30), (-0.15137, -0.10291, -0.20173), H, 5)
    if case == "entirely outside":
        hp[:, 0] += 10.0
    scene = F.scene(gq)
    ref = so.e_scene(spec, pts, lnk, hp.double(), F, 0.01)
    n_in, n_out = int(ref["inside"].sum()), int((~ref["inside"]).sum())
    e, ge = _op(gq, hand, samples, hp, scene, 0.01)
    if case == "entirely outside":
        assert n_in == 0
        assert (e == 0).all() and (ge == 0).all()
        return
    _assert_guards(ref, 0.01, case)
    assert n_in >= 20 and n_out >= 20, (n_in, n_out)
    # samples outside contribute exactly nothing: the oracle with those samples zeroed by an independent test of the box
    lo = np.asarray(F.origin, dtype=np.float64)
    hi = lo + float(F.voxel) * (np.array(F.shape) - 1)
    keep = ((ref["x"] >= lo) & (ref["x"] <= hi)).all(-1)
    assert np.array_equal(keep, ref["inside"])
    ref2 = so.e_scene(spec, pts, lnk, hp.double(), F, 0.01, keep=torch.tensor(keep))
    assert np.array_equal(ref2["E"], ref["E"])
    _assert_matches((e, ge), (ref["E"], ref["grad"]), case)


# ---------------------------------------------------------------------------------------------------------------
# 5. per-row upstream, accumulate, reproducibility (the C entry itself)
# ---------------------------------------------------------------------------------------------------------------
def test_upstream_vectors_accumulate_and_reproducibility(gq):
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    pts, lnk = _default_samples("allegro")
    pts, lnk = pts[lnk != 3], lnk[lnk != 3]  # a link without samples
    samples = gq.ops.SurfaceSamples(hand, pts, lnk)
    B, L = 7, hand.L
    F = _field("random", (100, 96, 104), (-0.5, -0.48, -0.52), 0.01, 11)
    scene = F.scene(gq)
    hp, ref = _guarded_pose(spec, B, pts, lnk, F, 0.01, 7, 5)
    hp = hp.cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)

    def run(up, w, accumulate, bufs=None):
        wrench, gRt = bufs or (torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda"))
        e = torch.empty(B, device="cuda")
        gq.ops._scene_call(scene.grid, 0.01, hp, samples.points, samples.link, L, Rg.contiguous(), LT.contiguous(), up, w, e,
                           accumulate, wrench, gRt)
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
    # a non-uniform upstream per row == the per-row scaled result (one rounding apart)
    uw = torch.linspace(0.5, 3.0, B, device="cuda")
    vec = run(uw, 0.0, 0)
    for got, unit, u in ((vec[0], one[0], uw.view(B, 1, 1)), (vec[1], one[1], uw.view(B, 1))):
        want = unit * u
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=4 * EPS32, atol=4 * EPS32 * float(want.abs().max()))
    assert torch.equal(vec[2], one[2])  # the energy is unweighted
    sca = run(None, 2.5, 0)
    np.testing.assert_allclose(sca[0].cpu().numpy(), (2.5 * one[0]).cpu().numpy(), rtol=4 * EPS32,
                               atol=4 * EPS32 * float(one[0].abs().max()) * 2.5)
    # accumulate = 1 on pre-filled buffers == pre-fill + the accumulate = 0 result, bit for bit
    gen = torch.Generator().manual_seed(1)
    pre = [torch.randn(*s, generator=gen).cuda() for s in ((B, L, 6), (B, 12))]
    acc = run(uw, 0.0, 1, [p.clone() for p in pre])
    for a, p, v in zip(acc[:2], pre, vec[:2]):
        assert torch.equal(a, p + v)
    assert torch.equal(acc[0][:, 3], pre[0][:, 3])  # left alone


# ---------------------------------------------------------------------------------------------------------------
# 6. the fused launch against the query, and the class surface
# ---------------------------------------------------------------------------------------------------------------
def _class_surface(gq, g, hp, idx, sm, scene, margin):
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel

    hm = HandModel(get_hand_spec("allegro"), "cuda")
    hm.set_surface_points(*sm)
    if scene is not None:
        hm.set_scene(scene, margin)
    be, n_obj = int(g["batch_size_each"]), int(g["n_obj"])
    om = ObjectModel(batch_size_each=be, num_samples=g["obj0_surface_points"].shape[0])
    om.initialize_from_meshes([g[f"obj{i}_face_verts"] for i in range(n_obj)],
                              surface_points_list=[g[f"obj{i}_surface_points"] for i in range(n_obj)])
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    return hm, om


def test_fused_launch_equals_the_query_and_the_class_surface(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    sm = (samples.points.cpu().numpy(), samples.link.cpu().numpy())
    F = _field("random", (62, 64, 80))
    scene = F.scene(gq)
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    hp[:, 2] += 0.1
    idx = torch.tensor(g["contact_idx"]).cuda()
    margin = 0.01
    e_op, g_op = _op(gq, hand, samples, hp.cpu(), scene, margin, scale=1.0)
    hm, om = _class_surface(gq, g, hp, idx, sm, scene, margin)
    phi = gq.ops.scene_distance(hm.get_surface_points().detach(), scene)
    hinge = torch.relu(margin - phi).sum(-1).cpu().numpy()
    assert (hinge > 0).all()
    print(f"[fused vs query] E_scene max abs diff {np.abs(e_op - hinge).max():.3e} (max {hinge.max():.3e})")
    np.testing.assert_allclose(e_op, hinge, rtol=1e-5, atol=1e-6)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    losses = calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_fc", "E_pen", "E_spen", "E_joints", "E_scene"],
                              svd_gain=0.1)
    np.testing.assert_allclose(losses["E_scene"].detach().cpu().numpy(), hinge, rtol=1e-5, atol=1e-6)
    losses["E_scene"].sum().backward()
    g_cls = hm.hand_pose.grad.cpu().numpy()
    gerr = np.linalg.norm(g_cls - g_op) / np.linalg.norm(g_op)
    print(f"[class surface vs scene_terms] grad rel diff {gerr:.3e}")
    assert gerr <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# 7. a NaN pose is ordinary input
# ---------------------------------------------------------------------------------------------------------------
def test_nan_translation_gives_a_nan_row_and_leaves_the_others(gq, golden_dir):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    hand = _hand("allegro")
    samples = gq.ops.SurfaceSamples(hand, g["opt_surface_points"], g["opt_surface_link"])
    scene = _field("random", (62, 64, 80)).scene(gq)
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    B, L = hp.shape[0], hand.L
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg, LT, _, _, _, _ = gq.ops.fk_contacts(hp, idx, hand)
    bad = hp.clone()
    bad[2, 1] = float("nan")
    out = []
    for pose in (hp, bad):
        e, wrench, gRt = torch.empty(B, device="cuda"), torch.empty(B, L, 6, device="cuda"), torch.empty(B, 12, device="cuda")
        gq.ops._scene_call(scene.grid, 0.0, pose, samples.points, samples.link, L, Rg.contiguous(), LT.contiguous(), None, 1.0, e,
                           0, wrench, gRt)  # raises if the launch returns an error
        torch.cuda.synchronize()
        out.append((e, wrench, gRt))
    keep = torch.tensor([0, 1, 3], device="cuda")
    assert torch.isnan(out[1][0][2]) and torch.isfinite(out[0][0]).all() and (out[0][0] > 0).all()
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a[keep], b[keep])


# ---------------------------------------------------------------------------------------------------------------
# 8. the set-up constructors
# ---------------------------------------------------------------------------------------------------------------
def _box_triangles(lo, hi):
    """A closed box as 12 triangles, outward orientation."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c = np.array([[lo[0] if not i & 1 else hi[0], lo[1] if not i & 2 else hi[1], lo[2] if not i & 4 else hi[2]] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # -z +z -y +y -x +x
    tris = []
    for a, b, cc, d in quads:
        tris += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    fv = np.array(tris, dtype=np.float32)
    n = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    assert (np.einsum("fk,fk->f", n, fv.mean(1) - 0.5 * (lo + hi)) > 0).all()
    return fv


def test_from_meshes_matches_the_sdf_oracle(gq, golden_dir):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    fvs = [_box_triangles((0.06, -0.05, -0.04), (0.12, 0.03, 0.05)), g["obj0_face_verts"]]
    origin, shape, voxel = (-0.081, -0.067, -0.071), (6, 5, 4), 0.04
    scene = gq.ops.SceneSDF.from_meshes(fvs, origin, shape, voxel)
    torch.cuda.synchronize()
    assert scene.shape == shape and scene.values.dtype == torch.float32 and scene.values.is_cuda
    nodes = scene.node_positions()
    assert nodes.shape == shape + (3,)
    x = nodes.reshape(-1, 3).cpu()
    want = np.asarray(origin)[None, None, None] + voxel * np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    np.testing.assert_allclose(nodes.cpu().numpy(), want, rtol=0, atol=1e-7)
    ref = None
    for fv in fvs:
        d2, sgn, _, _ = osdf.compute_sdf(x.double(), torch.as_tensor(fv, dtype=torch.float64))
        p = (sgn * d2.sqrt()).numpy()
        ref = p if ref is None else np.minimum(ref, p)
    got = scene.values.reshape(-1).cpu().numpy()
    print(f"[from_meshes] max abs err {np.abs(got - ref).max():.3e}, inside nodes {int((ref < 0).sum())} of {len(ref)}")
    assert (ref < 0).sum() >= 3 and (ref > 0).sum() >= 60  # phi is positive outside
    assert (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 2e-7).all()


def test_from_point_clouds_matches_the_cloud_contract(gq):
    """The box as an oriented cloud, against the surfel contract of DESIGN 13 evaluated in numpy fp64: nearest centre, disc of
    radius rho, sign of the height over it.  A node whose two nearest centres tie within 1e-5 may take either."""
    rng = np.random.default_rng(11)
    lo, hi = np.array([0.06, -0.05, -0.04]), np.array([0.12, 0.03, 0.05])
    ps, ns = [], []
    for a in range(3):
        for s, v in ((-1.0, lo[a]), (1.0, hi[a])):
            q = rng.uniform(lo, hi, (150, 3))
            q[:, a] = v
            nn = np.zeros((150, 3))
            nn[:, a] = s
            ps.append(q), ns.append(nn)
    p, n = np.concatenate(ps).astype(np.float32), np.concatenate(ns).astype(np.float32)
    origin, shape, voxel = (-0.081, -0.067, -0.071), (6, 5, 4), 0.04
    scene = gq.ops.SceneSDF.from_point_clouds([p], [n], origin, shape, voxel)
    rho = float(np.float32(meshes.cloud_radius(p)))
    x = scene.node_positions().reshape(-1, 3).cpu().numpy().astype(np.float64)
    got = scene.values.reshape(-1).cpu().numpy()
    d = ((x[:, None] - p[None].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]

    def surfel(j):
        pj, nj = p[j].astype(np.float64), n[j].astype(np.float64)
        v = x - pj
        h = (v * nj).sum(-1)
        lat = v - h[:, None] * nj
        ell = np.linalg.norm(lat, axis=1)
        closest = pj + lat * np.where(ell <= rho, 1.0, rho / np.maximum(ell, 1e-300))[:, None]
        return np.where(h >= 0, 1.0, -1.0) * np.linalg.norm(x - closest, axis=1)

    r1, r2 = surfel(order[:, 0]), surfel(order[:, 1])
    k = np.arange(len(x))
    tie = d[k, order[:, 1]] - d[k, order[:, 0]] <= 1e-5 * d[k, order[:, 1]] + 1e-12
    ok1 = np.abs(got - r1) <= 1e-4 * np.abs(r1) + 2e-7
    ok2 = np.abs(got - r2) <= 1e-4 * np.abs(r2) + 2e-7
    print(f"[from_point_clouds] rho {rho:.4e}, max abs err to the winner {np.abs(got - r1).max():.3e}, near-ties {int(tie.sum())}")
    assert (ok1 | (tie & ok2)).all() and tie.sum() <= 2
    assert (r1 < 0).sum() >= 1 and (r1 > 0).sum() >= 60


# ---------------------------------------------------------------------------------------------------------------
# 9. the stepper
# ---------------------------------------------------------------------------------------------------------------
S_SHAPE, S_ORIGIN, S_H = (100, 100, 100), (-0.5013, -0.4987, -0.5021), 0.01


@functools.lru_cache(maxsize=None)
def _wall(c=0.02):
    """A half-space through the workspace: a wall the hands of the fixtures reach into."""
    return so.affine(S_SHAPE, S_ORIGIN, S_H, c=c)


def _stepper(gq, g, n_contact, hand=None, **kw):
    n_obj, be = int(g["n_obj"]), int(g["batch_size_each"])
    fvs = [g[f"obj{i}_face_verts"] for i in range(n_obj)]
    sps = np.stack([g[f"obj{i}_surface_points"] for i in range(n_obj)])
    return gq.stepper.GraspStepper(hand or _hand("allegro"), gq.ops.MeshSet(fvs), torch.tensor(sps), be, n_contact, **kw)


STATE = ("hand_pose", "contact_idx", "energy", "grad", "terms", "ema", "step_count", "accept")
TT = {"E_prior": 2.0, "E_wall": 3.0}


@pytest.mark.parametrize("tabletop", [False, True])
def test_zero_weight_is_the_stepper_without_a_scene(gq, golden_dir, tabletop):
    g = _load(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    base = dict(weights=dict(TT), surface_samples=sm) if tabletop else {}
    with_scene = dict(base, scene=_wall().scene(gq), scene_margin=0.01)
    with_scene["weights"] = dict(base.get("weights", {}), E_scene=0.0)
    sts = [_stepper(gq, g, 4, **base), _stepper(gq, g, 4, **with_scene)]
    assert not sts[1].scene_mode and sts[1].scene is None and sts[1].term_names == sts[0].term_names
    assert sts[1]._fuse_loop == (not tabletop) and sts[1].terms.shape == sts[0].terms.shape
    assert (sts[1].samples is None) == (not tabletop)
    for st in sts:
        st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
        for s in (1, 2, 3):
            st.step(draws=(f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")))
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(sts[0], k), getattr(sts[1], k)), k


@pytest.mark.parametrize("tabletop", [False, True])
def test_stepper_evaluate_in_scene_mode(gq, golden_dir, tabletop):
    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec, hand = get_hand_spec("allegro"), _hand("allegro")
    sm = (g["opt_surface_points"], g["opt_surface_link"])
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    hp[:, 2] += 0.1
    idx = torch.tensor(g["contact_idx"]).cuda()
    F = _field("random", (62, 64, 80))
    scene, margin, w = F.scene(gq), 0.01, 50.0
    base = dict(weights=dict(TT), surface_samples=sm) if tabletop else dict(surface_samples=sm)
    st0 = _stepper(gq, g, 4, **base)
    st1 = _stepper(gq, g, 4, **dict(base, weights=dict(base.get("weights", {}), E_scene=w), scene=scene, scene_margin=margin))
    nT = 8 if tabletop else 6
    assert st1.scene_mode and not st1._fuse_loop and st1.terms.shape == (nT, hp.shape[0]) and st1.tabletop == tabletop
    t0, tot0, g0 = st0.evaluate(hp, idx)
    t1, tot1, g1 = st1.evaluate(hp, idx)
    torch.cuda.synchronize()
    names = ["E_dis", "E_fc", "E_pen", "E_spen", "E_joints"] + (["E_prior", "E_wall"] if tabletop else []) + ["E_scene"]
    assert list(t1) == names and list(t0) == names[:-1]
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k
    samples = gq.ops.SurfaceSamples(hand, *sm)
    Rg, LT, _, _, _, ws = gq.ops.fk_contacts(hp, idx, hand)
    es = gq.ops.scene_terms(hp, hand, samples, idx, Rg, LT, ws, scene, margin)
    assert torch.equal(t1["E_scene"], es) and (es > 0).all()
    d_tot = (tot1.double() - tot0.double()).cpu().numpy()
    want = (w * es.double()).cpu().numpy()
    rel = np.abs(d_tot - want) / np.abs(tot1.double().cpu().numpy())
    print(f"[evaluate tabletop={tabletop}] total - parts rel err max {rel.max():.3e}")
    assert rel.max() <= 3e-4
    ref = so.e_scene(spec, sm[0], sm[1], hp.double().cpu(), F, margin, scale=w)
    _assert_guards(ref, margin, f"evaluate tabletop={tabletop}")
    want_g = g0.double().cpu().numpy() + ref["grad"]
    gerr = np.linalg.norm(g1.double().cpu().numpy() - want_g) / np.linalg.norm(want_g)
    print(f"[evaluate tabletop={tabletop}] grad vs sum of parts rel err {gerr:.3e}")
    assert gerr <= 1e-3


def test_scene_iterations_match_the_class_surface(gq, golden_dir):
    """Five iterations (the third one re-initialises two rows), teacher-forced from the class-surface state: the loop of
    tests/test_gpu_tabletop.py::test_tabletop_iterations_match_the_class_surface with the scene term."""
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
    w = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0, "E_scene": 50.0}
    st = _stepper(gq, g, 4, weights={"E_scene": 50.0}, surface_samples=sm, scene=scene, scene_margin=margin)
    hm, om = _class_surface(gq, g, f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda(), sm, scene, margin)
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
        print(f"[iteration {s}] total_new rel err max {rel.max():.3e}, E_scene max {float(st.terms_new[5].max()):.4f}, "
              f"min margin {float((u_ac - p).abs().min()):.3e}, accepted {int(accept.sum())}/{B}")
        assert rel.max() < 3e-4, rel
        assert float(st.terms_new[5].max()) > 0, "no sample inside the wall in this iteration"
        np.testing.assert_allclose(st.terms_new[5].cpu().numpy(), losses["E_scene"].detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
        assert st.accept.bool().tolist() == accept.tolist()
        if s == 3:
            assert accept[mask.cuda()].all()
        acc = st.accept.bool()
        assert torch.equal(st.terms[5][acc], st.terms_new[5][acc])
        assert torch.equal(st.terms[5][~acc], terms_before[5][~acc])
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


@pytest.mark.parametrize("B,mode,tabletop", [(8, "one grid", False), (384, "graph branches", False), (8, "one grid", True)])
def test_graph_replay_equals_eager_steps(gq, golden_dir, B, mode, tabletop):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    weights = dict(TT, E_scene=50.0) if tabletop else {"E_scene": 50.0}
    out = []
    for graph in (False, True):
        st = gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights=weights, surface_samples=sm,
                                     scene=_wall().scene(gq), scene_margin=0.01)
        st.reset(hp, idx)
        assert float(st.terms[-1].max()) > 0 and st.term_names[-1] == "E_scene"
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


def test_obstacles_moved_in_place_between_graph_replays(gq, golden_dir):
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    hand = _hand("allegro")
    B = 8
    fv, sp, n, hp, idx, draws = _graph_scene(B)
    F1, F2 = _wall(), _wall(-0.01)  # the wall moves 3 cm
    mk = lambda scene: gq.stepper.GraspStepper(hand, gq.ops.MeshSet([fv]), sp, B, n, weights={"E_scene": 50.0}, surface_samples=sm,
                                               scene=scene, scene_margin=0.01)
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


# ---------------------------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(gq, golden_dir):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    g = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    with pytest.raises(ValueError, match="E_scene"):
        _stepper(gq, g, 4, weights={"E_scene": 1.0})
    with pytest.raises(ValueError, match="E_scene"):
        _stepper(gq, g, 4, weights={"E_scene": -1.0}, scene=_wall().scene(gq))
    hp = torch.tensor(g["opt_hand_pose"], dtype=torch.float32).cuda()
    hm, om = _class_surface(gq, g, hp, torch.tensor(g["contact_idx"]).cuda(), (g["opt_surface_points"], g["opt_surface_link"]),
                            None, 0.0)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    with pytest.raises(ValueError, match="E_scene"):
        calculate_energy(hm, om, energy_fnc=fn, energy_names=["E_dis", "E_scene"], svd_gain=0.1)
    # a hand with more than 64 links (a synthetic n_links)
    scene = _wall().scene(gq)
    scene.check(4, 64, 512)
    with pytest.raises(ValueError, match="scene.*n_links"):
        scene.check(4, 65, 512)
    with pytest.raises(ValueError, match="voxel"):
        gq.ops.SceneSDF(torch.zeros(2, 2, 2, device="cuda"), (0.0, 0.0, 0.0), 0.0)
    with pytest.raises(ValueError, match="nx"):
        gq.ops.SceneSDF(torch.zeros(1, 2, 2, device="cuda"), (0.0, 0.0, 0.0), 0.1)
