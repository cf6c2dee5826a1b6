"""The pruned cluster search of the contact query (csrc/sdf_dev.h: gq_sdf_wave_query) against the exhaustive fp64 oracle with tied
sets (tests/_sdf_set_oracle.py): stand-alone through ops.sdf_meshset -- one mesh, many meshes with ragged query counts on both
block mappings, two and four clusters per round -- and fused into the FK forward launch.  EVERY query is judged; a pruning miss
is an error of the order of the cluster spacing, not a rounding effect, so no share of the queries is allowed to differ.  The
meshes are the zoo of the oracle module: more than 256 clusters (the second pass), fewer than 64 faces and partial clusters,
clusters whose normals cancel or that are not planar, meshes away from the origin, thin, tiny, with slivers and zero-area faces."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _sdf_set_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

NONFINITE = np.array([[np.nan, np.nan, np.nan], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0], [-np.inf, np.inf, 0.0],
                      [1e30, 0.0, 0.0], [1e30, -1e30, 1e30]], dtype=np.float32)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


@functools.lru_cache(maxsize=None)
def _tool():
    return so.ClusterTool()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Mesh, its clusters, its finite queries and their oracle: computed once, shared by the tests, never modified."""
    fv = so.mesh(name)
    perm, boxes = _tool().clusters(fv)
    pts = so.queries(fv, boxes, seed=so.ZOO.index(name))
    pts.setflags(write=False)
    atol = so.atol_for(fv, pts)
    return {"fv": fv, "perm": perm, "boxes": boxes, "pts": pts, "atol": atol, "ref": so.exhaustive(pts, fv, atol)}


def _np(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def _judge_non_finite(pts, d2, sg, nrm, cls, tag):
    """A query with a non-finite or overflowing coordinate: finite outputs, or what sdf_dev.h documents for all-NaN distances."""
    for p, a, s, n, c in zip(pts, d2, sg, nrm, cls):
        documented = np.isinf(a) and a > 0 and s == 1 and np.array_equal(c.view(np.int32), p.view(np.int32)) and (n == 0).all()
        assert documented or (np.isfinite(a) and np.isfinite(n).all() and np.isfinite(c).all() and s in (1, -1)), (tag, p, a, s, n, c)


def _meshset_into_poisoned_buffers(gq, ms, p, qpm):
    """gq_sdf_forward_meshset writing into buffers that hold NaN / -77: a query that no block answers cannot pass on what an
    earlier launch left in recycled memory."""
    N, C = p.shape[0], gq.C
    d2, nrm, cls = (torch.full(s, float("nan"), device="cuda") for s in ((N,), (N, 3), (N, 3)))
    sg = torch.full((N,), -77, dtype=torch.int32, device="cuda")
    C.call("gq_sdf_forward_meshset", ms.handle, C.f32(p), N, int(qpm), C.f32(d2), C.i32(sg), C.f32(nrm), C.f32(cls), C.stream_ptr())
    return _np((d2, sg, nrm, cls))


@pytest.mark.parametrize("mesh", so.ZOO)
def test_meshset_query_matches_exhaustive_oracle(gq, mesh):
    c = _case(mesh)
    nf = len(c["pts"])
    pts = np.concatenate([c["pts"][:nf // 2], NONFINITE, c["pts"][nf // 2:]])  # the odd queries sit among ordinary ones
    fin = np.r_[np.arange(nf // 2), np.arange(nf // 2 + len(NONFINITE), len(pts))]
    ms = gq.ops.MeshSet([c["fv"]])
    assert ms.n_faces == len(c["fv"])
    p = torch.tensor(pts, device="cuda")
    d2, sg, nrm, cls = _np(gq.ops.sdf_meshset(p, ms, len(pts)))
    so.judge(c["ref"], c["pts"], d2[fin], sg[fin], nrm[fin], cls[fin], c["atol"], mesh)
    odd = slice(nf // 2, nf // 2 + len(NONFINITE))
    _judge_non_finite(NONFINITE, d2[odd], sg[odd], nrm[odd], cls[odd], mesh)
    # the unpruned face loop on the same tensors
    d2l = _np(torch.ops.graspqp_amd.compute_sdf(p[fin], torch.tensor(c["fv"], device="cuda")))[0]
    np.testing.assert_allclose(d2[fin], d2l, rtol=1e-5, atol=1e-10, err_msg=mesh)


NINE = ("triangle", "open65", "sphere5", "box", "open63", "soup", "superquadric", "open127", "shell")
SEVENTEEN = NINE + ("translated", "flat", "millimetre", "degenerate_sliver", "open64", "box", "triangle", "superquadric")


@pytest.mark.parametrize("names", [NINE[:7], NINE[:8], NINE, SEVENTEEN], ids=["7", "8", "9", "17"])
def test_many_meshes_and_ragged_counts(gq, names):
    """Query q of a launch belongs to mesh q // queries_per_mesh.  From 8 meshes on the blocks are dealt to the meshes by XCD
    (blocks b and b + 8 share one): the set sizes sit on both sides of that switch and are no multiples of 8, the counts per mesh
    no multiples of the 4 queries of a block.  Every query against the oracle of its own mesh, and both mappings bit for bit, into
    buffers filled with NaN so that a query nobody answers shows."""
    cases = [_case(n) for n in names]
    assert len({len(c["fv"]) for c in cases}) >= 7
    ms = gq.ops.MeshSet([c["fv"] for c in cases])
    picks = [np.random.default_rng(50 + i).choice(len(c["pts"]), 64, replace=False) for i, c in enumerate(cases)]
    try:
        for qpm in (1, 3, 5, 64):
            pts = np.concatenate([c["pts"][ix[:qpm]] for c, ix in zip(cases, picks)])
            p = torch.tensor(pts, device="cuda")
            outs = []
            for plain in (0, 1):
                gq.C.call("gq_debug_set_sdf_mapping", plain)
                outs.append(_meshset_into_poisoned_buffers(gq, ms, p, qpm))
            assert _same_bits(outs[0], outs[1]), (len(names), qpm)
            assert _same_bits(outs[0], _np(gq.ops.sdf_meshset(p, ms, qpm)))  # mapping 1 is still set: the op has no path of its own
            d2, sg, nrm, cls = outs[0]
            for m, (c, ix) in enumerate(zip(cases, picks)):
                s = slice(m * qpm, (m + 1) * qpm)
                so.judge(so.subset(c["ref"], ix[:qpm]), pts[s], d2[s], sg[s], nrm[s], cls[s], c["atol"][ix[:qpm]],
                         f"{len(names)} meshes, {qpm} queries each, mesh {m} ({names[m]})")
    finally:
        gq.C.call("gq_debug_set_sdf_mapping", 0)


@pytest.mark.parametrize("mesh", ["sphere5", "soup", "translated"])
def test_topk_two_equals_topk_four(gq, mesh):
    """gq_debug_set_sdf_topk (bench.py --sdf_topk): two clusters per round instead of four.  sdf_dev.h: "the answer does not
    depend on it"."""
    c = _case(mesh)
    pts = np.concatenate([c["pts"], NONFINITE])
    p = torch.tensor(pts, device="cuda")
    ms = gq.ops.MeshSet([c["fv"]])
    four = _np(gq.ops.sdf_meshset(p, ms, len(pts)))
    try:
        gq.C.call("gq_debug_set_sdf_topk", 2)
        two = _np(gq.ops.sdf_meshset(p, ms, len(pts)))
    finally:
        gq.C.call("gq_debug_set_sdf_topk", 0)
    assert _same_bits(two, four)
    n = len(c["pts"])
    so.judge(c["ref"], c["pts"], two[0][:n], two[1][:n], two[2][:n], two[3][:n], c["atol"], f"{mesh}, two clusters per round")


def test_search_really_prunes(gq):
    """The oracle tests would pass on a search that quietly visits every cluster, or that never enters its second pass of 256
    clusters.  The visit counters of the kernel (gq_debug_set_pen_counters: [0] += cluster visits, [1] += queries) show the
    first; queries placed a hair above faces of the clusters 256..319 (found through the same Morton order) show the second."""
    c = _case("sphere5")
    fv, perm = c["fv"], c["perm"]
    nC = len(c["boxes"])
    assert nC == 320
    ms = gq.ops.MeshSet([fv])
    far = torch.tensor(c["pts"][:400], device="cuda")  # the far field at 4 x and 20 x the extent
    cnt = torch.zeros(12, dtype=torch.int64, device="cuda")
    # one face of every cluster of the second pass, the query 1e-4 x the extent off its centre along its normal
    faces = perm[64 * np.arange(256, nC) + 17]
    late = (fv[faces].astype(np.float64).mean(1) + meshes.face_normals(fv[faces]) * 1e-4 * 0.05).astype(np.float32)
    gq.C.call("gq_debug_set_pen_counters", ctypes.c_void_p(cnt.data_ptr()))
    try:
        gq.ops.sdf_meshset(far, ms, len(far))
        torch.cuda.synchronize()
        visits, queries, most = (int(v) for v in cnt[:3])
        cnt.zero_()
        out = _np(gq.ops.sdf_meshset(torch.tensor(late, device="cuda"), ms, len(late)))
        visits2, queries2 = (int(v) for v in cnt[:2])
    finally:
        gq.C.call("gq_debug_set_pen_counters", None)
    assert queries == len(far) and 1 <= visits / queries < nC / 2 and 1 <= most < nC, (visits, queries, most)
    assert queries2 == len(late) and 1 <= visits2 / queries2 < nC / 2, (visits2, queries2)
    atol = so.atol_for(fv, late)
    ref = so.exhaustive(late, fv, atol)
    so.judge(ref, late, *out, atol, "queries of the second pass")
    where = np.empty(len(perm), dtype=np.int64)
    where[perm] = np.arange(len(perm)) // 64  # face -> cluster
    assert (where[ref["tie_f"]] >= 256).all()  # every face that may win sits in the second pass: the kernel went there
    assert np.array_equal(where[faces], np.arange(256, nC))


def _poses(spec, B, seed, centres):
    g = torch.Generator().manual_seed(seed)
    t = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=-1) * 0.1 + torch.tensor(centres, dtype=torch.float32)
    th = torch.tensor(spec.default_state, dtype=torch.float32)[None] + 0.3 * torch.randn(B, spec.n_dofs, generator=g)
    return torch.cat([t, torch.randn(B, 6, generator=g), th], 1)


@pytest.mark.parametrize("hand_name,n,be,names", [
    ("allegro", 2, 3, ("soup", "translated")), ("allegro", 3, 3, ("soup", "translated")), ("allegro", 12, 3, ("soup", "translated")),
    ("allegro", 13, 3, ("soup", "translated")), ("allegro", 25, 3, ("soup", "translated")), ("shadow_hand", 16, 3, ("soup", "translated")),
    ("allegro", 12, 171, ("soup", "translated", "shell"))])  # 513 rows: the query is a launch of its own (three meshes: 513 is odd)
def test_fused_fk_query_matches_oracle(gq, hand_name, n, be, names):
    """The contact query inside the FK forward launch (gq_fk_forward with a gqSdfDesc): the block of a row answers its n queries
    with 64 * min(n, 12) threads -- 2 wavefronts; 3; one round of 12; 13 = 7 x 2 rounds; 25 = 9 x 3 with a partial last round --
    at the contact points it has just computed.  Judged at the GPU's own contact points, read back and widened to float64."""
    spec = get_hand_spec(hand_name)
    fvs = [so.mesh(nm) for nm in names]
    ctr = [0.5 * (f.reshape(-1, 3).min(0) + f.reshape(-1, 3).max(0)) for f in fvs]
    sps = np.stack([meshes.surface_points(f, 256, oversample=4, seed=3) for f in fvs])
    B = be * len(fvs)
    hand = gq.ops.HandHandle(spec)
    ms = gq.ops.MeshSet(fvs)
    hp = _poses(spec, B, 31, np.repeat(np.stack(ctr), be, 0)).cuda()  # every hand about its own object
    idx = torch.randint(spec.n_contact_candidates, (B, n), generator=torch.Generator().manual_seed(2)).cuda()
    st = gq.stepper.GraspStepper(hand, ms, torch.tensor(sps), be, n, seed=5)
    assert st._can_fuse
    st.pose_new.copy_(hp)
    st.idx_new.copy_(idx)
    st._evaluate(st.pose_new, st.idx_new, gq.C.stream_ptr(), fused=True)
    torch.cuda.synchronize()
    assert st._fk_sdf_attached == (B <= 512) and (B == 513 or B == 6)
    cp = st.cpts.reshape(-1, 3)
    got = _np((st.d2.reshape(-1), st.sgn.reshape(-1), st.onrm.reshape(-1, 3), st.closest.reshape(-1, 3)))
    alone = _np(gq.ops.sdf_meshset(cp, ms, be * n))
    assert _same_bits(got, alone)
    pts = cp.cpu().numpy()
    rows = np.arange(B) if B <= 64 else np.sort(np.random.default_rng(8).choice(B, 64, replace=False))
    for m, fv in enumerate(fvs):
        q = (rows[rows // be == m][:, None] * n + np.arange(n)).reshape(-1)
        assert len(q) > 0
        atol = so.atol_for(fv, pts[q])
        so.judge(so.exhaustive(pts[q], fv, atol), pts[q], *(a[q] for a in got), atol, f"{hand_name} n={n} B={B} mesh {names[m]}")
