"""GPU tests of the TSDF surfel extraction (include/graspqp_hip.h, "target objects from depth images").

1. Parity with the fp64 oracle (tests/_surfel_oracle.py), which reads the very float32 volume the kernels read: the count and the
   order exactly, positions at rtol 1e-5 / atol 1e-6 (the bound of the same grid geometry in _tsdf_oracle.assert_parity), normals
   by angle on the non-ambiguous edges within 4 x the largest angle between the oracle's own float32 and float64 normals on the
   case, at least 1e-5 rad.  Cases: one cell (2,2,2); layouts A and B and the 12^3 sphere volume fused ON THE DEVICE by
   SceneTSDF.integrate (at least 50 surfels each, at most 1 % ambiguous); the hand-made volumes of so.hand_made(), which go
   through the op with their own weight, region and min_weight.  The host build of the same body (tests/test_surfel_body_host.py)
   measured at most 1.2e-8 m and 1.7e-7 rad on these cases.
2. No tolerance: run to run, a capacity below the total, the counting call, a region against the filtered whole, a captured graph
   behind integrate, extract_clouds against surfels.
3. Through to the object: ObjectModel.initialize_from_tsdf against initialize_from_point_clouds on the same arrays, bit for bit in
   cal_distance and in four GraspStepper iterations."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _surfel_oracle as so  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402

to = so.to
SENTINEL = -7777.0


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _op(gq, D, W, origin, voxel, trunc, min_weight=1.0, region=None, capacity=None):
    """The registered op's body on a volume given as arrays -> (points, normals, count) as CUDA tensors; capacity None is the
    counting call.  The outputs start as SENTINEL."""
    values, weight = _dev(D, torch.float32), _dev(W, torch.float32)
    G = values.shape[0]
    grids = gq.ops._clutter_grids(values, origin, voxel)
    ws = gq.ops._ws(gq.ops._size_call("gq_tsdf_surfels_workspace_bytes", ctypes.byref(grids)), values.device)
    count = torch.full((G, 2), -1, dtype=torch.int32, device="cuda")
    P = N = None
    if capacity is not None:
        P, N = torch.full((G, capacity, 3), SENTINEL, device="cuda"), torch.full((G, capacity, 3), SENTINEL, device="cuda")
    gq.ops._Eager.tsdf_surfels(values, weight, [float(o) for o in origin], float(voxel), [] if region is None else list(region),
                               float(min_weight), float(trunc), P, N, count, ws)
    torch.cuda.synchronize()
    return P, N, count


def _exact(gq, D, W, origin, voxel, trunc, min_weight=1.0, region=None):
    _, _, count = _op(gq, D, W, origin, voxel, trunc, min_weight, region)
    assert (count[:, 1] == 0).all()
    cap = max(int(count[:, 0].max()), 1)
    P, N, count2 = _op(gq, D, W, origin, voxel, trunc, min_weight, region, cap)
    assert torch.equal(count2[:, 0], count[:, 0]) and torch.equal(count2[:, 1], count[:, 0])
    for g in range(P.shape[0]):  # slots beyond the count are not touched
        assert (P[g, int(count[g, 0]):] == SENTINEL).all() and (N[g, int(count[g, 0]):] == SENTINEL).all()
    return P, N, count2


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


class _Fused:
    """A case of so.fused fused ON THE DEVICE: the SceneTSDF, and its volume back on the host for the oracle."""

    def __init__(self, gq, name):
        if name == "sphere":
            self.trunc = 3 * so.SPHERE_VOXEL
            shape, voxel = so.SPHERE_SHAPE, so.SPHERE_VOXEL
            origin = tuple(float(c) - 0.5 * float(np.float32(voxel)) * (n - 1) for c, n in zip(to.SPHERE[0], shape))
            self.cam, self.depth, labels = (_dev(a) for a in to.cameras(4))
            self.depth = gq.ops.keep_label(self.depth, labels, 1)
            self.kw = dict(depth_range=to.DEPTH_RANGE)
            self.t = gq.ops.SceneTSDF(origin, shape, voxel, self.trunc, n_grids=1)
        else:
            vol, tT, skip, n = to.layout(name)
            self.trunc = to.TRUNC
            self.cam, self.depth, labels = (_dev(a) for a in to.cameras(n))
            self.kw = dict(labels=labels, target_T=_dev(tT), skip=_dev(skip), depth_range=to.DEPTH_RANGE)
            self.t = gq.ops.SceneTSDF([float(o) for o in vol.out.origin], vol.out.shape, float(vol.out.voxel), self.trunc, n_grids=vol.out.n_grids)
        self.fuse(self.t)
        torch.cuda.synchronize()
        self.D, self.W = _np(self.t._stack, self.t._weight)

    def fuse(self, t, depth=None):
        return t.integrate(self.depth if depth is None else depth, to.INTRINSICS, self.cam, **self.kw)


@pytest.fixture(scope="module")
def fused(gq):
    return {name: _Fused(gq, name) for name in ("A", "B", "sphere")}


# ---------------------------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------
def test_one_cell(gq):
    D, W, origin, voxel, trunc, mw, region, _ = so.tiny()
    P, N, count = _exact(gq, D, W, origin, voxel, trunc, mw, region)
    ref = so.assert_parity(*_np(P, N, count), D, W, origin, voxel, trunc, mw, region, "(2,2,2)")
    assert len(ref[0]["edges"]) == 4


@pytest.mark.parametrize("name,min_weight", [("A", 1.0), ("B", 1.0), ("sphere", 1.0), ("sphere", 2.0)])
def test_surfels_of_a_device_fused_volume_match_the_oracle(gq, fused, name, min_weight):
    c = fused[name]
    t = c.t
    found = [len(r["edges"]) for r in so.extract(c.D, c.W, t.origin, t.voxel, c.trunc, min_weight)]
    assert sum(found) >= 50 and min(found) > 0, found  # the case does not pass empty
    cap = max(found) + 5
    P, N, count = t.surfels(cap, min_weight)
    torch.cuda.synchronize()
    assert P.shape == (t.n_grids, cap, 3) and N.shape == P.shape and count.dtype == torch.int32 and count.shape == (t.n_grids, 2)
    so.assert_parity(*_np(P, N, count), c.D, c.W, t.origin, t.voxel, c.trunc, min_weight, None, f"{name} min_weight {min_weight}")
    # run to run, into the same buffers and into fresh ones
    first = (P.clone(), N.clone(), count.clone())
    out = t.surfels(cap, min_weight, out=(P.fill_(SENTINEL), N.fill_(SENTINEL), count.zero_()))
    again = t.surfels(cap, min_weight)
    torch.cuda.synchronize()
    assert out[0] is P and out[1] is N and out[2] is count
    for g in range(t.n_grids):
        n = found[g]
        assert all(_bits(a[g, :n], b[g, :n]) and _bits(a[g, :n], c_[g, :n]) for a, b, c_ in zip(first[:2], out[:2], again[:2]))
        assert (P[g, n:] == SENTINEL).all() and (N[g, n:] == SENTINEL).all()
    assert torch.equal(first[2], count) and torch.equal(first[2], again[2])


@pytest.mark.parametrize("name", sorted(so.hand_made()))
def test_hand_made_volumes(gq, name):
    D, W, origin, voxel, trunc, mw, region, want = so.hand_made()[name]
    P, N, count = _exact(gq, D, W, origin, voxel, trunc, mw, region)
    ref = so.assert_parity(*_np(P, N, count), D, W, origin, voxel, trunc, mw, region, name)[0]
    if want is not None:
        assert int(count[0, 0]) == want
    if name == "lonely_pairs":
        assert int(ref["fallback"].sum()) == 1
        got = {tuple(e): tuple(n) for e, n in zip(ref["edges"].tolist(), N[0].cpu().tolist())}
        assert got[(4, 3, 4, 2)] == (0.0, 0.0, -1.0) and got[(4, 1, 12, 0)] == (1.0, 0.0, 0.0)
    if name == "seam_z":
        assert ((ref["edges"][:, 3] == 2) & (ref["edges"][:, 2] == 15)).sum() >= 20
    if name == "one_pair":
        assert ref["edges"].tolist() == [[2, 1, 8, 2]]


# ---------------------------------------------------------------------------------------------------------------
# 2. no tolerance
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_capacity_below_the_total_and_the_counting_call(gq, fused, name):
    c = fused[name]
    t = c.t
    args = (c.D, c.W, t.origin, t.voxel, c.trunc)
    full_P, full_N, full = _exact(gq, *args)
    cap = int(full[:, 0].min()) - 9  # below every grid's total, inside a tile's run of crossings
    assert cap >= 10
    P2, N2, count2 = _op(gq, *args, capacity=cap)
    assert torch.equal(count2[:, 0], full[:, 0]) and (count2[:, 1] == cap).all()
    assert _bits(P2, full_P[:, :cap]) and _bits(N2, full_N[:, :cap])
    so.assert_parity(*_np(P2, N2, count2), *args, 1.0, None, f"{name} capacity {cap}", capacity=cap)
    # one grid, one buffer with room behind the capacity: the rows behind it are not touched
    g = t.n_grids - 1
    one = gq.ops._clutter_grids(t._stack[g:g + 1], t.origin, t.voxel)
    buf_P, buf_N = torch.full((cap + 3, 3), SENTINEL, device="cuda"), torch.full((cap + 3, 3), SENTINEL, device="cuda")
    cnt = torch.zeros(1, 2, dtype=torch.int32, device="cuda")
    ws = gq.ops._ws(gq.ops._size_call("gq_tsdf_surfels_workspace_bytes", ctypes.byref(one)), "cuda")
    gq.C.call("gq_tsdf_surfels", ctypes.byref(one), gq.C.f32(t._stack[g:g + 1]), gq.C.f32(t._weight[g:g + 1]), None, 1.0, c.trunc, gq.C.f32(buf_P),
              gq.C.f32(buf_N), ctypes.c_int64(cap), gq.C.i32(cnt), gq.C.ptr(ws), gq.C.stream_ptr())
    torch.cuda.synchronize()
    assert cnt.tolist() == [[int(full[g, 0]), cap]]
    assert _bits(buf_P[:cap], full_P[g, :cap]) and _bits(buf_N[:cap], full_N[g, :cap])
    assert (buf_P[cap:] == SENTINEL).all() and (buf_N[cap:] == SENTINEL).all()


def test_bounds_give_the_whole_extraction_filtered(gq, fused):
    c = fused["A"]
    t = c.t
    region = [1, 8, 2, 7, 3, 17]
    lo = [t.origin[a] + t.voxel * region[2 * a] for a in range(3)]
    hi = [t.origin[a] + t.voxel * (region[2 * a + 1] - 1) for a in range(3)]
    assert t._region((lo, hi)) == region
    e = so.extract(c.D, c.W, t.origin, t.voxel, c.trunc)[0]["edges"]
    b = e[:, :3] + np.eye(3, dtype=np.int64)[e[:, 3]]
    keep = ((e[:, :3] >= region[0::2]) & (e[:, :3] < region[1::2]) & (b >= region[0::2]) & (b < region[1::2])).all(1)
    assert 0 < keep.sum() < len(e)
    whole, sub = t.surfels(len(e)), t.surfels(len(e), bounds=(lo, hi))
    torch.cuda.synchronize()
    assert sub[2].tolist() == [[int(keep.sum())] * 2]
    so.assert_parity(*_np(*sub), c.D, c.W, t.origin, t.voxel, c.trunc, 1.0, region, "bounds")
    k = torch.as_tensor(keep).cuda()
    assert _bits(sub[0][0, :int(keep.sum())], whole[0][0][k]) and _bits(sub[1][0, :int(keep.sum())], whole[1][0][k])


def test_surfels_in_a_captured_graph_behind_integrate(gq, fused):
    c = fused["B"]
    new = lambda: gq.ops.SceneTSDF(c.t.origin, c.t.shape, c.t.voxel, c.trunc, n_grids=c.t.n_grids)
    cap = int(max(len(r["edges"]) for r in so.extract(c.D, c.W, c.t.origin, c.t.voxel, c.trunc))) + 40
    depth = c.depth.clone()
    t = new()
    out = c.fuse(t, depth).surfels(cap)  # warm-up outside the capture: buffers and workspace exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        t.reset()
        c.fuse(t, depth).surfels(cap, out=out)
    for o in out[:2]:
        o.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    eager = c.fuse(new()).surfels(cap)
    torch.cuda.synchronize()
    n = eager[2][:, 0].tolist()
    assert torch.equal(out[2], eager[2]) and all(_bits(out[k][g, :n[g]], eager[k][g, :n[g]]) for k in (0, 1) for g in range(len(n)))
    # other images, written in place: the replay extracts the surface of the new volume
    moved = torch.where(depth > 0, depth + 0.004, depth)
    depth.copy_(moved)
    for o in out[:2]:
        o.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    eager2 = c.fuse(new(), moved).surfels(cap)
    torch.cuda.synchronize()
    n2 = eager2[2][:, 0].tolist()
    assert torch.equal(out[2], eager2[2]) and all(_bits(out[k][g, :n2[g]], eager2[k][g, :n2[g]]) for k in (0, 1) for g in range(len(n2)))
    assert all((out[k][g, n2[g]:] == SENTINEL).all() for k in (0, 1) for g in range(len(n2)))
    assert not _bits(out[0][1, :min(n[1], n2[1])], eager[0][1, :min(n[1], n2[1])])  # and not the old one


def test_extract_clouds_is_surfels_trimmed(gq, fused):
    c = fused["B"]
    clouds = c.t.extract_clouds()
    P, N, count = c.t.surfels(400)
    torch.cuda.synchronize()
    assert len(clouds) == 3 and [len(p) for p, _ in clouds] == count[:, 0].tolist() == count[:, 1].tolist()
    for g, (p, n) in enumerate(clouds):
        assert p.is_cuda and p.shape == n.shape == (int(count[g, 0]), 3) and _bits(p, P[g, :len(p)]) and _bits(n, N[g, :len(p)])
    two = fused["sphere"].t.extract_clouds(min_weight=2.0)
    assert len(two) == 1 and 50 <= len(two[0][0]) < len(fused["sphere"].t.extract_clouds()[0][0])


# ---------------------------------------------------------------------------------------------------------------
# 3. through to the object
# ---------------------------------------------------------------------------------------------------------------
def test_object_from_tsdf_equals_the_object_from_the_same_clouds(gq, fused):
    from graspqp_amd.core.object_model import ObjectModel

    t = fused["sphere"].t
    (p, n), = t.extract_clouds()
    be, ns = 4, 64
    assert len(p) >= 100
    a, b = ObjectModel(batch_size_each=be, num_samples=ns), ObjectModel(batch_size_each=be, num_samples=ns)
    a.initialize_from_tsdf(t)
    b.initialize_from_point_clouds([p.cpu().numpy()], [n.cpu().numpy()])
    assert a.object_mesh_list is None and a.object_code_list == ["obj0"] and _bits(a.surface_points_each, b.surface_points_each)
    assert np.array_equal(a._cloudset.radius, b._cloudset.radius)
    gen = torch.Generator().manual_seed(11)
    x = (torch.tensor(to.SPHERE[0]) + 0.05 * torch.randn(be, 9, 3, generator=gen)).cuda()
    da, na, ca = a.cal_distance(x, with_closest_points=True)
    db, nb, cb = b.cal_distance(x, with_closest_points=True)
    assert _bits(da, db) and _bits(na, nb) and _bits(ca, cb) and torch.isfinite(da).all()
    # the normals point outward: queries 8 cm from the centre, on the side the cameras saw, and queries near the centre get
    # distances of opposite signs
    u = torch.nn.functional.normalize(torch.randn(be, 9, 3, generator=gen), dim=-1)
    u[..., 2] = u[..., 2].abs()
    centre = torch.tensor(to.SPHERE[0])
    d_far, d_in = a.cal_distance((centre + 0.08 * u).cuda())[0], a.cal_distance((centre + 0.005 * u).cuda())[0]
    assert (torch.sign(d_far) == -torch.sign(d_in.median())).float().mean() > 0.9 and (torch.sign(d_in) == torch.sign(d_in.median())).float().mean() > 0.9
    hand = gq.ops.HandHandle(get_hand_spec("allegro"))
    runs = []
    for om in (a, b):
        st = gq.stepper.GraspStepper(hand, om._cloudset, om.surface_points_each, be, 4, seed=3)
        st.set_hulls(om.convex_hulls())
        st.initialize()
        for _ in range(4):
            st.step()
        torch.cuda.synchronize()
        runs.append((st.energy.clone(), st.hand_pose.clone()))
    assert _bits(runs[0][0], runs[1][0]) and _bits(runs[0][1], runs[1][1]) and torch.isfinite(runs[0][0]).all()
    with pytest.raises(ValueError, match=r"grid 0 yields \d+ surfels"):
        ObjectModel(batch_size_each=be, num_samples=2000).initialize_from_tsdf(t)


# ---------------------------------------------------------------------------------------------------------------
# refusals, through the Python surface
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(gq, fused):
    t = fused["A"].t
    for kw, word in ((dict(capacity=0), "capacity"), (dict(capacity=(1 << 24) + 1), "capacity"), (dict(capacity=8, min_weight=float("nan")), "min_weight"),
                     (dict(capacity=8, bounds=((1.0, 1.0, 1.0), (2.0, 2.0, 2.0))), "bounds"),
                     (dict(capacity=8, out=(torch.empty(1, 7, 3, device="cuda"),) * 2 + (torch.empty(1, 2, dtype=torch.int32, device="cuda"),)), "out")):
        with pytest.raises(ValueError, match=word):
            t.surfels(**kw)
    with pytest.raises(ValueError, match="surfels: min_weight"):
        t.extract_clouds(min_weight=float("inf"))
    bad = gq.ops.SceneTSDF(t.origin, t.shape, t.voxel, 0.02, n_grids=1)
    bad.trunc = float("nan")
    with pytest.raises(ValueError, match="trunc"):
        bad.surfels(8)
    P = torch.full((1, 8, 3), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="count"):  # the op's own shape check
        gq.ops._Eager.tsdf_surfels(t._stack, t._weight, list(t.origin), t.voxel, [], 1.0, t.trunc, P, P.clone(), torch.zeros(2, 2, dtype=torch.int32, device="cuda"),
                                   t._surfel_workspace())
    with pytest.raises(RuntimeError, match="workspace"):
        gq.ops._Eager.tsdf_surfels(t._stack, t._weight, list(t.origin), t.voxel, [], 1.0, t.trunc, P, P.clone(), torch.zeros(1, 2, dtype=torch.int32, device="cuda"),
                                   torch.empty(8, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert (P == SENTINEL).all()  # a refused call writes nothing
