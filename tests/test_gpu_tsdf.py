"""GPU tests of the TSDF fusion (include/graspqp_hip.h, "scenes from depth images").

1. Parity with the fp64 oracle (tests/_tsdf_oracle.py) on layouts A (one world grid (9,8,17), three cameras) and B (three posed
   grids (5,9,17), four cameras, skip = [1, -1, 7]) on the nodes the oracle does not mark ambiguous: the weight exactly, the values
   at rtol 1e-5 / atol 1e-6 -- the bound of the same pose chain in the compose tests; the chain rounds by a few 1e-7 m and
   the running mean adds V 6e-8 relative; the host build of the same body measured at most 6.4e-8 m on these layouts
   (tests/test_tsdf_body_host.py).  The case asserts on the oracle's own output that at most 5 % of the nodes are ambiguous, at
   least 50 % are updated by some view and at least 10 % end inside the band (to.assert_parity).
2. No-tolerance cases: V views in one launch against V launches, run to run, identity poses against none, the stack form against
   the single grid, nodes outside every frustum, labels without skip, NaN poses, a captured graph replayed after in-place writes of
   its inputs, reset.
3. Through to the stepper (allegro, two objects) and to scene_compose's base, bit for bit against plain scene objects on clones."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _clutter_oracle as co  # noqa: E402
import _tsdf_oracle as to  # noqa: E402
from test_gpu_clutter import STATE, W_BOTH, _bits, _sm, _stepper, _two_objects  # noqa: E402  (the two-object fixtures of the clutter tests)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


def _new(gq, vol, stack=True, **kw):
    out = vol.out
    return gq.ops.SceneTSDF([float(o) for o in out.origin], out.shape, float(out.voxel), to.TRUNC, n_grids=out.n_grids if stack else None, **kw)


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class _Case:
    """A layout on the device: the images, labels and poses as CUDA tensors, and the oracle's result of fusing all of them."""

    def __init__(self, name):
        self.vol, tT, skip, self.n = to.layout(name)
        self.cam_np, self.depth_np, self.labels_np = to.cameras(self.n)
        self.tT_np, self.skip_np = tT, skip
        self.cam, self.depth, self.labels = _dev(self.cam_np), _dev(self.depth_np), _dev(self.labels_np)
        self.tT, self.skip = _dev(tT), _dev(skip)
        self.ref = self.vol.copy()
        self.info = to.integrate(self.ref, self.depth_np, self.labels_np, self.cam_np, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, skip)

    def fuse(self, t, views=slice(None), labels=True, skip=True, target=True):
        return t.integrate(self.depth[views], to.INTRINSICS, self.cam[views], labels=self.labels[views] if labels else None,
                           target_T=self.tT if target else None, skip=self.skip if skip else None, depth_range=to.DEPTH_RANGE)


@pytest.fixture(scope="module")
def cases():
    return {name: _Case(name) for name in "AB"}


def _same(a, b):
    return _bits(a._stack, b._stack) and _bits(a._weight, b._weight)


# ---------------------------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_integrate_matches_the_oracle(gq, cases, name):
    c = cases[name]
    t = _new(gq, c.vol)
    assert float(t.values.max()) == float(t.values.min()) == np.float32(-to.TRUNC) and float(t.weight.abs().max()) == 0
    assert c.fuse(t) is t
    torch.cuda.synchronize()
    to.assert_parity(t._stack.cpu().numpy(), t._weight.cpu().numpy(), c.ref, c.info, f"layout {name}")
    again = c.fuse(_new(gq, c.vol))
    assert _same(t, again)  # run to run
    assert t.scene.values.data_ptr() == t._stack.data_ptr() and t.values is t.scene.values  # the scene IS the volume


# ---------------------------------------------------------------------------------------------------------------
# 2. no tolerance
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 3, 4])
def test_views_in_one_launch_equal_one_launch_per_view(gq, cases, V):
    c = cases["B"]
    one = c.fuse(_new(gq, c.vol), slice(0, V))
    many = _new(gq, c.vol)
    for v in range(V):
        c.fuse(many, slice(v, v + 1))
    torch.cuda.synchronize()
    assert _same(one, many) and float(one.weight.max()) == V
    if V > 1:
        assert not _bits(one._stack, c.fuse(_new(gq, c.vol), slice(0, V - 1))._stack)  # the last view counts
    # a single (H,W) image with a (3,4) pose is a batch of one
    single = _new(gq, c.vol).integrate(c.depth[0], to.INTRINSICS, c.cam[0], labels=c.labels[0], target_T=c.tT.reshape(3, 3, 4), skip=c.skip,
                                       depth_range=to.DEPTH_RANGE)
    assert _same(single, c.fuse(_new(gq, c.vol), slice(0, 1)))


def test_no_target_poses_are_identity_poses_and_the_stack_form_is_the_single_grid(gq, cases):
    c = cases["A"]
    plain = c.fuse(_new(gq, c.vol))
    c.tT = _dev(co.identity(1).numpy())
    try:
        posed = c.fuse(_new(gq, c.vol))
    finally:
        c.tT = None
    single = c.fuse(_new(gq, c.vol, stack=False))
    torch.cuda.synchronize()
    assert isinstance(single.scene, gq.ops.SceneSDF) and isinstance(plain.scene, gq.ops.SceneSDFSet)
    assert single.values.shape == to.A_SHAPE and single.weight.shape == to.A_SHAPE and plain.values.shape == (1,) + to.A_SHAPE
    assert _same(plain, posed) and _same(plain, single)
    assert _bits(single.values, plain.values[0]) and _bits(single.weight, plain.weight[0])


def test_nodes_outside_every_frustum_keep_unknown_and_weight_zero(gq, cases):
    c = cases["A"]
    away = to.Volume(1, to.A_SHAPE, (1.0, -0.035, -0.04), to.VOXEL, 0.0)  # a metre to the side of what the cameras look at
    t = c.fuse(_new(gq, away, unknown=0.0125))
    torch.cuda.synchronize()
    assert (t.values == 0.0125).all() and (t.weight == 0).all()
    # and inside the layout itself: the nodes the oracle leaves alone keep both, bit for bit
    t = c.fuse(_new(gq, c.vol))
    left = torch.as_tensor(~c.info["updated"] & ~c.info["ambiguous"]).cuda()
    assert int(left.sum()) > 100 and (t._stack[left] == np.float32(-to.TRUNC)).all() and (t._weight[left] == 0).all()


def test_labels_without_skip_and_a_negative_skip_are_no_labels(gq, cases):
    c = cases["B"]
    none = c.fuse(_new(gq, c.vol), labels=False, skip=False)
    only_labels = c.fuse(_new(gq, c.vol), skip=False)
    only_skip = c.fuse(_new(gq, c.vol), labels=False)
    keep, c.skip = c.skip, _dev(np.array([-1, -1, -5], dtype=np.int32))
    try:
        negative = c.fuse(_new(gq, c.vol))
    finally:
        c.skip = keep
    carved = c.fuse(_new(gq, c.vol))
    torch.cuda.synchronize()
    assert _same(none, only_labels) and _same(none, only_skip) and _same(none, negative)
    assert not _bits(none._stack[0], carved._stack[0]) and _bits(none._stack[1:], carved._stack[1:])  # label 1 is the sphere, 7 nobody


def test_nan_poses(gq, cases):
    c = cases["B"]
    good = c.fuse(_new(gq, c.vol))
    # the second view's pose: every node of every grid sees it
    cam = c.cam_np.copy()
    cam[1, 0, 3] = float("nan")
    ref = c.vol.copy()
    info = to.integrate(ref, c.depth_np, c.labels_np, cam, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, c.tT_np, c.skip_np)
    keep, c.cam = c.cam, _dev(cam)
    try:
        t = c.fuse(_new(gq, c.vol))
    finally:
        c.cam = keep
    torch.cuda.synchronize()
    assert np.isnan(ref.D).all() and np.array_equal(np.isnan(t._stack.cpu().numpy()), np.isnan(ref.D))
    ok = ~info["ambiguous"]
    assert np.array_equal(t._weight.cpu().numpy()[ok], ref.W[ok]) and ref.W.max() == 3  # the other three views still count
    # the pose of grid 1: exactly its nodes are NaN, with the weight they came with; the other grids do not notice
    tT = c.tT_np.copy()
    tT[1, 2, 1] = float("nan")
    ref = c.vol.copy()
    to.integrate(ref, c.depth_np, c.labels_np, c.cam_np, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, c.skip_np)
    keep, c.tT = c.tT, _dev(tT)
    try:
        t = c.fuse(_new(gq, c.vol))
    finally:
        c.tT = keep
    torch.cuda.synchronize()
    assert np.array_equal(np.isnan(t._stack.cpu().numpy()), np.isnan(ref.D)) and np.isnan(ref.D[1]).all() and not np.isnan(ref.D[[0, 2]]).any()
    assert (t._weight[1] == 0).all() and _bits(t._stack[[0, 2]], good._stack[[0, 2]]) and _bits(t._weight[[0, 2]], good._weight[[0, 2]])


def test_integrate_in_a_captured_graph_follows_in_place_writes(gq, cases):
    c = cases["B"]
    depth, labels, cam, skip = c.depth[:2].clone(), c.labels[:2].clone(), c.cam[:2].clone(), c.skip.clone()
    call = lambda t, d, l, T, s: t.integrate(d, to.INTRINSICS, T, labels=l, target_T=c.tT, skip=s, depth_range=to.DEPTH_RANGE)
    t = call(_new(gq, c.vol), depth, labels, cam, skip)  # warm-up outside the capture: the state is one call old
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(t, depth, labels, cam, skip)
    graph.replay()
    torch.cuda.synchronize()
    twice = call(call(_new(gq, c.vol), depth, labels, cam, skip), depth, labels, cam, skip)
    assert _same(t, twice) and float(t.weight.max()) == 4
    prior = (t._stack.clone(), t._weight.clone())
    depth.copy_(c.depth[2:4]), labels.copy_(c.labels[2:4]), cam.copy_(c.cam[2:4])  # in place: the replay reads the new inputs
    skip.copy_(_dev(np.array([-1, 1, 0], dtype=np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    eager, old = _new(gq, c.vol), _new(gq, c.vol)
    for o in (eager, old):
        o._stack.copy_(prior[0]), o._weight.copy_(prior[1])
    call(eager, c.depth[2:4], c.labels[2:4], c.cam[2:4], _dev(np.array([-1, 1, 0], dtype=np.int32)))
    call(old, c.depth[:2], c.labels[:2], c.cam[:2], c.skip)
    torch.cuda.synchronize()
    assert _same(t, eager) and not _bits(t._stack, old._stack)


def test_reset_then_integrate_reproduces_the_first_result(gq, cases):
    c = cases["A"]
    t = c.fuse(_new(gq, c.vol, stack=False))
    first = (t.values.clone(), t.weight.clone())
    assert t.reset() is t
    assert (t.values == np.float32(-to.TRUNC)).all() and (t.weight == 0).all()
    c.fuse(t)
    torch.cuda.synchronize()
    assert _bits(t.values, first[0]) and _bits(t.weight, first[1])
    # W already at max_weight stays, and D still moves
    full = _new(gq, c.vol, max_weight=2.0)
    c.fuse(full, slice(0, 2))
    two = full._stack.clone()
    c.fuse(full, slice(2, 3))
    assert float(full.weight.max()) == 2 and not _bits(two, full._stack)


# ---------------------------------------------------------------------------------------------------------------
# 3. through to the stepper and to scene_compose
# ---------------------------------------------------------------------------------------------------------------
S_SHAPE, S_H = (40, 40, 40), 0.01  # +-19.5 cm about each object's frame: the hands of the fixtures stand 12 cm from it


def _bin(gq, views):
    """A two-object volume of the plane-and-sphere scene, the objects' frames a few cm apart above the table."""
    vol = to.Volume(2, S_SHAPE, co.centred(S_SHAPE, S_H), S_H, -to.TRUNC)
    tT = co.poses(2, 23, 0.03)
    tT[:, 2, 3] += 0.05
    cam, depth, labels = to.cameras(4)
    t = _new(gq, vol)
    fuse = lambda v: t.integrate(_dev(depth[v]), to.INTRINSICS, _dev(cam[v]), labels=_dev(labels[v]), target_T=tT.cuda(),
                                 skip=_dev(np.array([1, -1], dtype=np.int32)), depth_range=to.DEPTH_RANGE)
    fuse(views)
    return t, fuse


def _state(st):
    return [getattr(st, k).clone() for k in STATE] + [st.terms_new.clone(), st.total_new.clone()]


def _equal(a, b):
    return all(_bits(x.float(), y.float()) if x.is_floating_point() else torch.equal(x, y) for x, y in zip(a, b))


def test_stepper_on_the_fused_volume_equals_a_stepper_on_a_clone(gq, golden_dir):
    be = 4
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    t, _ = _bin(gq, slice(0, 3))
    clone = gq.ops.SceneSDFSet(t.values.clone(), t.origin, t.voxel)
    assert clone.values.data_ptr() != t.values.data_ptr()
    out = []
    for scene in (t.scene, clone):
        st = _stepper(gq, be, sm, weights=dict(W_BOTH), scene=scene)
        assert st.clutter and st.term_names[5:] == ("E_scene", "E_approach")
        st.reset(hp, idx)
        assert float(st.terms[5].max()) > 0 and float(st.terms[6].max()) > 0
        for d in draws[:3]:
            st.step(draws=d)
        torch.cuda.synchronize()
        out.append(_state(st))
    assert _equal(*out) and torch.isfinite(out[0][2]).all()


def test_a_further_integrate_between_two_graph_replays(gq, golden_dir):
    be = 192
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    t, fuse = _bin(gq, slice(0, 2))
    st = _stepper(gq, be, sm, weights=dict(W_BOTH), scene=t.scene)
    st.reset(hp, idx)
    st.capture()
    assert st.graph_mode == "graph branches"
    st.step(draws=draws[0])
    torch.cuda.synchronize()
    after_one = {k: getattr(st, k).clone() for k in STATE}
    old = t.values.clone()
    fuse(slice(2, 4))  # two more frames, one launch, into the memory the graph reads
    st.step(draws=draws[1])
    torch.cuda.synchronize()
    got = _state(st)
    assert not _bits(old, t.values)
    refs = []
    for values in (t.values.clone(), old):
        ref = _stepper(gq, be, sm, weights=dict(W_BOTH), scene=gq.ops.SceneSDFSet(values, t.origin, t.voxel))
        ref.reset(hp, idx)
        ref.capture()
        for k in STATE:
            getattr(ref, k).copy_(after_one[k])
        ref.step(draws=draws[1])
        torch.cuda.synchronize()
        refs.append(_state(ref))
    assert _equal(got, refs[0])
    assert not _equal(got, refs[1]) and not _bits(got[-2][5], refs[1][-2][5])  # E_scene of the proposal read the new volume
    assert torch.isfinite(got[2]).all()


def test_the_fused_world_grid_as_the_base_of_scene_compose(gq, cases):
    c = cases["A"]
    t = c.fuse(_new(gq, c.vol, stack=False))
    out, tT, parts, pT, ex, _ = co.layout(co.SEEDS[0], "random")
    scenes = [F.scene(gq) for F in parts]
    stacks = []
    for base in (t.scene, gq.ops.SceneSDF(t.values.clone(), t.origin, t.voxel), None):
        stack = gq.ops.SceneSDFSet.empty(out.n_grids, [float(o) for o in out.origin], out.shape, float(out.voxel))
        stack.values.fill_(-7.0)
        gq.ops.scene_compose(stack, tT.cuda(), scenes, pT.cuda(), ex.cuda(), base, co.FAR)
        stacks.append(stack.values)
    torch.cuda.synchronize()
    assert _bits(stacks[0], stacks[1]) and not _bits(stacks[0], stacks[2]) and torch.isfinite(stacks[0]).all()


# ---------------------------------------------------------------------------------------------------------------
# refusals, through the Python surface
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(gq, cases):
    c = cases["B"]
    T = gq.ops.SceneTSDF
    o, shape = [0.0, 0.0, 0.0], (4, 4, 4)
    for kw, word in ((dict(trunc=0.0), "trunc"), (dict(trunc=float("nan")), "trunc"), (dict(max_weight=0.5), "max_weight"),
                     (dict(unknown=float("inf")), "unknown"), (dict(n_grids=0), "n_grids")):
        with pytest.raises(ValueError, match=word):
            T(o, shape, 0.01, **{"trunc": 0.02, **kw})
    with pytest.raises(ValueError, match="nx"):
        T(o, (1, 4, 4), 0.01, 0.02)
    t = _new(gq, c.vol)
    before = (t._stack.clone(), t._weight.clone())
    ok = dict(depth=c.depth, intrinsics=to.INTRINSICS, cam_T=c.cam, labels=c.labels, target_T=c.tT, skip=c.skip, depth_range=to.DEPTH_RANGE)
    bad = [
        (dict(depth=c.depth[None]), "depth"), (dict(cam_T=c.cam[:3]), "cam_T"), (dict(labels=c.labels[:3]), "labels"),
        (dict(skip=c.skip[:2]), "skip"), (dict(target_T=c.tT[:2]), "target_T"), (dict(intrinsics=(0.0, 45.0, 1.0, 1.0)), "fx"),
        (dict(intrinsics=(45.0, float("nan"), 1.0, 1.0)), "fy"), (dict(intrinsics=(45.0, 45.0, float("inf"), 1.0)), "cx"),
        (dict(intrinsics=(45.0, 45.0, 1.0)), "intrinsics"), (dict(depth_range=(0.0, 2.0)), "depth_min"),
        (dict(depth_range=(0.05, 0.04)), "depth_max"),
        (dict(depth=c.depth[:1].repeat(65, 1, 1), cam_T=c.cam[:1].repeat(65, 1, 1), labels=None), "n_views"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            t.integrate(**{**ok, **kw})
    with pytest.raises(ValueError, match="tsdf"):
        t.integrate(**{**ok, "depth_range": (float("nan"), 2.0)})
    torch.cuda.synchronize()
    assert _bits(t._stack, before[0]) and _bits(t._weight, before[1])  # a refused call writes nothing
    # contiguous float32 / int32 CUDA tensors are read in place; anything else is converted once
    assert t.integrate(c.depth.double().cpu().numpy(), to.INTRINSICS, c.cam_np, labels=c.labels.long(), target_T=c.tT_np, skip=list(to.B_SKIP),
                       depth_range=to.DEPTH_RANGE) is t
    assert _same(t, c.fuse(_new(gq, c.vol)))
