"""GPU tests of the Euclidean distance field of a TSDF (include/graspqp_hip.h, "Euclidean distance field from a fused TSDF";
DESIGN 19).

1. Parity with the fp64 brute-force oracle (tests/_esdf_oracle.py), which reads the very float32 volume the kernels read, on EVERY
   node at the project's grid bound, rtol 1e-5 / atol 1e-6; in-band and void nodes must equal D bit for bit.  There are no
   ambiguous nodes: every floating-point quantity enters the result continuously and every decision is an exact float32 test.  The
   host build of the same bodies (tests/test_esdf_body_host.py) measured at most 5.4e-8 m on these volumes.
2. No tolerance: run to run, a stack against its grids, src untouched, a captured graph replayed after src was overwritten in
   place, a second call with ``out`` allocates nothing.
3. Behaviour: deep inside the analytic sphere the TSDF has no gradient and the ESDF has one that points outward.
4. Through to the stepper (allegro, two objects): a stepper on ``tsdf.esdf`` against one on a clone, and integrate + esdf between
   two replays of the captured iteration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402,F401

import _esdf_oracle as eo  # noqa: E402
import _surfel_oracle as so  # noqa: E402
from test_gpu_clutter import DIST, STATE, W_BOTH, _bits, _hand, _sm, _two_objects  # noqa: E402  (the two-object fixtures of the clutter tests)
from test_gpu_tsdf import _bin, _equal, _state  # noqa: E402  (the fused two-object volume of the TSDF tests)


@pytest.fixture(scope="module")
def gq():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from graspqp_amd import _C, ops, stepper

    _C.lib()
    return type("gq", (), {"ops": ops, "C": _C, "stepper": stepper})


ORIGIN = (0.01, -0.02, 0.03)


def _scene(gq, D, voxel):
    v = torch.as_tensor(np.ascontiguousarray(D, dtype=np.float32)).cuda()
    return (gq.ops.SceneSDFSet if v.dim() == 4 else gq.ops.SceneSDF)(v, ORIGIN, voxel)


def _esdf(gq, D, voxel, trunc, dmax):
    """ops.scene_esdf on a volume given as an array -> the result on the host; src must come back untouched."""
    src = _scene(gq, D, voxel)
    keep = src.values.clone()
    out = gq.ops.scene_esdf(src, trunc, dmax)
    torch.cuda.synchronize()
    assert type(out) is type(src) and out.shape == src.shape and out.origin == src.origin and out.voxel == src.voxel
    assert out.values.data_ptr() != src.values.data_ptr() and _bits(src.values, keep)
    return out.values.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# 1. parity with the oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_fused_layouts_match_the_oracle(gq, name):
    D, _, _, voxel, trunc = so.fused(name)  # "A" (1,9,8,17), "B" (3,5,9,17); R = 6: above nx = 5, below nz = 17
    dmax = 0.06
    _, info = eo.assert_parity(_esdf(gq, D, voxel, trunc, dmax), D, voxel, trunc, dmax, name)
    for g, i in enumerate(info):  # the case is not hollow
        mid = i["out"] & (i["e"] > np.float32(trunc)) & (i["e"] < np.float32(dmax))
        assert i["crossings"] >= 50 and i["band"].mean() >= 0.10 and mid.mean() >= 0.25, (name, g, i["crossings"], i["band"].mean(), mid.mean())
        assert (i["out"] & (D[g] >= 0)).any() and (i["out"] & (D[g] < 0)).any(), (name, g)


def test_analytic_sphere_matches_the_oracle(gq):
    D, _, voxel, trunc = eo.analytic("sphere")  # (20,18,22) at 5 mm, R = 16
    eo.assert_parity(_esdf(gq, D, voxel, trunc, 0.08), D, voxel, trunc, 0.08, "sphere")


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_long_lines_match_the_oracle(gq, axis):
    D, voxel, trunc, dmax = eo.long_lines(axis)  # 150 nodes along the axis, R = 100: lines over three wavefronts
    _, info = eo.assert_parity(_esdf(gq, D, voxel, trunc, dmax), D, voxel, trunc, dmax, f"long axis {axis}")
    e = info[0]["e"] / voxel
    assert info[0]["crossings"] >= 100 and ((e > 60) & (e < eo.LONG_R)).any() and (e > eo.LONG_R).any()


@pytest.mark.parametrize("name", sorted(eo.hand_made()))
def test_hand_made_volumes(gq, name):
    D, voxel, trunc, dmax = eo.hand_made()[name]
    got = _esdf(gq, D, voxel, trunc, dmax)
    phi, info = eo.assert_parity(got, D, voxel, trunc, dmax, name)
    T, M = np.float32(trunc), np.float32(dmax)
    if name == "zero":  # 0.0 and -0.0 are free: in band, kept, and the occupied nodes next to them are half a ... one voxel away
        assert info[0]["crossings"] == 12 and got[2, 2, 8] == 0 and np.signbit(got[3, 1, 9]) and got[2, 2, 9] == -T and got[0, 0, 0] < -T
    if name == "at_trunc":  # t = 1/2, and both ends are out of band: half a voxel, held to trunc
        assert info[0]["crossings"] == 30 and not info[0]["band"].any() and (got[:, :, 8] == -T).all() and (got[:, :, 9] == T).all()
        assert np.allclose(got[:, :, 12], 3.5 * voxel, rtol=1e-6) and np.allclose(got[:, :, 0], -M)
    if name == "non_finite":
        assert np.isnan(got[1, 1, 8]) and got[2, 3, 9] == np.inf and got[4, 2, 8] == -np.inf and info[0]["void"].sum() == 6
        plain = eo.esdf(np.where(np.isfinite(D), D, np.float32(0.001)), voxel, trunc, dmax)[1][0]["crossings"]
        assert info[0]["crossings"] < plain  # a void end cuts its edges
    if name == "no_crossing_free":
        assert np.array_equal(got, D)
    if name == "no_crossing_occupied":
        assert (got[np.isfinite(D)] == -M).all() and np.isnan(got[0, 0, :3]).all()
    if name == "one_cell":
        assert got.shape == (2, 2, 2) and info[0]["crossings"] == 4
    if name == "max_distance_is_trunc":
        assert (np.abs(got[info[0]["out"]]) == T).all()
    if name == "window_beyond_every_axis":
        assert (np.abs(got) < M).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. no tolerance
# ---------------------------------------------------------------------------------------------------------------
def test_run_to_run_stack_against_grids_and_no_allocation_with_out(gq):
    D, _, _, voxel, trunc = so.fused("B")
    src = _scene(gq, D, voxel)
    out = gq.ops.scene_esdf(src, trunc, 0.06)
    first = out.values.clone()
    for g in range(D.shape[0]):  # each grid of the stack against the single-grid call, both forms
        one = gq.ops.scene_esdf(src.scene(g), trunc, 0.06)
        assert isinstance(one, gq.ops.SceneSDF) and _bits(one.values, first[g])
        assert _bits(gq.ops.scene_esdf(_scene(gq, D[g:g + 1], voxel), trunc, 0.06).values[0], first[g])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out.values.fill_(-7.0)
    assert gq.ops.scene_esdf(src, trunc, 0.06, out=out) is out
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and _bits(out.values, first)
    assert not _bits(gq.ops.scene_esdf(src, trunc, 0.05).values, first)  # max_distance counts


def test_esdf_in_a_captured_graph_follows_src(gq):
    D, _, _, voxel, trunc = so.fused("B")
    src = _scene(gq, D, voxel)
    out = gq.ops.scene_esdf(src, trunc, 0.06)  # warm-up outside the capture: the output and the workspace exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gq.ops.scene_esdf(src, trunc, 0.06, out=out)
    other = torch.as_tensor(np.ascontiguousarray(D[[2, 0, 1]])).cuda()
    src.values.copy_(other)  # in place: the replay reads the new volume
    out.values.fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    fresh = gq.ops.scene_esdf(_scene(gq, D[[2, 0, 1]], voxel), trunc, 0.06)
    torch.cuda.synchronize()
    assert _bits(out.values, fresh.values) and _bits(src.values, other) and not _bits(out.values[0], out.values[1])


# ---------------------------------------------------------------------------------------------------------------
# 3. behaviour
# ---------------------------------------------------------------------------------------------------------------
def test_deep_inside_the_tsdf_is_flat_and_the_esdf_points_outward(gq):
    D, _, voxel, trunc = eo.analytic("sphere")
    T = np.float32(-trunc)
    deep = np.ones(tuple(n - 1 for n in D.shape), dtype=bool)  # cells whose eight nodes all hold -trunc
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                deep &= D[di:D.shape[0] - 1 + di, dj:D.shape[1] - 1 + dj, dk:D.shape[2] - 1 + dk] == T
    src = _scene(gq, D, voxel)
    centre = np.asarray(ORIGIN) + voxel * 0.5 * (np.asarray(D.shape) - 1) + eo.SPHERE_C  # the sphere's centre in the scene's frame
    # 400 points 6 .. 10 mm from the centre (at the centre itself the distance has its kink and a direction means nothing), of
    # which the data select those whose cell is flat in the TSDF
    rng = np.random.default_rng(3)
    draws = [(rng.standard_normal(3), rng.uniform(0.006, 0.010)) for _ in range(400)]  # a direction, then a radius, per point
    radial = np.stack([d / np.linalg.norm(d) for d, _ in draws])
    pts = centre + np.array([r for _, r in draws])[:, None] * radial
    cell = np.floor((pts - np.asarray(ORIGIN)) / voxel).astype(int)
    keep = deep[tuple(cell.T)]
    pts, radial = pts[keep], radial[keep]
    assert len(pts) >= 100, len(pts)
    esdf = gq.ops.scene_esdf(src, trunc, 0.08)
    grads = []
    for scene in (src, esdf):
        x = torch.as_tensor(pts, dtype=torch.float32).cuda().requires_grad_(True)
        phi = gq.ops.scene_distance(x, scene)
        phi.sum().backward()
        grads.append(x.grad.cpu().numpy().astype(np.float64))
        assert torch.isfinite(phi).all()
    assert (grads[0] == 0).all()  # exactly flat
    norm = np.linalg.norm(grads[1], axis=1)
    ang = np.degrees(np.arccos(np.clip((grads[1] * radial).sum(1) / norm, -1, 1)))
    print(f"[deep] {len(pts)} points in {int(deep.sum())} flat cells: |grad esdf| {norm.min():.3f} .. {norm.max():.3f}, angle to radial max {ang.max():.1f} deg")
    assert norm.min() > 0.4 and ang.max() < 30.0


# ---------------------------------------------------------------------------------------------------------------
# 4. through to the stepper
# ---------------------------------------------------------------------------------------------------------------
def _stepper(gq, be, sm, scene):
    fv, sp, n, _, _, _ = _two_objects(be)
    surf = torch.tensor(np.stack([sp, sp]))
    return gq.stepper.GraspStepper(_hand("allegro"), gq.ops.MeshSet([fv, fv]), surf, be, n, surface_samples=sm, scene_margin=0.03,
                                   approach_distance=DIST, approach_stations=4, weights=dict(W_BOTH), scene=scene)


def test_stepper_on_the_esdf_equals_a_stepper_on_a_clone(gq, golden_dir):
    be = 4
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    t, _ = _bin(gq, slice(0, 3))
    field = t.esdf(0.06)
    assert field is t.esdf(0.06) and isinstance(field, gq.ops.SceneSDFSet) and 0.03 > t.trunc
    clone = gq.ops.SceneSDFSet(field.values.clone(), field.origin, field.voxel)
    out = []
    for scene in (field, clone):
        st = _stepper(gq, be, sm, scene)
        assert st.clutter and st.term_names[5:] == ("E_scene", "E_approach")
        st.reset(hp, idx)
        assert float(st.terms[5].max()) > 0 and float(st.terms[6].max()) > 0
        for d in draws[:3]:
            st.step(draws=d)
        torch.cuda.synchronize()
        out.append(_state(st))
    assert _equal(*out) and torch.isfinite(out[0][2]).all()
    assert float(field.values.abs().max()) > t.trunc and _bits(field.values[t.values.abs() < t.trunc], t.values[t.values.abs() < t.trunc])


def test_integrate_and_esdf_between_two_graph_replays(gq, golden_dir):
    be = 192
    sm = _sm(golden_dir)
    _, _, _, hp, idx, draws = _two_objects(be)
    t, fuse = _bin(gq, slice(0, 2))
    field = t.esdf(0.06)
    st = _stepper(gq, be, sm, field)
    st.reset(hp, idx)
    st.capture()
    st.step(draws=draws[0])
    torch.cuda.synchronize()
    after_one = {k: getattr(st, k).clone() for k in STATE}
    old = field.values.clone()
    fuse(slice(2, 4))  # two more frames, then the field again, into the memory the graph reads
    assert t.esdf(0.06) is field
    st.step(draws=draws[1])
    torch.cuda.synchronize()
    got = _state(st)
    assert not _bits(old, field.values)
    refs = []
    for values in (field.values.clone(), old):
        ref = _stepper(gq, be, sm, gq.ops.SceneSDFSet(values, field.origin, field.voxel))
        ref.reset(hp, idx)
        ref.capture()
        for k in STATE:
            getattr(ref, k).copy_(after_one[k])
        ref.step(draws=draws[1])
        torch.cuda.synchronize()
        refs.append(_state(ref))
    assert _equal(got, refs[0]) and torch.isfinite(got[2]).all()
    assert not _equal(got, refs[1]) and not _bits(got[-2][5], refs[1][-2][5])  # E_scene of the proposal read the NEW field
