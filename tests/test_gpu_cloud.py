"""GPU tests of objects given as oriented point clouds (surfel signed distance, include/graspqp_hip.h): the query against a
brute-force fp64 oracle written here, on clouds chosen for the ways the grid walk can go wrong; several clouds in one set;
an analytic sphere; the backward; the class surface and the stepper on a cloud object; lifetime.

Tolerances of the query are the project's own for this output contract (tests/test_gpu_parity.py::_check_sdf): sqrt(dist_sq)
and |x - closest| rtol 1e-4 / atol 2e-7, closest 1e-5, normals atol 5e-3 where the distance exceeds 1e-5, sign equal where
|h| > 1e-5.  A row whose two smallest squared centre distances differ (fp64) by at most 1e-5 g2 + 1e-12 -- a hundred fp32
ulps of the ranking value -- is a near-tie and may match the oracle evaluated at either candidate; at most 1 % of a cloud's
queries may be such rows."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cpu  # noqa: E402
from ref_cpu import models as omodels  # noqa: E402

from _parity import assert_tail_within_fp32_noise, rel_err  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402

DEFAULT_W = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}


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


# ---------------------------------------------------------------------------------------------------------------
# the oracle: numpy fp64 on the fp32 inputs
# ---------------------------------------------------------------------------------------------------------------
def _unit64(n):
    n = np.asarray(n, dtype=np.float64)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _nearest_two(x, p):
    """Indices of the two nearest centres (what a stable sort of the squared distances puts first: arg-min takes the smallest
    index among equals) and those two squared distances."""
    x, p = np.asarray(x, dtype=np.float64), np.asarray(p, dtype=np.float64)
    j1, j2 = np.empty(len(x), dtype=np.int64), np.empty(len(x), dtype=np.int64)
    g1, g2 = np.empty(len(x)), np.empty(len(x))
    for a in range(0, len(x), 256):
        d = ((x[a:a + 256, None, :] - p[None]) ** 2).sum(-1)
        k = np.arange(d.shape[0])
        j1[a:a + 256] = d.argmin(1)
        g1[a:a + 256] = d[k, j1[a:a + 256]]
        if p.shape[0] > 1:
            d[k, j1[a:a + 256]] = np.inf
            j2[a:a + 256] = d.argmin(1)
            g2[a:a + 256] = d[k, j2[a:a + 256]]
        else:
            j2[a:a + 256], g2[a:a + 256] = 0, np.inf
    return j1, j2, g1, g2


def _surfel(x, p, n, rho, j):
    """The six formulas at sample j -> (dist_sq, sign, normal, closest, h)."""
    x, pj, nj = np.asarray(x, dtype=np.float64), np.asarray(p, dtype=np.float64)[j], _unit64(n)[j]
    v = x - pj
    h = (v * nj).sum(-1)
    lat = v - h[:, None] * nj
    l = np.linalg.norm(lat, axis=1)
    scale = np.where(l <= rho, 1.0, rho / np.maximum(l, 1e-300))
    closest = pj + lat * scale[:, None]
    diff = x - closest
    d2 = (diff**2).sum(-1)
    sign = np.where(h >= 0, 1, -1)
    normal = np.where((l <= rho)[:, None], sign[:, None] * nj, diff / np.maximum(np.sqrt(d2), 1e-300)[:, None])
    return d2, sign, normal, closest, h


def _rows_match(out, x, ref):
    d2, sg, nrm, cls = out
    od2, osg, onrm, ocls, h = ref
    od = np.sqrt(od2)
    tol = 2e-7 + 1e-4 * od
    ok = np.abs(np.sqrt(d2.astype(np.float64)) - od) <= tol
    ok &= np.abs(np.linalg.norm(np.asarray(x, dtype=np.float64) - cls, axis=1) - od) <= tol
    ok &= np.abs(cls - ocls).max(1) <= 1e-5
    ok &= (od <= 1e-5) | (np.abs(nrm - onrm).max(1) <= 5e-3)
    ok &= (np.abs(h) <= 1e-5) | (sg == osg)
    return ok


def _query(gq, cs, x, qpo):
    out = gq.ops.sdf_cloud(torch.tensor(x, device="cuda"), cs, qpo)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check_cloud(out, x, p, n, rho, tag, near_cap=0.01):
    """``near_cap``: the share of near-tie rows the inputs may have (1 % everywhere but on the needle, see there); whatever it
    is, at most 1 % of the queries may NEED the allowance, i.e. match the runner-up and not the winner."""
    j1, j2, g1, g2 = _nearest_two(x, p)
    near = np.isfinite(g2) & ((g2 - g1) <= 1e-5 * np.where(np.isfinite(g2), g2, 0.0) + 1e-12)
    ok1 = _rows_match(out, x, _surfel(x, p, n, rho, j1))
    ok2 = _rows_match(out, x, _surfel(x, p, n, rho, j2))
    print(f"[{tag}] {len(x)} queries, near-ties {int(near.sum())}, rows matching the winner {int(ok1.sum())}, the runner-up only "
          f"{int((~ok1 & ok2).sum())}, max |sqrt(d2) - oracle| {np.abs(np.sqrt(out[0]) - np.sqrt(_surfel(x, p, n, rho, j1)[0])).max():.3e}")
    assert near.mean() <= near_cap, f"{tag}: {near.mean():.4f} of the queries are near-ties"
    assert (near & ~ok1).mean() <= 0.01, f"{tag}: {(near & ~ok1).mean():.4f} of the queries take the runner-up"
    bad = ~(ok1 | (near & ok2))
    assert not bad.any(), f"{tag}: rows {np.nonzero(bad)[0][:10]} differ from the oracle"
    assert np.isin(out[1], (-1, 1)).all() and out[1].dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------
# the clouds
# ---------------------------------------------------------------------------------------------------------------
def _fibonacci(N, r):
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / N
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    return (r * d).astype(np.float32), d.astype(np.float32)


def _cloud(name):
    """-> (points, normals, radius or None, extent, oracle points / normals if they differ from the stored ones)."""
    rng = np.random.default_rng(11)
    if name == "fibonacci":
        p, n = _fibonacci(642, 0.05)
        return p, n, None, 0.1, None
    if name == "box":  # 100 random samples per face with the face normal: sharp edges
        half = np.array([0.03, 0.04, 0.05])
        ps, ns = [], []
        for a in range(3):
            for s in (-1.0, 1.0):
                q = rng.uniform(-1, 1, (100, 3)) * half
                q[:, a] = s * half[a]
                nn = np.zeros((100, 3))
                nn[:, a] = s
                ps.append(q), ns.append(nn)
        return np.concatenate(ps).astype(np.float32), np.concatenate(ns).astype(np.float32), None, 0.1, None
    if name == "sheets":  # two parallel sheets 2 mm apart, opposite normals
        u = np.linspace(-0.04, 0.04, 16)
        gx, gy = np.meshgrid(u, u, indexing="ij")
        top = np.stack([gx.ravel(), gy.ravel(), np.full(256, 0.001)], 1)
        bot = top * np.array([1, 1, -1.0])
        n = np.concatenate([np.tile([0, 0, 1.0], (256, 1)), np.tile([0, 0, -1.0], (256, 1))])
        return np.concatenate([top, bot]).astype(np.float32), n.astype(np.float32), None, 0.08, None
    if name == "needle":  # collinear
        p = np.zeros((65, 3))
        p[:, 0] = np.linspace(-0.04, 0.04, 65)
        return p.astype(np.float32), np.tile([0, 0, 1.0], (65, 1)).astype(np.float32), None, 0.08, None  # far queries: see _queries
    if name == "one_point":
        return np.array([[0.01, -0.02, 0.03]], np.float32), np.array([[1.0, 2.0, 2.0]], np.float32), 0.01, 0.05, None
    if name == "duplicates":  # 64 distinct points, each stored twice with the same normal; rho of the distinct points (the
        p = rng.uniform(-0.03, 0.03, (64, 3)).astype(np.float32)  # default would be 0: every nearest neighbour is a copy)
        n = rng.normal(size=(64, 3)).astype(np.float32)
        return np.concatenate([p, p]), np.concatenate([n, n]), meshes.cloud_radius(p), 0.06, (p, n)
    if name == "random":
        return (rng.uniform(-0.05, 0.05, (20000, 3)).astype(np.float32), rng.normal(size=(20000, 3)).astype(np.float32), None, 0.1,
                None)
    raise KeyError(name)


def _queries(p, extent, Q, seed, far_axis=None):
    """The first 50 exactly on samples, 50 at 10 x extent (outside the grid), the rest normal(0, 0.8 extent) about the centre.
    ``far_axis``: the far queries lie within 60 degrees of that axis.  Seen from afar broadside, neighbouring samples of a
    line with spacing s are near-ties by geometry (relative gap of the squared distances <= s^2 / D^2 = 2.4e-6 for the
    needle), which would spend the near-tie allowance on the inputs alone; towards its ends the end point wins clearly."""
    rng = np.random.default_rng(seed)
    ctr = 0.5 * (p.min(0) + p.max(0)).astype(np.float64)
    x = ctr + rng.normal(0.0, 0.8 * extent, (Q, 3))
    x[:50] = p[rng.integers(0, len(p), 50)]
    d = rng.normal(size=(50, 3))
    if far_axis is not None:
        a = np.asarray(far_axis, dtype=np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        along = d @ a
        flip = np.abs(along) < 0.5  # mirror the broadside directions into the cones: swap the axial and the radial part
        radial = d - along[:, None] * a
        rn = np.linalg.norm(radial, axis=1)
        d[flip] = (np.sign(along[flip]) + (along[flip] == 0))[:, None] * rn[flip, None] * a + (np.abs(along[flip]) / rn[flip])[:, None] * radial[flip]
    x[50:100] = ctr + 10.0 * extent * d / np.linalg.norm(d, axis=1, keepdims=True)
    return x.astype(np.float32)


@pytest.mark.parametrize("name", ["fibonacci", "box", "sheets", "needle", "one_point", "duplicates", "random"])
def test_query_matches_the_brute_force_oracle(gq, name):
    p, n, radius, extent, distinct = _cloud(name)
    cs = gq.ops.PointCloudSet([p], [n], radius)
    rho = float(cs.radius[0])
    assert rho > 0 and (radius is not None or rho == np.float32(meshes.cloud_radius(p)))
    x = _queries(p, extent, 3000, 5, far_axis=(1.0, 0.0, 0.0) if name == "needle" else None)
    out = _query(gq, cs, x, 3000)
    again = _query(gq, cs, x, 3000)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out, again)), "the query must be bitwise reproducible"
    op, on = distinct if distinct is not None else (p, n)
    # The needle cannot meet the 1 % cap on near-tie ROWS with these queries, whatever the kernel does: a query whose foot
    # falls within 1e-5 g2 / (2 s) of the midpoint of two neighbours (spacing s = L / 64) is one, i.e. a share 1e-5 g2 / s^2
    # of the queries abreast of the needle.  With g2 = y^2 + z^2 of mean 2 (0.8 L)^2 and P(|x| < L / 2) = 0.47 that is
    # 0.47 * 1e-5 * 1.28 * 64^2 = 2.5 % at any scale (the oracle alone counts 77 of 3 000).  Its cap on the inputs is 3 %;
    # the cap of 1 % on the rows that take the runner-up holds for it as for every cloud.
    _check_cloud(out, x, op, on, rho, name, near_cap=0.03 if name == "needle" else 0.01)
    # a query lying on a sample: distance 0 and that sample's normal (its first copy for the duplicates)
    j1 = _nearest_two(x[:50], op)[0]
    assert np.abs(out[0][:50]).max() <= (2e-7) ** 2 and (out[1][:50] == 1).all()
    np.testing.assert_allclose(out[2][:50], _unit64(on)[j1], atol=1e-6)
    cs.close()


@pytest.mark.parametrize("name", ["fibonacci", "box", "sheets", "needle", "random"])
def test_queries_near_the_surface(gq, name):
    """Where the contacts of a converged grasp are: a sample plus normal(0, 1.5 rho).  These queries end in the shell walk
    (the first, second, ... shell confirms the winner), the far ones of the test above in the scan of all points."""
    p, n, radius, _, _ = _cloud(name)
    cs = gq.ops.PointCloudSet([p], [n], radius)
    rho = float(cs.radius[0])
    rng = np.random.default_rng(17)
    x = (p[rng.integers(0, len(p), 2000)].astype(np.float64) + rng.normal(0.0, 1.5 * rho, (2000, 3))).astype(np.float32)
    _check_cloud(_query(gq, cs, x, 2000), x, p, n, rho, name + " near")
    cs.close()


def test_several_clouds_in_one_set(gq):
    clouds = [meshes.mesh_to_cloud(meshes.icosphere(2, 0.04), 63, seed=1), meshes.mesh_to_cloud(meshes.superquadric(3, 32, 16), 1000, seed=2),
              meshes.mesh_to_cloud(meshes.box(), 4097, seed=3)]
    cs = gq.ops.PointCloudSet([c[0] for c in clouds], [c[1] for c in clouds])
    assert cs.n_obj == 3 and cs.n_points == 63 + 1000 + 4097
    for qpo in (65, 1):  # 195 queries: not a multiple of the wavefronts per block; and one query per cloud
        sel = np.r_[45:55, 95:150] if qpo == 65 else np.array([120])  # 5 on samples, 5 far away, 55 around the cloud
        x = np.concatenate([_queries(c[0], float((c[0].max(0) - c[0].min(0)).max()), 165, 20 + i)[sel] for i, c in enumerate(clouds)])
        out = _query(gq, cs, x, qpo)
        for i, (p, n) in enumerate(clouds):
            sl = slice(i * qpo, (i + 1) * qpo)
            _check_cloud(tuple(o[sl] for o in out), x[sl], p, n, float(cs.radius[i]), f"cloud {i} qpo={qpo}")
    with pytest.raises(RuntimeError, match="queries_per_object"):
        gq.ops.sdf_cloud(torch.zeros(10, 3, device="cuda"), cs, 5)
    cs.close()


def test_non_finite_and_huge_queries(gq):
    """A non-finite query has no nearest centre: NaN outputs with sign +1, and the rows beside it are untouched.  A finite query
    a light-second away still gets a sample of the cloud (every centre is a near-tie there: only the contract's shape is asked)."""
    p, n = _fibonacci(642, 0.05)
    cs = gq.ops.PointCloudSet([p], [n])
    x = np.array([[np.nan, 0, 0], [0.06, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0.01], [3e8, 0, 0], [-1e6, 2e7, 3.0], [0, 0, 0.049],
                  [1e25, 0, 0]], np.float32)  # the last one: d^2 overflows fp32
    d2, sg, nrm, cls = _query(gq, cs, x, len(x))
    bad = [0, 2, 3, 7]
    assert np.isnan(d2[bad]).all() and np.isnan(nrm[bad]).all() and np.isnan(cls[bad]).all() and (sg[bad] == 1).all()
    ok = [1, 4, 5, 6]
    assert np.isfinite(d2[ok]).all() and np.isfinite(cls[ok]).all() and np.allclose(np.linalg.norm(nrm[ok], axis=1), 1.0, atol=1e-5)
    assert np.allclose(np.linalg.norm(cls[ok], axis=1), 0.05, atol=float(cs.radius[0]))  # on a disc of the sphere
    _check_cloud(tuple(o[[1, 6]] for o in (d2, sg, nrm, cls)), x[[1, 6]], p, n, float(cs.radius[0]), "beside non-finite rows")
    assert sg[1] == 1 and sg[6] == -1
    cs.close()


def test_analytic_sphere(gq):
    from scipy.spatial import cKDTree

    r, N = 0.05, 2562
    p, n = _fibonacci(N, r)
    rng = np.random.default_rng(3)
    s = rng.normal(size=(200000, 3))
    s = r * s / np.linalg.norm(s, axis=1, keepdims=True)
    c = float(cKDTree(p.astype(np.float64)).query(s)[0].max())  # covering radius of the cloud, sampled
    d = rng.normal(size=(3000, 3))
    x = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(r - 0.02, r + 0.03, (3000, 1))).astype(np.float32)
    cs = gq.ops.PointCloudSet([p], [n])
    d2, sg, _, _ = _query(gq, cs, x, 3000)
    nx = np.linalg.norm(x.astype(np.float64), axis=1)
    bound = 1.1 * nx * c * c / (2 * r * r) + 1e-6
    err = np.abs(sg * np.sqrt(d2.astype(np.float64)) - (nx - r))
    print(f"[sphere] covering radius {c:.3e}, rho {float(cs.radius[0]):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    clear = np.abs(nx - r) > bound
    assert clear.sum() > 2000 and (sg[clear] == np.sign(nx - r)[clear]).all()
    cs.close()


def test_backward_through_the_dispatcher(gq):
    p, n = meshes.mesh_to_cloud(meshes.box(), 700, seed=4)
    cs = gq.ops.PointCloudSet([p], [n])
    x = torch.randn(257, 3, device="cuda").mul(0.06).requires_grad_()
    w = torch.randn(257, device="cuda")
    d2, sg, nrm, cls = torch.ops.graspqp_amd.sdf_cloud(x, cs.hid, 257)
    assert d2.requires_grad and not sg.requires_grad and not nrm.requires_grad and not cls.requires_grad
    (d2 * w).sum().backward()
    want = (2 * (x.detach() - cls) * w[:, None]).cpu().numpy()
    np.testing.assert_allclose(x.grad.cpu().numpy(), want, rtol=1e-6, atol=1e-9)
    # (sign / normal / closest are non-differentiable outputs: their upstream in the backward is None); the wrapper's route
    # gives the same bits
    x2 = x.detach().clone().requires_grad_()
    out2 = gq.ops.sdf_cloud(x2, cs, 257)
    (out2[0] * w).sum().backward()
    assert torch.equal(x2.grad, x.grad) and all(torch.equal(a, b) for a, b in zip(out2, (d2, sg, nrm, cls)))
    e = gq.ops.sdf_cloud(torch.zeros(0, 3, device="cuda"), cs, 1)
    assert e[0].shape == (0,) and e[3].shape == (0, 3)
    cs.close()


# ---------------------------------------------------------------------------------------------------------------
# class surface and stepper on a cloud object
# ---------------------------------------------------------------------------------------------------------------
class _OracleCloudObject:
    """fp64 (or fp32) stand-in of a cloud ObjectModel for ref_cpu.calculate_energy: cal_distance is the oracle above with torch
    autograd (only dist_sq carries a gradient, through x - closest with closest held constant)."""

    def __init__(self, p, n, rho, surface_points, batch_size_each, dtype=torch.float64):
        self.p, self.n, self.rho, self.dtype, self.batch_size_each = p, n, rho, dtype, batch_size_each
        sp = torch.as_tensor(surface_points, dtype=dtype)[None]
        self.surface_points_tensor = sp.repeat_interleave(batch_size_each, dim=0)
        self.object_scale_tensor = torch.ones(1, batch_size_each, dtype=dtype)

    @property
    def cog(self):
        return self.surface_points_tensor.mean(dim=1)

    def cal_distance(self, x):
        B, m, _ = x.shape
        xf = x.reshape(-1, 3)
        xn = xf.detach().double().numpy()
        _, sign, normal, closest, _ = _surfel(xn, self.p, self.n, self.rho, _nearest_two(xn, self.p)[0])
        d2 = ((xf - torch.as_tensor(closest, dtype=self.dtype)) ** 2).sum(-1)
        sgn = torch.as_tensor(sign, dtype=self.dtype)
        dis = torch.sqrt(d2 + 1e-8) * (-sgn)
        return dis.reshape(B, m), (torch.as_tensor(normal, dtype=self.dtype) * sgn[:, None]).reshape(B, m, 3)


def _sphere_scene(golden_dir, fixture):
    g = _load(golden_dir, fixture)
    r = float(np.linalg.norm(g["obj0_face_verts"].reshape(-1, 3), axis=1).max())
    p, n = _fibonacci(2562, r)
    return g, p, n, g["obj0_surface_points"]


def _class_surface(gq, spec, p, n, sp, be, hp, idx, names=tuple(DEFAULT_W)):
    from graspqp_amd.core.energy import calculate_energy
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.core.object_model import ObjectModel
    from graspqp_amd.metrics import GraspSpanMetricFactory as GF

    hm = HandModel(spec, "cuda")
    om = ObjectModel(batch_size_each=be, num_samples=sp.shape[0])
    om.initialize_from_point_clouds([p], [n], surface_points_list=[sp])
    assert om.object_mesh_list is None and om.object_face_verts_list is None and om._meshset is None
    hm.set_parameters(hp.clone().requires_grad_(), idx)
    fn = GF.create(GF.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
    return hm, om, fn, lambda: calculate_energy(hm, om, energy_fnc=fn, energy_names=list(names), svd_gain=0.1)


def test_class_surface_matches_the_oracle(gq, golden_dir):
    g, p, n, sp = _sphere_scene(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    spec = get_hand_spec("allegro")
    be = int(g["batch_size_each"])
    hp = torch.tensor(g["hand_pose"], dtype=torch.float32)
    idx = torch.tensor(g["contact_idx"])
    hm, om, _, energy = _class_surface(gq, spec, p, n, sp, be, hp.cuda(), idx.cuda())
    rho = float(om._cloudset.radius[0])
    losses = energy()
    sum(DEFAULT_W[k] * losses[k] for k in DEFAULT_W if k != "E_fc").sum().backward(retain_graph=True)
    g_rest = hm.hand_pose.grad.clone().cpu().numpy()
    (DEFAULT_W["E_fc"] * losses["E_fc"]).sum().backward()  # accumulates: the gradient of the total
    g_all = hm.hand_pose.grad.cpu().numpy()
    res = {}
    for dt in (torch.float64, torch.float32):
        oh = omodels.OracleHand(spec, dt)
        oo = _OracleCloudObject(p, n, rho, sp, be, dt)
        hpo = hp.to(dt).requires_grad_()
        oh.set_parameters(hpo, idx)
        lo = ref_cpu.calculate_energy(oh, oo, box_form=True)
        res[dt] = (lo, oh)
    lo, oh = res[torch.float64]
    for k in ("E_dis", "E_pen", "E_spen", "E_joints"):
        np.testing.assert_allclose(losses[k].detach().cpu().numpy(), lo[k].detach().numpy(), rtol=3e-4, atol=3e-6, err_msg=k)
    e64 = lo["E_fc"].detach().numpy()
    assert_tail_within_fp32_noise(rel_err(losses["E_fc"].detach().cpu().numpy(), e64),
                                  rel_err(res[torch.float32][0]["E_fc"].detach().double().numpy(), e64), "E_fc on a cloud")
    sum(DEFAULT_W[k] * lo[k] for k in DEFAULT_W if k != "E_fc").sum().backward(retain_graph=True)
    go = oh.hand_pose.grad.clone().numpy()
    gerr = np.linalg.norm(g_rest - go) / np.linalg.norm(go)
    (DEFAULT_W["E_fc"] * lo["E_fc"]).sum().backward()  # accumulates: the gradient of the total
    ga = oh.hand_pose.grad.numpy()
    gerr_all = np.linalg.norm(g_all - ga) / np.linalg.norm(ga)
    print(f"[class surface] grad rel err without E_fc {gerr:.3e}, with E_fc {gerr_all:.3e}")
    assert gerr < 1e-3 and gerr_all < 5e-3


def _cloud_stepper(gq, p, n, sp, be, **kw):
    return gq.stepper.GraspStepper(_hand("allegro"), gq.ops.PointCloudSet([p], [n]), torch.tensor(sp)[None], be, 4, **kw)


def test_stepper_evaluate_matches_the_class_surface(gq, golden_dir):
    g, p, n, sp = _sphere_scene(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    spec, be = get_hand_spec("allegro"), 8  # the fixture's eight poses on ONE cloud
    hp = torch.tensor(g["hand_pose0"], dtype=torch.float32).cuda()
    idx = torch.tensor(g["contact_idx0"]).cuda()
    assert hp.shape[0] == 8
    st = _cloud_stepper(gq, p, n, sp, be)
    assert st.cloud and st._sdf_desc is None
    terms, total, grad = st.evaluate(hp, idx)
    hm, om, _, energy = _class_surface(gq, spec, p, n, sp, be, hp, idx)
    losses = energy()
    tot = sum(DEFAULT_W[k] * losses[k] for k in DEFAULT_W)
    tot.sum().backward()
    for k in DEFAULT_W:
        np.testing.assert_allclose(terms[k].cpu().numpy(), losses[k].detach().cpu().numpy(), rtol=2e-4, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(total.cpu().numpy(), tot.detach().cpu().numpy(), rtol=2e-4)
    assert (hm.hand_pose.grad - grad).norm() <= 2e-3 * grad.norm()
    # the stepper's four buffers are the op's outputs on its contact points, bit for bit
    d2, sg, nrm, cls = gq.ops.sdf_cloud(st.cpts.reshape(-1, 3), st.objs, be * 4)
    assert torch.equal(d2, st.d2.reshape(-1)) and torch.equal(sg, st.sgn.reshape(-1)) and torch.equal(cls, st.closest.reshape(-1, 3))
    dis, nrm2, cls2 = om.cal_distance(st.cpts, with_closest_points=True)
    assert dis.shape == (8, 4) and nrm2.shape == (8, 4, 3) and torch.equal(cls2.reshape(-1, 3), cls)
    # what export_poses writes for this object (it only calls cal_distance, also with all contact candidates at once)
    from graspqp_amd.export import snapshot_dicts

    (data,) = snapshot_dicts(hm, tot.detach(), om, 1, 8)
    assert data["values"].shape == (8,) and data["parameters"]["root_pose"].shape == (8, 7)
    for key in ("grasp_velocities", "full_grasp_velocities", "grasp_velocities_off"):
        assert all(torch.isfinite(v).all() and v.shape == (8,) for v in data[key].values()), key


@pytest.mark.parametrize("tabletop", [False, True])
def test_iterations_match_the_class_surface(gq, golden_dir, tabletop):
    """Five iterations (the third one re-initialises two rows), teacher-forced from the class-surface state: the loop of
    tests/test_gpu_tabletop.py::test_tabletop_iterations_match_the_class_surface on a cloud object."""
    from graspqp_amd.core.optimizer import MalaStar

    C = gq.C
    g, p, n, sp = _sphere_scene(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    ge = _load(golden_dir, "energy_allegro_sphere_b4_n4.npz")
    sm = (ge["opt_surface_points"], ge["opt_surface_link"])
    be = B = g["hand_pose0"].shape[0]  # the fixture's eight poses on ONE cloud
    spec = get_hand_spec("allegro")
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    w = dict(DEFAULT_W)
    kw = {}
    if tabletop:
        w.update({"E_prior": 2.0, "E_wall": 3.0})
        kw = dict(weights={"E_prior": 2.0, "E_wall": 3.0}, surface_samples=sm)
    st = _cloud_stepper(gq, p, n, sp, be, **kw)
    hm, om, fn, energy_terms = _class_surface(gq, spec, p, n, sp, be, f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda(), tuple(w))
    if tabletop:
        hm.set_surface_points(*sm)

    def total():
        losses = energy_terms()
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
    for s in range(1, 6):
        grad = hm.hand_pose.grad
        st.hand_pose.copy_(hm.hand_pose.detach())
        st.contact_idx.copy_(hm.contact_point_indices)
        st.grad.copy_(torch.zeros_like(st.grad) if grad is None else grad)
        st.energy.copy_(energy)
        st.ema.copy_(opt.ema_grad_hand_pose)
        st.step_count.copy_(opt.step)
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
        pr = torch.exp((energy - new_energy.detach()) / T)
        cands = [f32(f"s{s}_u_accept")] + [torch.rand(B, generator=torch.Generator().manual_seed(1000 * s + k)).cuda() for k in range(8)]
        u_ac = next(u for u in cands if bool(((u - pr).abs() >= 1e-3).all()))
        with torch.no_grad():
            accept, T_cls = opt.accept_step(energy, new_energy, rm, z, 1.0, u_accept=u_ac)
        assert torch.allclose(T_cls, T)
        if s == 3:
            st.step_reset(mask, new_pose, new_idx, draws=(u_sw, n_ix, u_ac))
        else:
            st.step(draws=(u_sw, n_ix, u_ac))
        torch.cuda.synchronize()
        rel = ((st.total_new - new_energy.detach()).abs() / new_energy.detach().abs().clamp_min(1e-12)).cpu().numpy()
        print(f"[iteration {s} tabletop={tabletop}] total_new rel err max {rel.max():.3e}, accepted {int(accept.sum())}/{B}")
        assert rel.max() < 3e-4, rel
        assert st.accept.bool().tolist() == accept.tolist()
        if s == 3:
            assert accept[mask.cuda()].all()
        np.testing.assert_allclose(st.energy.cpu().numpy(), energy.cpu().numpy(), rtol=3e-4)
        np.testing.assert_allclose(st.hand_pose.cpu().numpy(), hm.hand_pose.detach().cpu().numpy(), rtol=1e-5, atol=2e-6)
        assert torch.equal(st.contact_idx, hm.contact_point_indices)
        assert not st._fk_sdf_attached


@pytest.mark.parametrize("fork", [None, True])
def test_graph_replay_equals_eager_steps(gq, golden_dir, fork):
    g, p, n, sp = _sphere_scene(golden_dir, "mala_allegro_sphere_b8_n4.npz")
    be = g["hand_pose0"].shape[0]
    f32 = lambda k: torch.tensor(g[k], dtype=torch.float32).cuda()
    draws = [(f32(f"s{s}_u_switch"), torch.tensor(g[f"s{s}_new_idx"]).cuda(), f32(f"s{s}_u_accept")) for s in (1, 2, 3)]
    out = []
    for graph in (False, True):
        st = _cloud_stepper(gq, p, n, sp, be)
        st.reset(f32("hand_pose0"), torch.tensor(g["contact_idx0"]).cuda())
        if graph:
            st.capture(fork=fork)
            assert st.graph_mode == ("graph branches" if fork else "one grid")
        for d in draws:
            st.step(draws=d)
        torch.cuda.synchronize()
        assert not st._fk_sdf_attached  # the FK forward launch never carries the object query of a cloud
        out.append([getattr(st, k).clone() for k in ("hand_pose", "contact_idx", "energy", "grad", "terms", "accept")])
    for a, b, k in zip(out[0], out[1], ("hand_pose", "contact_idx", "energy", "grad", "terms", "accept")):
        assert torch.equal(a, b), k
    assert torch.isfinite(out[0][2]).all()


def test_initialize_and_run_on_a_cloud_object(gq):
    """ObjectModel on a cloud -> GraspStepper.initialize / run (with a re-initialisation) -> cal_distance of the result: the
    flow of scripts/fit.py; surface points by farthest-point sampling of the cloud's own points."""
    from graspqp_amd.core.object_model import ObjectModel

    p, n = meshes.mesh_to_cloud(meshes.superquadric(3, 32, 16), 3000, seed=6)
    om = ObjectModel(batch_size_each=8, num_samples=256)
    om.initialize_from_point_clouds([p], [n])
    sp = om.surface_points_each
    assert sp.shape == (1, 256, 3)
    rows = {tuple(r) for r in p.tolist()}
    assert all(tuple(r) in rows for r in sp[0].cpu().numpy().tolist()) and len({tuple(r) for r in sp[0].cpu().tolist()}) == 256
    st = gq.stepper.GraspStepper(_hand("allegro"), om._cloudset, sp, 8, 4, seed=3)
    st.set_hulls(om.convex_hulls())
    st.initialize()
    e0 = st.energy.clone()
    st.capture(iters=2)
    st.run(12, reset_epochs=3, z_score_threshold=0.5)
    torch.cuda.synchronize()
    assert torch.isfinite(st.energy).all() and torch.isfinite(st.hand_pose).all() and not torch.equal(e0, st.energy)
    dis, nrm = om.cal_distance(st.cpts)
    assert torch.isfinite(dis).all() and torch.allclose(nrm.norm(dim=-1), torch.ones(8, 4, device="cuda"), atol=1e-4)


def test_lifetime(gq):
    import ctypes

    def live():
        v = ctypes.c_int64(0)
        gq.C.call("gq_setup_live_allocations", ctypes.byref(v))
        return v.value

    base = live()
    p, n = _fibonacci(200, 0.05)
    cs = gq.ops.PointCloudSet([p, p], [n, n])
    assert live() == base + 6  # two host tables, four device arrays
    hid = cs.hid
    cs.close()
    assert live() == base
    with pytest.raises(RuntimeError):
        gq.ops.sdf_cloud(torch.zeros(2, 3, device="cuda"), cs, 1)
    with pytest.raises(RuntimeError):
        torch.ops.graspqp_amd.sdf_cloud(torch.zeros(2, 3, device="cuda"), hid, 1)
    for bad in ([np.zeros((3, 3), np.float32)], [np.full((3, 3), np.nan, np.float32)]):  # zero / non-finite normals
        with pytest.raises(RuntimeError, match="normal"):
            gq.ops.PointCloudSet([p[:3]], bad, 0.01)
    assert live() == base
