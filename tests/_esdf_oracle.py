"""The ESDF contract (include/graspqp_hip.h, "Euclidean distance field from a fused TSDF") written in numpy, in float64 on the
float32 volume a kernel is given: a brute force over the list of crossing points, not separable, so it shares no structure with
the kernels.  Per grid, h = voxel:
  void(n): D(n) not finite -> phi = D;  free(n): D(n) >= 0;  crossing(a, c): a and b = a + e_c finite, free(a) != free(b)
  p = a + t e_c, t = D_a / (D_a - D_b);  e(n) = h min_p |n - p|, +inf without a crossing
  in band (|D| < trunc): phi = D;  else phi = sign min(max(e, trunc), max_distance)
Every decision is an exact test on the float32 inputs (trunc, max_distance and voxel are taken as float32 values), so there are no
ambiguous nodes: the kernel's result must match on every node."""
import numpy as np

RTOL, ATOL = 1e-5, 1e-6  # the project's grid bound


def crossings(D):
    """D (nx,ny,nz) float32 -> (n,3) float64 crossing points in node units, the x edges first."""
    D = np.asarray(D, dtype=np.float32)
    D64 = D.astype(np.float64)
    fin = np.isfinite(D)
    with np.errstate(invalid="ignore"):
        free = D >= 0
    pts = []
    for c in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[c], b[c] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        m = fin[a] & fin[b] & (free[a] != free[b])
        idx = np.argwhere(m).astype(np.float64)
        t = D64[a][m] / (D64[a][m] - D64[b][m])
        assert ((t >= 0) & (t <= 1)).all()
        idx[:, c] += t
        pts.append(idx)
    return np.concatenate(pts, 0)


def distance(D, voxel):
    """-> e (nx,ny,nz) float64 in metres, +inf where the grid has no crossing; and the number of crossings."""
    P = crossings(D)
    shape = np.asarray(D).shape
    if not len(P):
        return np.full(shape, np.inf), 0
    X = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    e2 = np.empty(len(X))
    step = max(1, (1 << 22) // len(P))
    for s in range(0, len(X), step):
        d = X[s:s + step, None, :] - P[None]
        e2[s:s + step] = (d * d).sum(-1).min(1)
    return (np.sqrt(e2) * float(np.float32(voxel))).reshape(shape), len(P)


def esdf(D, voxel, trunc, max_distance):
    """D (G,nx,ny,nz) or (nx,ny,nz) float32 -> (phi float64 of D's shape, info): info is a list of one dict per grid with
    ``e`` (metres), ``crossings``, and the masks ``void``, ``band``, ``out`` (finite and out of band)."""
    D = np.asarray(D, dtype=np.float32)
    stack = D if D.ndim == 4 else D[None]
    trunc32, dmax = np.float32(trunc), float(np.float32(max_distance))
    phi, info = np.empty(stack.shape, dtype=np.float64), []
    for g, Dg in enumerate(stack):
        e, n = distance(Dg, voxel)
        fin = np.isfinite(Dg)
        with np.errstate(invalid="ignore"):
            band = fin & (np.abs(Dg) < trunc32)  # float32 comparison: exact
            s = np.where(Dg >= 0, 1.0, -1.0)
        far = s * np.minimum(np.maximum(e, float(trunc32)), dmax)
        phi[g] = np.where(band | ~fin, Dg.astype(np.float64), far)
        info.append(dict(e=e, crossings=n, void=~fin, band=band, out=fin & ~band))
    return (phi if D.ndim == 4 else phi[0]), info


def assert_parity(got, D, voxel, trunc, max_distance, tag):
    """A float32 result against the oracle on EVERY node: rtol 1e-5 / atol 1e-6, in-band and void nodes bit for bit.
    -> (phi, info) of the oracle."""
    D = np.asarray(D, dtype=np.float32)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == D.shape, (tag, got.dtype, got.shape)
    phi, info = esdf(D, voxel, trunc, max_distance)
    gs, Ds, ps = (x if D.ndim == 4 else x[None] for x in (got, D, phi))
    for g, i in enumerate(info):
        keep = i["void"] | i["band"]
        assert np.array_equal(gs[g][keep].view(np.int32), Ds[g][keep].view(np.int32)), (tag, g, "band and void nodes keep D's bits")
        o = i["out"]
        err = np.abs(gs[g][o].astype(np.float64) - ps[g][o])
        print(f"[{tag}] grid {g}: {i['crossings']} crossings, {int(i['band'].sum())} in band, {int(o.sum())} out of band, "
              f"{int(i['void'].sum())} void, max |phi - oracle| {err.max(initial=0):.3e} m")
        np.testing.assert_allclose(gs[g][o], ps[g][o], rtol=RTOL, atol=ATOL, err_msg=f"{tag} grid {g}")
    return phi, info


# ---- the volumes the host-body and the GPU tests share ---------------------------------------------------------------------
A_SHAPE, A_VOXEL, A_TRUNC = (20, 18, 22), 0.005, 0.015
SPHERE_C, SPHERE_R = np.array([0.003, -0.002, 0.001]), 0.03
PLANE_N, PLANE_D = np.array([0.36, -0.48, 0.8]), 0.0013


def analytic(name):
    """-> (D float32 (20,18,22), true signed distance float64, voxel, trunc): a plane or a sphere of radius 30 mm as a clipped exact
    distance on 5 mm voxels centred on the origin, trunc = 3 voxels.  Positive outside."""
    x = np.stack(np.meshgrid(*[A_VOXEL * (np.arange(s) - 0.5 * (s - 1)) for s in A_SHAPE], indexing="ij"), -1)
    true = x @ PLANE_N - PLANE_D if name == "plane" else np.linalg.norm(x - SPHERE_C, axis=-1) - SPHERE_R
    return np.clip(true, -A_TRUNC, A_TRUNC).astype(np.float32), true, A_VOXEL, A_TRUNC


def node_positions(shape, voxel):
    return np.stack(np.meshgrid(*[voxel * (np.arange(s) - 0.5 * (s - 1)) for s in shape], indexing="ij"), -1)


LONG_VOXEL, LONG_TRUNC, LONG_R = 0.005, 0.015, 100


def long_lines(axis):
    """-> (D float32, voxel, trunc, max_distance): 150 nodes along ``axis``, 3 and 4 along the others (in cyclic order), a smooth
    random field: waves of a different period and phase on every line over the first third of the long axis, many sign changes,
    then 100 nodes of plain free space, so that distances of up to about 100 nodes occur and the window R = 100 is used in full."""
    rng = np.random.default_rng(100 + axis)
    shape = [0, 0, 0]
    shape[axis], shape[(axis + 1) % 3], shape[(axis + 2) % 3] = 150, 3, 4
    k = np.arange(150, dtype=np.float64)
    other = [shape[a] for a in range(3) if a != axis]
    period, phase = rng.uniform(9.0, 23.0, other), rng.uniform(0, 2 * np.pi, other)
    f = 0.03 * np.cos(2 * np.pi * k[None, None, :] / period[..., None] + phase[..., None])
    f = f + 0.004 * rng.standard_normal(f.shape).cumsum(-1) / np.sqrt(1 + k)
    ramp = np.clip((k - 44.0) / 6.0, 0, 1)  # free space from node 50 on
    f = (1 - ramp) * f + ramp * 0.05
    D = np.clip(np.moveaxis(f, -1, axis), -LONG_TRUNC, LONG_TRUNC).astype(np.float32)
    assert D.shape == tuple(shape)
    return D, LONG_VOXEL, LONG_TRUNC, LONG_R * LONG_VOXEL


def hand_made():
    """-> {name: (D float32 (nx,ny,nz), voxel, trunc, max_distance)}: the volumes that put one rule each to the test."""
    rng = np.random.default_rng(19)
    shape, voxel, trunc = (6, 5, 18), 0.01, 0.03
    T = np.float32(trunc)
    z = (np.arange(shape[2]) - 8.37) * voxel
    x = (np.arange(shape[0]) - 2.2) * voxel
    base = np.clip(0.9 * z[None, None, :] + 0.3 * x[:, None, None] + 0.002 * rng.standard_normal(shape), -trunc, trunc).astype(np.float32)
    cases = {}
    d = np.full(shape, -T)
    d[2, 2, 8], d[3, 1, 9] = 0.0, -0.0  # two free nodes in occupied space: each is a crossing's end at t = 0
    cases["zero"] = (d, voxel, trunc, 0.09)
    d = np.full(shape, -T)
    d[:, :, 9:] = T  # every sign change is between +-trunc exactly: the crossings sit at k = 8.5, no node is in band
    cases["at_trunc"] = (d, voxel, trunc, 0.07)
    d = base.copy()
    d[1, 1, 8], d[2, 3, 9], d[4, 2, 8], d[3, 3, 7], d[0, 0, 0], d[5, 4, 17] = np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan
    cases["non_finite"] = (d, voxel, trunc, 0.08)
    cases["no_crossing_free"] = (np.full(shape, np.float32(0.02)), voxel, trunc, 0.05)  # in band: D is kept
    d = np.full(shape, -T)
    d[0, 0, :3] = np.nan  # out of band, no crossing, some void: -max_distance everywhere else
    cases["no_crossing_occupied"] = (d, voxel, trunc, 0.05)
    i, j, k = np.meshgrid(np.arange(2.0), np.arange(2.0), np.arange(2.0), indexing="ij")
    cases["one_cell"] = ((0.05 * (k - 0.4) + 0.004 * (i - 0.5) - 0.003 * j).astype(np.float32), 0.0125, 0.011, 0.05)
    cases["max_distance_is_trunc"] = (base.copy(), voxel, trunc, trunc)
    cases["window_beyond_every_axis"] = (base.copy(), voxel, trunc, 0.4)  # R = 40 > 18
    return cases
