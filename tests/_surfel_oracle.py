"""The surfel extraction contract (include/graspqp_hip.h, "target objects from depth images") written in numpy, in float64 on the
float32 volume a kernel is given, and once more in float32 for the noise floor of the normals.  Per grid, inside the half-open
node region:
  observed(n): n in the grid, D(n) finite, W(n) >= min_weight
  crossing(a, c): a and b = a + e_c in the region, both observed, (D_a >= 0) != (D_b >= 0), |D_a| < trunc, |D_b| < trunc
  t = D_a / (D_a - D_b),  p = x_a + t voxel e_c
  d_c(m) = (D(m+e_c) - D(m-e_c)) / 2, one-sided where one neighbour is observed, 0 where none is
  g_c(n) = (1,2,1) x (1,2,1) mean of d_c over the observed nodes of the 3 x 3 neighbourhood of n transverse to c
  v = (1 - t) g(a) + t g(b),  normal = v / |v| if |v|^2 > 1e-20 else e_c sign(D_b - D_a)
Every test that decides whether an edge exists is exact on the float32 inputs, so the oracle and a kernel find the same edges;
the output order is (tile of 4 x 4 x 16 nodes, x slowest; node in the tile, z fastest; axis).  An edge is ``ambiguous`` only where
|v|^2 is within a factor 4 of the fallback's threshold."""
import numpy as np

import _tsdf_oracle as to

TILE = (4, 4, 16)
MIN_NORM2 = 1e-20


def _shift(A, off):
    """A (nx,ny,nz) moved so that out[n] = A[n + off], NaN where n + off leaves the grid."""
    out = np.full_like(A, np.nan)
    src, dst = [], []
    for o, n in zip(off, A.shape):
        lo, hi = max(0, -o), min(n, n - o)
        if hi <= lo:
            return out
        dst.append(slice(lo, hi)), src.append(slice(lo + o, hi + o))
    out[tuple(dst)] = A[tuple(src)]
    return out


def _unit(c):
    e = [0, 0, 0]
    e[c] = 1
    return e


def gradients(Dn, dtype):
    """Dn (nx,ny,nz): D where observed, NaN elsewhere -> g (nx,ny,nz,3) of the contract in ``dtype`` (NaN where n is unobserved)."""
    Dn = Dn.astype(dtype)
    seen = ~np.isnan(Dn)
    g = np.zeros(Dn.shape + (3,), dtype=dtype)
    half, zero = dtype(0.5), dtype(0)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            e = np.array(_unit(c))
            hi, lo = _shift(Dn, e), _shift(Dn, -e)
            a, b = ~np.isnan(lo), ~np.isnan(hi)
            d = np.where(a & b, half * (hi - lo), np.where(b, hi - Dn, np.where(a, Dn - lo, zero))).astype(dtype)
            d = np.where(seen, d, np.nan).astype(dtype)
            u, v = [x for x in range(3) if x != c]
            num, den = np.zeros(Dn.shape, dtype=dtype), np.zeros(Dn.shape, dtype=dtype)
            for du in (-1, 0, 1):
                for dv in (-1, 0, 1):
                    off = [0, 0, 0]
                    off[u], off[v] = du, dv
                    dm = _shift(d, off)
                    ok = ~np.isnan(dm)
                    w = dtype((2 - abs(du)) * (2 - abs(dv)))
                    num = (num + np.where(ok, w * dm, zero)).astype(dtype)
                    den = (den + np.where(ok, w, zero)).astype(dtype)
            g[..., c] = np.where(seen, num / np.where(den > 0, den, 1), np.nan)
    return g


def extract(D, W, origin, voxel, trunc, min_weight=1.0, region=None, dtype=np.float64):
    """D (G,nx,ny,nz) float32, W like D or None -> a list of G dicts in the contract's order: ``points`` (n,3), ``normals`` (n,3) in
    ``dtype``, ``edges`` (n,4) int = (i,j,k,c), ``ambiguous`` (n) bool, ``fallback`` (n) bool."""
    D = np.asarray(D, dtype=np.float32)
    assert D.ndim == 4
    G, shape = D.shape[0], D.shape[1:]
    trunc, min_weight, voxel = np.float32(trunc), np.float32(min_weight), np.float32(voxel)
    origin = np.asarray(origin, dtype=np.float32)
    reg = [0, shape[0], 0, shape[1], 0, shape[2]] if region is None else [int(r) for r in region]
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    inreg = np.ones(shape, dtype=bool)
    for a in range(3):
        inreg &= (idx[..., a] >= reg[2 * a]) & (idx[..., a] < reg[2 * a + 1])
    out = []
    for g in range(G):
        with np.errstate(invalid="ignore"):
            seen = np.isfinite(D[g])
            if W is not None:
                seen &= np.asarray(W, dtype=np.float32)[g] >= min_weight
            Dn = np.where(seen, D[g], np.float32(np.nan))
            band = seen & (np.abs(Dn) < trunc)  # float32 comparisons: exact
        grad = gradients(Dn, dtype)
        rows = []
        for c in range(3):
            e = _unit(c)
            with np.errstate(invalid="ignore"):
                Db = _shift(Dn, e)
                cross = inreg & (_shift(inreg.astype(np.float32), e) == 1) & band & (np.abs(Db) < trunc) & ((Dn >= 0) != (Db >= 0))
            cross &= ~np.isnan(Db)
            ijk = idx[cross]
            rows.append(np.concatenate([ijk, np.full((len(ijk), 1), c)], 1))
        edges = np.concatenate(rows, 0).astype(np.int64)
        # the launch's order: tile (x slowest), thread in the tile (z fastest), axis
        i, j, k, c = edges.T
        nt = [-(-n // t) for n, t in zip(shape, TILE)]
        tile = ((i // TILE[0]) * nt[1] + j // TILE[1]) * nt[2] + k // TILE[2]
        tid = ((i % TILE[0]) * TILE[1] + j % TILE[1]) * TILE[2] + k % TILE[2]
        edges = edges[np.lexsort((c, tid, tile))]
        i, j, k, c = edges.T
        n = len(edges)
        a = (i, j, k)
        b = tuple(x + (c == ax) for ax, x in enumerate(a))
        Da, Db = Dn[a].astype(dtype), Dn[b].astype(dtype)
        t = Da / (Da - Db) if n else np.zeros(0, dtype=dtype)
        assert ((t >= 0) & (t <= 1)).all()
        P = (origin.astype(dtype)[None] + voxel.astype(dtype) * edges[:, :3].astype(dtype)).astype(dtype)
        P[np.arange(n), c] += (t * voxel.astype(dtype)).astype(dtype)
        v = ((dtype(1) - t)[:, None] * grad[a] + t[:, None] * grad[b]).astype(dtype)
        n2 = (v * v).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            good = n2 > dtype(MIN_NORM2)
            N = np.where(good[:, None], v / np.sqrt(np.where(good, n2, 1))[:, None], 0).astype(dtype)
        fb = ~good
        N[fb, c[fb]] = np.where(Db[fb] > Da[fb], 1, -1)
        with np.errstate(invalid="ignore"):
            amb = ~((n2 > 4 * MIN_NORM2) | (n2 < MIN_NORM2 / 4))
        out.append(dict(points=P, normals=N, edges=edges, ambiguous=amb, fallback=fb))
    return out


def angle(a, b):
    """Angle in radians between the rows of two arrays of unit vectors, accurate for small angles."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 2 * np.arcsin(np.clip(0.5 * np.linalg.norm(a - b, axis=-1), 0, 1))


NORMAL_FLOOR = 1e-5  # rad


def assert_parity(points, normals, count, D, W, origin, voxel, trunc, min_weight, region, tag, min_surfels=0, capacity=None):
    """float32 results of an extraction, (G,cap,3), (G,cap,3), (G,2), against the oracle on the same volume: the count exactly, the
    order (a wrong order misplaces positions by a voxel), positions at rtol 1e-5 / atol 1e-6 (the bound of the same grid geometry
    in _tsdf_oracle.assert_parity), normals by angle on the non-ambiguous edges, within 4 x the largest angle between the oracle's
    own float32 and float64 normals on the case, at least 1e-5 rad (the device sums the <= 18 stencil terms in another order).
    On the oracle's own output at most 1 % of the edges may be ambiguous and every grid must yield ``min_surfels``.
    -> the oracle's float64 result."""
    ref = extract(D, W, origin, voxel, trunc, min_weight, region)
    ref32 = extract(D, W, origin, voxel, trunc, min_weight, region, dtype=np.float32)
    points, normals, count = np.asarray(points), np.asarray(normals), np.asarray(count)
    for g, (r, r32) in enumerate(zip(ref, ref32)):
        n = len(r["edges"])
        assert np.array_equal(r["edges"], r32["edges"])
        cap = points.shape[1] if capacity is None else capacity
        m = min(n, cap)
        assert tuple(count[g]) == (n, m), (tag, g, tuple(count[g]), n, m)
        amb = r["ambiguous"] | r32["ambiguous"]
        assert n >= min_surfels and amb.sum() <= 0.01 * max(n, 1), (tag, g, n, int(amb.sum()))
        ok = ~amb
        floor = float(angle(r32["normals"][ok], r["normals"][ok]).max()) if ok.any() else 0.0
        bound = max(4 * floor, NORMAL_FLOOR)
        np.testing.assert_allclose(points[g, :m], r["points"][:m], rtol=1e-5, atol=1e-6, err_msg=f"{tag} grid {g}")
        got = normals[g, :m].astype(np.float64)
        assert np.abs(np.linalg.norm(got, axis=-1) - 1).max(initial=0) < 1e-5, tag
        err = angle(got[ok[:m]], r["normals"][:m][ok[:m]])
        print(f"[{tag}] grid {g}: {n} surfels, {int(amb.sum())} ambiguous, {int(r['fallback'].sum())} fallback normals, max position "
              f"err {np.abs(points[g, :m] - r['points'][:m]).max(initial=0):.3e} m, normal angle max {err.max(initial=0):.3e} rad "
              f"(oracle f32 vs f64 {floor:.3e}, bound {bound:.3e})")
        assert err.max(initial=0) <= bound, (tag, g, float(err.max()), bound)
        fb = r["fallback"][:m] & ok[:m]
        assert np.array_equal(got[fb], r["normals"][:m][fb]), tag  # the fallback is an exact axis
    return ref


# ---- the cases the host-body and the GPU tests share --------------------------------------------------------------------------
SPHERE_SHAPE, SPHERE_VOXEL = (12, 12, 12), 0.01


def keep_label(depth, labels, label):
    """ops.keep_label on numpy arrays: the depth where the pixel carries ``label``, 0 (no measurement) elsewhere."""
    return np.where(np.asarray(labels) == label, depth, np.float32(0)).astype(np.float32)


def fused(name):
    """-> (D float32 (G,nx,ny,nz), W float32, origin, voxel, trunc) of a case fused by the TSDF oracle (rounded to float32: the
    extraction's input): "A", "B" the layouts of _tsdf_oracle; "sphere" a 12^3 grid of voxel 0.01 centred on to.SPHERE, fused from
    the four cameras with only the sphere's pixels kept, trunc = 3 voxel."""
    if name == "sphere":
        trunc = 3 * SPHERE_VOXEL
        origin = tuple(float(c) - 0.5 * float(np.float32(SPHERE_VOXEL)) * (n - 1) for c, n in zip(to.SPHERE[0], SPHERE_SHAPE))
        vol = to.Volume(1, SPHERE_SHAPE, origin, SPHERE_VOXEL, -trunc)
        cam, depth, labels = to.cameras(4)
        to.integrate(vol, keep_label(depth, labels, 1), None, cam, to.INTRINSICS, to.DEPTH_RANGE, trunc)
    else:
        vol, tT, skip, n = to.layout(name)
        trunc = to.TRUNC
        cam, depth, labels = to.cameras(n)
        to.integrate(vol, depth, labels, cam, to.INTRINSICS, to.DEPTH_RANGE, trunc, 64.0, tT, skip)
    return vol.D.astype(np.float32), vol.W.astype(np.float32), vol.out.origin, float(vol.out.voxel), trunc


def tiny():
    """A (2,2,2) grid, one cell: every stencil neighbour lies outside the grid.  -> the tuple of ``hand_made``'s values."""
    i, j, k = np.meshgrid(np.arange(2.0), np.arange(2.0), np.arange(2.0), indexing="ij")
    d = (0.011 * (k - 0.4) + 0.004 * (i - 0.5) - 0.003 * j).astype(np.float32)
    return d[None], np.ones_like(d)[None], (0.1, -0.2, 0.3), 0.0125, 0.02, 1.0, None, None


def hand_made():
    """-> {name: (D (1,nx,ny,nz) float32, W or None, origin, voxel, trunc, min_weight, region or None, expected count or None)}: the
    volumes that put one rule each to the test."""
    rng = np.random.default_rng(7)
    shape, voxel, trunc, origin = (6, 5, 18), 0.01, 0.03, (-0.02, 0.01, 0.0)
    z = (np.arange(shape[2]) - 8.37) * voxel
    x = (np.arange(shape[0]) - 2.2) * voxel
    base = np.clip(0.6 * z[None, None, :] + 0.3 * x[:, None, None] + 0.002 * rng.standard_normal(shape), -trunc, trunc).astype(np.float32)
    ones = np.ones(shape, dtype=np.float32)
    cases = {}
    d = base.copy()
    d[2, 2, 8], d[3, 1, 9] = 0.0, -0.0  # an exact zero is on the free side; -0.0 >= 0 holds too
    cases["zero"] = (d, ones, None, None)
    d = base.copy()
    d[:, :, :8], d[:, :, 8:] = -np.float32(trunc), np.float32(trunc)  # every sign change is between +-trunc exactly: no crossing
    cases["at_trunc"] = (d, ones, None, 0)
    d = base.copy()
    d[1, 1, 8], d[2, 3, 9], d[4, 2, 8], d[3, 3, 7] = np.nan, np.inf, -np.inf, np.nan
    cases["non_finite"] = (d, ones, None, None)
    cases["no_weight"] = (base.copy(), None, None, None)
    w = ones.copy()
    w[rng.random(shape) < 0.4] = 2.0
    w[rng.random(shape) < 0.1] = 0.0
    cases["min_weight_2"] = (base.copy(), w, None, None, 2.0)
    d = base.copy()
    d[2, 1, 8], d[2, 1, 9] = -0.004, 0.003
    cases["one_pair"] = (d, ones, (2, 3, 1, 2, 8, 10), 1)
    d = np.full(shape, np.nan, dtype=np.float32)
    d[2, 2, 4], d[2, 3, 4] = 0.01, -0.02  # a pair without any other observed node: each sees only the other, the normal is -e_y
    d[4, 1, 12], d[5, 1, 12] = -0.01, 0.005  # +e_x, on the grid's last plane
    d[4, 3, 3:7] = (-0.01, 0.02, -0.01, 0.02)  # the middle edge's central differences cancel: the fallback, -e_z
    cases["lonely_pairs"] = (d, ones, None, 5)
    zs = (np.arange(shape[2]) - 15.4) * voxel  # the surface between the planes k = 15 and 16: b in the next tile along z
    d = np.clip(0.8 * zs[None, None, :] + 0.2 * x[:, None, None] + 0.001 * rng.standard_normal(shape), -trunc, trunc).astype(np.float32)
    cases["seam_z"] = (d, ones, None, None)
    out = {}
    for k, v in cases.items():
        d, w, region, n = v[:4]
        out[k] = (d[None], None if w is None else w[None], origin, voxel, trunc, v[4] if len(v) > 4 else 1.0, region, n)
    return out
