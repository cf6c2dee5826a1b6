"""Exhaustive fp64 oracle of the mesh distance query, with TIED SETS, and the meshes and queries the cluster-search tests share.
TEST INFRASTRUCTURE (tests/test_sdf_set_oracle.py checks it on closed forms; tests/test_gpu_sdf_cluster_search.py and
tests/test_cluster_bound_host.py use it).

``exhaustive`` runs ``oracle/ref_cpu/sdf.py``'s closest point over ALL faces in float64, chunked, and keeps for every query p
the exact minimum and the tied set T(p) = every face within ``tol_d`` (in distance) of it, each with its own closest point and
sign.  ``judge`` then holds a kernel's answer (dist_sq, sign, normal, closest) of EVERY query against that set -- no share of
the queries is allowed to differ:

  * |sqrt(d2) - sqrt(d2_min)| <= 1e-5 sqrt(d2_min) + atol, atol = 2e-7 max(1, max|coordinate of the mesh and of p| / 0.1): the suite's fp32 contract
    (2e-7 at coordinates of 0.1 m, tests/test_gpu_parity.py) scaled with the coordinates as the fp32 spacing is; tol_d = atol;
  * |p - closest| = sqrt(d2) to the same tolerance;
  * some face of T(p) has its closest point within tol_d + 1e-5 sqrt(d2_min) of the kernel's, and -- where sqrt(d2_min) > 1e-5 --
    the kernel's sign;
  * where sqrt(d2_min) > 1e-4 the normal is within NORMAL_TOL of (p - closest) / |p - closest| formed in float64 from the
    kernel's own outputs (the direction is NOT multiplied by the sign: oracle/ref_cpu/sdf.py and csrc/tri.h, the TorchSDF
    contract).

A face that csrc/tri.h treats as degenerate (gq_make_face: it collapses to a segment) counts as its three edges, sign +1."""
import os
import subprocess
import tempfile

import numpy as np
import torch

from ref_cpu import sdf as osdf

import _host_program

from graspqp_amd.utils import meshes


# ---------------------------------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------------------------------
NORMAL_TOL = 2e-4  # the suite's rule for normals (tests/test_gpu_parity.py, the box hierarchy against the face loop)
# Queries with a coordinate above 0.1 m: the UNPRUNED face loop (torch.ops.graspqp_amd.compute_sdf) misses 2e-4 there.  Measured on
# an MI355X, mesh "translated" (superquadric(5, 48, 24) + (0.5, -0.3, 0.8)), query (0.5661777257919312, -0.30769991874694824,
# 0.7880868315696716), distance 1.1851e-4: error 2.4849e-4, the same for the cluster search (same face, same finish).  The kernel
# forms the normal from the residual in the face's frame; the reference direction is formed from the float32 closest point, whose
# spacing at 0.79 (6e-8) is 5e-4 of that distance.  Twice the measured error; every other mesh of the zoo stays below 1.7e-5.
NORMAL_TOL_ABOVE_0P1 = 2 * 2.4849e-4


def atol_for(fv, pts):
    """Per query (N,): 2e-7 at coordinates up to 0.1 m, growing with the largest coordinate of the mesh and of THAT query (a query
    with a non-finite coordinate: of the mesh alone)."""
    p = np.abs(np.asarray(pts, dtype=np.float64)).max(1)
    big = np.maximum(float(np.abs(np.asarray(fv, dtype=np.float64)).max()), np.where(np.isfinite(p), p, 0.0))
    return 2e-7 * np.maximum(1.0, big / 0.1)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _degenerate(fv):
    """The rule of gq_make_face (csrc/tri.h), in float64."""
    ab, ac = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    L, lc = np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1)
    e1 = np.where((L > 0)[:, None], ab / np.where(L > 0, L, 1.0)[:, None], ac / np.where(lc > 0, lc, 1.0)[:, None])
    cx = (ac * e1).sum(1)
    cy = np.linalg.norm(ac - cx[:, None] * e1, axis=1)
    return ~((L > 0) & (cy > 1e-6 * lc) & (L * cy > 1e-15))


def _segment_closest(p, u, v):
    """p (n,1,3), u, v (1,G,3) -> closest points (n,G,3) of the segments u-v."""
    d = v - u
    L2 = (d * d).sum(-1)
    t = ((p - u) * d).sum(-1) / np.where(L2 > 0, L2, 1.0)
    t = np.where(L2 > 0, np.clip(t, 0.0, 1.0), 0.0)
    return u + t[..., None] * d


def per_face(pts, fv):
    """All pairs: closest point (..,N,F,3) float64 and squared distance (..,N,F) of every query (..,N,3) to every face (..,F,3,3);
    leading dimensions pair the query sets with the meshes.  Small inputs only."""
    p, f = np.asarray(pts, dtype=np.float64), np.asarray(fv, dtype=np.float64)
    if p.ndim > 2:
        deg = _degenerate(f.reshape(-1, 3, 3)).reshape(f.shape[:-2])
        plain = ~deg.any(-1)
        q = np.empty(p.shape[:-1] + (f.shape[-3], 3))
        if plain.any():
            q[plain] = osdf.closest_point_on_triangles(torch.from_numpy(p[plain])[..., :, None, :],
                                                       torch.from_numpy(f[plain])[..., None, :, :, :]).numpy()
        for i in zip(*np.nonzero(~plain)):
            q[i] = per_face(p[i], f[i])[0]
        return q, ((p[..., :, None, :] - q) ** 2).sum(-1)
    q = osdf.closest_point_on_triangles(torch.from_numpy(p)[:, None, :], torch.from_numpy(f)[None]).numpy().copy()
    deg = _degenerate(f)
    if deg.any():
        g = f[deg]
        best, bq = None, None
        for i, j in ((0, 1), (0, 2), (1, 2)):
            c = _segment_closest(p[:, None, :], g[None, :, i], g[None, :, j])
            d2 = ((p[:, None, :] - c) ** 2).sum(-1)
            if best is None:
                best, bq = d2, c
            else:
                m = d2 < best
                best, bq = np.where(m, d2, best), np.where(m[..., None], c, bq)
        q[:, deg] = bq
    d2 = ((p[:, None, :] - q) ** 2).sum(-1)
    return q, d2


def exhaustive(pts, fv, tol_d, pairs=1_500_000):
    """-> dict: d2_min (N,), and the tied sets as parallel arrays over all (query, face) pairs with
    sqrt(d2_f) <= sqrt(d2_min) + tol_d (a number, or one per query):  tie_q (query index, ascending), tie_f (face), tie_closest (.,3), tie_sign (+1 / -1:
    dot(p - closest, face normal) >= 0 -> +1, a degenerate face +1).  Queries with a non-finite coordinate get d2_min = nan and
    no pair.  Chunked over the queries so that a chunk holds at most ``pairs`` (query, face) pairs."""
    p, f = np.asarray(pts, dtype=np.float64), np.asarray(fv, dtype=np.float64)
    N, F = len(p), len(f)
    fn = np.cross(f[:, 1] - f[:, 0], f[:, 2] - f[:, 0])
    fn[_degenerate(f)] = 0.0
    d2_min = np.full(N, np.nan)
    tol_d = np.broadcast_to(np.asarray(tol_d, dtype=np.float64), (N,))
    tq, tf, tc, ts = [], [], [], []
    fin = np.flatnonzero(np.isfinite(p).all(1))
    step = max(1, pairs // max(F, 1))
    for s in range(0, len(fin), step):
        ix = fin[s:s + step]
        q, d2 = per_face(p[ix], f)
        d = np.sqrt(d2)
        dm = d.min(1)
        d2_min[ix] = d2.min(1)
        a, b = np.nonzero(d <= dm[:, None] + tol_d[ix][:, None])
        c = q[a, b]
        tq.append(ix[a]), tf.append(b), tc.append(c)
        ts.append(np.where(((p[ix][a] - c) * fn[b]).sum(1) >= 0, 1, -1))
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)
    return {"d2_min": d2_min, "tie_q": cat(tq, (0,), np.int64), "tie_f": cat(tf, (0,), np.int64),
            "tie_closest": cat(tc, (0, 3), np.float64), "tie_sign": cat(ts, (0,), np.int64), "tol_d": tol_d}


def subset(ref, idx):
    """The oracle's result for the queries ``idx`` (in that order; an index may repeat)."""
    idx = np.asarray(idx, dtype=np.int64)
    order = np.argsort(ref["tie_q"], kind="stable")
    tq = ref["tie_q"][order]
    lo, hi = np.searchsorted(tq, idx, "left"), np.searchsorted(tq, idx, "right")
    take = np.concatenate([order[a:b] for a, b in zip(lo, hi)]) if len(idx) else np.zeros(0, np.int64)
    return {"d2_min": ref["d2_min"][idx], "tie_q": np.repeat(np.arange(len(idx)), hi - lo), "tie_f": ref["tie_f"][take],
            "tie_closest": ref["tie_closest"][take], "tie_sign": ref["tie_sign"][take], "tol_d": ref["tol_d"][idx]}


def judge(ref, pts, d2, sign, normal, closest, atol, tag=""):
    """Every finite query's answer against the rule of the module docstring (``atol``: a number, or one per query); raises with the worst query of the first rule that
    fails (the query, the oracle's faces, the kernel's answer).  ``normal`` None skips the normal rule."""
    p = np.asarray(pts, dtype=np.float64)
    d2, cl = np.asarray(d2, dtype=np.float64), np.asarray(closest, dtype=np.float64)
    sg = np.asarray(sign).astype(np.int64)
    fin = np.isfinite(p).all(1)
    assert np.array_equal(fin, ~np.isnan(ref["d2_min"]))
    dm = np.sqrt(ref["d2_min"])
    tol = 1e-5 * dm + np.broadcast_to(np.asarray(atol, dtype=np.float64), dm.shape)

    def fail(what, err, bad):
        i = int(np.flatnonzero(bad)[np.argmax(np.where(bad, err, -np.inf)[bad])])
        t = ref["tie_q"] == i
        raise AssertionError(
            f"{tag}: {what}: {int(bad.sum())} of {int(fin.sum())} queries; worst: query {i} p = {p[i].tolist()}, error {err[i]:.3e}"
            f" (allowed {tol[i]:.3e}); oracle: distance {dm[i]:.9e}, faces {ref['tie_f'][t].tolist()} signs {ref['tie_sign'][t].tolist()}"
            f" closest {ref['tie_closest'][t][:2].tolist()}; kernel: distance {np.sqrt(d2[i]):.9e} sign {sg[i]} closest {cl[i].tolist()}")

    with np.errstate(invalid="ignore"):
        e1 = np.abs(np.sqrt(d2) - dm)
        bad = fin & ~(e1 <= tol)
        if bad.any():
            fail("distance", e1, bad)
        e2 = np.abs(np.linalg.norm(p - cl, axis=1) - np.sqrt(d2))
        bad = fin & ~(e2 <= tol)
        if bad.any():
            fail("|p - closest| != sqrt(dist_sq)", e2, bad)
        q = ref["tie_q"]
        gap = np.linalg.norm(ref["tie_closest"] - cl[q], axis=1)
        ok_pair = (gap <= ref["tol_d"][q] + 1e-5 * dm[q]) & ((dm[q] <= 1e-5) | (ref["tie_sign"] == sg[q]))
        ok = np.zeros(len(p), dtype=bool)
        np.logical_or.at(ok, q, ok_pair)
        bad = fin & ~ok
        if bad.any():
            best = np.full(len(p), np.inf)
            np.minimum.at(best, q, gap)
            fail("no tied face has the kernel's closest point and sign", best, bad)
        if normal is not None:
            diff = p - cl
            want = diff / np.linalg.norm(diff, axis=1, keepdims=True)
            e4 = np.abs(np.asarray(normal, dtype=np.float64) - want).max(1)
            tol = np.where(np.abs(p).max(1) > 0.1, NORMAL_TOL_ABOVE_0P1, NORMAL_TOL)
            bad = fin & (dm > 1e-4) & ~(e4 <= tol)
            if bad.any():
                fail("normal", e4, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the clusters of a mesh, from the host build of csrc/cluster_bound.h
# ---------------------------------------------------------------------------------------------------------------------------
class ClusterTool:
    """tests/cluster_bound_host.cpp built once into a directory of its own (``sanitize``: with AddressSanitizer and UBSan, as a
    stand-alone program).  A failure of the program -- a sanitizer report included -- raises."""

    def __init__(self, workdir=None, sanitize=False):
        self._tmp = None
        if workdir is None:
            self._tmp = tempfile.TemporaryDirectory(prefix="gq_cluster_bound_")
            workdir = self._tmp.name
        self.dir = str(workdir)
        self.exe = _host_program.build("cluster_bound_host", self.dir, sanitize=sanitize)

    def _run(self, mode, blob):
        a, b = os.path.join(self.dir, "in.bin"), os.path.join(self.dir, "out.bin")
        with open(a, "wb") as f:
            f.write(blob)
        subprocess.check_call([self.exe, mode, a, b])
        return np.fromfile(b, dtype=np.float32)

    def clusters(self, fv):
        """-> (perm (F,) position -> face, boxes (n_clusters,16) float32): cluster k holds the faces perm[64 k : 64 k + 64]."""
        fv = np.ascontiguousarray(fv, dtype=np.float32).reshape(-1, 3, 3)
        F = len(fv)
        raw = self._run("bound", np.int32(F).tobytes() + fv.tobytes())
        nC = int(raw[:1].view(np.int32)[0])
        assert nC == (F + 63) // 64 and raw.size == 1 + F + 16 * nC
        perm = raw[1:1 + F].view(np.int32).astype(np.int64)
        assert np.array_equal(np.sort(perm), np.arange(F))
        return perm, raw[1 + F:].reshape(nC, 16).copy()

    def lower_bounds(self, boxes, pts):
        """boxes (C,16), pts (C,P,3) float32 -> (C,P) float32: 0.9999f * gq_cluster_lb, the number the search compares."""
        boxes, pts = np.ascontiguousarray(boxes, dtype=np.float32), np.ascontiguousarray(pts, dtype=np.float32)
        C, P = pts.shape[:2]
        raw = self._run("lb", np.array([C, P], dtype=np.int32).tobytes() + boxes.tobytes() + pts.tobytes())
        assert raw.size == C * P
        return raw.reshape(C, P)


def box_points(boxes):
    """Centre and eight corners of every oriented cluster box -> (C,9,3) float64."""
    b = np.asarray(boxes, dtype=np.float64)
    ctr, ax, h = b[:, 0:3], np.stack([b[:, 4:7], b[:, 8:11], b[:, 12:15]], 1), b[:, [3, 7, 11]]
    s = np.array([[0, 0, 0]] + [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    return ctr[:, None, :] + np.einsum("sk,ck,ckj->csj", s, h, ax)


# ---------------------------------------------------------------------------------------------------------------------------
# the mesh zoo
# ---------------------------------------------------------------------------------------------------------------------------
def sliver_sheet(width, n=32, Lx=0.05, seed=5):
    """The ribbon sheet of tests/test_gpu_parity.py::test_sdf_sliver_faces_...: 2 n needle triangles, Lx long and ``width`` wide,
    in a general orientation -> (faces (2n,3,3) float32, rotation (3,3), shift (3,)): local (x, y, h) -> world x q^T + shift."""
    rng = np.random.default_rng(seed)
    tris = []
    for i in range(n):
        y0, y1 = i * width, (i + 1) * width
        tris += [[(0, y0, 0), (Lx, y0, 0), (Lx, y1, 0)], [(0, y0, 0), (Lx, y1, 0), (0, y1, 0)]]
    fv = np.array(tris, dtype=np.float64)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    shift = np.array([0.013, -0.021, 0.008])
    return (fv @ q.T + shift).astype(np.float32), q, shift


def degenerate_faces():
    """The six zero-area faces of tests/test_gpu_parity.py::test_sdf_degenerate_faces_... -> (6,3,3) float32."""
    P = lambda *v: np.array(v, dtype=np.float64)
    a, b, c = P(0.06, 0.0, 0.0), P(0.09, 0.01, 0.0), P(0.06, 0.03, 0.02)
    return np.stack([
        np.stack([a, a, c]),                                  # a == b: the segment a-c
        np.stack([b, b, b]),                                  # a point
        np.stack([P(-0.06, 0, 0), P(-0.10, 0, 0), P(-0.08, 0, 0)]),      # collinear, c between a and b
        np.stack([P(0, 0.06, 0), P(0, 0.08, 0), P(0, 0.11, 0)]),         # collinear, c beyond b
        np.stack([P(0, -0.06, 0.01), P(0.02, -0.08, 0), P(0.02, -0.08, 0)]),   # b == c
        np.stack([P(0, 0, 0.07), P(0.01, 0.02, 0.09), P(0, 0, 0.07)]),         # a == c
    ]).astype(np.float32)


def _soup(n=2048, edge=0.005, cube=0.10, seed=17):
    rng = np.random.default_rng(seed)
    tri = edge * np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.75 ** 0.5, 0]]) - edge * np.array([0.5, 0.75 ** 0.5 / 3, 0])
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.linalg.det(q))[:, None, None]
    ctr = rng.uniform(-cube / 2, cube / 2, size=(n, 1, 3))
    return (np.einsum("vk,njk->nvj", tri, q) + ctr).astype(np.float32)


def _shell():
    a = meshes.icosphere(3, 0.05).astype(np.float64)
    b = (0.98 * a)[:, [0, 2, 1]]
    out = np.empty((2 * len(a), 3, 3))
    out[0::2], out[1::2] = a, b
    return out.astype(np.float32)


_ZOO = {
    "sphere5": lambda: meshes.icosphere(5),                                   # 20480 faces, 320 clusters: the second pass of 256
    "superquadric": lambda: meshes.superquadric(5, 48, 24),
    "box": lambda: meshes.box(),                                              # 12 faces
    "triangle": lambda: meshes.icosphere(2)[:1],
    "open63": lambda: meshes.icosphere(2)[:63],
    "open64": lambda: meshes.icosphere(2)[:64],
    "open65": lambda: meshes.icosphere(2)[:65],
    "open127": lambda: meshes.icosphere(2)[:127],
    "shell": _shell,                                                          # two sheets, interleaved: cluster normals cancel
    "soup": _soup,                                                            # Morton patches that are not planar
    "translated": lambda: (meshes.superquadric(5, 48, 24).astype(np.float64) + np.array([0.5, -0.3, 0.8])).astype(np.float32),
    "flat": lambda: (meshes.superquadric(5, 48, 24).astype(np.float64) * np.array([1.0, 0.05, 1.0])).astype(np.float32),
    "millimetre": lambda: (lambda f: (f * (1e-3 / (f.reshape(-1, 3).max(0) - f.reshape(-1, 3).min(0)).max())).astype(np.float32))(
        meshes.superquadric(5, 48, 24).astype(np.float64)),
    "degenerate_sliver": lambda: np.concatenate([meshes.icosphere(3), degenerate_faces(), sliver_sheet(2e-6)[0]]),
}
ZOO = tuple(_ZOO)
_MADE = {}


def mesh(name):
    """(F,3,3) float32, C-contiguous; the same array on every call (do not modify)."""
    if name not in _MADE:
        _MADE[name] = np.ascontiguousarray(_ZOO[name](), dtype=np.float32)
        _MADE[name].setflags(write=False)
    return _MADE[name]


def queries(fv, boxes, seed=0, n_far=(250, 150), n_near=400, n_vert=150, n_hair=200, n_box=350):
    """Finite queries of one mesh, float32: far field at 4 x and 20 x the extent, near and inside at 0.7 x, exactly on vertices,
    a hair (1e-4 x the extent) off face centres, and centres and corners of the mesh's own cluster boxes (at most ``n_box`` of
    them, drawn at random).  Extent = the largest distance of a vertex coordinate from the centre of the bounding box."""
    rng = np.random.default_rng(seed)
    v = np.asarray(fv, dtype=np.float64).reshape(-1, 3)
    ctr = 0.5 * (v.min(0) + v.max(0))
    ext = float(np.abs(v - ctr).max())
    bp = box_points(boxes).reshape(-1, 3)
    if len(bp) > n_box:
        bp = bp[rng.choice(len(bp), n_box, replace=False)]
    fc = np.asarray(fv, dtype=np.float64).mean(1)
    return np.concatenate([
        ctr + rng.normal(size=(n_far[0], 3)) * ext * 4.0,
        ctr + rng.normal(size=(n_far[1], 3)) * ext * 20.0,
        ctr + rng.normal(size=(n_near, 3)) * ext * 0.7,
        v[rng.integers(0, len(v), n_vert)],
        fc[rng.integers(0, len(fc), n_hair)] + rng.normal(size=(n_hair, 3)) * 1e-4 * ext,
        bp,
    ]).astype(np.float32)
