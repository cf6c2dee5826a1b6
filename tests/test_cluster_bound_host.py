"""The bound of the pruned cluster search (csrc/cluster_bound.h), compiled for the HOST with AddressSanitizer and UBSan and run as
a program of its own (tests/cluster_bound_host.cpp): for every 64-face cluster of every mesh of the zoo, and for more than 2000
points per cluster -- far, near, on the cluster's vertices, a hair off its faces, on the faces and corners of its box -- the number
the search compares, 0.9999f * lb_fp32(p), must not exceed the exact fp64 squared distance from p to the cluster's faces.  Nothing
is added: the `pad` of gq_cluster_bound and the factor 0.9999 are all the slack the design claims to need.  A box that is too
tight lets the search skip the cluster that holds the closest face.  No GPU involved."""
import numpy as np
import pytest

import _sdf_set_oracle as so

N_POINTS = 2032


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return so.ClusterTool(tmp_path_factory.mktemp("cluster_bound"), sanitize=True)


def _special(name):
    rng = np.random.default_rng(23)
    tri = np.array([[0.01, 0.02, 0.03], [0.015, 0.021, 0.03], [0.012, 0.027, 0.034]])
    if name == "identical":          # all 64 faces identical
        fv = np.repeat(tri[None], 64, 0)
    elif name == "zero_area":        # every face a segment or a point
        a, b = rng.uniform(-0.02, 0.02, size=(2, 64, 3))
        fv = np.stack([a, a, b], 1)
        fv[::8] = a[::8, None, :]
    elif name == "one_point":        # all vertices one point
        fv = np.tile(tri[0], (64, 3, 1))
    elif name == "cancelling":       # every face twice, once per winding, side by side: the summed normal is exactly zero
        half = so.mesh("open64")[:32].astype(np.float64)
        fv = np.empty((64, 3, 3))
        fv[0::2], fv[1::2] = half, half[:, [0, 2, 1]]
    else:                            # coordinates near 10 m
        assert name == "near_10m"
        fv = so.mesh("superquadric")[:64].astype(np.float64) + np.array([10.0, -9.0, 8.0])
    return np.ascontiguousarray(fv, dtype=np.float32)


SPECIAL = ("identical", "zero_area", "one_point", "cancelling", "near_10m")


def _points(fv, perm, boxes, seed):
    """(C, N_POINTS, 3) float32 and the clusters' faces (C,64,3,3) float64 (a partial cluster repeats its first face)."""
    rng = np.random.default_rng(seed)
    f64 = fv.astype(np.float64)
    C = len(boxes)
    v = f64.reshape(-1, 3)
    ext = max(float(np.abs(v - 0.5 * (v.min(0) + v.max(0))).max()), 1e-6)
    faces = np.empty((C, 64, 3, 3))
    pts = np.empty((C, N_POINTS, 3))
    b = boxes.astype(np.float64)
    ctr, ax, h = b[:, 0:3], np.stack([b[:, 4:7], b[:, 8:11], b[:, 12:15]], 1), b[:, [3, 7, 11]]
    corners = so.box_points(boxes)[:, 1:]
    for c in range(C):
        ids = perm[64 * c:64 * c + 64]
        faces[c] = f64[np.r_[ids, np.full(64 - len(ids), ids[0])]]
        cv = faces[c].reshape(-1, 3)
        rad = max(float(np.abs(cv - ctr[c]).max()), 1e-7)
        on_box = rng.uniform(-1, 1, size=(500, 3))
        k = rng.integers(0, 3, 500)
        on_box[np.arange(500), k] = rng.choice([-1.0, 1.0], 500)                   # on one of the six faces of the box
        on_box[250:] *= 1.0 + np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), (250, 1)))  # and from a hair to 1 % outside it
        fc = faces[c].mean(1)
        pts[c] = np.concatenate([
            ctr[c] + rng.normal(size=(250, 3)) * ext * 4.0,                       # far field
            ctr[c] + rng.normal(size=(150, 3)) * ext * 20.0,
            ctr[c] + rng.normal(size=(500, 3)) * rad * np.exp(rng.uniform(np.log(0.3), np.log(3.0), (500, 1))),  # near
            cv[rng.integers(0, len(cv), 300)],                                    # on the cluster's vertices
            fc[rng.integers(0, 64, 300)] + rng.normal(size=(300, 3)) * 1e-4 * ext,  # a hair off its faces
            ctr[c] + (on_box * h[c]) @ ax[c],
            ctr[c] + np.concatenate([(corners[c] - ctr[c]) * s for s in (1.0, 1.0 + 1e-6, 1.0 + 1e-4, 2.0)]),
        ])
    return pts.astype(np.float32), faces


def _check(tool, fv, seed):
    perm, boxes = tool.clusters(fv)
    assert np.isfinite(boxes).all() and (boxes[:, [3, 7, 11]] > 0).all() and (boxes[:, 15] == 0).all()
    axes = boxes[:, [4, 5, 6, 8, 9, 10, 12, 13, 14]].astype(np.float64).reshape(-1, 3, 3)
    np.testing.assert_allclose(axes @ axes.transpose(0, 2, 1), np.broadcast_to(np.eye(3), axes.shape), atol=1e-6)
    pts, faces = _points(fv, perm, boxes, seed)
    lb = tool.lower_bounds(boxes, pts).astype(np.float64)
    assert np.isfinite(lb).all() and (lb >= 0).all()
    exact = np.empty_like(lb)
    for s in range(0, len(boxes), 8):
        exact[s:s + 8] = so.per_face(pts[s:s + 8].astype(np.float64), faces[s:s + 8])[1].min(-1)
    over = lb > exact  # NO slack
    if over.any():
        c, i = np.unravel_index(np.argmax(np.where(over, lb - exact, -np.inf)), lb.shape)
        raise AssertionError(f"{int(over.sum())} of {lb.size} bounds exceed the exact distance; worst: cluster {c} (faces "
                             f"{perm[64 * c:64 * c + 64][:4].tolist()}...), p = {pts[c, i].tolist()}: 0.9999 lb = {lb[c, i]:.9e} > d2 = "
                             f"{exact[c, i]:.9e}; box = {boxes[c].tolist()}")
    return lb, exact


@pytest.mark.parametrize("name", so.ZOO)
def test_lower_bound_never_exceeds_the_exact_distance(tool, name):
    fv = so.mesh(name)
    lb, exact = _check(tool, fv, 100 + so.ZOO.index(name))
    assert lb.shape == ((len(fv) + 63) // 64, N_POINTS)
    # the bound is a bound, not zero: far away (the first 400 points of a cluster) it is positive
    assert (lb[:, :400] > 0).mean() > 0.99
    if name in ("sphere5", "superquadric", "translated"):  # and for a nearly planar patch it is tight there
        assert np.median(lb[:, :400] / exact[:, :400]) > 0.9


@pytest.mark.parametrize("name", SPECIAL)
def test_lower_bound_on_degenerate_clusters(tool, name):
    fv = _special(name)
    assert fv.shape == (64, 3, 3)
    lb, exact = _check(tool, fv, 7)
    assert lb.shape == (1, N_POINTS) and (lb[:, :400] > 0).mean() > 0.99


def test_clusters_are_the_morton_runs_of_64(tool):
    """What the program reports is the clustering the search sees: every cluster's vertices lie inside its box (in float64, up to
    the rounding of the stored centre), partial last clusters included."""
    for name in ("open63", "open65", "open127", "soup", "sphere5"):
        fv = so.mesh(name)
        perm, boxes = tool.clusters(fv)
        b = boxes.astype(np.float64)
        for c in range(len(boxes)):
            v = fv[perm[64 * c:64 * c + 64]].astype(np.float64).reshape(-1, 3) - b[c, 0:3]
            for k, o in enumerate((4, 8, 12)):
                assert (np.abs(v @ b[c, o:o + 3]) <= b[c, 3 + 4 * k] + 1e-7 * np.abs(fv).max()).all(), (name, c, k)
