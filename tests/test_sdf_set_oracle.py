"""Self-check of the exhaustive tied-set oracle (tests/_sdf_set_oracle.py) on closed forms: the box, the sliver sheet and the
segment faces of tests/test_gpu_parity.py.  The minimum, the tied set T(p), and the closest point and sign of every face in it.
No GPU involved."""
import numpy as np
import pytest

import _sdf_set_oracle as so
from graspqp_amd.utils import meshes

TOL = 2e-7


def _ties(ref, i):
    t = ref["tie_q"] == i
    return ref["tie_f"][t], ref["tie_closest"][t], ref["tie_sign"][t]


def _faces_touching(fv, point):
    return np.flatnonzero((np.abs(fv.astype(np.float64) - point).max(2) < 1e-12).any(1))


def test_box_minimum_ties_closest_points_and_signs():
    fv = meshes.box()
    h = np.array([0.03, 0.04, 0.05], dtype=np.float32).astype(np.float64)  # the mesh is float32
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.normal(size=(400, 3)) * 0.06, rng.uniform(-1, 1, size=(200, 3)) * h * 0.999])
    special = np.array([[0.0, 0.0, 0.1],        # above the middle of the top: both triangles of that side, one closest point
                        [0.06, 0.08, 0.10],     # on the diagonal through a corner: every face at that corner
                        [0.0, 0.0, 0.0],        # the centre: the nearest sides are x = +-0.03, four triangles, inside
                        [0.011, 0.017, 0.2]])   # above the top, off its diagonal: one face
    pts = np.concatenate([special, pts])
    ref = so.exhaustive(pts, fv, TOL)
    q = np.abs(pts) - h
    outside = (q > 0).any(1)
    want = np.where(outside, np.linalg.norm(np.maximum(q, 0), axis=1), -q.max(1))
    np.testing.assert_allclose(np.sqrt(ref["d2_min"]), want, rtol=1e-12, atol=1e-15)
    assert outside[4:].sum() > 100 and (~outside[4:]).sum() > 100
    # every tie: its closest point is at the minimum distance (within tol_d), lies on the box, and its sign is out / in
    d = np.linalg.norm(pts[ref["tie_q"]] - ref["tie_closest"], axis=1)
    assert (d <= np.sqrt(ref["d2_min"])[ref["tie_q"]] + TOL).all() and (d >= np.sqrt(ref["d2_min"])[ref["tie_q"]] - 1e-15).all()
    on = np.abs(np.abs(ref["tie_closest"]) - h)
    assert (on.min(1) < 1e-15).all() and (np.abs(ref["tie_closest"]) <= h + 1e-15).all()
    fn = meshes.face_normals(fv)[ref["tie_f"]]
    # (a face tied through its BORDER may see p from behind: the faces that hold the minimum itself have the box's sign)
    strict = ((np.abs(want)[ref["tie_q"]] > 1e-9) & (np.abs(((pts[ref["tie_q"]] - ref["tie_closest"]) * fn).sum(1)) > 1e-12)
              & (d <= np.sqrt(ref["d2_min"])[ref["tie_q"]] + 1e-15))
    assert np.array_equal(np.unique(ref["tie_q"][strict]), np.arange(len(pts)))
    assert (ref["tie_sign"][strict] == np.where(outside, 1, -1)[ref["tie_q"]][strict]).all()
    assert np.array_equal(np.unique(ref["tie_q"]), np.arange(len(pts)))  # no query without its minimum
    f, c, s = _ties(ref, 0)
    top = np.flatnonzero((fv[:, :, 2] == np.float32(0.05)).all(1))
    assert sorted(f) == sorted(top) and len(f) == 2 and np.allclose(c, [0, 0, h[2]], atol=1e-15) and (s == 1).all()
    f, c, s = _ties(ref, 1)
    assert sorted(f) == sorted(_faces_touching(fv, h)) and 3 <= len(f) <= 6
    assert np.allclose(c, h, atol=1e-15) and (s == 1).all()
    f, c, s = _ties(ref, 2)
    assert sorted(f) == sorted(np.flatnonzero((fv[:, :, 0] == fv[:, :1, 0]).all(1))) and len(f) == 4 and (s == -1).all()
    f, c, s = _ties(ref, 3)
    assert len(f) == 1 and f[0] in top and np.allclose(c[0], [0.011, 0.017, h[2]], atol=1e-15) and s[0] == 1


@pytest.mark.parametrize("width", [4e-4, 2e-6])
def test_sliver_sheet_height_projection_and_face(width):
    fv, rot, shift = so.sliver_sheet(width)
    rng = np.random.default_rng(5)
    N, n, Lx = 600, 32, 0.05
    uv = np.stack([rng.uniform(0.02, 0.98, N) * Lx, rng.uniform(0.02, 0.98, N) * n * width], 1)
    hgt = np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), N)) * rng.choice([-1.0, 1.0], N)
    pts = (np.concatenate([uv, hgt[:, None]], 1) @ rot.T + shift).astype(np.float32).astype(np.float64)
    ref = so.exhaustive(pts, fv, TOL)
    # the sheet's plane through the ROUNDED vertices, in float64 (the rounding to fp32 bends the sheet by ~4e-9)
    loc = (pts - shift) @ rot
    np.testing.assert_allclose(np.sqrt(ref["d2_min"]), np.abs(loc[:, 2]), rtol=1e-6, atol=1e-8)
    assert np.array_equal(np.unique(ref["tie_q"]), np.arange(N))
    big = np.abs(loc[:, 2])[ref["tie_q"]] > 1e-7
    assert (ref["tie_sign"][big] == np.sign(loc[:, 2])[ref["tie_q"]][big]).all()
    foot = (ref["tie_closest"] - shift) @ rot
    # a tied face's closest point lies in the sheet, no farther than the minimum + tol_d: sideways by sqrt((d + tol)^2 - d^2) at most
    dm = np.sqrt(ref["d2_min"])[ref["tie_q"]]
    assert np.abs(foot[:, 2]).max() < 1e-8
    assert (np.linalg.norm(foot[:, :2] - loc[ref["tie_q"], :2], axis=1) <= 1.01 * np.sqrt((dm + TOL) ** 2 - dm ** 2) + 1e-8).all()
    nearest = np.linalg.norm(pts[ref["tie_q"]] - ref["tie_closest"], axis=1) <= dm + 1e-12  # the minimum itself: the projection
    assert nearest.any() and np.abs(foot[nearest, :2] - loc[ref["tie_q"][nearest], :2]).max() < 1e-5
    # the face the projection falls into is in the tied set (ribbon i = faces 2 i, 2 i + 1)
    ribbon = np.floor(loc[:, 1] / width).astype(int)
    has = np.zeros(N, dtype=bool)
    np.logical_or.at(has, ref["tie_q"], ref["tie_f"] // 2 == ribbon[ref["tie_q"]])
    clear = np.abs(loc[:, 1] / width - np.round(loc[:, 1] / width)) > 0.05  # not within rounding of a ribbon's border
    assert has[clear].all() and clear.mean() > 0.8


def test_segment_faces_distance_closest_point_and_sign():
    fv = so.degenerate_faces()
    f64 = fv.astype(np.float64)
    assert so._degenerate(f64).all() and not so._degenerate(meshes.icosphere(2).astype(np.float64)).any()
    rng = np.random.default_rng(9)
    pts = np.concatenate([f64.mean(1)[rng.integers(0, 6, 400)] + rng.normal(size=(400, 3)) * 0.01, rng.normal(size=(200, 3)) * 0.06])
    pts = np.concatenate([f64[1, :1], np.array([[-0.08, 0.0, 0.003]]), pts])  # ON the point face; above a collinear face
    q, d2 = so.per_face(pts, fv)

    def seg(p, u, v):
        d = v - u
        L2 = (d * d).sum()
        t = np.clip(((p - u) @ d) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(p))
        c = u + t[:, None] * d
        return ((p - c) ** 2).sum(1), c

    ends = [(0, 2), (0, 0), (0, 1), (0, 2), (0, 1), (0, 1)]  # the segment every face collapses to, by corner indices
    for k, (i, j) in enumerate(ends):
        w2, wc = seg(pts, f64[k, i], f64[k, j])
        np.testing.assert_allclose(d2[:, k], w2, rtol=1e-12, atol=1e-30)
        np.testing.assert_allclose(q[:, k], wc, rtol=0, atol=1e-15)
    ref = so.exhaustive(pts, fv, TOL)
    np.testing.assert_allclose(ref["d2_min"], d2.min(1), rtol=0, atol=0)
    assert (ref["tie_sign"] == 1).all()  # a zero normal: dot(p - closest, 0) >= 0
    f, c, s = _ties(ref, 0)
    assert list(f) == [1] and ref["d2_min"][0] == 0.0 and np.array_equal(c[0], f64[1, 0])
    f, c, s = _ties(ref, 1)
    assert list(f) == [2] and np.allclose(c[0], [-0.08, 0, 0], atol=1e-9) and abs(ref["d2_min"][1] - 9e-6) < 1e-15
    # in a mesh with regular faces around them the segments still decide their share, and ties hold faces of both kinds
    mixed = np.concatenate([meshes.icosphere(1, 0.03), fv])
    ref2 = so.exhaustive(pts, mixed, TOL)
    reg = so.exhaustive(pts, mixed[:-6], TOL)
    np.testing.assert_allclose(ref2["d2_min"], np.minimum(reg["d2_min"], ref["d2_min"]), rtol=0, atol=0)
    assert 0.2 < (ref["d2_min"] < reg["d2_min"]).mean() < 1.0


def test_judge_accepts_the_oracle_and_refuses_a_neighbouring_face():
    """The rule itself: the oracle's own answer passes; the answer of the second-closest face -- a pruning miss -- does not."""
    fv = meshes.icosphere(2, 0.05)
    rng = np.random.default_rng(3)
    pts = (rng.normal(size=(300, 3)) * 0.05).astype(np.float32)
    atol = so.atol_for(fv, pts)
    big = np.abs(pts).max(1).astype(np.float64)
    assert atol.shape == (300,) and (atol[big <= 0.1] == 2e-7).all() and np.allclose(atol[big > 0.1], 2e-7 * big[big > 0.1] / 0.1, rtol=1e-12, atol=0)
    assert 0.1 < (big > 0.1).mean() < 0.9
    assert so.atol_for(fv + np.float32(0.8), pts * 0.1) == pytest.approx(2e-7 * 8.5, rel=1e-6)
    ref = so.exhaustive(pts, fv, atol)
    q, d2 = so.per_face(pts, fv)
    order = np.argsort(d2, axis=1)
    fn = np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]).astype(np.float64)

    def answer(rank):
        f = order[:, rank]
        c = q[np.arange(len(pts)), f]
        diff = pts - c
        return (d2[np.arange(len(pts)), f], np.where((diff * fn[f]).sum(1) >= 0, 1, -1), diff / np.linalg.norm(diff, axis=1, keepdims=True), c)

    so.judge(ref, pts, *answer(0), atol, "oracle")
    with pytest.raises(AssertionError, match="distance"):
        so.judge(ref, pts, *answer(1), atol, "second face")
    a = answer(0)
    with pytest.raises(AssertionError, match="closest point and sign"):
        so.judge(ref, pts, a[0], -a[1], a[2], a[3], atol, "flipped sign")
    with pytest.raises(AssertionError, match="normal"):
        so.judge(ref, pts, a[0], a[1], -a[2], a[3], atol, "flipped normal")
    nonfinite = np.concatenate([pts, [[np.nan, 0, 0], [np.inf, 0, 0]]]).astype(np.float32)
    ref3 = so.exhaustive(nonfinite, fv, so.atol_for(fv, nonfinite))
    assert np.isnan(ref3["d2_min"][-2:]).all() and ref3["tie_q"].max() == len(pts) - 1
