"""The device body of the TSDF integration (csrc/tsdf_dev.h: one node through every view, on top of clutter_dev.h's pose chain)
compiled for the HOST with AddressSanitizer and UBSan, run as a program of its own and compared with the fp64 oracle
(tests/_tsdf_oracle.py) under the bounds and conditions of the GPU test: the weight exactly and D at rtol 1e-5 / atol 1e-6 on the
non-ambiguous nodes.  Every image, label and grid buffer is an allocation of exactly its size, so a pixel or node read outside
it, or a float -> int conversion of an out-of-range value, ends the program with a non-zero status.  No GPU involved."""
import subprocess

import numpy as np
import pytest

import _host_program
import _tsdf_oracle as to

EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)  # a camera at the origin looking along +z of the world


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    d = tmp_path_factory.mktemp("tsdf_body")
    exe = _host_program.build("tsdf_body_host", d)

    def run(vol, depth, labels, cam_T, intrinsics, depth_range, trunc, max_weight=64.0, target_T=None, skip=None):
        """The arguments of to.integrate; ``vol`` is the state BEFORE the call and is left alone.  -> (D, W) float32.  A sanitizer
        report or any other failure of the program raises (check_call)."""
        out = vol.out
        depth = np.asarray(depth, dtype=np.float32)
        depth = depth[None] if depth.ndim == 2 else depth
        V, H, W = depth.shape
        f4, i4 = (lambda a: np.asarray(a, dtype=np.float32).tobytes()), (lambda a: np.asarray(a, dtype=np.int32).tobytes())
        with open(d / "in.bin", "wb") as f:
            f.write(i4((out.n_grids,) + out.shape) + f4(list(out.origin) + [out.voxel]))
            f.write(i4([target_T is not None, skip is not None, labels is not None]) + i4([V, H, W]))
            f.write(f4(list(intrinsics) + list(depth_range) + [trunc, max_weight]))
            if target_T is not None:
                f.write(f4(target_T))
            if skip is not None:
                f.write(i4(skip))
            f.write(f4(cam_T) + f4(depth))
            if labels is not None:
                f.write(i4(labels))
            f.write(f4(vol.D) + f4(vol.W))
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])  # a sanitizer report is a non-zero exit
        raw = np.fromfile(d / "out.bin", dtype=np.float32)
        n = vol.D.size
        assert raw.size == 2 * n
        return raw[:n].reshape(vol.D.shape), raw[n:].reshape(vol.D.shape)

    return run


def _both(body, vol, *args, **kw):
    """The host body and the oracle on the same prior state -> (got_D, got_W, the oracle's volume, its info)."""
    got_D, got_W = body(vol, *args, **kw)
    ref = vol.copy()
    info = to.integrate(ref, *args, **kw)
    return got_D, got_W, ref, info


def _bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


@pytest.mark.parametrize("name", ["A", "B"])
def test_body_matches_the_oracle_on_the_gpu_layouts(body, name):
    vol, tT, skip, n = to.layout(name)
    cam, depth, labels = to.cameras(n)
    got_D, got_W, ref, info = _both(body, vol, depth, labels, cam, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, skip)
    to.assert_parity(got_D, got_W, ref, info, f"layout {name}")
    # V views in one pass are V passes of one view, bit for bit
    step = vol
    for v in range(n):
        D1, W1 = body(step, depth[v], labels[v], cam[v:v + 1], to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, skip)
        step = vol.copy()
        step.D, step.W = D1.astype(np.float64), W1.astype(np.float64)
    assert _bits(D1, got_D) and _bits(W1, got_W)
    if name == "B":  # grid 0 takes the sphere's rays as free: it differs from the same grid without a skipped label
        plain_D, _ = body(vol, depth, labels, cam, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, None)
        assert not _bits(plain_D[0], got_D[0]) and _bits(plain_D[1:], got_D[1:])


def test_nodes_behind_the_camera_at_z_zero_and_just_under_depth_min(body):
    """Camera at the origin looking along +z; node planes at z = (k - 2) / 128 exactly (k = 2 is z = 0), depth_min one ulp above the
    plane k = 6: planes 0..6 are skipped before any division, planes 7.. are free space in front of a wall at 1 m."""
    h = 1.0 / 128
    vol = to.Volume(1, (2, 2, 10), (-h, -h, -2 * h), h, -0.02)
    dmin = float(np.nextafter(np.float32(4 * h), np.float32(1)))
    depth = np.full((1, 3, 3), 1.0, dtype=np.float32)
    got_D, got_W, ref, info = _both(body, vol, depth, None, EYE[None], (1.0, 1.0, 1.0, 1.0), (dmin, 2.0), 0.02)
    assert info["ambiguous"][..., 6].all() and not info["ambiguous"][..., 7:].any()  # the oracle's guard sees the plane one ulp under
    assert (got_W[..., :7] == 0).all() and _bits(got_D[..., :7], np.float32(-0.02) * np.ones((1, 2, 2, 7), dtype=np.float32))
    assert (got_W[..., 7:] == 1).all() and (got_D[..., 7:] == np.float32(0.02)).all()
    to.assert_parity(got_D, got_W, ref, info, "z range", caps=False)


@pytest.mark.parametrize("fx", [1e30, 3e38])
def test_nodes_projecting_far_outside_the_image(body, fx):
    """x in {-0.1, 0, 0.1}, z in {0.05, 0.15}: with fx = 3e38, u is -inf, cx or +inf on the near plane and +-2e38 on the far one;
    with fx = 1e30 it is +-2e30 / +-6.7e29.  Only the nodes on the optical axis are in the image."""
    vol = to.Volume(1, (3, 3, 2), (-0.1, -0.1, 0.05), 0.1, -0.02)
    assert float(np.float32(0.1) * 1 + np.float32(-0.1)) == 0.0
    depth = np.full((1, 5, 4), 1.0, dtype=np.float32)
    got_D, got_W = body(vol, depth, None, EYE[None], (fx, fx, 1.0, 2.0), (0.01, 2.0), 0.02)
    want = np.zeros((1, 3, 3, 2), dtype=np.float32)
    want[0, 1, 1, :] = 1
    assert np.array_equal(got_W, want)
    assert (got_D[want == 1] == np.float32(0.02)).all() and _bits(got_D[want == 0], np.full(16, -0.02, dtype=np.float32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 3e38])
def test_non_finite_and_huge_poses(body, bad):
    """A camera pose or a target pose with a NaN / +-inf entry: the node is NaN and its weight is what it was before that view.
    3e38 stays finite or overflows along the chain: the node is untouched or NaN, its weight unchanged either way."""
    vol, tT, skip, n = to.layout("B")
    cam, depth, labels = to.cameras(2)
    args = (to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0)
    good_D, good_W = body(vol, depth[0], labels[0], cam[:1], *args, tT, skip)
    assert (good_W == 1).mean() > 0.5
    # the second view's pose is bad: the first view's weight stands
    cam_bad = cam.copy()
    cam_bad[1, 1, 3] = bad
    got_D, got_W = body(vol, depth, labels, cam_bad, *args, tT, skip)
    assert _bits(got_W, good_W)
    if np.isfinite(bad):
        assert (np.isnan(got_D) | (got_D.view(np.int32) == good_D.view(np.int32))).all()
    else:
        assert np.isnan(got_D).all()
    # the pose of grid 1 is bad: its nodes are NaN with the weight they came with, the other grids do not notice
    start = vol.copy()
    start.W[:] = 3.0
    ok_D, ok_W = body(start, depth, labels, cam, *args, tT, skip)
    tT_bad = tT.copy()
    tT_bad[1, 2, 3] = bad
    got_D, got_W = body(start, depth, labels, cam, *args, tT_bad, skip)
    assert _bits(got_D[[0, 2]], ok_D[[0, 2]]) and _bits(got_W[[0, 2]], ok_W[[0, 2]]) and (ok_W[[0, 2]] > 3).any()
    assert (got_W[1] == 3).all()
    if np.isfinite(bad):
        assert (np.isnan(got_D[1]) | (got_D[1] == np.float32(-to.TRUNC))).all()
    else:
        assert np.isnan(got_D[1]).all()
        ref = start.copy()
        info = to.integrate(ref, depth, labels, cam, *args, tT_bad, skip)
        assert np.isnan(ref.D[1]).all() and (ref.W[1] == 3).all()
        to.assert_parity(got_D, got_W, ref, info, f"target pose {bad}", caps=False)


def test_pixels_that_are_no_measurement(body):
    """Node column (i,j) projects to pixel (col i, row j) of a 3 x 3 image holding 0, a negative depth, NaN, +inf, a depth beyond
    depth_max, one below depth_min and three measurements: only those three columns change."""
    nan, inf = float("nan"), float("inf")
    depth = np.array([[[0.0, -1.0, nan], [inf, 1.005, 1.005], [3.0, 0.04, 1.005]]], dtype=np.float32)
    vol = to.Volume(1, (3, 3, 2), (-0.01, -0.01, 1.0), 0.01, -0.02)
    got_D, got_W, ref, info = _both(body, vol, depth, None, EYE[None], (100.0, 100.0, 1.0, 1.0), (0.05, 2.0), 0.02)
    assert not info["ambiguous"].any()
    want = np.isin(depth[0].T, np.float32(1.005))  # [i][j] = pixel (row j, col i)
    assert int(want.sum()) == 3 and np.array_equal(got_W[0] == 1, np.repeat(want[:, :, None], 2, 2)) and (got_W[0][~want] == 0).all()
    assert _bits(got_D[0][~want], np.full((6, 2), -0.02, dtype=np.float32))
    to.assert_parity(got_D, got_W, ref, info, "pixels", caps=False)
    assert np.allclose(got_D[0][want], [0.005, -0.005], atol=1e-6)


def test_a_one_by_one_image(body):
    vol, _, _, _ = to.layout("A")
    K = (3.0, 3.0, 0.0, 0.0)  # the one pixel spans +-1/6 in x / z
    cam = to.look_at(to.EYES[3], to.LOOK, up=(0.0, 1.0, 0.0))
    depth, labels = to.render(cam, K, 1, 1, to.PLANE_Z, to.SPHERE)
    assert depth.shape == (1, 1) and labels[0, 0] == 1
    got_D, got_W, ref, info = _both(body, vol, depth, labels, cam[None], K, to.DEPTH_RANGE, to.TRUNC)
    assert 0.2 < info["updated"].mean() < 1.0
    to.assert_parity(got_D, got_W, ref, info, "1 x 1", caps=False)


def test_a_full_weight_stays_and_the_distance_still_moves(body):
    vol, _, _, n = to.layout("A")
    cam, depth, labels = to.cameras(n)
    vol.D[:], vol.W[:] = 0.01, 4.0
    got_D, got_W, ref, info = _both(body, vol, depth, labels, cam, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 4.0)
    assert (got_W == 4).all()
    moved = info["updated"] & ~info["ambiguous"] & (np.abs(ref.D - 0.01) > 1e-4)
    assert moved.mean() > 0.5 and (np.abs(got_D[moved] - np.float32(0.01)) > 5e-5).all()
    to.assert_parity(got_D, got_W, ref, info, "full weight")


def test_the_smallest_grid(body):
    vol = to.Volume(1, (2, 2, 2), (0.0, -0.01, 0.06), 0.01, -to.TRUNC)  # about the sphere's top
    cam, depth, labels = to.cameras(3)
    got_D, got_W, ref, info = _both(body, vol, depth, labels, cam, to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC)
    assert info["updated"].all() and not info["ambiguous"].any()
    to.assert_parity(got_D, got_W, ref, info, "(2,2,2)", caps=False)
