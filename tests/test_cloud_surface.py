"""CPU-side checks of the point-cloud objects (surfel signed distance): C ABI, argument validation, the registered op, the
default radius, the ObjectModel entry and the code-object metadata of the new kernel.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name in ("gq_cloudset_create", "gq_cloudset_destroy", "gq_cloud_forward", "gq_cloud_check"):
        assert name in protos, name
        assert hasattr(lib, name), name
    assert len(protos["gq_cloud_check"][1]) == 5 and len(protos["gq_cloudset_create"][1]) == 6
    assert len(protos["gq_cloud_forward"][1]) == 9 == len(protos["gq_sdf_forward_meshset"][1])
    src = open(_C.HEADER_PATH).read()
    doc = src[src.index("oriented point clouds"):src.index("gq_cloud_check(")]
    for word in ("ties to the smallest index", "closest = p_j + lat min(1, rho / l)", "sign = +1 if h >= 0", "gq_sdf_backward"):
        assert word in doc, word


def _check(n_obj, sizes, radii, n_points, qpo):
    off = np.zeros(len(sizes) + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    rad = np.asarray(radii, dtype=np.float32)
    lib = _C.lib()
    rc = lib.gq_cloud_check(n_obj, off.ctypes.data_as(ctypes.c_void_p), rad.ctypes.data_as(ctypes.c_void_p), n_points, qpo)
    return rc, lib.gq_last_error()


@pytest.mark.parametrize("args,word", [
    ((2, [5, 0], [0.01, 0.01], 8, 4), b"N = 0"),                      # an empty cloud
    ((0, [], [], 0, 4), b"n_obj"),
    ((2, [5, 7], [0.01, 0.0], 8, 4), b"rho"),
    ((2, [5, 7], [0.01, -1.0], 8, 4), b"rho"),
    ((2, [5, 7], [float("nan"), 0.01], 8, 4), b"rho"),
    ((2, [5, 7], [0.01, 0.01], 8, 0), b"queries_per_object"),
    ((2, [5, 7], [0.01, 0.01], 8, -4), b"queries_per_object"),
    ((2, [5, 7], [0.01, 0.01], 9, 4), b"n_points"),
    ((1, [(1 << 20) + 1], [0.01], 4, 4), b"2^20"),
])
def test_check_rejects_bad_arguments_with_a_message(args, word):
    assert _check(2, [5, 7], [0.01, 0.02], 8, 4)[0] == 0
    assert _check(1, [1 << 20], [0.01], 3, 3)[0] == 0
    rc, msg = _check(*args)
    assert rc != 0
    assert b"cloud" in msg and word in msg, msg


def test_create_refuses_bad_clouds_before_touching_the_device():
    """Zero / non-finite normals, non-finite points and bad radii return the argument-error status with the validation's own
    message and no handle: nothing has touched a device by then (a HIP failure would carry another status)."""
    lib = _C.lib()
    off = np.array([0, 3], dtype=np.int32)
    rad = np.array([0.01], dtype=np.float32)
    pts = np.arange(9, dtype=np.float32).reshape(3, 3)
    nrm = np.tile(np.array([[0.0, 0.0, 2.0]], dtype=np.float32), (3, 1))
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def create(p, n, r):
        h = ctypes.c_void_p(0)
        rc = lib.gq_cloudset_create(vp(p), vp(n), vp(off), vp(r), 1, ctypes.byref(h))
        return rc, lib.gq_last_error(), h

    for bad_n, word in ((np.zeros_like(nrm), b"normal"), (np.where(np.eye(3) > 0, np.nan, nrm).astype(np.float32), b"normal"),
                        (np.full_like(nrm, np.inf), b"normal")):
        rc, msg, h = create(pts, bad_n, rad)
        assert rc == 2 and word in msg and not h.value, (rc, msg)
    bad_p = pts.copy()
    bad_p[1, 2] = np.inf
    rc, msg, h = create(bad_p, nrm, rad)
    assert rc == 2 and b"point" in msg and not h.value
    rc, msg, h = create(pts, nrm, np.array([0.0], dtype=np.float32))
    assert rc == 2 and b"rho" in msg and not h.value


def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "sdf_cloud") and hasattr(ops, "PointCloudSet") and hasattr(ops._Eager, "sdf_cloud")
    N = 70
    with FakeTensorMode():
        d2, sg, nrm, cls = ns.sdf_cloud(torch.empty(N, 3, device="cuda"), 1, 35)
        assert d2.shape == (N,) and d2.dtype == torch.float32
        assert sg.shape == (N,) and sg.dtype == torch.int32
        assert nrm.shape == (N, 3) and cls.shape == (N, 3)
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.sdf_cloud(torch.zeros(N, 3), 1, 35)


def test_default_radius_is_twice_the_median_neighbour_distance():
    from scipy.spatial import cKDTree

    from graspqp_amd.utils import meshes

    p = np.random.default_rng(7).normal(size=(500, 3)).astype(np.float32) * 0.03
    d, _ = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=2)
    assert meshes.cloud_radius(p) == 2.0 * float(np.median(d[:, 1]))
    with pytest.raises(ValueError, match="radius"):
        meshes.cloud_radius(p[:1])


def test_mesh_to_cloud_is_seeded_and_oriented():
    from graspqp_amd.utils import meshes

    fv = meshes.box()
    p, n = meshes.mesh_to_cloud(fv, 300, seed=9)
    p2, n2 = meshes.mesh_to_cloud(fv, 300, seed=9)
    assert p.dtype == np.float32 and n.dtype == np.float32 and p.shape == (300, 3) and n.shape == (300, 3)
    assert np.array_equal(p, p2) and np.array_equal(n, n2)
    assert np.array_equal(p, meshes.sample_surface(fv, 300, seed=9).astype(np.float32))
    half = np.array([0.03, 0.04, 0.05])
    axis = np.abs(n).argmax(1)  # on a box about the origin: the normal of a sample is the outward axis of its face
    assert np.allclose(np.abs(n).max(1), 1.0) and np.allclose(np.take_along_axis(p * n, axis[:, None], 1)[:, 0], half[axis], atol=1e-6)


def test_object_model_refuses_a_cloud_smaller_than_num_samples():
    from graspqp_amd.core.object_model import ObjectModel

    om = ObjectModel(batch_size_each=2, num_samples=100)
    p = np.random.default_rng(1).normal(size=(60, 3)).astype(np.float32)
    with pytest.raises(ValueError, match=r"60 .*100"):
        om.initialize_from_point_clouds([p], [p])


def test_new_kernel_resources():
    """The query kernel: no scratch, and within the 64-register step (8 wavefronts per SIMD) it was built at -- the library has
    it at 64 VGPRs with four point records in flight per lane."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "cloud" in k}
    assert sorted(new) == ["gq_cloud_wave_kernel"], sorted(new)
    r = new["gq_cloud_wave_kernel"]
    assert r["scratch"] == 0 and r["lds_static"] == 0, r
    assert r["vgpr"] + r["agpr"] <= 64, r
