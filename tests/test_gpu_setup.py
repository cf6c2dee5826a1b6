"""The set-up objects of the C ABI (gqMeshSet, gqBvh, gqPointGrid, gqHand) and their Python wrappers: every allocation
is freed exactly once (gq_setup_live_allocations counts what the owners hold), the first call per mesh may come from
any stream, and an object lives on the device of the tensor it serves."""
import ctypes
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from graspqp_amd import _C, ops  # noqa: E402
from graspqp_amd.hands import get_hand_spec  # noqa: E402
from graspqp_amd.utils import meshes  # noqa: E402


def _live():
    n = ctypes.c_int64(-1)
    _C.call("gq_setup_live_allocations", ctypes.byref(n))
    return int(n.value)


def _open_piece():
    return np.ascontiguousarray(meshes.icosphere(1, 0.03)[:36], dtype=np.float32)  # 36 faces of an OPEN surface


def _meshset_with_occupancy():
    ms = ops.MeshSet([_open_piece()])
    _C.call("gq_meshset_build_occupancy", ms.handle)
    return ms


@pytest.mark.parametrize("kind", ["meshset", "bvh", "pointgrid", "hand"])
def test_setup_objects_free_what_they_allocate(kind):
    make = {
        "meshset": _meshset_with_occupancy,
        "bvh": lambda: ops.Bvh(_open_piece()),
        "pointgrid": lambda: ops.PointGrid(np.random.default_rng(0).normal(size=(1, 64, 3)).astype(np.float32)),
        "hand": lambda: ops.HandHandle("allegro"),
    }[kind]
    gc.collect()
    base = _live()
    obj = make()
    held = _live() - base
    assert held > 0
    hid = getattr(obj, "hid", None)
    if hid is not None:
        assert ops._handle(hid) is obj
    obj.close()
    assert _live() == base
    obj.close()  # idempotent
    assert _live() == base
    if hid is not None:
        with pytest.raises(RuntimeError, match="no longer exists"):
            ops._handle(hid)
    del obj
    gc.collect()
    assert _live() == base
    for _ in range(20):
        obj = make()
        assert _live() - base == held  # the same number for every object of this kind
        obj.close()
    assert _live() == base
    obj = make()  # without close(): the wrapper's end frees it
    del obj
    gc.collect()
    assert _live() == base


@pytest.mark.parametrize("route", ["bvh", "clusters"])
def test_first_call_per_mesh_on_a_side_stream(route):
    """The acceleration data is built on the first call; that call may be made on any stream, and returns what the same
    call on the default stream returns (another copy of the mesh tensor: its own first call)."""
    rng = np.random.default_rng(3)
    if route == "bvh":
        fv, N = _open_piece(), 32768
    else:
        fv, N = np.ascontiguousarray(meshes.superquadric(0), dtype=np.float32), 256  # 9024 faces
    pts = torch.tensor((rng.normal(size=(N, 3)) * float(np.abs(fv).max())).astype(np.float32), device="cuda")
    f_side, f_main = torch.tensor(fv, device="cuda"), torch.tensor(fv, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = ops.compute_sdf(pts, f_side)
    s.synchronize()
    assert (id(f_side), route) in ops._MESH_CACHE
    main = ops.compute_sdf(pts, f_main)
    torch.cuda.synchronize()
    assert (id(f_main), route) in ops._MESH_CACHE
    for a, b in zip(side, main):
        assert torch.equal(a, b)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second device")
def test_objects_live_on_the_device_of_their_tensor():
    """Tensors on cuda:1 while cuda:0 is current: the same bits as the same calls made with cuda:1 current."""
    rng = np.random.default_rng(4)
    fv = np.ascontiguousarray(get_hand_spec("shadow_hand").link_faces(5), dtype=np.float32)
    pts_h = (rng.normal(size=(32768, 3)) * float(np.abs(fv).max()) * 2.0).astype(np.float32)
    nz, B = 128, 2
    A = rng.normal(size=(B, nz, nz))
    Q_h = (A @ A.transpose(0, 2, 1) / nz + np.eye(nz)).astype(np.float32)
    p_h = rng.normal(size=(B, nz)).astype(np.float32)

    def run():
        dev = torch.device("cuda", 1)
        sdf = ops.compute_sdf(torch.tensor(pts_h, device=dev), torch.tensor(fv, device=dev))
        qp = ops.box_qp(torch.tensor(Q_h, device=dev), torch.tensor(p_h, device=dev), torch.zeros(B, nz, device=dev),
                        torch.ones(B, nz, device=dev))
        torch.cuda.synchronize(dev)
        return [t.cpu() for t in (*sdf, *qp)]

    assert torch.cuda.current_device() == 0
    other = run()
    with torch.cuda.device(1):
        own = run()
    for a, b in zip(other, own):
        assert torch.equal(a, b)
