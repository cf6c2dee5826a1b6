"""CPU-side checks of the TSDF surfel extraction (target objects from depth images): the C ABI, every refusal of the host-only
argument check and its ValueError on the Python surface, the registered op, ``keep_label``, the code-object metadata of the three
kernels, and the fp64 oracle's own geometric check on a sphere.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import _surfel_oracle as so
from graspqp_amd import _C

to = so.to
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
NAN, INF = float("nan"), float("inf")


def test_header_declares_and_library_exports_the_entries():
    protos, lib = _C.parse_header(), _C.lib()
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    want = {"gq_tsdf_surfels_check": [P, P, F, F, I, L], "gq_tsdf_surfels_workspace_bytes": [P, P],
            "gq_tsdf_surfels": [P, P, P, P, F, F, P, P, L, P, P, P]}
    for name, args in want.items():
        assert name in protos and hasattr(lib, name), name
        assert protos[name][1] == args, name


def _grids(n_grids=3, shape=(9, 8, 17), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.ClutterGrids()
    g.values = values  # never dereferenced: the check is host only
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(grids=None, region=None, min_weight=1.0, trunc=0.02, has_outputs=1, capacity=100):
    reg = None if region is None else (ctypes.c_int32 * 6)(*region)
    return _C.lib().gq_tsdf_surfels_check(ctypes.byref(grids or _grids()), reg, min_weight, trunc, has_outputs, capacity)


BAD = [
    (dict(grids=_grids(shape=(1, 2, 2))), b"nx"), (dict(grids=_grids(voxel=0.0)), b"voxel"), (dict(grids=_grids(values=None)), b"values"),
    (dict(grids=_grids(n_grids=0)), b"n_grids"), (dict(grids=_grids(n_grids=129, shape=(256, 256, 256))), b"tiles"),
    (dict(trunc=0.0), b"trunc"), (dict(trunc=-0.01), b"trunc"), (dict(trunc=NAN), b"trunc"), (dict(trunc=INF), b"trunc"),
    (dict(min_weight=NAN), b"min_weight"), (dict(min_weight=INF), b"min_weight"), (dict(min_weight=-INF), b"min_weight"),
    (dict(capacity=0), b"capacity"), (dict(capacity=-3), b"capacity"), (dict(capacity=(1 << 24) + 1), b"capacity"),
    (dict(capacity=(1 << 24) + 1, has_outputs=0), b"capacity"),
    (dict(region=(0, 0, 0, 8, 0, 17)), b"region"), (dict(region=(3, 3, 0, 8, 0, 17)), b"region"), (dict(region=(-1, 9, 0, 8, 0, 17)), b"region"),
    (dict(region=(0, 10, 0, 8, 0, 17)), b"region"), (dict(region=(0, 9, 0, 9, 0, 17)), b"region"), (dict(region=(0, 9, 0, 8, 5, 18)), b"region"),
    (dict(region=(0, 9, 0, 8, 9, 4)), b"region"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{w.decode()}-{i}" for i, (_, w) in enumerate(BAD)])
def test_check_refuses_with_a_message_that_names_the_argument(kw, word):
    lib = _C.lib()
    assert _check() == 0
    # the limits themselves pass
    assert _check(capacity=1) == 0 and _check(capacity=1 << 24) == 0 and _check(capacity=0, has_outputs=0) == 0
    assert _check(region=(0, 9, 0, 8, 0, 17)) == 0 and _check(region=(8, 9, 7, 8, 16, 17)) == 0 and _check(min_weight=-2.0, trunc=1e-6) == 0
    assert _check(grids=_grids(n_grids=128, shape=(256, 256, 256))) == 0  # 2^23 tiles
    assert _check(**kw) != 0
    msg = lib.gq_last_error()
    assert msg.startswith(b"surfels:") and word in msg, msg


def test_null_arguments_and_the_workspace_size():
    lib = _C.lib()
    g = _grids()
    assert lib.gq_tsdf_surfels_check(None, None, 1.0, 0.02, 1, 10) != 0
    assert lib.gq_last_error().startswith(b"surfels:") and b"grids" in lib.gq_last_error()
    n = ctypes.c_size_t(0)
    assert lib.gq_tsdf_surfels_workspace_bytes(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 3 * (3 * 2 * 2) * 2 * 4  # per tile of 4 x 4 x 16 nodes: its count and its prefix
    assert lib.gq_tsdf_surfels_workspace_bytes(ctypes.byref(g), None) != 0 and b"bytes" in lib.gq_last_error()
    assert lib.gq_tsdf_surfels_workspace_bytes(None, ctypes.byref(n)) != 0 and b"grids" in lib.gq_last_error()
    # the launch refuses before it touches the device: the same check, then its own pointers
    call = lambda **kw: lib.gq_tsdf_surfels(*[{**dict(grids=ctypes.byref(g), values=0x1000, weight=0x2000, region=None, min_weight=1.0, trunc=0.02,
                                                      points=0x3000, normals=0x4000, capacity=10, count=0x5000, workspace=0x6000, stream=None), **kw}[k]
                                              for k in ("grids", "values", "weight", "region", "min_weight", "trunc", "points", "normals", "capacity",
                                                        "count", "workspace", "stream")])
    for kw, word in ((dict(trunc=NAN), b"trunc"), (dict(capacity=0), b"capacity"), (dict(values=0x1008), b"values"), (dict(values=None), b"values"),
                     (dict(normals=None), b"normals"), (dict(points=None), b"points"), (dict(count=None), b"count"), (dict(workspace=None), b"workspace")):
        assert call(**kw) != 0, kw
        assert lib.gq_last_error().startswith(b"surfels:") and word in lib.gq_last_error(), (kw, lib.gq_last_error())


def test_python_surface_signatures_and_value_errors():
    from graspqp_amd import ops
    from graspqp_amd.core.object_model import ObjectModel

    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()][1:]
    E = inspect.Parameter.empty
    assert sig(ops.SceneTSDF.surfels) == [("capacity", E), ("min_weight", 1.0), ("bounds", None), ("out", None)]
    assert sig(ops.SceneTSDF.extract_clouds) == [("min_weight", 1.0), ("bounds", None)]
    assert sig(ObjectModel.initialize_from_tsdf) == [("tsdf", E), ("min_weight", 1.0), ("bounds", None), ("radius", None), ("object_code_list", None)]
    assert [p for p in inspect.signature(ops.keep_label).parameters] == ["depth", "labels", "label"]
    assert "synchronisation" in ops.SceneTSDF.extract_clouds.__doc__
    # the volume's geometry and the checks are host work: a volume in host memory shows every refusal as a ValueError
    t = ops.SceneTSDF((0.0, 0.0, 0.0), (4, 5, 6), 0.01, 0.02, n_grids=2, device="cpu")
    for kw, word in ((dict(capacity=0), "capacity"), (dict(capacity=(1 << 24) + 1), "capacity"), (dict(capacity=8, min_weight=NAN), "min_weight"),
                     (dict(capacity=8, bounds=((1.0, 1.0, 1.0), (2.0, 2.0, 2.0))), "bounds"), (dict(capacity=8, bounds=((0.0, NAN, 0.0), (1.0, 1.0, 1.0))), "bounds"),
                     (dict(capacity=8, out=(torch.empty(2, 7, 3), torch.empty(2, 8, 3), torch.empty(2, 2, dtype=torch.int32))), "out")):
        with pytest.raises(ValueError, match=word):
            t.surfels(**kw)
    with pytest.raises(ValueError, match="min_weight"):
        t.extract_clouds(min_weight=INF)
    # bounds -> the nodes inside the box, ends included, clipped to the grid
    assert t._region(None) == [] and t._region(((0.005, -1.0, 0.0), (0.02, 1.0, 0.03))) == [1, 3, 0, 5, 0, 4]
    with pytest.raises(RuntimeError, match="CUDA"):  # and nothing computes on the host
        t.surfels(8)


def test_keep_label():
    from graspqp_amd import ops

    depth = torch.tensor([[0.5, 0.6, 0.7], [0.8, 0.0, 1.0]])
    labels = torch.tensor([[1, 0, 1], [-1, 1, 2]], dtype=torch.int32)
    assert torch.equal(ops.keep_label(depth, labels, 1), torch.tensor([[0.5, 0.0, 0.7], [0.0, 0.0, 0.0]]))
    assert torch.equal(ops.keep_label(depth, labels, 7), torch.zeros(2, 3)) and torch.equal(depth[0], torch.tensor([0.5, 0.6, 0.7]))
    cam, d, lab = to.cameras(2)
    got = ops.keep_label(d, lab, 1)  # arrays come back as a tensor, (V,H,W) like the input
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), so.keep_label(d, lab, 1)) and 0 < int((got > 0).sum()) < (d > 0).sum()
    with pytest.raises(ValueError, match="shape"):
        ops.keep_label(depth, labels[:1], 1)


def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "tsdf_surfels") and hasattr(ops._Eager, "tsdf_surfels")
    schema = ns.tsdf_surfels.default._schema
    assert [a.name for a in schema.arguments] == ["values", "weight", "origin", "voxel", "region", "min_weight", "trunc", "points", "normals",
                                                   "count", "workspace"]
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["points", "normals", "count", "workspace"]
    G, cap = 3, 11
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        v, w, c, ws = e(G, 4, 5, 6), e(G, 4, 5, 6), e(G, 2, dtype=torch.int32), e(1024, dtype=torch.uint8)
        assert ns.tsdf_surfels(v, w, [0.0, 0.0, 0.0], 0.1, [], 1.0, 0.02, e(G, cap, 3), e(G, cap, 3), c, ws) is None
        assert ns.tsdf_surfels(v, None, [0.0, 0.0, 0.0], 0.1, [0, 4, 0, 5, 1, 6], 1.0, 0.02, None, None, c, ws) is None
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.tsdf_surfels(z(G, 2, 2, 2), None, [0.0, 0.0, 0.0], 0.1, [], 1.0, 0.02, None, None, z(G, 2, dtype=torch.int32), z(64, dtype=torch.uint8))


def test_new_kernel_resources():
    """Three kernels with surfel in their names, named clear of the sets the other surface tests pin: no scratch, no spills, eight
    wavefronts per SIMD, the tile of the stencil's halo in LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "surfel" in k}
    assert sorted(new) == ["gq_surfel_count_kernel", "gq_surfel_emit_kernel", "gq_surfel_scan_kernel"], sorted(new)
    for name, r in new.items():
        assert not any(w in name for w in ("scene", "approach", "clutter", "tabletop", "cloud", "tsdf")), name
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["waves_per_simd"] == 8 and r["max_threads"] == 256, (name, r)
    tile = (4 + 3) * (4 + 3) * (16 + 3) * 4  # D with the -1 .. +2 halo
    for name in ("gq_surfel_count_kernel", "gq_surfel_emit_kernel"):  # the tile, four wavefront counts, the linker's alignment
        assert tile + 16 <= new[name]["lds_static"] <= tile + 32, (name, new[name])


# -------------------------------------------------------------------------------------------------------------------
# the oracle's own checks
# -------------------------------------------------------------------------------------------------------------------
def test_oracle_order_is_tile_thread_axis_and_a_region_filters():
    D, W, origin, voxel, trunc = so.fused("A")
    r = so.extract(D, W, origin, voxel, trunc)[0]
    e = r["edges"]
    nt = [-(-n // t) for n, t in zip(D.shape[1:], so.TILE)]
    key = [(((i // 4) * nt[1] + j // 4) * nt[2] + k // 16, ((i % 4) * 4 + j % 4) * 16 + k % 16, c) for i, j, k, c in e.tolist()]
    assert key == sorted(key) and len(set(key)) == len(key) and len(e) >= 50
    assert np.abs(np.linalg.norm(r["normals"], axis=1) - 1).max() < 1e-12
    region = (1, 8, 2, 7, 3, 17)
    sub = so.extract(D, W, origin, voxel, trunc, region=region)[0]
    b = e[:, :3] + np.eye(3, dtype=np.int64)[e[:, 3]]
    lo, hi = np.array(region[0::2]), np.array(region[1::2])
    keep = ((e[:, :3] >= lo) & (e[:, :3] < hi) & (b >= lo) & (b < hi)).all(1)
    assert np.array_equal(sub["edges"], e[keep]) and np.array_equal(sub["normals"], r["normals"][keep])  # the stencils read the whole grid


def test_oracle_a_plane_gives_its_normal_and_its_points():
    n = np.array([0.36, -0.48, 0.8])
    shape, voxel, origin = (7, 6, 9), 0.01, (-0.03, -0.025, -0.04)
    x = np.stack(np.meshgrid(*[o + voxel * np.arange(s) for o, s in zip(origin, shape)], indexing="ij"), -1)
    D = (x @ n - 0.0013).astype(np.float32)
    r = so.extract(D[None], None, origin, voxel, 0.05)[0]
    assert len(r["edges"]) > 40 and not r["ambiguous"].any() and not r["fallback"].any()
    assert np.abs(r["points"] @ n - 0.0013).max() < 1e-8 and so.angle(r["normals"], np.broadcast_to(n, r["normals"].shape)).max() < 1e-5


def test_oracle_the_cloud_of_the_sphere_lies_on_the_sphere():
    """160 x 128 images at f = 180 from the four cameras, only the sphere's pixels kept, a 24^3 volume of 5 mm voxels about the
    sphere, trunc = 3 voxels.  This oracle measures 573 surfels, radial error median 0.41 mm and max 0.67 voxel, normal angle
    median 3.6 deg, p99 17.0 deg, max 29 deg at min_weight 1 (at min_weight 2: 351 surfels, median 0.28 mm, max 0.63 voxel).  The
    tails sit at the silhouettes of the projective TSDF, the integration's business.  Bounds: those of the issue."""
    K, Wd, H, voxel, shape = (180.0, 180.0, 79.5, 63.5), 160, 128, 0.005, (24, 24, 24)
    trunc = 3 * voxel
    origin = tuple(float(c) - 0.5 * float(np.float32(voxel)) * (n - 1) for c, n in zip(to.SPHERE[0], shape))
    cam, depth, labels = to.cameras(4, K, Wd, H)
    vol = to.Volume(1, shape, origin, voxel, -trunc)
    to.integrate(vol, so.keep_label(depth, labels, 1), None, cam, K, to.DEPTH_RANGE, trunc)
    r = so.extract(vol.D.astype(np.float32), vol.W.astype(np.float32), vol.out.origin, voxel, trunc)[0]
    c, R = np.array(to.SPHERE[0]), to.SPHERE[1]
    d = r["points"] - c
    radial = np.abs(np.linalg.norm(d, axis=1) - R)
    ang = np.degrees(so.angle(r["normals"], d / np.linalg.norm(d, axis=1, keepdims=True)))
    print(f"[sphere] {len(radial)} surfels, radial median {1e3 * np.median(radial):.3f} mm max {radial.max() / voxel:.3f} voxel, normal angle "
          f"median {np.median(ang):.2f} p99 {np.percentile(ang, 99):.2f} max {ang.max():.2f} deg")
    assert len(radial) >= 300
    assert radial.max() <= voxel and np.median(ang) <= 6.0 and np.percentile(ang, 99) <= 25.0
