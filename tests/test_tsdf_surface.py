"""CPU-side checks of the TSDF fusion (scenes from depth images, integrated on the device into scene grids): the C ABI and the
struct's mirror, every refusal of the host-only argument check, the registered op, the code-object metadata of the new kernel, and
the fp64 oracle's own self-checks.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _tsdf_oracle as to
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_tsdf_check", 5), ("gq_tsdf_integrate", 9)):
        assert name in protos, name
        assert hasattr(lib, name), name
        assert len(protos[name][1]) == n_args, name
    assert protos["gq_tsdf_check"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    assert protos["gq_tsdf_integrate"][1] == [ctypes.c_void_p] * 6 + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    src = open(_C.HEADER_PATH).read()
    block = src[src.index("typedef struct gqDepthViews"):src.index("} gqDepthViews;")]
    order = ["depth;", "labels;", "cam_T;", "int n_views, width, height;", "float fx, fy, cx, cy;", "float depth_min, depth_max;"]
    at = [block.index(f) for f in order]
    assert at == sorted(at)
    assert [f[0] for f in _C.DepthViews._fields_] == ["depth", "labels", "cam_T", "n_views", "width", "height", "fx", "fy", "cx", "cy",
                                                      "depth_min", "depth_max"]
    # the struct's layout from its fields: three pointers, three ints, six floats, padded to the pointer's alignment
    p = ctypes.sizeof(ctypes.c_void_p)
    raw = 3 * p + 3 * ctypes.sizeof(ctypes.c_int) + 6 * ctypes.sizeof(ctypes.c_float)
    D = _C.DepthViews
    assert ctypes.sizeof(D) == (raw + p - 1) // p * p
    assert (D.depth.offset, D.labels.offset, D.cam_T.offset, D.n_views.offset, D.height.offset, D.fx.offset, D.depth_max.offset) == \
        (0, p, 2 * p, 3 * p, 3 * p + 8, 3 * p + 12, 3 * p + 32)


def _grids(n_grids=3, shape=(2, 2, 2), origin=(0.0, 0.0, 0.0), voxel=0.1, values=0x1000):
    g = _C.ClutterGrids()
    g.values = values  # never dereferenced: the check is host only
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _views(**kw):
    v = _C.DepthViews()
    v.depth, v.labels, v.cam_T = 0x2000, None, 0x3000
    v.n_views, v.width, v.height = 3, 640, 480
    v.fx, v.fy, v.cx, v.cy = 500.0, 510.0, 319.5, 239.5
    v.depth_min, v.depth_max = 0.05, 5.0
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def _check(grids=None, views=None, trunc=0.02, max_weight=64.0, unknown=-0.02):
    return _C.lib().gq_tsdf_check(ctypes.byref(grids or _grids()), ctypes.byref(views or _views()), trunc, max_weight, unknown)


NAN, INF = float("nan"), float("inf")
GRID_BAD = [
    (dict(shape=(1, 2, 2)), b"nx"), (dict(shape=(2, 1, 2)), b"ny"), (dict(shape=(2, 2, 1)), b"nz"),
    (dict(shape=(1 << 10, 1 << 10, (1 << 8) + 1)), b"nx*ny*nz"), (dict(voxel=0.0), b"voxel"), (dict(voxel=NAN), b"voxel"),
    (dict(voxel=INF), b"voxel"), (dict(origin=(0.0, NAN, 0.0)), b"origin"), (dict(values=None), b"values"),
    (dict(n_grids=0), b"n_grids"), (dict(n_grids=65537), b"n_grids"),
]
VIEW_BAD = [
    (dict(depth=None), b"depth"), (dict(cam_T=None), b"cam_T"), (dict(n_views=0), b"n_views"), (dict(n_views=65), b"n_views"),
    (dict(width=0), b"width"), (dict(width=8193), b"width"), (dict(height=0), b"height"), (dict(height=8193), b"height"),
    (dict(fx=0.0), b"fx"), (dict(fx=-1.0), b"fx"), (dict(fx=NAN), b"fx"), (dict(fx=INF), b"fx"),
    (dict(fy=0.0), b"fy"), (dict(fy=-1.0), b"fy"), (dict(fy=NAN), b"fy"), (dict(fy=INF), b"fy"),
    (dict(cx=NAN), b"cx"), (dict(cx=-INF), b"cx"), (dict(cy=NAN), b"cy"), (dict(cy=INF), b"cy"),
    (dict(depth_min=0.0), b"depth_min"), (dict(depth_min=-0.1), b"depth_min"), (dict(depth_min=NAN), b"depth_min"),
    (dict(depth_min=INF), b"depth_min"), (dict(depth_max=0.04), b"depth_max"), (dict(depth_max=NAN), b"depth_max"),
    (dict(depth_max=INF), b"depth_max"),
]
SCALAR_BAD = [
    (dict(trunc=0.0), b"trunc"), (dict(trunc=-0.01), b"trunc"), (dict(trunc=NAN), b"trunc"), (dict(trunc=INF), b"trunc"),
    (dict(max_weight=0.5), b"max_weight"), (dict(max_weight=NAN), b"max_weight"), (dict(max_weight=INF), b"max_weight"),
    (dict(unknown=NAN), b"unknown"), (dict(unknown=INF), b"unknown"), (dict(unknown=-INF), b"unknown"),
]
BAD = ([(dict(grids=_grids(**kw)), w) for kw, w in GRID_BAD] + [(dict(views=_views(**kw)), w) for kw, w in VIEW_BAD] + SCALAR_BAD)


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{w.decode()}-{i}" for i, (_, w) in enumerate(BAD)])
def test_check_refuses_with_a_message_that_names_the_argument(kw, word):
    lib = _C.lib()
    assert _check() == 0
    # the limits themselves pass
    assert _check(views=_views(n_views=1, width=1, height=1)) == 0 and _check(views=_views(n_views=64, width=8192, height=8192)) == 0
    assert _check(views=_views(depth_max=0.05, labels=0x4000)) == 0 and _check(max_weight=1.0, unknown=0.02, trunc=1e-6) == 0
    assert _check(grids=_grids(n_grids=1)) == 0 and _check(grids=_grids(n_grids=65536)) == 0
    assert _check(**kw) != 0
    msg = lib.gq_last_error()
    assert b"tsdf" in msg and word in msg, msg


def test_check_refuses_null_arguments_and_too_many_tiles():
    lib = _C.lib()
    g, v = _grids(), _views()
    assert lib.gq_tsdf_check(None, ctypes.byref(v), 0.02, 64.0, -0.02) != 0
    assert b"tsdf" in lib.gq_last_error() and b"grids" in lib.gq_last_error()
    assert lib.gq_tsdf_check(ctypes.byref(g), None, 0.02, 64.0, -0.02) != 0
    assert b"tsdf" in lib.gq_last_error() and b"views" in lib.gq_last_error()
    # the launch's own limit, the compose kernel's: n_grids x tiles of 4 x 4 x 16 nodes
    assert _check(grids=_grids(n_grids=128, shape=(256, 256, 256))) == 0  # 2^23 tiles
    assert _check(grids=_grids(n_grids=129, shape=(256, 256, 256))) != 0
    assert b"tsdf" in lib.gq_last_error() and b"tiles" in lib.gq_last_error()
    # the launch refuses before it touches the device: the same check, then its own pointers
    assert lib.gq_tsdf_integrate(ctypes.byref(g), 0x1000, 0x5000, None, ctypes.byref(_views(n_views=0)), None, 0.02, 64.0, None) != 0
    assert b"tsdf" in lib.gq_last_error() and b"n_views" in lib.gq_last_error()
    assert lib.gq_tsdf_integrate(ctypes.byref(g), 0x1008, 0x5000, None, ctypes.byref(v), None, 0.02, 64.0, None) != 0
    assert b"tsdf" in lib.gq_last_error() and b"values" in lib.gq_last_error()
    assert lib.gq_tsdf_integrate(ctypes.byref(g), 0x1000, None, None, ctypes.byref(v), None, 0.02, 64.0, None) != 0
    assert b"tsdf" in lib.gq_last_error() and b"weight" in lib.gq_last_error()


def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "tsdf_integrate") and hasattr(ops._Eager, "tsdf_integrate") and hasattr(ops, "SceneTSDF")
    schema = ns.tsdf_integrate.default._schema
    assert [a.name for a in schema.arguments][:4] == ["values", "weight", "origin", "voxel"]
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["values", "weight"]
    # the stack crosses the dispatcher as (values, origin, voxel), as in scene_compose, whose schema did not change
    compose = ns.scene_compose.default._schema
    assert [(a.name, str(a.type)) for a in compose.arguments][:3] == [("out_values", "Tensor"), ("origin", "List[float]"), ("voxel", "float")]
    assert [str(a.type) for a in schema.arguments if a.name in ("values", "origin", "voxel")] == ["Tensor", "List[float]", "float"]
    G, V, H, W = 3, 2, 5, 7
    K, rng, origin = [45.0, 45.0, 3.0, 2.0], [0.05, 2.0], [0.0, 0.0, 0.0]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        v, w = e(G, 4, 5, 6), e(G, 4, 5, 6)
        assert ns.tsdf_integrate(v, w, origin, 0.1, e(V, H, W), e(V, H, W, dtype=torch.int32), e(V, 12), K, rng, e(G, 12),
                                 e(G, dtype=torch.int32), 0.02, 64.0) is None
        assert ns.tsdf_integrate(v, w, origin, 0.1, e(V, H, W), None, e(V, 12), K, rng, None, None, 0.02, 64.0) is None
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.tsdf_integrate(z(G, 2, 2, 2), z(G, 2, 2, 2), origin, 0.1, z(V, H, W), None, z(V, 12), K, rng, None, None, 0.02, 64.0)


def test_new_kernel_resources():
    """Exactly one kernel with tsdf in its name, named clear of the sets the other surface tests pin: no scratch, no spills, and the
    22 VGPRs DESIGN 17 states (the target was at most 64: eight wavefronts per SIMD)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "tsdf" in k}
    assert sorted(new) == ["gq_tsdf_integrate_kernel"], sorted(new)
    r = new["gq_tsdf_integrate_kernel"]
    assert not any(w in "gq_tsdf_integrate_kernel" for w in ("scene", "approach", "clutter", "tabletop", "cloud"))
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds_static"] == 0, r
    assert r["vgpr"] + r["agpr"] == 22 and r["waves_per_simd"] == 8, r
    assert r["max_threads"] == 256, r  # a tile of 4 x 4 x 16 nodes


# -------------------------------------------------------------------------------------------------------------------
# the fp64 oracle's own self-checks
# -------------------------------------------------------------------------------------------------------------------
def _top_down():
    """A camera 0.5 m above the origin looking straight down the world's z axis, and its image of the bare plane z = 0."""
    cam = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.5]], dtype=np.float32)
    depth, labels = to.render(cam, to.INTRINSICS, to.IMG_W, to.IMG_H, 0.0, ((0.0, 0.0, -1.0), 0.1))  # the sphere is under the table
    assert (labels == 0).all() and np.abs(depth.astype(np.float64) - 0.5).max() < 1e-7
    return cam, depth, labels


def test_oracle_a_camera_looking_straight_down_at_a_plane():
    cam, depth, labels = _top_down()
    vol, _, _, _ = to.layout("A")
    info = to.integrate(vol, depth, labels, cam[None], to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC)
    zw = vol.out.nodes().numpy()[..., 2]
    seen = info["updated"][0]
    assert np.array_equal(seen, zw >= -to.f32(to.TRUNC))  # every node in the frustum down to the band's far side, none below it
    assert np.abs(vol.D[0][seen] - np.clip(zw[seen], -to.f32(to.TRUNC), to.f32(to.TRUNC))).max() <= 1e-12
    assert (vol.W[0][seen] == 1).all() and (vol.W[0][~seen] == 0).all() and (vol.D[0][~seen] == -to.f32(to.TRUNC)).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_oracle_views_in_one_call_equal_one_call_per_view(name):
    vol, tT, skip, n = to.layout(name)
    cam, depth, labels = to.cameras(n)
    args = (to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT, skip)
    one = vol.copy()
    info = to.integrate(one, depth, labels, cam, *args)
    many, amb, upd = vol.copy(), False, False
    for v in range(n):
        i = to.integrate(many, depth[v], labels[v], cam[v:v + 1], *args)
        amb, upd = amb | i["ambiguous"], upd | i["updated"]
    assert np.array_equal(one.D, many.D) and np.array_equal(one.W, many.W)
    assert np.array_equal(info["ambiguous"], amb) and np.array_equal(info["updated"], upd)
    assert one.W.max() == n and to.conditions(one, info)[1] > 0.5


def test_oracle_a_skipped_label_carves_its_rays():
    vol, tT, skip, n = to.layout("B")
    cam, depth, labels = to.cameras(n)
    assert list(skip) == [1, -1, 7] and (labels == 1).sum() > 50 and not (labels == 7).any()
    args = (to.INTRINSICS, to.DEPTH_RANGE, to.TRUNC, 64.0, tT)
    carved, plain, unlabelled = vol.copy(), vol.copy(), vol.copy()
    to.integrate(carved, depth, labels, cam, *args, skip)
    to.integrate(plain, depth, labels, cam, *args, None)
    to.integrate(unlabelled, depth, None, cam, *args, skip)
    assert np.array_equal(plain.D, unlabelled.D) and np.array_equal(plain.W, unlabelled.W)
    assert np.array_equal(carved.D[1:], plain.D[1:]) and np.array_equal(carved.W[1:], plain.W[1:])  # -1 and an absent label skip nothing
    # grid 0: nodes inside the sphere were occupied or unseen; with the sphere's rays free they are free space
    xw = vol.out.nodes().numpy() @ tT[0, :, :3].astype(np.float64).T + tT[0, :, 3]
    inside = np.linalg.norm(xw - np.array(to.SPHERE[0]), axis=-1) < to.SPHERE[1] - 0.01
    assert inside.sum() >= 20 and (plain.D[0][inside] < 0).all() and (carved.D[0][inside] > 0.5 * to.TRUNC).all()
    assert (carved.D[0] >= plain.D[0] - 1e-15).all() and (carved.W[0] >= plain.W[0]).all()


def test_oracle_refuses_an_image_that_touches_the_depth_range():
    vol, _, _, _ = to.layout("A")
    cam, depth, labels = _top_down()
    with pytest.raises(AssertionError, match="range"):
        to.integrate(vol, depth, labels, cam[None], to.INTRINSICS, (0.05, 0.50001), to.TRUNC)
