"""CPU-side checks of the Euclidean distance field of a TSDF (ESDF): the C ABI, every refusal of the host-only argument check and
its ValueError on the Python surface, the registered op, the code-object metadata of the kernels, and the fp64 oracle's own
checks on analytic fields.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import _esdf_oracle as eo
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
NAN, INF = float("nan"), float("inf")
SRC, DST, WS = 0x1000, 1 << 40, 1 << 41  # never dereferenced: the check is host only


def test_header_declares_and_library_exports_the_entries():
    protos, lib = _C.parse_header(), _C.lib()
    P, F = ctypes.c_void_p, ctypes.c_float
    want = {"gq_esdf_check": [P, P, F, F, P], "gq_esdf_workspace_bytes": [P, P], "gq_esdf": [P, P, P, F, F, P, P]}
    for name, args in want.items():
        assert name in protos and hasattr(lib, name), name
        assert protos[name][1] == args and protos[name][0] is ctypes.c_int, name
    header = open(_C.HEADER_PATH).read()
    assert "at most 1024 nodes" in header and "max(e, trunc), max_distance" in header  # the contract and the axis limit are stated


def _grids(values=SRC, n_grids=3, shape=(9, 8, 17), origin=(0.0, 0.25, -0.5), voxel=0.125):
    g = _C.ClutterGrids()
    g.values = values
    g.n_grids = n_grids
    g.nx, g.ny, g.nz = shape
    g.origin = (ctypes.c_float * 3)(*origin)
    g.voxel = voxel
    return g


def _check(src=None, dst=None, trunc=0.25, max_distance=1.0, workspace=WS, **both):
    src = src if src is not None else _grids(**both)
    dst = dst if dst is not None else _grids(values=DST, **both)
    ref = lambda g: None if g == "null" else ctypes.byref(g)
    return _C.lib().gq_esdf_check(ref(src), ref(dst), trunc, max_distance, workspace)


BAD = [
    (dict(src="null"), b"src"), (dict(dst="null"), b"dst"), (dict(src=_grids(values=None)), b"src values"),
    (dict(dst=_grids(values=None)), b"dst values"), (dict(workspace=None), b"workspace"),
    # what gq_clutter_check refuses, for either stack
    (dict(src=_grids(shape=(1, 8, 17))), b"src: clutter"), (dict(src=_grids(voxel=0.0)), b"voxel"), (dict(src=_grids(n_grids=0)), b"n_grids"),
    (dict(src=_grids(origin=(0.0, NAN, 0.0))), b"origin"), (dict(dst=_grids(values=DST, shape=(9, 1, 17))), b"dst: clutter"),
    (dict(dst=_grids(values=DST, voxel=INF)), b"dst: clutter"), (dict(dst=_grids(values=DST, n_grids=70000)), b"dst: clutter"),
    # dst is not src's twin
    (dict(dst=_grids(values=DST, n_grids=2)), b"dst n_grids"), (dict(dst=_grids(values=DST, shape=(9, 8, 16))), b"dst shape"),
    (dict(dst=_grids(values=DST, shape=(8, 9, 17))), b"dst shape"), (dict(dst=_grids(values=DST, origin=(0.0, 0.25, 0.5))), b"dst origin[2]"),
    (dict(dst=_grids(values=DST, voxel=0.25)), b"dst voxel"),
    (dict(dst=_grids(values=SRC)), b"alias"), (dict(dst=_grids(values=SRC + 4 * (3 * 9 * 8 * 17 - 1))), b"alias"),
    (dict(dst=_grids(values=DST), src=_grids(values=DST + 64)), b"alias"),
    (dict(trunc=0.0), b"trunc"), (dict(trunc=-0.25), b"trunc"), (dict(trunc=NAN), b"trunc"), (dict(trunc=INF), b"trunc"),
    (dict(max_distance=NAN), b"max_distance"), (dict(max_distance=INF), b"max_distance"), (dict(max_distance=0.2), b"max_distance"),
    (dict(max_distance=512.1), b"max_distance"),  # R = 4097
    (dict(shape=(1025, 2, 2)), b"nx"), (dict(shape=(2, 1025, 2)), b"ny"), (dict(shape=(2, 2, 1025)), b"nz"),
    (dict(n_grids=257, shape=(1024, 512, 512)), b"tiles"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{w.decode().replace(' ', '_')}-{i}" for i, (_, w) in enumerate(BAD)])
def test_check_refuses_with_a_message_that_names_the_argument(kw, word):
    lib = _C.lib()
    assert _check() == 0
    # the limits themselves pass
    assert _check(max_distance=0.25) == 0 and _check(max_distance=512.0) == 0 and _check(trunc=1e-30, max_distance=1e-30) == 0  # R = 4096
    assert _check(shape=(1024, 2, 2)) == 0 and _check(shape=(2, 1024, 2)) == 0 and _check(shape=(2, 2, 1024)) == 0
    assert _check(n_grids=256, shape=(1024, 512, 512)) == 0  # 2^23 tiles
    assert _check(dst=_grids(values=SRC + 4 * 3 * 9 * 8 * 17)) == 0  # dst right behind src
    assert _check(**kw) != 0
    msg = lib.gq_last_error()
    assert msg.startswith(b"esdf:") and word in msg, msg


def test_the_workspace_size_and_the_launch_refuses_before_it_touches_the_device():
    lib = _C.lib()
    g, d = _grids(), _grids(values=DST)
    n = ctypes.c_size_t(0)
    assert lib.gq_esdf_workspace_bytes(ctypes.byref(g), ctypes.byref(n)) == 0
    assert n.value == 3 * (3 * 9 * 8 * 17) * 4  # three buffers of the stack's size
    assert lib.gq_esdf_workspace_bytes(ctypes.byref(g), None) != 0 and b"bytes" in lib.gq_last_error()
    assert lib.gq_esdf_workspace_bytes(None, ctypes.byref(n)) != 0 and b"src" in lib.gq_last_error()
    bad = _grids(shape=(1, 2, 2))
    assert lib.gq_esdf_workspace_bytes(ctypes.byref(bad), ctypes.byref(n)) != 0 and b"nx" in lib.gq_last_error()
    call = lambda **kw: lib.gq_esdf(*[{**dict(src=ctypes.byref(g), dst=ctypes.byref(d), dst_values=DST, trunc=0.25, max_distance=1.0, workspace=WS,
                                              stream=None), **kw}[k] for k in ("src", "dst", "dst_values", "trunc", "max_distance", "workspace", "stream")])
    for kw, word in ((dict(trunc=NAN), b"trunc"), (dict(max_distance=0.1), b"max_distance"), (dict(workspace=None), b"workspace"),
                     (dict(dst_values=DST + 8), b"dst_values"), (dict(dst_values=None), b"dst_values"), (dict(dst=ctypes.byref(g)), b"alias")):
        assert call(**kw) != 0, kw
        assert lib.gq_last_error().startswith(b"esdf:") and word in lib.gq_last_error(), (kw, lib.gq_last_error())


def test_python_surface_signatures_and_value_errors():
    from graspqp_amd import ops

    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ops.scene_esdf) == [("src", E), ("trunc", E), ("max_distance", E), ("out", None)]
    assert sig(ops.SceneTSDF.esdf)[1:] == [("max_distance", E), ("out", None)]
    doc = " ".join(ops.SceneTSDF.esdf.__doc__.split())
    assert "may now go up to ``max_distance``" in doc and "remain projective" in doc
    # the geometry and the checks are host work: a volume in host memory shows every refusal as a ValueError
    o = (0.0, 0.0, 0.0)
    t = ops.SceneTSDF(o, (4, 5, 6), 0.01, 0.02, n_grids=2, device="cpu")
    S = lambda G=2, shape=(4, 5, 6), origin=o, voxel=0.01: ops.SceneSDFSet(torch.zeros((G,) + shape), origin, voxel, device="cpu")
    for kw, word in ((dict(max_distance=0.01), "max_distance"), (dict(max_distance=NAN), "max_distance"), (dict(max_distance=INF), "max_distance"),
                     (dict(max_distance=41.0), "max_distance"), (dict(max_distance=0.05, out=S(G=3)), "n_grids"),
                     (dict(max_distance=0.05, out=S(shape=(4, 5, 7))), "shape"), (dict(max_distance=0.05, out=S(origin=(0.0, 0.0, 0.01))), "origin"),
                     (dict(max_distance=0.05, out=S(voxel=0.02)), "voxel"), (dict(max_distance=0.05, out=t.scene), "alias"),
                     (dict(max_distance=0.05, out=ops.SceneSDF(torch.zeros(4, 5, 6), o, 0.01, device="cpu")), "out must be")):
        with pytest.raises(ValueError, match=word):
            t.esdf(**kw)
    with pytest.raises(ValueError, match="nx"):
        ops.SceneTSDF(o, (1025, 2, 2), 0.01, 0.02, device="cpu").esdf(0.05)
    with pytest.raises(ValueError, match="trunc"):
        ops.scene_esdf(t.scene, NAN, 0.05)
    with pytest.raises(ValueError, match="trunc"):
        ops.scene_esdf(t.scene, 0.0, 0.05)
    with pytest.raises(ValueError, match="src must be"):
        ops.scene_esdf(t, 0.02, 0.05)
    with pytest.raises(RuntimeError, match="CUDA"):  # and nothing computes on the host
        t.esdf(0.05)
    one = ops.SceneTSDF(o, (4, 5, 6), 0.01, 0.02, device="cpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        one.esdf(0.02)  # the limit max_distance == trunc passes the check
    assert isinstance(one._esdf_scene, ops.SceneSDF) and isinstance(t._esdf_scene, ops.SceneSDFSet) and t._esdf_scene.shape == (4, 5, 6)


def test_op_is_registered_with_a_fake_kernel():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "scene_esdf") and hasattr(ops._Eager, "scene_esdf")
    schema = ns.scene_esdf.default._schema
    assert [a.name for a in schema.arguments] == ["values", "origin", "voxel", "trunc", "max_distance", "out_values", "workspace"]
    assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["out_values", "workspace"]
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        assert ns.scene_esdf(e(3, 4, 5, 6), [0.0, 0.0, 0.0], 0.1, 0.02, 0.06, e(3, 4, 5, 6), e(4096, dtype=torch.uint8)) is None
    z = torch.zeros
    with pytest.raises(NotImplementedError):  # no CPU kernel behind the dispatcher
        ns.scene_esdf(z(1, 2, 2, 2), [0.0, 0.0, 0.0], 0.1, 0.02, 0.06, z(1, 2, 2, 2), z(96, dtype=torch.uint8))


def test_new_kernel_resources():
    """Five kernels with edt in their names (a seed and an envelope per tile form, the envelope that finishes), named clear of the
    sets the other surface tests pin: no scratch, no spills, at most 64 registers, eight wavefronts per SIMD; the tile is dynamic
    LDS, sized by the line."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "edt" in k}
    assert sorted(new) == ["gq_edt_env_kernel<false, false>", "gq_edt_env_kernel<true, false>", "gq_edt_env_kernel<true, true>",
                           "gq_edt_seed_kernel<false>", "gq_edt_seed_kernel<true>"], sorted(new)
    for name, r in new.items():
        assert not any(w in name for w in ("scene", "approach", "clutter", "tabletop", "cloud", "tsdf", "surfel", "exact_kernel")), name
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["lds_static"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["waves_per_simd"] == 8 and r["max_threads"] == 256, (name, r)


# -------------------------------------------------------------------------------------------------------------------
# the oracle's own checks
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,median,worst", [("sphere", 0.033, 0.12), ("plane", 0.015, 1.1)])
def test_oracle_out_of_band_distances_are_the_true_ones(name, median, worst):
    """Clipped exact distances on 5 mm voxels, trunc = 3 voxels: out of band phi is the true distance to a fraction of a voxel.  The
    plane's 1.1-voxel maximum sits at the grid's border, where the nearest surface point lies outside the grid: a grid knows only
    its own crossings.  The figures are those of the issue, within 20 %."""
    D, true, voxel, trunc = eo.analytic(name)
    phi, info = eo.esdf(D, voxel, trunc, 0.08)
    out = info[0]["out"]
    err = np.abs(phi - np.clip(np.abs(true), trunc, 0.08) * np.sign(true))[out] / voxel
    print(f"[{name}] {info[0]['crossings']} crossings, out-of-band |phi - truth| median {np.median(err):.4f} max {err.max():.4f} voxel")
    assert out.sum() > 4000 and 0.8 * median <= np.median(err) <= 1.2 * median and 0.8 * worst <= err.max() <= 1.2 * worst
    assert np.array_equal(phi[info[0]["band"]], D[info[0]["band"]].astype(np.float64))
    if name == "plane":  # the worst node is on the grid's border
        worst_at = np.argwhere(out)[np.argmax(err)]
        assert any(i == 0 or i == n - 1 for i, n in zip(worst_at, D.shape))


def test_oracle_without_a_crossing_and_with_max_distance_at_trunc():
    cases = eo.hand_made()
    D, voxel, trunc, dmax = cases["no_crossing_occupied"]
    phi, info = eo.esdf(D, voxel, trunc, dmax)
    assert info[0]["crossings"] == 0 and np.isinf(info[0]["e"]).all() and (phi[info[0]["out"]] == -np.float32(dmax)).all()
    assert np.isnan(phi[info[0]["void"]]).all() and info[0]["void"].sum() == 3
    phi, info = eo.esdf(np.where(np.isfinite(D), -D, D), voxel, trunc, dmax)  # the same in free space
    assert (phi[info[0]["out"]] == np.float32(dmax)).all()
    D, voxel, trunc, dmax = cases["max_distance_is_trunc"]
    phi, info = eo.esdf(D, voxel, trunc, dmax)
    assert info[0]["crossings"] > 0 and 0 < info[0]["out"].sum() < D.size
    assert (np.abs(phi[info[0]["out"]]) == np.float32(trunc)).all() and (np.abs(phi[info[0]["band"]]) < np.float32(trunc)).all()


def test_oracle_a_stack_is_its_grids_and_trunc_is_compared_in_float32():
    D = np.stack([eo.analytic("sphere")[0], eo.analytic("plane")[0]])
    phi, _ = eo.esdf(D, eo.A_VOXEL, eo.A_TRUNC, 0.08)
    for g in range(2):
        assert np.array_equal(phi[g], eo.esdf(D[g], eo.A_VOXEL, eo.A_TRUNC, 0.08)[0])
    # float32(0.015) < 0.015 as doubles: a clipped node compared against the double would count as in band
    assert float(np.float32(eo.A_TRUNC)) < eo.A_TRUNC
    _, info = eo.esdf(D[0], eo.A_VOXEL, eo.A_TRUNC, 0.08)
    assert not (info[0]["band"] & (np.abs(D[0]) == np.float32(eo.A_TRUNC))).any() and (np.abs(D[0]) == np.float32(eo.A_TRUNC)).sum() > 1000
