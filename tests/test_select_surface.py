"""CPU-side checks of the grasp-set selection: the C ABI, every refusal of the two host-only argument checks with its message, the
Python surface, the gates of GraspStepper.select on names only, the code-object metadata of the new kernels and the link moments of
an Allegro ``SurfaceSamples`` against a direct fp64 sum over its samples.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

from graspqp_amd import _C, export, ops, stepper
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.utils import meshes

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
NAN, INF = float("nan"), float("inf")
HP, RG, LT, MOM, SCORE, TERMS, SEL, NSEL, NFEAS, FEAS, WS, DIST = (0x1000 * i for i in range(1, 13))  # never dereferenced
B, BE, L, NT = 140, 70, 23, 3
NEED = B * L * 48 + B * 8


def _tol(*v):
    return (ctypes.c_float * len(v))(*v)


def test_header_declares_and_library_exports_the_entries():
    protos, lib = _C.parse_header(), _C.lib()
    P, F, I, Q, Z = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    common = [P, I, P, P, P, I, Q, Q, Q]
    want = {"gq_grasp_select_workspace_bytes": [Q, I, P],
            "gq_grasp_select_check": common + [P, P, P, I, Q, F, P, P, P, P, P, Z],
            "gq_grasp_select": common + [P, P, P, I, Q, F, P, P, P, P, P, Z, P],
            "gq_grasp_distances_check": common + [P, P, Z], "gq_grasp_distances": common + [P, P, Z, P]}
    for name, args in want.items():
        assert name in protos and hasattr(lib, name), name
        assert protos[name][1] == args and protos[name][0] is ctypes.c_int, name
    header = open(_C.HEADER_PATH).read()
    for words in ("The reference has no counterpart", "data.py:97-102,105-150", "n_l |dA c_l + db|^2 + tr(dA C_l dA')",
                  "a NaN term under a gate", "strict: radius = 0 suppresses nothing", "There is no fill with infeasible rows",
                  "No atomics, no block waits for another"):
        assert words in header, words  # the contract is stated


def _select(**kw):
    a = dict(hand_pose=HP, pose_dim=25, Rg=RG, link_T=LT, link_moments=MOM, n_links=L, n_samples=512, batch=B, batch_each=BE,
             score=SCORE, terms=TERMS, tol=_tol(0.0, INF, 1e-3), n_terms=NT, K=8, radius=0.01, sel=SEL, n_selected=NSEL,
             n_feasible=NFEAS, feasible=FEAS, workspace=WS, workspace_bytes=NEED)
    a.update(kw)
    return _C.lib().gq_grasp_select_check(*a.values())


def _distances(**kw):
    a = dict(hand_pose=HP, pose_dim=25, Rg=RG, link_T=LT, link_moments=MOM, n_links=L, n_samples=512, batch=B, batch_each=BE,
             dist=DIST, workspace=WS, workspace_bytes=NEED)
    a.update(kw)
    return _C.lib().gq_grasp_distances_check(*a.values())


COMMON_BAD = [(dict(hand_pose=None), b"hand_pose"), (dict(Rg=None), b"Rg"), (dict(link_T=None), b"link_T"),
              (dict(link_moments=None), b"link_moments"), (dict(workspace=None), b"workspace"), (dict(pose_dim=2), b"pose_dim"),
              (dict(n_links=0), b"n_links"), (dict(n_links=65), b"n_links"), (dict(n_samples=0), b"n_samples"),
              (dict(batch_each=0), b"batch_each"), (dict(batch=B + 1), b"batch"), (dict(batch=0), b"batch"),
              (dict(batch=1 << 31, batch_each=1 << 10, workspace_bytes=1 << 62), b"batch"),
              (dict(workspace_bytes=NEED - 1), b"workspace too small")]
SELECT_BAD = COMMON_BAD + [
    (dict(score=None), b"score"), (dict(sel=None), b"sel"), (dict(n_selected=None), b"n_selected"), (dict(n_feasible=None), b"n_feasible"),
    (dict(feasible=None), b"feasible"), (dict(terms=None), b"terms"), (dict(tol=None), b"tol"), (dict(n_terms=17), b"n_terms"),
    (dict(n_terms=-1), b"n_terms"), (dict(tol=_tol(0.0, NAN, 0.0)), b"tol[1]"), (dict(K=0), b"K"), (dict(K=BE + 1), b"K"),
    (dict(radius=NAN), b"radius"), (dict(radius=-1e-30), b"radius"), (dict(radius=INF), b"radius"),
    (dict(batch_each=1 << 30, batch=1 << 30, workspace_bytes=1 << 62), b"batch_each")]
DIST_BAD = COMMON_BAD + [(dict(dist=None), b"dist"), (dict(batch_each=4097, batch=4097, workspace_bytes=1 << 40), b"batch_each")]


@pytest.mark.parametrize("kw,word", SELECT_BAD, ids=[f"{w.decode()}-{i}" for i, (_, w) in enumerate(SELECT_BAD)])
def test_select_check_refuses_with_a_message_that_names_the_argument(kw, word):
    assert _select() == 0
    # the limits themselves pass
    assert _select(K=1) == 0 and _select(K=BE) == 0 and _select(radius=0.0) == 0 and _select(n_links=64, workspace_bytes=1 << 40) == 0
    assert _select(n_terms=0, terms=None, tol=None) == 0 and _select(tol=_tol(*[INF] * 16), n_terms=16) == 0
    assert _select(tol=_tol(-INF, -1.0, INF)) == 0 and _select(pose_dim=3) == 0
    assert _select(batch_each=(1 << 30) - 1, batch=(1 << 30) - 1, workspace_bytes=1 << 62) == 0
    assert _select(**kw) != 0
    msg = _C.lib().gq_last_error()
    assert b"grasp_select" in msg and word in msg, msg


@pytest.mark.parametrize("kw,word", DIST_BAD, ids=[f"{w.decode()}-{i}" for i, (_, w) in enumerate(DIST_BAD)])
def test_distances_check_refuses_with_a_message_that_names_the_argument(kw, word):
    assert _distances() == 0 and _distances(batch_each=4096, batch=8192, workspace_bytes=1 << 40) == 0
    assert _distances(**kw) != 0
    msg = _C.lib().gq_last_error()
    assert b"grasp_select" in msg and b"grasp_distances" in msg and word in msg, msg


def test_the_workspace_size_and_the_launches_refuse_before_they_touch_the_device():
    lib = _C.lib()
    n = ctypes.c_size_t(0)
    assert lib.gq_grasp_select_workspace_bytes(256, 23, ctypes.byref(n)) == 0 and n.value == 256 * 23 * 48 + 256 * 8
    assert lib.gq_grasp_select_workspace_bytes(256, 23, None) != 0 and b"grasp_select" in lib.gq_last_error()
    assert lib.gq_grasp_select(HP, 25, RG, LT, MOM, L, 512, B, BE, SCORE, TERMS, _tol(0.0, 0.0, 0.0), NT, 8, NAN, SEL, NSEL, NFEAS, FEAS,
                               WS, NEED, None) != 0 and b"radius" in lib.gq_last_error()
    assert lib.gq_grasp_select(HP, 25, RG, LT, MOM, L, 512, B, BE, SCORE, TERMS, _tol(0.0, 0.0, 0.0), NT, 8, 0.01, SEL, NSEL, NFEAS,
                               FEAS, WS, NEED - 1, None) != 0 and b"workspace too small" in lib.gq_last_error()
    assert lib.gq_grasp_distances(HP, 25, RG, LT, MOM, L, 512, B, 0, DIST, WS, NEED, None) != 0
    assert b"batch_each" in lib.gq_last_error()


def test_python_surface_signatures():
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ops.grasp_distances) == [("hand_pose", E), ("Rg", E), ("LT", E), ("samples", E), ("batch_each", E)]
    assert sig(ops.grasp_select) == [("hand_pose", E), ("Rg", E), ("LT", E), ("samples", E), ("batch_each", E), ("score", E),
                                     ("terms", E), ("tol", E), ("k", E), ("radius", E)]
    assert ops.GraspSelection._fields == ("sel", "n_selected", "n_feasible", "feasible")
    assert sig(stepper.GraspStepper.select) == [("self", E), ("k", E), ("radius", 0.01), ("gates", None), ("score", None)]
    assert sig(export.export_poses)[-1] == ("selection", None) and sig(export.snapshot_dicts)[-1] == ("selection", None)
    import torch

    assert hasattr(torch.ops.graspqp_amd, "grasp_select") and hasattr(torch.ops.graspqp_amd, "grasp_distances")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.grasp_distances(torch.zeros(4, 25), torch.zeros(4, 9), torch.zeros(4, 23, 12), None, 4)


def test_gates_by_name():
    names = stepper.TERM_NAMES + ("E_scene", "E_approach")
    tol = stepper.select_tolerances
    assert tol(names) == [INF] * 5 + [0.0, 0.0]  # None: the obstacle terms that are on, at 0
    assert tol(stepper.TERM_NAMES) == [INF] * 5  # none on: nothing gated
    assert tol(names + ("E_pregrasp",)) == [INF] * 5 + [0.0] * 3
    assert tol(names, {"E_pen": 1e-3}) == [INF, INF, 1e-3, INF, INF, INF, INF]  # explicit gates replace the default
    assert tol(names, {"E_scene": 0.0, "E_pen": 0.5})[5] == 0.0 and tol(names, {}) == [INF] * 7
    for bad in ({"E_pregrasp": 0.0}, {"E_wall": 0.0}, {"e_scene": 0.0}, {"total": 1.0}):  # switched off, or no term at all
        with pytest.raises(ValueError, match="unknown or switched-off"):
            tol(names, bad)
    with pytest.raises(ValueError, match="NaN"):
        tol(names, {"E_scene": NAN})


def test_new_kernel_resources():
    """Three new kernels: no scratch, no spills, 256 threads; the two that stage a row's world transforms hold 64 links x 12 floats of
    them, 64 x 10 floats of link moments and the reduction slots: at most 5760 bytes of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    for name in ("gq_grasp_prepare_kernel", "gq_grasp_select_kernel", "gq_grasp_distance_kernel"):
        assert name in res, name
        r = res[name]
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["max_threads"] == 256, (name, r)
        assert r["vgpr"] + r["agpr"] <= 128 and r["lds_static"] <= 5760, (name, r)
    assert res["gq_grasp_prepare_kernel"]["lds_static"] == 0 and res["gq_grasp_select_kernel"]["lds_static"] >= 3072 + 2560


def test_link_moments_of_allegro_against_a_direct_sum():
    spec = get_hand_spec("allegro")
    pts, lnk = meshes.hand_surface_samples(spec, 512)
    s = ops.SurfaceSamples(spec, pts, lnk, device="cpu")
    m = s.link_moments
    assert m.shape == (spec.n_links, 10) and m.dtype.is_floating_point and m is s.link_moments  # built once
    m = m.numpy().astype(np.float64)
    P, Lk = s.points.numpy().astype(np.float64), s.link.numpy()
    assert m[:, 0].sum() == s.Ns == 512
    for l in range(spec.n_links):
        p = P[Lk == l]
        if len(p) == 0:
            assert not m[l].any()
            continue
        c = p.sum(0) / len(p)
        C = sum(np.outer(q - c, q - c) for q in p)
        want = np.asarray([len(p), *c, C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]])
        # stored as float32: half an ulp of each entry
        assert np.all(np.abs(m[l] - want) <= 2.0 ** -24 * np.abs(want) + 1e-30), (l, m[l], want)
        assert np.linalg.eigvalsh(C).min() >= -1e-18
