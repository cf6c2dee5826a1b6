"""CPU-side checks of the scene-aware initialisation (screened hull candidates): the C ABI, every refusal of the host-only argument
check of gq_init_select, the launches' refusals before they touch the device, the Python surface and the code-object metadata of
the new kernels.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import sys

import pytest

from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")
NAN, INF = float("nan"), float("inf")
PTS, PEN, SEL, NF, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000  # never dereferenced: the check is host only


def test_header_declares_and_library_exports_the_entries():
    protos, lib = _C.parse_header(), _C.lib()
    P, F, L, Z = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_size_t
    want = {"gq_init_candidates": [P, P], "gq_init_select": [P, P, L, L, L, F, P, P, P, Z, P],
            "gq_init_select_workspace_bytes": [L, L, P], "gq_init_select_check": [P, P, L, L, L, F, P, P, P],
            "gq_init_penalty": [P, F, P, F, L, P, P]}
    for name, args in want.items():
        assert name in protos and hasattr(lib, name), name
        assert protos[name][1] == args and protos[name][0] is ctypes.c_int, name
    header = open(_C.HEADER_PATH).read()
    for words in ("what gq_init_convex_hull gives a row that picked sample m", "a NaN penalty is never in A",
                  "no atomics, no block waits for another", "fmaf(w_approach, e_approach[i], w_scene * e_scene[i])"):
        assert words in header, words  # the contract is stated


def _check(points=PTS, penalty=PEN, n_obj=2, M=128, K=16, tol=0.0, sel=SEL, n_feasible=NF, workspace=WS):
    return _C.lib().gq_init_select_check(points, penalty, n_obj, M, K, tol, sel, n_feasible, workspace)


BAD = [(dict(points=None), b"points"), (dict(penalty=None), b"penalty"), (dict(sel=None), b"sel"), (dict(n_feasible=None), b"n_feasible"),
       (dict(workspace=None), b"workspace"), (dict(n_obj=0), b"n_obj"), (dict(K=0), b"K"), (dict(K=-3), b"K"), (dict(M=15), b"M"),
       (dict(M=1 << 30, K=5), b"M"), (dict(tol=NAN), b"tol"), (dict(tol=-1e-30), b"tol"), (dict(tol=-INF), b"tol")]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{w.decode()}-{i}" for i, (_, w) in enumerate(BAD)])
def test_check_refuses_with_a_message_that_names_the_argument(kw, word):
    lib = _C.lib()
    assert _check() == 0
    # the limits themselves pass
    assert _check(M=16, K=16) == 0 and _check(K=1) == 0 and _check(M=(1 << 30) - 1) == 0 and _check(tol=INF) == 0 and _check(tol=-0.0) == 0
    assert _check(**kw) != 0
    msg = lib.gq_last_error()
    assert b"init_select" in msg and word in msg, msg


def test_the_workspace_size_and_the_launches_refuse_before_they_touch_the_device():
    lib = _C.lib()
    n = ctypes.c_size_t(0)
    assert lib.gq_init_select_workspace_bytes(3, 2100, ctypes.byref(n)) == 0 and n.value == 3 * 2100 * 4
    assert lib.gq_init_select_workspace_bytes(3, 2100, None) != 0 and b"init_select" in lib.gq_last_error()
    assert lib.gq_init_select(PTS, PEN, 2, 128, 16, NAN, SEL, NF, WS, 2 * 128 * 4, None) != 0 and b"tol" in lib.gq_last_error()
    assert lib.gq_init_select(PTS, PEN, 2, 128, 16, 0.0, SEL, NF, WS, 2 * 128 * 4 - 1, None) != 0
    assert b"init_select" in lib.gq_last_error() and b"workspace too small" in lib.gq_last_error()
    assert lib.gq_init_penalty(PTS, 1.0, PEN, 1.0, 16, None, None) != 0 and b"init_penalty" in lib.gq_last_error()
    # gq_init_candidates: a complete descriptor but batch_each != samples_per_object, then one without the shell outputs
    d = _C.InitDesc()
    for k in ("hull_face_verts", "hull_cdf", "hull_offsets", "default_state", "joints_lower", "joints_upper", "u_face", "u_len", "u_pose",
              "u_joint", "hand_pose", "shell_points", "shell_dirs", "workspace"):
        setattr(d, k, 0x1000)
    d.n_obj, d.batch_each, d.samples_per_object, d.n_dofs, d.workspace_bytes = 2, 16, 128, 16, 1 << 30
    assert lib.gq_init_candidates(ctypes.byref(d), None) != 0
    assert b"init_candidates" in lib.gq_last_error() and b"batch_each must equal samples_per_object" in lib.gq_last_error()
    d.batch_each, d.shell_dirs = 128, None
    assert lib.gq_init_candidates(ctypes.byref(d), None) != 0 and b"shell_dirs" in lib.gq_last_error()
    d.shell_dirs, d.workspace_bytes = 0x1000, 16
    assert lib.gq_init_candidates(ctypes.byref(d), None) != 0 and b"workspace too small" in lib.gq_last_error()
    assert lib.gq_init_candidates(None, None) != 0 and b"init_candidates" in lib.gq_last_error()


def test_python_surface_signatures():
    from graspqp_amd import stepper
    from graspqp_amd.core import initializations as ini

    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(ini.convex_hull_poses_screened) == [
        ("hand", E), ("hulls", E), ("n_obj", E), ("batch_each", E), ("samples", E), ("scene", E), ("scene_margin", E), ("w_scene", E),
        ("approach", None), ("args", None), ("generator", None), ("draws", None), ("samples_per_object", None), ("chunk_rows", 65536),
        ("tol", 0.0), ("return_info", False)]
    assert sig(stepper.GraspStepper.__init__)[-1] == ("init_avoid_scene", False)
    # the parent's signature of the unscreened route is untouched
    assert [n for n, _ in sig(ini.convex_hull_poses)] == ["hand_spec", "hulls", "n_obj", "batch_each", "args", "generator", "device", "draws",
                                                          "samples_per_object", "return_shell"]


def test_new_kernel_resources():
    """Three new kernels: no scratch, no spills, eight wavefronts per SIMD; the candidate kernel is the row body of the pose kernel
    and needs its registers; the select kernel is a 1024-thread block like the farthest-point pass."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    for name, threads in (("gq_init_candidate_kernel", 256), ("gq_init_penalty_kernel", 256), ("gq_init_select_kernel", 1024)):
        assert name in res, name
        r = res[name]
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 64 and r["waves_per_simd"] == 8 and r["max_threads"] == threads, (name, r)
    assert res["gq_init_candidate_kernel"]["vgpr"] == res["gq_init_pose_kernel"]["vgpr"]
    assert res["gq_init_select_kernel"]["lds_static"] <= 512
