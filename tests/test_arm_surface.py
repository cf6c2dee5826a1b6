"""The arm clearance term's surface without a GPU: the collision spheres of ops.ArmSpec and their validation, ops.arm_check and the
library's messages, the weight key, the order of the terms and the default gate of select, the stepper's arguments and their errors,
the C entries in the header and in the built library, the registered ops with their fake kernels, the new kernel's resources, the
tools' switches."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import _arm_oracle as ao
import _reach_oracle as ro
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_arm_spec_spheres_and_their_validation():
    arm = ro.arm_spec("elbow6")
    assert arm.n_spheres == 0 and arm.spheres is None
    a1 = arm.with_spheres([0, 5, 5], [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], [0.05, 0.04, 0.03])
    assert a1.n_spheres == 3 and a1.sphere_link.dtype == np.int32 and a1.sphere_centre.shape == (3, 3) and a1.sphere_radius.shape == (3,)
    assert arm.with_spheres([1, 2], np.zeros((2, 3)), 0.05).sphere_radius.tolist() == [0.05, 0.05]  # one radius for all
    assert a1.with_seeds(arm.seeds).n_spheres == 3  # the spheres stay with the arm
    for link, centre, radius, word in (([0, 6], np.zeros((2, 3)), [0.1, 0.1], "0..5"), ([-1], np.zeros((1, 3)), [0.1], "0..5"),
                                       ([0.5], np.zeros((1, 3)), [0.1], "integer"), ([0], np.zeros((1, 2)), [0.1], "centre"),
                                       ([0], np.zeros((2, 3)), [0.1], "centre"), ([0], np.full((1, 3), np.nan), [0.1], "centre"),
                                       ([0], np.zeros((1, 3)), [0.0], "radius"), ([0], np.zeros((1, 3)), [np.inf], "radius"),
                                       ([0], np.zeros((1, 3)), [0.1, 0.2], "radius"), ([], np.zeros((0, 3)), [], "64"),
                                       ([0] * 65, np.zeros((65, 3)), [0.1] * 65, "64")):
        with pytest.raises(ValueError, match=word):
            arm.with_spheres(link, centre, radius)
    assert arm.with_spheres([0] * 64, np.zeros((64, 3)), 0.1).n_spheres == 64
    # the link spheres: along every link's segment, capped at 64
    for name in ro.ARM_NAMES:
        a = ao.arm_spec(name)
        assert 6 <= a.n_spheres <= 64 and set(a.sphere_link.tolist()) == set(range(a.n_joints)), name
        assert (np.diff(a.sphere_link) >= 0).all() and (a.sphere_radius == ao.RADIUS).all()
        for j in range(a.n_joints):  # on the segment from the link's origin to the next joint's offset
            end = (a.joint_T[j + 1] if j + 1 < a.n_joints else a.tool_T)[:, 3]
            c = a.sphere_centre[a.sphere_link == j]
            t = c @ end / max(end @ end, 1e-300)
            assert np.allclose(c, np.outer(t, end), atol=1e-12) and t.min() >= 0 and t.max() <= 1 + 1e-12
            assert np.allclose(c[0], 0) and (len(c) == 1 or np.allclose(c[-1], end))
    assert ro.arm_spec("arm7").with_link_spheres(0.02, 0.005).n_spheres == 64
    for r, sp in ((0.0, 0.1), (0.05, 0.0), (np.nan, 0.1)):
        with pytest.raises(ValueError, match="with_link_spheres"):
            arm.with_link_spheres(r, sp)


def test_arm_check_messages():
    from graspqp_amd import ops

    arm = ao.arm_spec("arm7")
    ops.arm_check(arm)
    ops.arm_check(arm, distance=0.0, stations=0)  # the distance is not read without stations
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(margin=-0.01), "margin"), (dict(margin=nan), "margin"), (dict(margin=inf), "margin"), (dict(damping=0.0), "damping"),
                     (dict(damping=nan), "damping"), (dict(rot_scale=0.0), "rot_scale"), (dict(rot_scale=inf), "rot_scale"),
                     (dict(stations=4), "n_stations"), (dict(stations=-1), "n_stations"), (dict(stations=1.5), "stations"),
                     (dict(stations=2, distance=0.0), "distance"), (dict(stations=1, distance=nan), "distance"),
                     (dict(grasp_axis=(0, 0, 0)), "grasp_axis"), (dict(grasp_axis=(0, nan, 1)), "grasp_axis")):
        with pytest.raises(ValueError, match=word) as e:
            ops.arm_check(arm, who="GraspStepper", **kw)
        assert "arm" in str(e.value) and "GraspStepper" in str(e.value)
    with pytest.raises(ValueError, match="collision spheres"):
        ops.arm_check(ro.arm_spec("arm7"))
    with pytest.raises(ValueError, match="ArmSpec"):
        ops.arm_check("franka")
    # the stack and the batch
    g = _C.ClutterGrids()
    g.values, g.n_grids, g.nx, g.ny, g.nz, g.voxel = 8, 2, 4, 4, 4, 0.1
    ops.arm_check(arm, g, 8)
    with pytest.raises(ValueError, match="n_grids"):
        ops.arm_check(arm, g, 7)
    g.nx = 1
    with pytest.raises(ValueError, match="arm: grids"):
        ops.arm_check(arm, g, 8)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.arm_terms(torch.zeros(2, 25), None, torch.zeros(2, 4, dtype=torch.long), None, None, None, None, None, 1, None, (0, 0, 1), None)
    p = inspect.signature(ops.arm_terms).parameters
    assert list(p)[:12] == ["hand_pose", "hand", "idx", "Rg", "LT", "ws", "arm", "base_T", "batch_each", "scene", "grasp_axis", "reach_q"]
    assert (p["damping"].default, p["rot_scale"].default, p["stations"].default, p["distance"].default, p["margin"].default) == \
        (1e-6, 0.1, 0, 0.10, 0.0)


def test_weights_term_order_and_select_tolerances():
    from graspqp_amd import stepper as S

    assert S.ARM_TERMS == ("E_arm",)
    w = S.merge_weights(None)
    assert w["E_arm"] == 0.0 and {k: w[k] for k in S.DEFAULT_WEIGHTS} == S.DEFAULT_WEIGHTS
    assert S.merge_weights({"E_arm": 2.0})["E_arm"] == 2.0
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="E_arm"):
            S.merge_weights({"E_arm": bad})
    plan = S.term_plan({"E_scene": 1.0, "E_approach": 1.0, "E_pregrasp": 1.0, "E_reach": 1.0, "E_arm": 1.0})
    assert plan.term_names.index("E_reach") < plan.term_names.index("E_arm")  # appended after the reach term
    inf = float("inf")
    on = S.TERM_NAMES + S.SCENE_TERMS + S.REACH_TERMS + S.ARM_TERMS
    assert S.select_tolerances(on) == [inf] * 5 + [0.0, inf, 0.0]  # gated at 0 by default, like the other obstacle terms
    assert S.select_tolerances(on, {"E_arm": 1e-3}) == [inf] * 7 + [1e-3]
    off = S.TERM_NAMES + S.SCENE_TERMS + S.REACH_TERMS
    assert S.select_tolerances(off) == [inf] * 5 + [0.0, inf]  # only when the term is on
    with pytest.raises(ValueError, match="E_arm"):
        S.select_tolerances(off, {"E_arm": 0.0})
    # the launch sits right after the reach launch and before the FK backward, not among the obstacle terms (they run before it)
    # (the launch keys are followed by the FK backward: tests/test_gpu_stepper_terms.py)
    at = plan.launch.index
    assert max(at("scene"), at("approach"), at("pregrasp")) < at("reach") < at("arm") and plan.launch[-1] == "arm"
    assert "E_arm" not in S.OBSTACLE_TERMS


def test_stepper_arguments_and_errors():
    from graspqp_amd import ops
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.hands import get_hand_spec
    from graspqp_amd.stepper import GraspStepper

    p = inspect.signature(GraspStepper.__init__).parameters
    assert (p["arm_scene"].default, p["arm_margin"].default, p["arm_damping"].default, p["reach_damping"].default) == (None, None, 1e-6, 1e-4)
    p = inspect.signature(HandModel.set_arm_scene).parameters
    assert (p["scene"].default, p["margin"].default, p["damping"].default) == (None, None, 1e-6)
    # the argument checks come before the stepper touches the device, so stand-ins for the hand and the object set are enough to
    # reach them; no call below has a scene, so each is wrong in a later way too: reach first, then the spheres, then the scene (what
    # follows the scene -- the fall-backs of arm_scene and arm_margin, n_grids, arm_check -- needs a grid: tests/test_gpu_arm.py)
    hand = type("H", (), {"spec": get_hand_spec("allegro"), "L": 1, "J": 16, "S": 0})()
    objs = type("M", (), {"n_mesh": 1})()
    make = lambda **kw: GraspStepper(hand, objs, torch.zeros(1, 8, 3), 4, 4, device="cpu", **kw)
    base = np.eye(4)[:3]
    with_spheres, without = ao.arm_spec("arm7"), ro.arm_spec("arm7")
    with pytest.raises(ValueError, match=r'weights\["E_arm"\] > 0 needs weights\["E_reach"\] > 0'):
        make(weights={"E_arm": 1.0}, arm=with_spheres, arm_base=base)
    with pytest.raises(ValueError, match="collision spheres"):
        make(weights={"E_arm": 1.0, "E_reach": 1.0}, arm=without, arm_base=base)
    with pytest.raises(ValueError, match="arm_scene= or scene="):
        make(weights={"E_arm": 1.0, "E_reach": 1.0}, arm=with_spheres, arm_base=base)
    with pytest.raises(ValueError, match="arm_scene= or scene="):
        make(weights={"E_arm": 1.0, "E_reach": 1.0}, arm=with_spheres, arm_base=base, arm_scene="a shelf")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_arm_terms", 27), ("gq_arm_check", 11), ("gq_reach_terms", 22), ("gq_arm_create", 2)):
        assert name in protos and hasattr(lib, name) and len(protos[name][1]) == n_args, name
    header = open(_C.HEADER_PATH).read()
    i = header.index("E_arm")
    text = header[i:i + 6000]
    for word in ("minimum-norm", "lambda_a / sigma_min^2", "approximation", "log map", "frozen", "redundant", "fp64", "reach_q"):
        assert word in text, word
    names = [a.strip().split(" ")[-1].lstrip("*") for a in
             header[header.index("int gq_arm_terms("):].split(");")[0].split("(", 1)[1].replace("/*", ",/*").split(",") if "/*" not in a and "*/" not in a]
    want = ["arm", "grids", "rows_per_grid", "margin", "damping", "rot_scale", "sphere_link", "sphere_centre", "sphere_radius", "n_spheres",
            "hand_pose", "pose_dim", "Rg", "batch", "base_T", "n_obj", "batch_each", "grasp_axis", "distance", "n_stations", "reach_q",
            "up", "w", "e_arm", "accumulate", "gRt", "stream"]
    assert [n for n in names if n in want] == want, names
    ax = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    g = _C.ClutterGrids()
    g.values, g.n_grids, g.nx, g.ny, g.nz, g.voxel = 8, 1, 4, 4, 4, 0.1
    chk = lambda **kw: lib.gq_arm_check(*[dict(dict(g=ctypes.byref(g), b=8, r=8, n=7, s=19, m=0.01, l=1e-6, rho=0.1, d=0.1, k=2, a=ax), **kw)[x]
                                          for x in ("g", "b", "r", "n", "s", "m", "l", "rho", "d", "k", "a")])
    assert chk() == 0
    for kw, word in ((dict(n=9), b"n_joints"), (dict(s=65), b"n_spheres"), (dict(s=0), b"n_spheres"), (dict(k=4), b"n_stations"),
                     (dict(r=4), b"grids"), (dict(b=0), b"batch"), (dict(a=None), b"grasp_axis")):
        assert chk(**kw) == 2 and b"arm" in lib.gq_last_error() and word in lib.gq_last_error(), (kw, lib.gq_last_error())


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "arm_terms") and hasattr(ns, "arm_terms_backward")
    B = 6
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        for values in (e(24, 24, 20), e(2, 24, 24, 20)):
            args = (1, e(B, 25), e(B, 3, 3), e(2, 3, 4), 3, values, [0.0, 0.0, 0.0], 0.1, [0.0, 0.0, 1.0], 0.1, 2, e(B, 3, 7), 0.01, 1e-6, 0.1)
            E = ns.arm_terms(*args)
            assert E.shape == (B,) and E.dtype == torch.float32
            assert ns.arm_terms_backward(*args, e(B)).shape == (B, 12)


def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills, a wavefront per SIMD and station, 5 KB of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "gq_arm" in k}
    assert sorted(new) == ["gq_arm_kernel"], sorted(new)
    r = new["gq_arm_kernel"]
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["vgpr"] + r["agpr"] <= 128 and r["lds_static"] <= 5120, r


def test_tools_take_the_weight():
    for tool in ("soak.py", "fit_end_to_end.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert "--w_arm" in src, tool
    assert "arm_bench.json" in open(os.path.join(ROOT, "tools", "bench_arm.py")).read()
