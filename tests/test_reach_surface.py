"""The reach term's surface without a GPU: the weight key and its validation, the order of the terms, every validation error of
ops.ArmSpec, ops.reach_check and the stepper's arguments, ArmSpec.from_dh and ArmSpec.from_urdf against hand-written arrays, the C
entries in the header and in the built library, the registered ops, the new kernel's resources, the tools' switches."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import _reach_oracle as ro
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_merge_weights_knows_the_reach_term():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, REACH_TERMS, merge_weights

    assert REACH_TERMS == ("E_reach",)
    w = merge_weights(None)
    assert w["E_reach"] == 0.0 and {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS
    assert merge_weights({"E_reach": 1.0})["E_reach"] == 1.0
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="E_reach"):
            merge_weights({"E_reach": bad})
    with pytest.raises(ValueError, match="e_reach"):
        merge_weights({"e_reach": 1.0})


def test_term_names_order_and_select_tolerances():
    """E_reach is appended last, after E_squeeze; not gated by default (it is no obstacle term)."""
    from graspqp_amd import stepper as S

    plan = S.term_plan({"E_squeeze": 1.0, "E_reach": 1.0})
    assert plan.term_names.index("E_squeeze") < plan.term_names.index("E_reach")
    names = S.TERM_NAMES + S.SCENE_TERMS + S.SQUEEZE_TERMS + S.REACH_TERMS
    inf = float("inf")
    assert S.select_tolerances(names) == [inf] * 5 + [0.0, inf, inf]
    assert S.select_tolerances(names, {"E_reach": 1e-6}) == [inf] * 7 + [1e-6]
    with pytest.raises(ValueError, match="E_reach"):
        S.select_tolerances(S.TERM_NAMES, {"E_reach": 1e-6})  # a gate on the switched-off term
    assert "E_reach" not in S.OBSTACLE_TERMS
    # in reach mode the fused loop is off, and the launch sits between the squeeze launch and the FK backward
    # (the launch keys are followed by the FK backward: tests/test_gpu_stepper_terms.py)
    assert not S.term_plan({"E_reach": 1.0}).fuse_loop
    assert plan.launch.index("squeeze") < plan.launch.index("reach") and plan.launch[-1] == "reach"


def test_arm_spec_validation():
    from graspqp_amd import ops

    types, Ts, axes, lo, hi, tool = ro.arm_arrays("elbow6")
    arm = ops.ArmSpec(types, Ts, axes, lo, hi, tool)
    assert arm.n_joints == 6 and arm.n_seeds == 1 and np.allclose(arm.seeds[0], 0.5 * (lo + hi))  # the mid-range default
    assert arm.joint_T.shape == (6, 3, 4) and arm.tool_T.shape == (3, 4)
    bad = lambda **kw: dict(dict(joint_types=types, joint_T=Ts, joint_axis=axes, lower=lo, upper=hi, tool_T=tool), **kw)
    nan_lo, inf_hi, eq_hi = lo.copy(), hi.copy(), hi.copy()
    nan_lo[1], inf_hi[2], eq_hi[3] = np.nan, np.inf, lo[3]
    zero_axis = axes.copy()
    zero_axis[0] = 0
    for kw, word in ((dict(lower=nan_lo), "finite"), (dict(upper=inf_hi), "finite"), (dict(upper=eq_hi), "lower < upper"),
                     (dict(seeds=np.tile(hi + 0.1, (1, 1))), "inside"), (dict(seeds=np.zeros((9, 6))), "seeds"),
                     (dict(seeds=np.zeros((0, 6))), "seeds"), (dict(seeds=np.zeros((2, 5))), "seeds"),
                     (dict(joint_types=["revolute"] * 5 + ["screw"]), "screw"), (dict(joint_axis=zero_axis), "joint_axis"),
                     (dict(joint_T=Ts[:5]), "joint_T"), (dict(tool_T=np.full((3, 4), np.nan)), "tool_T"), (dict(lower=lo[:5]), "lower")):
        with pytest.raises(ValueError, match=word):
            ops.ArmSpec(**bad(**kw))
    with pytest.raises(ValueError, match="1..8"):
        ops.ArmSpec(["revolute"] * 9, np.tile(np.eye(4), (9, 1, 1)), np.tile([0, 0, 1.0], (9, 1)), [-1] * 9, [1] * 9)
    with pytest.raises(ValueError, match="1..8"):
        ops.ArmSpec([], np.zeros((0, 4, 4)), np.zeros((0, 3)), [], [])
    # 1 <= N <= 8 and 1 <= S <= 8 at their ends
    assert ro.arm_spec("chain8", 8).n_seeds == 8 and ro.arm_spec("chain8").n_joints == 8 and ro.arm_spec("short3").n_joints == 3


def test_reach_check_and_stepper_arguments():
    from graspqp_amd import ops
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.stepper import GraspStepper

    p = inspect.signature(GraspStepper.__init__).parameters
    assert (p["reach_iterations"].default, p["reach_damping"].default, p["reach_rot_scale"].default, p["reach_stations"].default,
            p["reach_distance"].default, p["arm"].default, p["arm_base"].default) == (24, 1e-4, 0.1, 0, 0.10, None, None)
    p = inspect.signature(ops.reach_terms).parameters
    assert list(p)[:10] == ["hand_pose", "hand", "idx", "Rg", "LT", "ws", "arm", "base_T", "batch_each", "grasp_axis"]
    assert (p["iterations"].default, p["damping"].default, p["rot_scale"].default, p["stations"].default, p["distance"].default,
            p["return_q"].default) == (24, 1e-4, 0.1, 0, 0.10, False)
    p = inspect.signature(HandModel.set_reach).parameters
    assert (p["iterations"].default, p["damping"].default, p["rot_scale"].default, p["stations"].default) == (24, 1e-4, 0.1, 0)
    arm = ro.arm_spec("arm7", 4)
    ops.reach_check(arm)
    ops.reach_check(arm, 0.0, 0)  # the distance is not read without stations
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(stations=4), "reach_stations"), (dict(stations=-1), "reach_stations"), (dict(stations=1.5), "reach_stations"),
                     (dict(stations=2, distance=0.0), "reach_distance"), (dict(stations=1, distance=inf), "reach_distance"),
                     (dict(stations=1, distance=nan), "reach_distance"), (dict(iterations=-1), "reach_iterations"),
                     (dict(iterations=5000), "reach_iterations"), (dict(damping=0.0), "reach_damping"), (dict(damping=nan), "reach_damping"),
                     (dict(damping=inf), "reach_damping"), (dict(rot_scale=0.0), "reach_rot_scale"), (dict(rot_scale=nan), "reach_rot_scale"),
                     (dict(grasp_axis=(0, 0, 0)), "grasp_axis"), (dict(grasp_axis=(0, nan, 1)), "grasp_axis")):
        with pytest.raises(ValueError, match=word):
            ops.reach_check(arm, who="GraspStepper", **kw)
    with pytest.raises(ValueError, match="ArmSpec"):
        ops.reach_check("franka")
    # arm_base: (3,4) for every object, or one per object
    assert tuple(ops.reach_base(np.eye(4)[:3], 3).shape) == (3, 3, 4) and tuple(ops.reach_base(np.tile(np.eye(4), (2, 1, 1)), 2).shape) == (2, 3, 4)
    for b, n in ((np.zeros((2, 3, 4)), 3), (np.zeros((3, 3)), 1), (np.full((3, 4), np.nan), 1)):
        with pytest.raises(ValueError, match="arm_base"):
            ops.reach_base(b, n, "GraspStepper")
    # the stepper checks them only when the term is on, and before it touches the device
    # the device: a stand-in hand and CPU tensors get as far as the checks -- the arm, the base, reach_check, then reach_base
    import types

    hand = types.SimpleNamespace(J=16, L=5, S=0, spec=types.SimpleNamespace(grasp_axis=(0.0, 0.0, 1.0)))
    make = lambda **kw: GraspStepper(hand, None, torch.zeros(2, 8, 3), 4, 4, weights={"E_reach": 1.0}, device="cpu", **kw)
    with pytest.raises(ValueError, match="needs arm="):
        make(arm_base=np.eye(4)[:3], reach_stations=7)
    with pytest.raises(ValueError, match="needs arm_base"):
        make(arm=arm, reach_stations=7)
    with pytest.raises(ValueError, match="GraspStepper: reach_stations"):
        make(arm=arm, arm_base=np.zeros((3, 3)), reach_stations=7)  # the base is wrong too: reach_check comes first
    with pytest.raises(ValueError, match="GraspStepper: arm_base"):
        make(arm=arm, arm_base=np.zeros((3, 3, 4)))  # three bases for two objects
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.reach_terms(torch.zeros(2, 25), None, torch.zeros(2, 4, dtype=torch.long), None, None, None, None, None, 1, (0, 0, 1))


def _dh_matrix(a, alpha, d, theta):
    ca, sa, ct, st = np.cos(alpha), np.sin(alpha), np.cos(theta), np.sin(theta)
    return np.array([[ct, -st * ca, st * sa, a * ct], [st, ct * ca, -ct * sa, a * st], [0, sa, ca, d], [0, 0, 0, 1.0]])


def test_from_dh_equals_the_hand_written_arrays():
    from graspqp_amd import ops

    H = np.pi / 2
    a, alpha, d, th0 = [0, -0.425, -0.392, 0, 0, 0], [H, 0, 0, H, -H, 0], [0.163, 0, 0, 0.134, 0.1, 0.1], [0, -H, 0, 0.3, 0, 0]
    lo, hi = [-3.0] * 6, [3.0] * 6
    tool = ro.T((0.01, 0.02, 0.12), (0.1, 0.2, 0.3))
    arm = ops.ArmSpec.from_dh(a, alpha, d, th0, lo, hi, tool_T=tool)
    row = lambda i: ro.T((0, 0, d[i]), (0, 0, th0[i])) @ ro.T((a[i], 0, 0), (alpha[i], 0, 0))
    hand = ops.ArmSpec(["revolute"] * 6, np.stack([np.eye(4)] + [row(i) for i in range(5)]), np.tile([0, 0, 1.0], (6, 1)), lo, hi,
                       row(5) @ tool)
    for k in ("joint_type", "joint_T", "joint_axis", "lower", "upper", "tool_T", "seeds"):
        assert np.allclose(getattr(arm, k), getattr(hand, k), atol=1e-15), k
    rng = np.random.default_rng(0)
    for _ in range(4):  # and both are the textbook product of DH matrices
        q = rng.uniform(lo, hi)
        want = np.eye(4)
        for i in range(6):
            want = want @ _dh_matrix(a[i], alpha[i], d[i], th0[i] + q[i])
        assert np.allclose(arm.fk(q), want @ tool, atol=1e-12)
    pr = ops.ArmSpec.from_dh([0.1, 0.2], [0, H], [0.3, 0.1], [0, 0], [-1, 0], [1, 0.4], joint_types=["revolute", "prismatic"])
    assert np.allclose(pr.fk([0.3, 0.25]), _dh_matrix(0.1, 0, 0.3, 0.3) @ _dh_matrix(0.2, H, 0.1 + 0.25, 0), atol=1e-12)
    with pytest.raises(ValueError, match="same length"):
        ops.ArmSpec.from_dh([0, 0], [0], [0, 0], [0, 0], [-1, -1], [1, 1])


_URDF_ARM7 = """<?xml version="1.0"?>
<robot name="arm7">
  <link name="world"/><link name="l0"/><link name="l1"/><link name="l2"/><link name="l3"/><link name="l4"/><link name="l5"/>
  <link name="l6"/><link name="l7"/><link name="mount"/><link name="flange"/><link name="side"/>
  <joint name="stand" type="fixed"><parent link="world"/><child link="l0"/><origin xyz="0.5 0 0.2" rpy="0 0 1.0"/></joint>
  <joint name="j1" type="revolute"><parent link="l0"/><child link="l1"/><origin xyz="0 0 0.333" rpy="0 0 0"/><axis xyz="0 0 1"/>
    <limit lower="-2.8973" upper="2.8973"/></joint>
  <joint name="j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0 0 0" rpy="-1.5707963267948966 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-1.7628" upper="1.7628"/></joint>
  <joint name="j3" type="revolute"><parent link="l2"/><child link="l3"/><origin xyz="0 -0.316 0" rpy="1.5707963267948966 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-2.8973" upper="2.8973"/></joint>
  <joint name="j4" type="revolute"><parent link="l3"/><child link="l4"/><origin xyz="0.0825 0 0" rpy="1.5707963267948966 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-3.0718" upper="-0.0698"/></joint>
  <joint name="j5" type="revolute"><parent link="l4"/><child link="l5"/><origin xyz="-0.0825 0.384 0" rpy="-1.5707963267948966 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-2.8973" upper="2.8973"/></joint>
  <joint name="j6" type="revolute"><parent link="l5"/><child link="l6"/><origin xyz="0 0 0" rpy="1.5707963267948966 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-0.0175" upper="3.7525"/></joint>
  <joint name="mount_fix" type="fixed"><parent link="l6"/><child link="mount"/><origin xyz="0.088 0 0"/></joint>
  <joint name="j7" type="revolute"><parent link="mount"/><child link="l7"/><origin rpy="1.5707963267948966 0 0"/>
    <axis xyz="0 0 2"/><limit lower="-2.8973" upper="2.8973"/></joint>
  <joint name="flange_fix" type="fixed"><parent link="l7"/><child link="flange"/><origin xyz="0 0 0.107"/></joint>
  <joint name="camera" type="fixed"><parent link="l4"/><child link="side"/><origin xyz="0 0.1 0"/></joint>
</robot>
"""


def test_from_urdf_equals_the_hand_written_arrays(tmp_path):
    from graspqp_amd import ops

    path = tmp_path / "arm7.urdf"
    path.write_text(_URDF_ARM7)
    want = ro.arm_spec("arm7")
    arm = ops.ArmSpec.from_urdf(str(path), "flange", "l0")  # a fixed joint folded into j7's transform, one into the tool
    for k in ("joint_type", "joint_T", "joint_axis", "lower", "upper", "tool_T", "seeds"):
        assert np.allclose(getattr(arm, k), getattr(want, k), atol=1e-15), k
    # without base_link the walk goes on to the root: the stand is folded into the first joint's transform
    full = ops.ArmSpec.from_urdf(str(path), "flange")
    q = want.seeds[0] + 0.1
    assert np.allclose(full.fk(q), ro.T((0.5, 0, 0.2), (0, 0, 1.0)) @ want.fk(q), atol=1e-12)
    assert ops.ArmSpec.from_urdf(str(path), "l4", "l1").n_joints == 3
    for tip, base, word in (("nowhere", None, "no link"), ("flange", "side", "not an ancestor"), ("l0", "l0", "no moving joint")):
        with pytest.raises(ValueError, match=word):
            ops.ArmSpec.from_urdf(str(path), tip, base)
    # nine moving joints are refused, a continuous joint too
    links = "".join(f'<link name="k{i}"/>' for i in range(10))
    joints = "".join(f'<joint name="r{i}" type="revolute"><parent link="k{i}"/><child link="k{i + 1}"/><axis xyz="0 0 1"/>'
                     f'<limit lower="-1" upper="1"/></joint>' for i in range(9))
    nine = tmp_path / "nine.urdf"
    nine.write_text(f'<robot name="nine">{links}{joints}</robot>')
    with pytest.raises(ValueError, match="9 moving joints"):
        ops.ArmSpec.from_urdf(str(nine), "k9")
    assert ops.ArmSpec.from_urdf(str(nine), "k8").n_joints == 8
    cont = tmp_path / "cont.urdf"
    cont.write_text('<robot name="c"><link name="a"/><link name="b"/><joint name="w" type="continuous"><parent link="a"/>'
                    '<child link="b"/></joint></robot>')
    with pytest.raises(ValueError, match="continuous"):
        ops.ArmSpec.from_urdf(str(cont), "b")
    # malformed joints raise ValueError too: no <child>, and a <mimic> joint (coupled joints are not supported)
    for body, word in (('<joint name="w" type="revolute"><parent link="a"/><limit lower="-1" upper="1"/></joint>', "lacks"),
                       ('<joint name="w" type="revolute"><parent link="a"/><child link="b"/><limit lower="-1" upper="1"/>'
                        '<mimic joint="v"/></joint>', "mimic")):
        bad = tmp_path / "bad.urdf"
        bad.write_text(f'<robot name="c"><link name="a"/><link name="b"/>{body}</robot>')
        with pytest.raises(ValueError, match=word):
            ops.ArmSpec.from_urdf(str(bad), "b")


def test_header_declares_and_library_exports_the_entries():
    protos = _C.parse_header()
    lib = _C.lib()
    for name, n_args in (("gq_reach_terms", 22), ("gq_reach_check", 8), ("gq_arm_create", 2), ("gq_arm_destroy", 1)):
        assert name in protos and hasattr(lib, name) and len(protos[name][1]) == n_args, name
    header = open(_C.HEADER_PATH).read()
    i = header.index("E_reach")
    assert "envelope" in header[i:i + 4000] and "approximation" in header[i:i + 4000]  # what the gradient is, and where it is not
    for name, n_args in (("gq_scene_total", 5), ("gq_fk_backward", 20), ("gq_squeeze_terms", 24), ("gq_approach_terms", 21)):
        assert len(protos[name][1]) == n_args, name  # the entries the term stands beside are what they were
    # the parameter check of the library, without a GPU
    import ctypes

    ax = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    assert lib.gq_reach_check(7, 4, 0.1, 2, 24, 1e-4, 0.1, ax) == 0
    assert lib.gq_reach_check(9, 4, 0.1, 2, 24, 1e-4, 0.1, ax) == 2 and b"n_joints" in lib.gq_last_error()
    assert lib.gq_reach_check(7, 9, 0.1, 2, 24, 1e-4, 0.1, ax) == 2 and b"n_seeds" in lib.gq_last_error()
    assert lib.gq_reach_check(7, 4, 0.1, 4, 24, 1e-4, 0.1, ax) == 2 and b"n_stations" in lib.gq_last_error()


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "reach_terms") and hasattr(ns, "reach_terms_backward")
    stand_in = type("A", (), {"N": 7})()  # what the fake kernels read of an arm: its joints
    hid = ops._register_handle(stand_in)
    B = 6
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        args = (hid, e(B, 25), e(B, 3, 3), e(2, 3, 4), 3, [0.0, 0.0, 1.0], 0.1, 2, 24, 1e-4, 0.1)
        E, q, seed = ns.reach_terms(*args)
        assert E.shape == (B,) and q.shape == (B, 3, 7) and seed.shape == (B, 3) and seed.dtype == torch.int32
        assert ns.reach_terms_backward(*args, e(B)).shape == (B, 12)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills, four wavefronts per SIMD, under 2 KB of LDS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "reach" in k}
    assert sorted(new) == ["gq_reach_kernel"], sorted(new)
    r = new["gq_reach_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["vgpr"] + r["agpr"] <= 128 and r["lds_static"] <= 2048, r


def test_tools_take_the_weight():
    for tool in ("soak.py", "fit_end_to_end.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert "--w_reach" in src and "--arm" in src, tool
    assert "reach_bench.json" in open(os.path.join(ROOT, "tools", "bench_reach.py")).read()
