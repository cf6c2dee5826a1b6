"""The squeeze term's surface without a GPU: the weight key and its validation, the parameters of the stepper, the op and the class
surface, the order of the terms, the C entry in the header and in the built library, the registered ops, the new kernel's resources.
E_manipulativity stays what it was: refused as a stepper weight."""
import inspect
import os
import sys

import pytest
import torch

from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_merge_weights_knows_the_squeeze_term():
    from graspqp_amd.stepper import DEFAULT_WEIGHTS, SQUEEZE_TERMS, merge_weights

    assert SQUEEZE_TERMS == ("E_squeeze",)
    w = merge_weights(None)
    assert w["E_squeeze"] == 0.0 and {k: w[k] for k in DEFAULT_WEIGHTS} == DEFAULT_WEIGHTS
    assert merge_weights({"E_squeeze": 250.0})["E_squeeze"] == 250.0
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="E_squeeze"):
            merge_weights({"E_squeeze": bad})
    with pytest.raises(ValueError, match="E_manipulativity"):  # the reference's name stays an unknown key of the stepper
        merge_weights({"E_manipulativity": 1.0})
    with pytest.raises(ValueError, match="e_squeeze"):
        merge_weights({"e_squeeze": 1.0})


def test_term_names_order_and_select_tolerances():
    """E_squeeze is appended last, after E_pregrasp (the stepper builds term_names in this order); not gated by default."""
    from graspqp_amd import stepper as S

    on = S.term_plan({"E_pregrasp": 1.0, "E_squeeze": 1.0}).term_names
    assert on.index("E_pregrasp") < on.index("E_squeeze")
    names = S.TERM_NAMES + S.SCENE_TERMS + S.PREGRASP_TERMS + S.SQUEEZE_TERMS
    inf = float("inf")
    assert S.select_tolerances(names) == [inf] * 5 + [0.0, 0.0, inf]
    assert S.select_tolerances(names, {"E_squeeze": 1e-4}) == [inf] * 7 + [1e-4]
    with pytest.raises(ValueError, match="E_squeeze"):
        S.select_tolerances(S.TERM_NAMES, {"E_squeeze": 1e-4})  # a gate on the switched-off term
    assert "E_squeeze" not in S.OBSTACLE_TERMS


def test_parameters_are_validated():
    from graspqp_amd import ops
    from graspqp_amd.core.hand_model import HandModel
    from graspqp_amd.stepper import GraspStepper

    p = inspect.signature(GraspStepper.__init__).parameters
    assert p["squeeze_min_travel"].default == 5e-3 and p["squeeze_damping"].default == 1e-3
    p = inspect.signature(ops.squeeze_terms).parameters
    assert list(p)[:10] == ["hand_pose", "hand", "idx", "Rg", "LT", "ws", "dist_sq", "obj_normal", "closest", "contact_pts"]
    assert p["min_travel"].default == 5e-3 and p["damping"].default == 1e-3
    p = inspect.signature(HandModel.set_squeeze).parameters
    assert p["min_travel"].default == 5e-3 and p["damping"].default == 1e-3
    ops.squeeze_check(None, 1, 5e-3, 1e-3)
    for tau, lam, word in ((0.0, 1e-3, "min_travel"), (-1e-3, 1e-3, "min_travel"), (float("inf"), 1e-3, "min_travel"),
                           (float("nan"), 1e-3, "min_travel"), (5e-3, 0.0, "damping"), (5e-3, -1.0, "damping"),
                           (5e-3, float("inf"), "damping"), (5e-3, float("nan"), "damping")):
        with pytest.raises(ValueError, match=word):
            ops.squeeze_check(None, 1, tau, lam, "GraspStepper")
    # the stepper checks them only when the term is on, and before it touches the device
    # the device: a stand-in hand and CPU tensors get as far as the check
    from graspqp_amd.hands import get_hand_spec

    hand = type("H", (), {"spec": get_hand_spec("allegro"), "L": 1, "J": 16, "S": 0})()
    make = lambda **kw: GraspStepper(hand, None, torch.zeros(1, 8, 3), 4, 4, device="cpu", **kw)
    with pytest.raises(ValueError, match="GraspStepper: squeeze_damping"):
        make(weights={"E_squeeze": 1.0}, squeeze_damping=0.0)
    with pytest.raises(ValueError, match="GraspStepper: squeeze_min_travel"):
        make(weights={"E_squeeze": 1.0}, squeeze_min_travel=float("nan"))
    with pytest.raises(ValueError, match="init_avoid_scene"):  # with the term off they are not read: a later wrong argument raises
        make(weights={"E_squeeze": 0.0}, squeeze_damping=0.0, init_avoid_scene=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.squeeze_terms(torch.zeros(2, 25), None, torch.zeros(2, 4, dtype=torch.long), None, None, None, None, None, None, None)


def test_header_declares_and_library_exports_the_entry():
    protos = _C.parse_header()
    lib = _C.lib()
    assert "gq_squeeze_terms" in protos and hasattr(lib, "gq_squeeze_terms")
    assert len(protos["gq_squeeze_terms"][1]) == 24
    header = open(_C.HEADER_PATH).read()
    i = header.index("E_squeeze")
    assert "core/energy.py:80-87" in header[i:i + 800] and "hand_model.py:1155-1218" in header[i:i + 800]  # its reference call sites
    for name, n_args in (("gq_scene_total", 5), ("gq_fk_backward", 20), ("gq_contact_jacobian", 9), ("gq_joint_velocities", 11),
                         ("gq_contact_jacobian_backward", 10), ("gq_pregrasp_terms", 23)):
        assert len(protos[name][1]) == n_args, name  # the entries the term stands beside are what they were


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops
    from graspqp_amd.hands import get_hand_spec

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "squeeze_terms") and hasattr(ns, "squeeze_terms_backward")
    stand_in = type("H", (), {"J": 16})()  # what the fake kernels read of a hand: its actuated joints
    hid = ops._register_handle(stand_in)
    B, n, L = 6, 5, 22
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        args = (hid, e(B, n, dtype=torch.long), e(B, 3, 3), e(B, L, 3, 4), e(64, dtype=torch.uint8), e(B, n), e(B, n, 3))
        E, th = ns.squeeze_terms(*args, 5e-3, 1e-3)
        assert E.shape == (B,) and th.shape == (B, 16)
        g_theta, g_R, g_cp = ns.squeeze_terms_backward(*args, e(B, n, 3), e(B, n, 3), 5e-3, 1e-3, e(B))
        assert g_theta.shape == (B, 16) and g_R.shape == (B, 3, 3) and g_cp.shape == (B, n, 3)
    assert get_hand_spec("allegro").n_dofs == 16


def test_new_kernel_resources():
    """The one new kernel: no scratch, no spills, four wavefronts per SIMD; the static LDS beside the dynamic normal matrix."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "squeeze" in k}
    assert sorted(new) == ["gq_squeeze_kernel"], sorted(new)
    r = new["gq_squeeze_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["vgpr"] + r["agpr"] <= 128, r
    assert r["lds_static"] + 64 * 65 * 8 <= 64 * 1024, r  # with the largest normal matrix still within 64 KB


def test_tools_take_the_weight():
    for tool in ("soak.py", "fit_end_to_end.py"):
        assert "--w_squeeze" in open(os.path.join(ROOT, "tools", tool)).read(), tool
    assert "squeeze_bench.json" in open(os.path.join(ROOT, "tools", "bench_squeeze.py")).read()
