"""The surface of the approach tracking term without a GPU: weights and term order, the parameter checks of the library, of
ops.track_check and of the stepper's arguments, the registered ops with their fake kernels, the new kernel's resources, and
export_poses / snapshot_dicts with an arm path, with and without a selection."""
import ctypes
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

import _reach_oracle as ro
from graspqp_amd import _C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "graspqp_amd", "lib", "libgraspqp_hip.so")


def test_merge_weights_and_term_order():
    from graspqp_amd import stepper as S

    assert S.TRACK_TERMS == ("E_track",)
    w = S.merge_weights(None)
    assert w["E_track"] == 0.0 and {k: w[k] for k in S.DEFAULT_WEIGHTS} == S.DEFAULT_WEIGHTS  # no default weight
    assert S.merge_weights({"E_track": 2.0})["E_track"] == 2.0
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="E_track"):
            S.merge_weights({"E_track": bad})
    # appended after ARM_TERMS; not gated by default, gated on request, refused when switched off
    plan = S.term_plan({"E_reach": 1.0, "E_arm": 1.0, "E_track": 1.0})
    assert plan.term_names.index("E_arm") < plan.term_names.index("E_track")
    names = S.TERM_NAMES + S.REACH_TERMS + S.ARM_TERMS + S.TRACK_TERMS
    inf = float("inf")
    assert S.select_tolerances(names) == [inf] * 6 + [0.0, inf]
    assert S.select_tolerances(names, {"E_track": 1e-6}) == [inf] * 7 + [1e-6]
    with pytest.raises(ValueError, match="E_track"):
        S.select_tolerances(S.TERM_NAMES + S.REACH_TERMS, {"E_track": 1e-6})
    # the launch order: reach, track, arm, FK backward
    assert plan.launch == ("reach", "track", "arm")  # (followed by the FK backward: tests/test_gpu_stepper_terms.py)
    p = inspect.signature(S.GraspStepper.__init__).parameters
    assert (p["track_waypoints"].default, p["track_updates"].default, p["arm_on_track"].default) == (8, 3, False)


def test_library_check_names_the_argument():
    protos, lib = _C.parse_header(), _C.lib()
    for name, n_args in (("gq_track_terms", 27), ("gq_track_check", 9)):
        assert name in protos and hasattr(lib, name) and len(protos[name][1]) == n_args, name
    for name, n_args in (("gq_reach_terms", 22), ("gq_arm_terms", 27), ("gq_scene_total", 5)):
        assert len(protos[name][1]) == n_args, name  # the entries the term stands beside are what they were
    header = open(_C.HEADER_PATH).read()
    i = header.index("E_track")
    assert "fixed point" in header[i:i + 5000] and "approximation" in header[i:i + 5000]  # what the gradient is, and where it is not
    ax = (ctypes.c_float * 3)(0.0, 0.0, 1.0)
    nan, inf = float("nan"), float("inf")

    def check(N=7, D=0.1, T=8, U=3, lam=1e-4, rho=0.1, K=0, sq=0, a=ax):
        return lib.gq_track_check(N, D, T, U, lam, rho, K, sq, a)

    assert check() == 0 and check(T=1, U=1) == 0 and check(T=64, U=16, K=2, sq=1) == 0 and check(T=7, K=2) == 0
    for kw, word in ((dict(N=0), b"n_joints"), (dict(N=9), b"n_joints"), (dict(T=0), b"n_waypoints"), (dict(T=65), b"n_waypoints"),
                     (dict(U=0), b"n_updates"), (dict(U=17), b"n_updates"), (dict(D=0.0), b"distance"), (dict(D=inf), b"distance"),
                     (dict(D=nan), b"distance"), (dict(lam=0.0), b"damping"), (dict(lam=inf), b"damping"), (dict(rho=0.0), b"rot_scale"),
                     (dict(rho=nan), b"rot_scale"), (dict(K=-1), b"n_stations"), (dict(K=4), b"n_stations"),
                     (dict(T=7, K=2, sq=1), b"track_station_q"), (dict(K=0, sq=1), b"track_station_q"),
                     (dict(a=(ctypes.c_float * 3)(0.0, 0.0, 0.0)), b"grasp_axis"), (dict(a=(ctypes.c_float * 3)(0.0, nan, 1.0)), b"grasp_axis")):
        assert check(**kw) == 2, kw
        msg = lib.gq_last_error()
        assert b"track" in msg and word in msg, (kw, msg)


def test_track_check_and_ops_signature():
    from graspqp_amd import ops
    from graspqp_amd.core.hand_model import HandModel

    p = inspect.signature(ops.track_terms).parameters
    assert list(p)[:11] == ["hand_pose", "hand", "idx", "Rg", "LT", "ws", "arm", "base_T", "batch_each", "grasp_axis", "q_start"]
    assert (p["waypoints"].default, p["updates"].default, p["return_path"].default, p["damping"].default, p["rot_scale"].default) == \
        (8, 3, False, 1e-4, 0.1)
    p = inspect.signature(HandModel.set_track).parameters
    assert (p["waypoints"].default, p["updates"].default) == (8, 3)
    arm = ro.arm_spec("arm7", 4)
    ops.track_check(arm)
    ops.track_check(arm, stations=2, with_station_q=True)
    for kw, word in ((dict(waypoints=0), "n_waypoints"), (dict(waypoints=65), "n_waypoints"), (dict(waypoints=2.5), "track_waypoints"),
                     (dict(updates=0), "n_updates"), (dict(updates=17), "n_updates"), (dict(updates=1.5), "track_updates"),
                     (dict(distance=0.0), "distance"), (dict(damping=0.0), "damping"), (dict(rot_scale=float("nan")), "rot_scale"),
                     (dict(stations=3, with_station_q=True), "track_station_q"), (dict(grasp_axis=(0, 0, 0)), "grasp_axis")):
        with pytest.raises(ValueError, match=word) as err:
            ops.track_check(arm, who="GraspStepper", **kw)
        assert "GraspStepper" in str(err.value)
    with pytest.raises(ValueError, match="ArmSpec"):
        ops.track_check("franka")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.track_terms(torch.zeros(2, 25), None, torch.zeros(2, 4, dtype=torch.long), None, None, None, None, None, 1, (0, 0, 1),
                        torch.zeros(2, 7))
    hm = types.SimpleNamespace(reach=None, grasp_axis=(0.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="set_reach"):
        HandModel.set_track(hm)
    hm.reach = (arm, None, 0.1, 0, 24, 1e-4, 0.1)
    with pytest.raises(ValueError, match="stations >= 1"):
        HandModel.set_track(hm)
    hm.reach = (arm, None, 0.1, 2, 24, 1e-4, 0.1)
    with pytest.raises(ValueError, match="n_waypoints"):
        HandModel.set_track(hm, waypoints=0)
    HandModel.set_track(hm, 4, 2)
    assert hm.track == (4, 2)


def test_stepper_argument_errors_come_before_the_device():
    """The stepper refuses a track weight without what it needs, naming it, before it touches the device: a stand-in hand and CPU
    tensors get as far as the checks."""
    from graspqp_amd.stepper import GraspStepper

    arm = ro.arm_spec("arm7", 4)
    hand = types.SimpleNamespace(J=16, L=5, S=0, spec=types.SimpleNamespace(grasp_axis=(0.0, 0.0, 1.0)))
    sp = torch.zeros(2, 8, 3)

    def make(weights, **kw):
        return GraspStepper(hand, None, sp, 4, 4, weights=weights, device="cpu", **kw)

    reach = dict(arm=arm, arm_base=np.eye(4)[:3], reach_stations=2)
    with pytest.raises(ValueError, match="E_reach"):
        make({"E_track": 1.0})
    with pytest.raises(ValueError, match="reach_stations >= 1"):
        make({"E_track": 1.0, "E_reach": 1.0}, arm=arm, arm_base=np.eye(4)[:3], reach_stations=0)
    with pytest.raises(ValueError, match="n_waypoints"):
        make({"E_track": 1.0, "E_reach": 1.0}, track_waypoints=65, **reach)
    with pytest.raises(ValueError, match="n_updates"):
        make({"E_track": 1.0, "E_reach": 1.0}, track_updates=0, **reach)
    with pytest.raises(ValueError, match="arm_on_track"):
        make({"E_reach": 1.0}, arm_on_track=True, **reach)  # neither term on
    with pytest.raises(ValueError, match="arm_on_track"):
        make({"E_reach": 1.0, "E_track": 1.0}, arm_on_track=True, **reach)  # E_arm off
    # (ops.track_check raised the n_waypoints / n_updates errors above on the CPU; the divisor rule of arm_on_track needs E_arm on,
    # which needs a grid: tests/test_gpu_track.py::test_arm_on_track_feeds_the_arm_term_the_path)


def test_ops_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from graspqp_amd import ops

    ns = torch.ops.graspqp_amd
    assert hasattr(ns, "track_terms") and hasattr(ns, "track_terms_backward")
    stand_in = type("A", (), {"N": 7})()  # what the fake kernels read of an arm: its joints
    hid = ops._register_handle(stand_in)
    B = 6
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        args = (hid, e(B, 25), e(B, 3, 3), e(2, 3, 4), 3, [0.0, 0.0, 1.0], 0.1, 8, 3, 1e-4, 0.1, e(B, 7))
        E, q, worst, step, sq = ns.track_terms(*args, 2)
        assert E.shape == (B,) and q.shape == (B, 9, 7) and worst.shape == (B,) and step.shape == (B,) and sq.shape == (B, 3, 7)
        assert ns.track_terms(*args, 0)[4].shape == (B, 0, 7)
        assert ns.track_terms_backward(*args, e(B)).shape == (B, 12)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_new_kernel_resources():
    """The one new kernel: one wavefront per block, no LDS, no scratch, no spills."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "track" in k}
    assert sorted(new) == ["gq_track_kernel"], sorted(new)
    r = new["gq_track_kernel"]
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r.get("sgpr_spills", 0) == 0, r
    assert r["lds_static"] == 0 and r["max_threads"] == 64 and r["vgpr"] + r["agpr"] <= 256, r  # two wavefronts per SIMD at least


def test_tools_take_the_weight():
    for tool in ("soak.py", "fit_end_to_end.py"):
        src = open(os.path.join(ROOT, "tools", tool)).read()
        assert "--w_track" in src and "--track_waypoints" in src and "--arm_on_track" in src, tool
    assert "track_bench.json" in open(os.path.join(ROOT, "tools", "bench_track.py")).read()


# ---- export ------------------------------------------------------------------------------------------------------------------------
def _snapshot_inputs(monkeypatch, B, J):
    """A stand-in hand model and a patched grasp_snapshot: snapshot_dicts reads nothing else."""
    from graspqp_amd import export

    names = [f"j{i}" for i in range(J)]
    snap = {"joint_positions": torch.arange(B * J, dtype=torch.float32).view(B, J), "root_pose": torch.arange(B * 7.0).view(B, 7),
            "values": torch.arange(B, dtype=torch.float32), "contact_idx": torch.arange(B * 4).view(B, 4)}
    for key in ("grasp_velocities", "full_grasp_velocities", "grasp_velocities_off"):
        snap[key] = torch.zeros(B, J)
    monkeypatch.setattr(export, "grasp_snapshot", lambda hm, energy, om: snap)
    return export, types.SimpleNamespace(_actuated_joints_names=names, _contact_links=["a"])


def test_export_arm_path_with_and_without_a_selection(monkeypatch, tmp_path):
    n_obj, be, T, N = 2, 4, 3, 7
    B = n_obj * be
    export, hm = _snapshot_inputs(monkeypatch, B, 5)
    path = torch.arange(B * (T + 1) * N, dtype=torch.float32).view(B, T + 1, N)
    plain = export.snapshot_dicts(hm, None, None, n_obj, be)
    assert all("arm_path" not in d for d in plain)  # absent: the dicts are what they were
    dicts = export.snapshot_dicts(hm, None, None, n_obj, be, arm_path=path)
    for a, d in enumerate(dicts):
        assert torch.equal(d["arm_path"], path[a * be:(a + 1) * be]) and torch.equal(d["values"], plain[a]["values"])
    # under a selection: the selected rows, in pick order
    sel = types.SimpleNamespace(sel=torch.tensor([[2, 0, 3, 1], [7, 5, 4, 6]], dtype=torch.int32), n_selected=torch.tensor([3, 1]),
                                n_feasible=torch.tensor([4, 2]))
    dicts = export.snapshot_dicts(hm, None, None, n_obj, be, selection=sel, arm_path=path)
    assert torch.equal(dicts[0]["arm_path"], path[[2, 0, 3]]) and torch.equal(dicts[1]["arm_path"], path[[7]])
    assert dicts[0]["selected_rows"].tolist() == [2, 0, 3] and dicts[1]["selected_rows"].tolist() == [3]
    assert torch.equal(dicts[0]["values"], torch.tensor([2.0, 0.0, 3.0]))
    for bad in (path[:-1], path[:, 0]):
        with pytest.raises(ValueError, match="arm_path"):
            export.snapshot_dicts(hm, None, None, n_obj, be, arm_path=bad)
    # export_poses passes it on and the file holds it
    files = export.export_poses(hm, None, None, ["objA", "objB"], be, str(tmp_path), "allegro", 4, "graspqp", selection=sel, arm_path=path)
    data = torch.load(files[0], weights_only=False)
    assert torch.equal(data["arm_path"], path[[2, 0, 3]])
    assert "arm_path" not in torch.load(export.export_poses(hm, None, None, ["objA", "objB"], be, str(tmp_path), "allegro", 4, "graspqp",
                                                            suffix="_plain")[0], weights_only=False)
