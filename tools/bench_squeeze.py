"""Timing and effect of the squeeze term on the bench scene: Allegro, 12 contacts, superquadric objects, 256 rows per
object.  Evidence run, not a test: one JSON record is printed and written to --out.

  launch     gq_squeeze_terms alone (energy, theta, g_theta, g_R and the contact-point gradient in one launch) at 1 x 256 and
             8 x 256 rows, against the composed route of existing launches on the same state: the torch expressions of the motion,
             gq_contact_jacobian, gq_joint_velocities, the torch expressions of r, g, v and dE/dJ, gq_joint_velocities again and
             gq_contact_jacobian_backward (what ops._JointVelocityResiduals runs, without its autograd bookkeeping and without the
             contact-point gradient, which the composed route leaves to autograd).  HIP events around 200 calls per window, the two
             routes alternating, medians of --rounds windows.  Host enqueue time is inside the windows on both sides.
  iteration  captured graphs in alternating windows of --steps replays at 1 x 256 rows: the default five-term stepper and the
             stepper with the weight; ms per iteration and evaluations per second.
  run        --run_iters iterations (default 2 000) of the reference's schedule from one seed without the weight and with each of
             --run_weights; the mean E_squeeze of the accepted states before and after, evaluated by the same launch.

usage: python tools/bench_squeeze.py [--w_squeeze 2000] [--steps 200] [--warmup 24] [--rounds 3] [--run_iters 2000] [--run_weights 2000,100000]
       [--out file.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--w_squeeze", type=float, default=2000.0)
ap.add_argument("--min_travel", type=float, default=5e-3)
ap.add_argument("--damping", type=float, default=1e-3)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--run_iters", type=int, default=2000)
ap.add_argument("--run_weights", default="2000,100000", help="the weights of the runs, beside the run without the term")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "squeeze_bench.json"))
args = ap.parse_args()

from graspqp_amd import _C, ops
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
spec = get_hand_spec("allegro")
hand = ops.HandHandle(spec)
n, BE = args.n_contact, 256
TAU, LAM = args.min_travel, args.damping


def stepper(n_obj, weights=None, seed=3):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    om = ObjectModel(batch_size_each=BE, num_samples=2500)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), BE, n, seed=seed, weights=weights, squeeze_min_travel=TAU,
                      squeeze_damping=LAM)
    st.set_hulls(om.convex_hulls())
    st.initialize()
    return st


def window(fn, n_calls):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n_calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / n_calls  # us


def alternate(fns, n_calls, warm=20):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, n_calls))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


rec = {"squeeze_bench": True, "hand": "allegro", "n_contact": n, "min_travel": TAU, "damping": LAM, "w_squeeze": args.w_squeeze,
       "rounds": args.rounds, "calls_per_window": 200, "device": torch.cuda.get_device_name(0), "launch": {}}

# ---- the launch alone --------------------------------------------------------------------------------------------------------
f32, i64 = _C.f32, _C.i64
for n_obj in (1, 8):
    st = stepper(n_obj)  # its buffers hold the kinematic state and the contact query of the accepted poses
    st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
    B, J = st.B, st.J
    idx, Rg, LT, ws = st.idx_new, st.Rg, st.link_T, st.fk_ws
    z = lambda *s: torch.zeros(*s, device="cuda")
    e, theta, g_theta, g_R, g_cp, g_th2 = z(B), z(B, J), z(B, J), z(B, 9), z(B, n, 3), z(B, J)
    c_up = args.w_squeeze / (3 * n)

    def fused():
        ops._squeeze_call(hand, idx, Rg, LT, ws, st.d2, st.obj_normal, st.closest, st.cpts, TAU, LAM, None, args.w_squeeze, e, theta, 0,
                          g_theta, g_R, None, g_cp)

    def composed():
        R = Rg.view(B, 3, 3)
        d = st.obj_normal * torch.sqrt(st.d2 + 1e-8).clamp(min=TAU).unsqueeze(-1)
        jc = ops.contact_jacobian(hand, idx, LT, ws).reshape(B, 3 * n, J)
        th, res, _ = ops.joint_velocities(jc, d.reshape(B, 3 * n), R, LAM)
        d_h = (R.transpose(1, 2).unsqueeze(1) @ d.unsqueeze(-1)).squeeze(-1).reshape(B, 3 * n)
        r = (jc @ th.unsqueeze(-1)).squeeze(-1) - d_h
        e_c = res.mean(-1)
        g = (2.0 * c_up) * r
        u, _, _ = ops.joint_velocities(jc, g, None, LAM)
        w = g - (jc @ u.unsqueeze(-1)).squeeze(-1)
        GJ = (w.unsqueeze(-1) * th.unsqueeze(1) - r.unsqueeze(-1) * u.unsqueeze(1)).contiguous()
        g_dh = (-w).reshape(B, n, 3)
        gR = (d.unsqueeze(-1) * g_dh.unsqueeze(-2)).sum(1).contiguous()
        _C.call("gq_contact_jacobian_backward", hand.handle, i64(idx), ctypes.c_int64(B), n, f32(LT), f32(GJ), f32(g_th2), _C.ptr(ws),
                ws.numel(), _C.stream_ptr())
        return e_c, gR

    e_c, gR_c = composed()
    fused()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    r = alternate({"gq_squeeze_terms": fused, "composed_route": composed}, 200)
    r.update({"rows": B, "launches_in_composed_route": "4 of csrc/export.hip + about 20 torch launches",
              "E_squeeze_mean": float(e.mean()),
              "agreement": {"E_rel": rel(e, e_c), "g_theta_rel": rel(g_theta, g_th2), "g_R_rel": rel(g_R, gR_c.reshape(B, 9))},
              "fused_over_composed": r["gq_squeeze_terms"]["median_us"] / r["composed_route"]["median_us"]})
    rec["launch"][f"{n_obj}x256"] = r
    print(json.dumps({f"{n_obj}x256": r}), flush=True)
    del st

# ---- the iteration -----------------------------------------------------------------------------------------------------------
steppers = {"default": stepper(1), "squeeze": stepper(1, {"E_squeeze": args.w_squeeze})}
for st in steppers.values():
    st.capture(iters=8 if st._fuse_loop and args.steps % 8 == 0 else 1)
    for _ in range(args.warmup):
        st.step()
    st.realign_draws()
torch.cuda.synchronize()
times = {k: [] for k in steppers}
for _ in range(args.rounds):
    for name, st in steppers.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            st.step()
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
        assert st._graph_pending == 0 and torch.isfinite(st.energy).all()
rec["iteration"] = {k: {"rows": BE, "graph_mode": steppers[k].graph_mode, "terms": len(steppers[k].term_names),
                        "steps_per_window": args.steps, "ms_per_iteration_median": float(np.median(v)), "ms_per_iteration_min": min(v),
                        "ms_per_iteration_max": max(v), "evals_per_s_median": BE / (1e-3 * float(np.median(v)))}
                    for k, v in times.items()}
print(json.dumps({"iteration": rec["iteration"]}), flush=True)

# ---- a run with and without the weight -------------------------------------------------------------------------------------------
probe = stepper(1, {"E_squeeze": args.w_squeeze}, seed=5)  # evaluates E_squeeze at another stepper's accepted state
rec["run"] = {"iterations": args.run_iters, "rows": BE, "reset_epochs": 600}
runs = [("without_weight", None)] + [(f"with_weight_{w:g}", {"E_squeeze": w}) for w in map(float, args.run_weights.split(","))]
for name, weights in runs:
    st = stepper(1, weights, seed=7)
    e0 = probe.evaluate(st.hand_pose, st.contact_idx)[0]["E_squeeze"].mean()
    dis0 = st.terms[0].mean()
    st.capture(iters=8 if st._fuse_loop else 1)
    st.run(args.run_iters, reset_epochs=600, z_score_threshold=1.0)
    terms = probe.evaluate(st.hand_pose, st.contact_idx)[0]
    assert torch.isfinite(st.energy).all()
    rec["run"][name] = {"E_squeeze_mean_initial": float(e0), "E_squeeze_mean_final": float(terms["E_squeeze"].mean()),
                        "E_squeeze_median_final": float(terms["E_squeeze"].median()), "E_dis_mean_initial": float(dis0),
                        "E_dis_mean_final": float(terms["E_dis"].mean()), "E_fc_mean_final": float(terms["E_fc"].mean()),
                        "E_pen_mean_final": float(terms["E_pen"].mean())}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
