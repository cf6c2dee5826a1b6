"""Timing and effect of the reach term on the bench scene: Allegro, 12 contacts, superquadric objects, 256 rows per
object, the ``arm7`` preset with its four seeds.  Evidence run, not a test: one JSON record is printed and written to --out
(profiles/reach_bench.json is such a record).

  launch     gq_reach_terms alone (energy, winning configurations, seeds and the gRt gradient in one launch) at 1 x 256 and 8 x 256
             rows, for K = 0 and K = 2 stations, against the same iteration composed from batched torch ops on the device (fp32: FK
             joint by joint, the log map, the Jacobian, torch.linalg.solve of the 6 x 6, cap and clamp, the minimum over the seeds).
             HIP events around --calls calls per window, the two routes alternating, medians of --rounds windows.  Host enqueue time
             is inside the windows on both sides.
  iteration  captured graphs in alternating windows of --steps replays at 1 x 256 rows: the default five-term stepper and the
             stepper with the term; ms per iteration and evaluations per second.
  run        --run_iters iterations (default 2 000) of the reference's schedule from one seed with weight 0 and with each of
             --run_weights: the mean E_reach, the share of rows under 1e-6 and the other terms, before and after, evaluated by the
             same launch.  --arm_base places the arm so that a good part of the initial rows is out of range.

usage: python tools/bench_reach.py [--steps 200] [--warmup 24] [--rounds 3] [--calls 50] [--run_iters 2000] [--run_weights 100,10000]
       [--arm_base X Y Z YAW] [--out file.json]
"""
import argparse
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
ap.add_argument("--w_reach", type=float, default=1000.0)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--run_iters", type=int, default=2000)
ap.add_argument("--run_weights", default="100,10000", help="the weights of the runs, beside the run without the term")
ap.add_argument("--arm_base", type=float, nargs=4, default=(-0.80, 0.0, -0.3, 0.0), metavar=("X", "Y", "Z", "YAW"))
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "reach_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.arm import arm_from_arg, base_from_arg
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
spec = get_hand_spec("allegro")
hand = ops.HandHandle(spec)
arm_spec = arm_from_arg("arm7")
arm = ops.ArmHandle(arm_spec)
base34 = base_from_arg(args.arm_base)
n, BE = args.n_contact, 256
M, LAM, RHO, CAP = 24, 1e-4, 0.1, 0.5
AXIS = [float(a) for a in spec.grasp_axis]


def stepper(n_obj, weights=None, seed=3, stations=0):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    om = ObjectModel(batch_size_each=BE, num_samples=2500)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), BE, n, seed=seed, weights=weights, arm=arm, arm_base=base34,
                      reach_stations=stations)
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


def alternate(fns, n_calls, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, n_calls))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


# ---- the same iteration from batched torch ops, fp32 on the device ---------------------------------------------------------------
dev = "cuda"
T44 = lambda t34: torch.cat([torch.as_tensor(t34, dtype=torch.float32, device=dev),
                             torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)], 0)
PRE = [T44(t) for t in arm_spec.joint_T]
TOOL = T44(arm_spec.tool_T)
AX = torch.as_tensor(arm_spec.joint_axis, dtype=torch.float32, device=dev)
HAT = torch.stack([torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float32) for a in arm_spec.joint_axis]).to(dev)
LO, HI = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (arm_spec.lower, arm_spec.upper))
SEEDS = torch.as_tensor(arm_spec.seeds, dtype=torch.float32, device=dev)
EYE3, EYE4, EYE6 = (torch.eye(k, device=dev) for k in (3, 4, 6))


def torch_fk(q, base):
    Tc, org, axs = base, [], []
    for j in range(arm_spec.n_joints):  # all revolute
        Mo = EYE4.repeat(q.shape[0], 1, 1)
        Mo[:, :3, :3] = EYE3 + torch.sin(q[:, j])[:, None, None] * HAT[j] + (1 - torch.cos(q[:, j]))[:, None, None] * (HAT[j] @ HAT[j])
        Tc = Tc @ PRE[j] @ Mo
        org.append(Tc[:, :3, 3])
        axs.append(Tc[:, :3, :3] @ AX[j])
    return Tc @ TOOL, torch.stack(org, 1), torch.stack(axs, 1)


def torch_err(Tee, ps, Rs):
    E = Rs @ Tee[:, :3, :3].transpose(1, 2)
    v = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], -1)
    s2 = (v * v).sum(-1)
    s = torch.sqrt(s2.clamp_min(1e-30))
    f = torch.where(s < 1e-6, 1.0 + s2 / 6.0, torch.atan2(s, 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1.0)) / s)
    return torch.cat([ps - Tee[:, :3, 3], RHO * f[:, None] * v], -1)


def torch_reach(t, R, base, K, D=0.10):
    B, S, N = t.shape[0], SEEDS.shape[0], arm_spec.n_joints
    a = torch.tensor(AXIS, device=dev)
    d = torch.tensor([D * k / K if K else 0.0 for k in range(K + 1)], device=dev)
    ps = (t[:, None] - d[None, :, None] * (R @ a)[:, None])[:, :, None].expand(B, K + 1, S, 3).reshape(-1, 3)
    Rs = R[:, None, None].expand(B, K + 1, S, 3, 3).reshape(-1, 3, 3)
    bs = base[:, None, None].expand(B, K + 1, S, 4, 4).reshape(-1, 4, 4)
    q = SEEDS[None, None].expand(B, K + 1, S, N).reshape(-1, N).clone()
    for _ in range(M):
        Tee, org, axs = torch_fk(q, bs)
        e = torch_err(Tee, ps, Rs)
        J = torch.cat([torch.linalg.cross(axs, Tee[:, None, :3, 3] - org, dim=-1), RHO * axs], -1).transpose(1, 2)
        dq = (J.transpose(1, 2) @ torch.linalg.solve(J @ J.transpose(1, 2) + LAM * EYE6, e[:, :, None]))[:, :, 0]
        m = dq.abs().amax(-1, keepdim=True)
        q = torch.minimum(torch.maximum(q + torch.where(m > CAP, dq * (CAP / m), dq), LO), HI)
    e = torch_err(torch_fk(q, bs)[0], ps, Rs)
    return (e * e).sum(-1).reshape(B, K + 1, S).amin(-1).mean(-1)


rec = {"reach_bench": True, "hand": "allegro", "arm": "arm7", "seeds": arm_spec.n_seeds, "iterations": M, "damping": LAM, "rot_scale": RHO,
       "arm_base": list(args.arm_base), "rounds": args.rounds, "calls_per_window": args.calls,
       "device": torch.cuda.get_device_name(0), "launch": {}}

# ---- the launch alone --------------------------------------------------------------------------------------------------------
for n_obj in (1, 8):
    st = stepper(n_obj)
    st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
    B = st.B
    pose, Rg = st.hand_pose.clone(), st.Rg.clone()
    base_T = torch.as_tensor(base34, dtype=torch.float32, device=dev)[None].expand(n_obj, 3, 4).contiguous()
    base44 = T44(base34)[None].expand(B, 4, 4)
    for K in (0, 2):
        e, q, sd, gRt = (torch.zeros(B, device=dev), torch.zeros(B, K + 1, arm.N, device=dev),
                         torch.zeros(B, K + 1, dtype=torch.int32, device=dev), torch.zeros(B, 12, device=dev))

        def fused():
            ops._reach_call(arm, pose, Rg, base_T, BE, AXIS, 0.10, K, M, LAM, RHO, None, args.w_reach, e, q, sd, 0, gRt)

        def composed():
            return torch_reach(pose[:, :3], Rg.view(B, 3, 3), base44, K)

        e_c = composed()
        fused()
        torch.cuda.synchronize()
        r = alternate({"gq_reach_terms": fused, "composed_route": composed}, args.calls)
        conv = e < 1e-8
        r.update({"rows": B, "stations": K, "E_reach_mean": float(e.mean()), "share_under_1e-6": float((e < 1e-6).float().mean()),
                  "agreement_max_abs_dE_on_converged_rows": float((e - e_c)[conv].abs().max()) if conv.any() else None,
                  "agreement_median_rel_dE": float(((e - e_c).abs() / e.clamp_min(1e-12)).median()),
                  "fused_over_composed": r["gq_reach_terms"]["median_us"] / r["composed_route"]["median_us"]})
        rec["launch"][f"{n_obj}x256_K{K}"] = r
        print(json.dumps({f"{n_obj}x256_K{K}": r}), flush=True)
    del st

# ---- the iteration -----------------------------------------------------------------------------------------------------------
steppers = {"default": stepper(1), "reach": stepper(1, {"E_reach": args.w_reach})}
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
probe = stepper(1, {"E_reach": args.w_reach}, seed=5)  # evaluates E_reach at another stepper's accepted state
rec["run"] = {"iterations": args.run_iters, "rows": BE, "reset_epochs": 600}
runs = [("weight_0", None)] + [(f"weight_{w:g}", {"E_reach": w}) for w in map(float, args.run_weights.split(","))]
for name, weights in runs:
    st = stepper(1, weights, seed=7)
    t0 = probe.evaluate(st.hand_pose, st.contact_idx)[0]
    st.capture(iters=8 if st._fuse_loop else 1)
    st.run(args.run_iters, reset_epochs=600, z_score_threshold=1.0)
    t1 = probe.evaluate(st.hand_pose, st.contact_idx)[0]
    assert torch.isfinite(st.energy).all()
    out = {}
    for tag, t in (("initial", t0), ("final", t1)):
        out[f"E_reach_mean_{tag}"] = float(t["E_reach"].mean())
        out[f"share_under_1e-6_{tag}"] = float((t["E_reach"] < 1e-6).float().mean())
        out.update({f"{k}_mean_{tag}": float(t[k].mean()) for k in ("E_dis", "E_fc", "E_pen", "E_spen", "E_joints")})
    rec["run"][name] = out
    print(json.dumps({name: out}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
