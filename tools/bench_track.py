"""Timing and effect of the approach tracking term on the bench scene: Allegro, 12 contacts, superquadric objects, 256
rows per object, the ``arm7`` preset with its four seeds and its link spheres, the shelf board of tools/bench_arm.py as the arm's
scene, K = 2 stations.  Evidence run, not a test: one JSON record is printed and written to --out (profiles/track_bench.json is such
a record).

  launch     gq_track_terms alone (energy, path, worst waypoint, largest move and the gRt gradient in one launch) at 1 x 256 and
             8 x 256 rows for (T, U) = (8, 3) and (4, 2): eager, replayed from a graph of --graph_calls launches, and against the same
             tracking composed from batched torch ops on the device (fp32: FK joint by joint, the log map, the Jacobian,
             torch.linalg.solve of the 6 x 6, cap and clamp, waypoint after waypoint), and beside gq_reach_terms (M = 24, K = 2) in the
             same call.  HIP events around the calls of a window, the routes alternating, medians of --rounds windows; host enqueue
             time is inside the eager windows.  Time per dependent pass: the launch over (T + 1)(U + 1) FK passes, the reach launch
             over M + 1.
  iteration  captured graphs in alternating windows of --steps replays at 1 x 256 rows: E_reach + E_arm, and the same with E_track.
  run        --run_iters iterations (default 2 000) of the reference's schedule from one seed: without the term, with --w_track, and
             with --w_track and arm_on_track; the share of rows with track_worst < 1e-6, with track_step < 0.3, and the other terms,
             before and after, evaluated by the same probe.

usage: python tools/bench_track.py [--steps 200] [--warmup 24] [--rounds 5] [--calls 200] [--composed_calls 3] [--run_iters 2000]
       [--w_track 10000] [--out file.json]
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
ap.add_argument("--w_reach", type=float, default=1e4)
ap.add_argument("--w_arm", type=float, default=100.0)
ap.add_argument("--w_track", type=float, default=1e4)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--composed_calls", type=int, default=3)
ap.add_argument("--graph_calls", type=int, default=50)
ap.add_argument("--graph_replays", type=int, default=10)
ap.add_argument("--run_iters", type=int, default=2000)
ap.add_argument("--arm_base", type=float, nargs=4, default=(-0.45, 0.0, -0.3, 0.0), metavar=("X", "Y", "Z", "YAW"))
ap.add_argument("--shelf_z", type=float, default=0.22)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "track_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.arm import arm_from_arg, base_from_arg
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
dev = "cuda"
spec = get_hand_spec("allegro")
hand = ops.HandHandle(spec)
arm_spec = arm_from_arg("arm7").with_link_spheres(0.05, 0.08)
arm = ops.ArmHandle(arm_spec)
base34 = base_from_arg(args.arm_base)
n, BE, K = args.n_contact, 256, 2
M, LAM, RHO, CAP, D = 24, 1e-4, 0.1, 0.5, 0.10
AXIS = [float(a) for a in spec.grasp_axis]
SHAPES = ((8, 3), (4, 2))

# the scene of tools/bench_arm.py: a shelf board 2 cm thick over the object
ORIGIN, SHAPE, VOXEL = (-0.8, -0.6, -0.5), (57, 49, 49), 0.025
ax = [ORIGIN[i] + VOXEL * torch.arange(SHAPE[i], dtype=torch.float64) for i in range(3)]
X = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)
d = (X - torch.tensor([0.0, 0.0, args.shelf_z], dtype=torch.float64)).abs() - torch.tensor([0.45, 0.45, 0.01], dtype=torch.float64)
scene = ops.SceneSDF((d.clamp_min(0).norm(dim=-1) + d.amax(-1).clamp_max(0)).to(torch.float32).to(dev), ORIGIN, VOXEL)


def stepper(n_obj, weights=None, seed=3, T=8, U=3, **kw):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    om = ObjectModel(batch_size_each=BE, num_samples=2500)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), BE, n, seed=seed, weights=weights, arm=arm, arm_base=base34,
                      reach_stations=K, reach_distance=D, arm_scene=scene, arm_margin=0.01, track_waypoints=T, track_updates=U, **kw)
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


def alternate(fns, warm=2):
    """fns: name -> (callable, calls per window, launches per call)"""
    for fn, _, _ in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, (fn, calls, per) in fns.items():
            out[k].append(window(fn, calls) / per)
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def graphed(fn, n_launches):
    """A captured graph of n_launches calls of fn on a side stream."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n_launches):
            fn()
    return g


# ---- the same tracking from batched torch ops, fp32 on the device ------------------------------------------------------------------
T44 = lambda t34: torch.cat([torch.as_tensor(t34, dtype=torch.float32, device=dev), torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)], 0)
PRE = [T44(t) for t in arm_spec.joint_T]
TOOL = T44(arm_spec.tool_T)
AX = torch.as_tensor(arm_spec.joint_axis, dtype=torch.float32, device=dev)
HAT = torch.stack([torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float32) for a in arm_spec.joint_axis]).to(dev)
LO, HI = (torch.as_tensor(v, dtype=torch.float32, device=dev) for v in (arm_spec.lower, arm_spec.upper))
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


def torch_track(t, R, base, q0, T, U):
    a = torch.tensor(AXIS, device=dev)
    Ra, q, Es = R @ a, q0.clone(), []
    for i in range(T + 1):
        ps = t - (D * (T - i) / T) * Ra
        for _ in range(U):
            Tee, org, axs = torch_fk(q, base)
            e = torch_err(Tee, ps, R)
            J = torch.cat([torch.linalg.cross(axs, Tee[:, None, :3, 3] - org, dim=-1), RHO * axs], -1).transpose(1, 2)
            dq = (J.transpose(1, 2) @ torch.linalg.solve(J @ J.transpose(1, 2) + LAM * EYE6, e[:, :, None]))[:, :, 0]
            m = dq.abs().amax(-1, keepdim=True)
            q = torch.minimum(torch.maximum(q + torch.where(m > CAP, dq * (CAP / m), dq), LO), HI)
        e = torch_err(torch_fk(q, base)[0], ps, R)
        Es.append((e * e).sum(-1))
    return torch.stack(Es, 1).mean(-1)


rec = {"track_bench": True, "hand": "allegro", "arm": "arm7", "seeds": arm_spec.n_seeds, "stations": K, "distance": D, "damping": LAM,
       "rot_scale": RHO, "arm_base": list(args.arm_base), "rounds": args.rounds, "calls_per_window": args.calls,
       "composed_calls_per_window": args.composed_calls, "graph": {"launches": args.graph_calls, "replays_per_window": args.graph_replays},
       "device": torch.cuda.get_device_name(0), "launch": {}}

# ---- the launch alone ------------------------------------------------------------------------------------------------------------
for n_obj in (1, 8):
    st = stepper(n_obj, {"E_reach": args.w_reach})
    st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
    B = st.B
    pose, Rg, reach_q = st.hand_pose.clone(), st.Rg.clone(), st.reach_q.clone()
    base_T = torch.as_tensor(base34, dtype=torch.float32, device=dev)[None].expand(n_obj, 3, 4).contiguous()
    base44 = T44(base34)[None].expand(B, 4, 4)
    z = lambda *s: torch.zeros(*s, device=dev)
    re, rq, rs, rg = z(B), z(B, K + 1, arm.N), torch.zeros(B, K + 1, dtype=torch.int32, device=dev), z(B, 12)

    def reach():
        ops._reach_call(arm, pose, Rg, base_T, BE, AXIS, D, K, M, LAM, RHO, None, args.w_reach, re, rq, rs, 0, rg)

    for T, U in SHAPES:
        e, q, worst, step, gRt = z(B), z(B, T + 1, arm.N), z(B), z(B), z(B, 12)

        def fused():
            ops._track_call(arm, pose, Rg, base_T, BE, AXIS, D, T, U, LAM, RHO, reach_q[:, K], K, None, args.w_track, e, q, worst, step,
                            None, 0, gRt)

        def composed():
            return torch_track(pose[:, :3], Rg.view(B, 3, 3), base44, reach_q[:, K], T, U)

        e_c = composed()
        fused()
        torch.cuda.synchronize()
        g_track, g_reach = graphed(fused, args.graph_calls), graphed(reach, args.graph_calls)
        r = alternate({"gq_track_terms": (fused, args.calls, 1), "gq_track_terms_graph": (g_track.replay, args.graph_replays, args.graph_calls),
                       "gq_reach_terms": (reach, args.calls, 1), "gq_reach_terms_graph": (g_reach.replay, args.graph_replays, args.graph_calls),
                       "composed_route": (composed, args.composed_calls, 1)})
        passes = (T + 1) * (U + 1)
        r.update({"rows": B, "waypoints": T, "updates": U, "dependent_passes": passes,
                  "us_per_pass_track_graph": r["gq_track_terms_graph"]["median_us"] / passes,
                  "us_per_pass_reach_graph": r["gq_reach_terms_graph"]["median_us"] / (M + 1),
                  "us_per_pass_track_eager": r["gq_track_terms"]["median_us"] / passes,
                  "us_per_pass_reach_eager": r["gq_reach_terms"]["median_us"] / (M + 1),
                  "E_track_mean": float(e.mean()), "share_worst_under_1e-6": float((worst < 1e-6).float().mean()),
                  "share_step_under_0.3": float((step < 0.3).float().mean()),
                  "agreement_median_rel_dE": float(((e - e_c).abs() / e.clamp_min(1e-12)).median()),
                  "fused_over_composed": r["gq_track_terms"]["median_us"] / r["composed_route"]["median_us"]})
        rec["launch"][f"{n_obj}x256_T{T}_U{U}"] = r
        print(json.dumps({f"{n_obj}x256_T{T}_U{U}": r}), flush=True)
    del st

# ---- the iteration ---------------------------------------------------------------------------------------------------------------
W0 = {"E_reach": args.w_reach, "E_arm": args.w_arm}
steppers = {"reach_arm": stepper(1, W0), "reach_arm_track": stepper(1, dict(W0, E_track=args.w_track))}
for st in steppers.values():
    st.capture(iters=1)
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
                        "ms_per_iteration_max": max(v)} for k, v in times.items()}
print(json.dumps({"iteration": rec["iteration"]}), flush=True)
del steppers

# ---- a run with and without the weight, and with the arm term on the path ----------------------------------------------------------
probe = stepper(1, dict(W0, E_track=args.w_track), seed=5)  # evaluates the terms at another stepper's accepted state
rec["run"] = {"iterations": args.run_iters, "rows": BE, "reset_epochs": 600, "w_reach": args.w_reach, "w_arm": args.w_arm,
              "w_track": args.w_track, "waypoints": 8, "updates": 3}
runs = [("no_track", W0, {}), ("track", dict(W0, E_track=args.w_track), {}),
        ("track_arm_on_track", dict(W0, E_track=args.w_track), {"arm_on_track": True})]
for name, weights, kw in runs:
    st = stepper(1, weights, seed=7, **kw)
    out = {}
    for tag in ("initial", "final"):
        if tag == "final":
            st.capture(iters=1)
            st.run(args.run_iters, reset_epochs=600, z_score_threshold=1.0)
            assert torch.isfinite(st.energy).all()
        t = probe.evaluate(st.hand_pose, st.contact_idx)[0]
        out[f"share_worst_under_1e-6_{tag}"] = float((probe.track_worst < 1e-6).float().mean())
        out[f"share_step_under_0.3_{tag}"] = float((probe.track_step < 0.3).float().mean())
        out[f"share_E_reach_under_1e-6_{tag}"] = float((t["E_reach"] < 1e-6).float().mean())
        out[f"share_E_arm_zero_{tag}"] = float((t["E_arm"] <= 0).float().mean())
        out.update({f"{k}_mean_{tag}": float(t[k].mean()) for k in probe.term_names})
    rec["run"][name] = out
    print(json.dumps({name: out}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
