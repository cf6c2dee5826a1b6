"""Timing and effect of the arm clearance term on the bench scene: Allegro, 12 contacts, superquadric objects, 256 rows
per object, the ``arm7`` preset with its link spheres (radius 0.05 m, one every 0.08 m), a shelf board above the object as the scene.
Evidence run, not a test: one JSON record is printed and written to --out (profiles/arm_bench.json is such a record).

  launch     gq_arm_terms alone (energy and the gRt gradient in one launch) at 1 x 256 and 8 x 256 rows, for K = 0 and K = 2
             stations, against the same term composed from batched torch ops on the device (fp32 link frames, sphere points, the
             trilinear sample and its gradient by gathers, the hinge, g_q, the Jacobian, an fp64 torch.linalg.solve of the 6 x 6, the
             gRt layout), and beside gq_reach_terms on the same rows.  Two figures per launch.  "median_us": HIP events around
             --calls eager calls per window (--composed_calls for the composed route), the routes alternating, medians of --rounds
             windows; host enqueue time is inside the windows on every side, and for a launch this short the figure IS the enqueue
             floor of back-to-back launches (it does not move with the rows or the stations), as the composed route's is mostly
             Python and launch overhead of its few hundred small ops.  "graph_us": --graph_calls launches captured in one graph and
             replayed, HIP events around --graph_replays replays: no host in the window, the device-side time per launch including
             the gap between two dependent-free kernels of one stream.
  iteration  captured graphs in alternating windows of --steps replays at 1 x 256 rows: the reach stepper (the parent's) and the
             stepper with the term; ms per iteration and evaluations per second.
  run        --run_iters iterations (default 2 000) of the reference's schedule from one seed with weight 0 and with each of
             --run_weights: the share of rows with E_arm = 0 and with E_reach < 1e-6, the means of both and the other terms, before
             and after, evaluated by the same launches.

usage: python tools/bench_arm.py [--steps 200] [--warmup 24] [--rounds 5] [--calls 2000] [--composed_calls 40] [--graph_calls 200]
       [--graph_replays 20] [--run_iters 2000] [--run_weights 10,100]
       [--arm_base X Y Z YAW] [--shelf_z 0.22] [--out file.json]
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
ap.add_argument("--w_arm", type=float, default=100.0)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--composed_calls", type=int, default=40)
ap.add_argument("--graph_calls", type=int, default=200)
ap.add_argument("--graph_replays", type=int, default=20)
ap.add_argument("--run_iters", type=int, default=2000)
ap.add_argument("--run_weights", default="10,100", help="the weights of the runs, beside the run without the term")
ap.add_argument("--arm_base", type=float, nargs=4, default=(-0.45, 0.0, -0.3, 0.0), metavar=("X", "Y", "Z", "YAW"))
ap.add_argument("--shelf_z", type=float, default=0.22, help="height of the shelf board above the object, metres")
ap.add_argument("--margin", type=float, default=0.01)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "arm_bench.json"))
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
n, BE = args.n_contact, 256
LAM_A, RHO, MARGIN = 1e-6, 0.1, args.margin
AXIS = [float(a) for a in spec.grasp_axis]

# the scene: a shelf board 2 cm thick over the object, 0.9 m x 0.9 m, open towards the arm's side below it; the exact box distance
ORIGIN, SHAPE, VOXEL = (-0.8, -0.6, -0.5), (57, 49, 49), 0.025
ax = [ORIGIN[i] + VOXEL * torch.arange(SHAPE[i], dtype=torch.float64) for i in range(3)]
X = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)
d = (X - torch.tensor([0.0, 0.0, args.shelf_z], dtype=torch.float64)).abs() - torch.tensor([0.45, 0.45, 0.01], dtype=torch.float64)
PHI = (d.clamp_min(0).norm(dim=-1) + d.amax(-1).clamp_max(0)).to(torch.float32)
scene = ops.SceneSDF(PHI.to(dev), ORIGIN, VOXEL)


def stepper(n_obj, weights=None, seed=3, stations=0):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    om = ObjectModel(batch_size_each=BE, num_samples=2500)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), BE, n, seed=seed, weights=weights, arm=arm, arm_base=base34,
                      reach_stations=stations, arm_scene=scene, arm_margin=MARGIN)
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
    """fns: name -> callable; n_calls: name -> calls per window"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, n_calls[k]))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v), "calls_per_window": n_calls[k]} for k, v in out.items()}


def graph_time(fn):
    """--graph_calls launches of fn in one captured graph; us per launch over --graph_replays replays, median of --rounds windows"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.graph_calls):
            fn()
    g.replay()
    v = [window(g.replay, args.graph_replays) / args.graph_calls for _ in range(args.rounds)]
    return {"graph_us": float(np.median(v)), "graph_us_min": min(v), "graph_us_max": max(v)}


# ---- the same term from batched torch ops on the device --------------------------------------------------------------------------
T44 = lambda t34: torch.cat([torch.as_tensor(t34, dtype=torch.float32, device=dev), torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)], 0)
PRE = [T44(t) for t in arm_spec.joint_T]
TOOL = T44(arm_spec.tool_T)
AX = torch.as_tensor(arm_spec.joint_axis, dtype=torch.float32, device=dev)
HAT = torch.stack([torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float32) for a in arm_spec.joint_axis]).to(dev)
LO, HI = (torch.as_tensor(np.asarray(v, np.float32), device=dev) for v in (arm_spec.lower, arm_spec.upper))
LINK = torch.as_tensor(arm_spec.sphere_link, dtype=torch.long, device=dev)
CTR = torch.as_tensor(arm_spec.sphere_centre, dtype=torch.float32, device=dev)
RAD = torch.as_tensor(arm_spec.sphere_radius, dtype=torch.float32, device=dev)
ON = (LINK[None, :] >= torch.arange(arm_spec.n_joints, device=dev)[:, None]).float()
EYE3, EYE4 = torch.eye(3, device=dev), torch.eye(4, device=dev)
EYE6 = torch.eye(6, device=dev, dtype=torch.float64)
GV, GO, GN = scene.values, torch.tensor(ORIGIN, device=dev), torch.tensor(SHAPE, device=dev)


def torch_sample(x):
    """phi, grad phi and inside of the trilinear interpolant at x (...,3)"""
    u = (x - GO) / VOXEL
    inside = ((u >= 0) & (u <= GN - 1)).all(-1)
    u = torch.where(inside[..., None], u, torch.zeros_like(u))
    i = torch.minimum(u.floor(), (GN - 2).float()).long()
    f = u - i
    v = [[[GV[i[..., 0] + a, i[..., 1] + b, i[..., 2] + c] for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    c = [[v[a][b][0] + fz * (v[a][b][1] - v[a][b][0]) for b in (0, 1)] for a in (0, 1)]
    dz = [[v[a][b][1] - v[a][b][0] for b in (0, 1)] for a in (0, 1)]
    c0, c1 = c[0][0] + fy * (c[0][1] - c[0][0]), c[1][0] + fy * (c[1][1] - c[1][0])
    e0, e1 = c[0][1] - c[0][0], c[1][1] - c[1][0]
    dz0, dz1 = dz[0][0] + fy * (dz[0][1] - dz[0][0]), dz[1][0] + fy * (dz[1][1] - dz[1][0])
    grad = torch.stack([c1 - c0, e0 + fx * (e1 - e0), dz0 + fx * (dz1 - dz0)], -1) / VOXEL
    return c0 + fx * (c1 - c0), grad, inside


def torch_arm(q, R, base, K, D=0.10, c_up=1.0):
    """q (B,K+1,N), R (B,3,3), base (B,4,4) -> (E_arm (B), gRt (B,12))"""
    B, K1, N = q.shape
    P = B * K1
    qf, Tc, W = q.reshape(P, N), base[:, None].expand(B, K1, 4, 4).reshape(P, 4, 4), []
    for j in range(N):  # all revolute
        Mo = EYE4.repeat(P, 1, 1)
        Mo[:, :3, :3] = EYE3 + torch.sin(qf[:, j])[:, None, None] * HAT[j] + (1 - torch.cos(qf[:, j]))[:, None, None] * (HAT[j] @ HAT[j])
        Tc = Tc @ PRE[j] @ Mo
        W.append(Tc)
    W = torch.stack(W, 1)
    pee = (Tc @ TOOL)[:, :3, 3]
    Wl = W[:, LINK]
    x = (Wl[..., :3, :3] @ CTR[None, :, :, None])[..., 0] + Wl[..., :3, 3]
    phi, grad, inside = torch_sample(x)
    h = torch.where(inside, torch.relu(MARGIN + RAD[None] - phi), torch.zeros_like(phi))
    f = -grad * (h > 0)[..., None]
    org, axs = W[:, :, :3, 3], (W[:, :, :3, :3] @ AX[None, :, :, None])[..., 0]
    col = torch.linalg.cross(axs[:, :, None].expand(P, N, x.shape[1], 3), x[:, None] - org[:, :, None], dim=-1)
    gq = ((col * f[:, None]).sum(-1) * ON[None]).sum(-1)
    free = ((LO < qf) & (qf < HI)).float()
    J = (torch.cat([torch.linalg.cross(axs, pee[:, None] - org, dim=-1), RHO * axs], -1) * free[:, :, None]).transpose(1, 2).double()
    y = torch.linalg.solve(J @ J.transpose(1, 2) + LAM_A * EYE6, J @ gq.double()[:, :, None])[:, :, 0].float().reshape(B, K1, 6)
    cu = c_up / K1
    dk = torch.tensor([D * k / K if K else 0.0 for k in range(K1)], device=dev)
    a = torch.tensor(AXIS, device=dev)
    gh = cu * torch.einsum("bji,bkj->bki", R, y[:, :, :3])  # R' c y_p
    th = (cu * RHO * torch.einsum("bji,bkj->bki", R, y[:, :, 3:])).sum(1)
    K9 = torch.einsum("bki,k,j->bij", gh, -dk, a)
    z = torch.zeros_like(th[:, 0])
    K9 = K9 + 0.5 * torch.stack([torch.stack([z, -th[:, 2], th[:, 1]], -1), torch.stack([th[:, 2], z, -th[:, 0]], -1),
                                 torch.stack([-th[:, 1], th[:, 0], z], -1)], -2)
    return h.sum(-1).reshape(B, K1).mean(-1), torch.cat([-gh.sum(1), K9.reshape(B, 9)], -1)


rec = {"arm_bench": True, "hand": "allegro", "arm": "arm7", "spheres": arm_spec.n_spheres, "damping": LAM_A, "rot_scale": RHO,
       "margin": MARGIN, "arm_base": list(args.arm_base), "scene": {"shelf_z": args.shelf_z, "shape": list(SHAPE), "voxel": VOXEL},
       "rounds": args.rounds, "calls_per_window": args.calls, "composed_calls_per_window": args.composed_calls,
       "graph_calls": args.graph_calls, "graph_replays": args.graph_replays,
       "note": "median_us of the two launches is the enqueue floor of eager back-to-back launches, not kernel time; graph_us is the "
               "device-side time per launch inside a replayed graph; the composed route is mostly Python and launch overhead", "device": torch.cuda.get_device_name(0), "launch": {}}

# ---- the launch alone --------------------------------------------------------------------------------------------------------
grids = ops._arm_scene_grids(scene)
for n_obj in (1, 8):
    for K in (0, 2):
        st = stepper(n_obj, {"E_reach": args.w_reach}, stations=K)
        st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
        B = st.B
        pose, Rg, q = st.hand_pose.clone(), st.Rg.clone(), st.reach_q.clone()
        base_T = st.arm_base
        base44 = T44(base34)[None].expand(B, 4, 4)
        e, gRt = torch.zeros(B, device=dev), torch.zeros(B, 12, device=dev)
        e_r, q_r, sd_r, g_r = torch.zeros(B, device=dev), torch.zeros_like(q), torch.zeros(B, K + 1, dtype=torch.int32, device=dev), torch.zeros(B, 12, device=dev)

        def fused():
            ops._arm_call(arm, grids, MARGIN, LAM_A, RHO, pose, Rg, base_T, BE, AXIS, 0.10, K, q, None, 1.0, e, 0, gRt)

        def composed():
            return torch_arm(q, Rg.view(B, 3, 3), base44, K)

        def reach():
            ops._reach_call(arm, pose, Rg, base_T, BE, AXIS, 0.10, K, 24, 1e-4, RHO, None, 1.0, e_r, q_r, sd_r, 0, g_r)

        e_c, g_c = composed()
        fused()
        torch.cuda.synchronize()
        r = alternate({"gq_arm_terms": fused, "composed_route": composed, "gq_reach_terms": reach},
                      {"gq_arm_terms": args.calls, "composed_route": args.composed_calls, "gq_reach_terms": args.calls})
        r["gq_arm_terms"].update(graph_time(fused))
        r["gq_reach_terms"].update(graph_time(reach))
        gn = gRt.norm(dim=-1)
        r.update({"rows": B, "stations": K, "E_arm_mean": float(e.mean()), "share_E_arm_0": float((e <= 0).float().mean()),
                  "agreement_max_abs_dE": float((e - e_c).abs().max()),
                  "agreement_gRt_rel_median": float(((gRt - g_c).norm(dim=-1)[gn > 0] / gn[gn > 0]).median()) if (gn > 0).any() else None,
                  "fused_over_composed": r["gq_arm_terms"]["median_us"] / r["composed_route"]["median_us"]})
        rec["launch"][f"{n_obj}x256_K{K}"] = r
        print(json.dumps({f"{n_obj}x256_K{K}": r}), flush=True)
        del st

# ---- the iteration -----------------------------------------------------------------------------------------------------------
steppers = {"reach": stepper(1, {"E_reach": args.w_reach}), "reach_arm": stepper(1, {"E_reach": args.w_reach, "E_arm": args.w_arm})}
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
                        "ms_per_iteration_max": max(v), "evals_per_s_median": BE / (1e-3 * float(np.median(v)))}
                    for k, v in times.items()}
print(json.dumps({"iteration": rec["iteration"]}), flush=True)
del steppers

# ---- a run with and without the weight -------------------------------------------------------------------------------------------
probe = stepper(1, {"E_reach": args.w_reach, "E_arm": args.w_arm}, seed=5)  # evaluates both terms at another stepper's accepted state
rec["run"] = {"iterations": args.run_iters, "rows": BE, "reset_epochs": 600, "w_reach": args.w_reach}
runs = [("weight_0", {"E_reach": args.w_reach})] + [(f"weight_{w:g}", {"E_reach": args.w_reach, "E_arm": w}) for w in map(float, args.run_weights.split(","))]
for name, weights in runs:
    st = stepper(1, weights, seed=7)
    t0 = probe.evaluate(st.hand_pose, st.contact_idx)[0]
    st.capture(iters=1)
    st.run(args.run_iters, reset_epochs=600, z_score_threshold=1.0)
    t1 = probe.evaluate(st.hand_pose, st.contact_idx)[0]
    assert torch.isfinite(st.energy).all()
    out = {}
    for tag, t in (("initial", t0), ("final", t1)):
        out[f"share_E_arm_0_{tag}"] = float((t["E_arm"] <= 0).float().mean())
        out[f"share_E_reach_under_1e-6_{tag}"] = float((t["E_reach"] < 1e-6).float().mean())
        out[f"share_both_{tag}"] = float(((t["E_arm"] <= 0) & (t["E_reach"] < 1e-6)).float().mean())
        out.update({f"{k}_mean_{tag}": float(t[k].mean()) for k in ("E_arm", "E_reach", "E_dis", "E_fc", "E_pen", "E_spen", "E_joints")})
    rec["run"][name] = out
    print(json.dumps({name: out}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
