"""Timing of the lift term: Allegro, 512 hand surface samples, the ``box`` scene (an open-topped bin around the object)
on an 80^3 grid of 5 mm, the object's points an even stride of its 2 500 surface points.  Evidence run, not a test: one JSON record
is printed and written to --out.

  launch     gq_lift_terms alone (energy, object share, link wrenches and gRt in one launch) at 256 and 2 048 rows for K in
             {1, 4, 8} stations and M in {0, 512} object points, eager and from a captured graph, against the composed route on the
             same inputs: gq_clutter_corridor_terms for the hand (the bits of the launch at H = 0, M = 0; here it stands for the hand's
             share of the work) plus, with M > 0, ops.scene_distance on the object's B K M station points (one query launch; the
             points are formed once outside the window, which favours the composed route).  HIP events around 200 launches (eager)
             or 50 replays of a graph of 4 launches per window, the two routes alternating, medians of --rounds windows.
  iteration  captured graphs in alternating windows of --steps replays at --batch_size rows: the default five-term stepper,
             scene + approach, and scene + approach + lift; ms per iteration and evaluations per second.

usage: python tools/bench_lift.py [--batch_size 256] [--steps 200] [--warmup 24] [--rounds 5] [--out file.json]
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
ap.add_argument("--hand", default="allegro")
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--grid", type=int, default=80)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--scene_margin", type=float, default=0.005)
ap.add_argument("--w_scene", type=float, default=50.0)
ap.add_argument("--w_approach", type=float, default=20.0)
ap.add_argument("--w_lift", type=float, default=20.0)
ap.add_argument("--lift_height", type=float, default=0.05)
ap.add_argument("--lift_retreat", type=float, default=0.08)
ap.add_argument("--stations", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "lift_bench.json"))
args = ap.parse_args()

from bench import make_initial_state
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
spec = get_hand_spec(args.hand)
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
hand = ops.HandHandle(spec)
n = args.n_contact
center = 0.5 * (fv.reshape(-1, 3).min(0) + fv.reshape(-1, 3).max(0))
origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in center]
scene = ops.SceneSDF.from_meshes(meshes.open_bin(center), origin, (args.grid,) * 3, args.voxel)
grids = ops._pregrasp_grids(scene.values, scene.origin, scene.voxel)
samples = ops.SurfaceSamples(hand, *meshes.hand_surface_samples(spec, 512))
U = ops.lift_direction((0.0, 0.0, 1.0))
H, D = args.lift_height, args.lift_retreat


def window(fn, n_calls):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n_calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / n_calls  # us


def alternate(fns, n_calls, per_call=1, warm=20):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, n_calls) / per_call)
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def graphed(fn, reps=4):
    """``reps`` launches of ``fn`` as one captured graph; -> replay()."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    return g.replay


rec = {"lift_bench": True, "hand": args.hand, "n_samples": samples.Ns, "grid": [args.grid] * 3, "voxel": args.voxel, "scene": "box",
       "height": H, "retreat": D, "direction": U, "margin": args.scene_margin, "rounds": args.rounds, "launches_per_window": 200,
       "device": torch.cuda.get_device_name(0)}

# ---- the launch alone --------------------------------------------------------------------------------------------------------
rec["launch"] = {}
worst = 0.0
for B in (256, 2048):
    hp, idx = make_initial_state(spec, fv, B, n, 1000)
    hp, idx = hp.cuda(), idx.cuda()
    L = hand.L
    Rg3, LT4, _, _, _, _ = ops.fk_contacts(hp, idx, hand)
    Rg, LT = Rg3.reshape(B, 9).contiguous(), LT4.reshape(B, L, 12).contiguous()
    z = lambda *s: torch.zeros(*s, device="cuda")
    e_l, e_o, e_a, gRt, wrench = z(B), z(B), z(B), z(B, 12), z(B, L, 6)
    back = (Rg3 @ torch.tensor(spec.grasp_axis, device="cuda", dtype=torch.float32)).reshape(B, 3)  # R a
    for K in (1, 4, 8):
        for M in (0, 512):
            pick = (torch.arange(M) * len(sp)) // max(M, 1)
            P = torch.tensor(sp)[pick][None].float().cuda().contiguous()  # (1,M,3)
            s_k = torch.arange(1, K + 1, device="cuda", dtype=torch.float32) / K
            carry = s_k[None, :, None] * (H * torch.tensor(U, device="cuda")[None, None] - D * back[:, None])  # (B,K,3)
            station_points = (P[0][None, None] + carry[:, :, None]).contiguous()  # (B,K,M,3), formed once: not in the window

            def fused():
                ops._lift_call(grids, args.scene_margin, 0.0, H, D, K, hp, samples.points, samples.link, L, Rg, LT, P, 1, B, M,
                               spec.grasp_axis, U, None, args.w_lift, e_l, e_o, 0, wrench, gRt)

            def composed():
                ops._approach_call(grids, args.scene_margin, max(D, 1e-3), K, hp, samples.points, samples.link, L, Rg, LT, spec.grasp_axis,
                                   None, args.w_lift, e_a, 0, wrench, gRt)
                if M:
                    ops.scene_distance(station_points, scene)

            r = {"eager": alternate({"gq_lift_terms": fused, "composed_route": composed}, 200)}
            r["graph"] = alternate({"gq_lift_terms": graphed(fused), "composed_route": graphed(composed)}, 50, per_call=4)
            fused()
            torch.cuda.synchronize()
            r["E_lift_mean"], r["object_share_mean"] = float(e_l.mean()), float(e_o.mean())
            r["rows_with_E_lift"] = int((e_l > 0).sum())
            r["launches_in_composed_route"] = 2 if M else 1
            for how in ("eager", "graph"):
                r[how]["lift_over_composed"] = r[how]["gq_lift_terms"]["median_us"] / r[how]["composed_route"]["median_us"]
                worst = max(worst, r[how]["lift_over_composed"])
            rec["launch"][f"B{B}_K{K}_M{M}"] = r
            print(json.dumps({f"B{B}_K{K}_M{M}": r}), flush=True)
rec["worst_lift_over_composed"] = worst

# ---- the iteration -----------------------------------------------------------------------------------------------------------
B = args.batch_size
hp, idx = make_initial_state(spec, fv, B, n, 1000)
hp, idx = hp.cuda(), idx.cuda()
corridor = dict(approach_distance=0.10, approach_stations=args.stations)
obstacle = dict(weights={"E_scene": args.w_scene, "E_approach": args.w_approach}, scene=scene, scene_margin=args.scene_margin, **corridor)
modes = {"default": {}, "scene+approach": obstacle,
         "scene+approach+lift": dict(obstacle, weights=dict(obstacle["weights"], E_lift=args.w_lift), lift_height=H, lift_retreat=D,
                                     lift_stations=args.stations)}
steppers = {}
for name, kw in modes.items():
    st = GraspStepper(hand, ops.MeshSet([fv]), torch.tensor(sp)[None], B, n, seed=1, **kw)
    st.reset(hp, idx)
    st.capture(iters=8 if st._fuse_loop and args.steps % 8 == 0 else 1)
    for _ in range(args.warmup):
        st.step()
    st.realign_draws()
    steppers[name] = st
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
rec["iteration"] = {k: {"rows": B, "graph_mode": steppers[k].graph_mode, "terms": len(steppers[k].term_names), "steps_per_window": args.steps,
                        "ms_per_iteration_median": float(np.median(v)), "ms_per_iteration_min": min(v), "ms_per_iteration_max": max(v),
                        "evals_per_s_median": B / (1e-3 * float(np.median(v)))} for k, v in times.items()}
rec["iteration"]["lift_object_points"] = int(steppers["scene+approach+lift"].lift_object_points.shape[1])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps({"iteration": rec["iteration"], "worst_lift_over_composed": worst}), flush=True)
