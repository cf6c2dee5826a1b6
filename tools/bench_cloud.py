"""Cost of a point-cloud object in the stepper beside the same surface as a mesh, on the scene of BASELINE config 2
(Allegro, one superquadric, 256 grasps, 12 contacts = 3 072 contact queries per iteration): the superquadric as a mesh
(gq_sdf_forward_meshset; attached to the FK forward launch at this batch) and as a 20 000-point oriented cloud of the same
surface (gq_cloud_forward, a launch of its own).  Both steppers replay captured hipGraphs, are warmed up, and are timed
alternately over windows of --steps iterations that end in a device synchronise.  Then the two contact queries on their
own, as launches of the ops on the steppers' contact points (HIP events around --query_reps launches): at the initial
state, where the contacts are centimetres off the surface, and at the state after the run.  Under ``rocprofv3
--kernel-trace --stats`` the same run gives the per-kernel times of gq_cloud_wave_kernel and gq_sdf_wave_kernel.
Evidence run, not a test: one JSON document is written to --out.

usage: python tools/bench_cloud.py [--steps 200] [--warmup 24] [--rounds 3] [--cloud_points 20000] [--out file.json]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--graph_iters", type=int, default=8)
ap.add_argument("--cloud_points", type=int, default=20000)
ap.add_argument("--query_reps", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "cloud_bench.json"))
args = ap.parse_args()

from bench import make_initial_state
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

spec = get_hand_spec(args.hand)
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
cp, cn = meshes.mesh_to_cloud(fv, args.cloud_points, seed=7)
hand = ops.HandHandle(spec)
hp, idx = make_initial_state(spec, fv, args.batch_size, args.n_contact, 1000)
objects = {"mesh": ops.MeshSet([fv]), "cloud": ops.PointCloudSet([cp], [cn])}
B, n = args.batch_size, args.n_contact


def time_query(name, pts):
    """mean microseconds of one stand-alone contact query on ``pts`` (B n, 3)."""
    fn = (lambda: ops.sdf_meshset(pts, objects["mesh"], B * n)) if name == "mesh" else (lambda: ops.sdf_cloud(pts, objects["cloud"], B * n))
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.query_reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / args.query_reps


steppers, query_us = {}, {}
for name, obj in objects.items():
    st = GraspStepper(hand, obj, torch.tensor(sp)[None], B, n, seed=1)
    st.reset(hp.cuda(), idx.cuda())
    steppers[name] = st
torch.cuda.synchronize()
pts0 = steppers["mesh"].cpts.reshape(-1, 3).clone()
query_us["initial_state"] = {k: time_query(k, pts0) for k in objects}
for st in steppers.values():
    st.capture(iters=max(d for d in (1, 2, 4, 8, 16, 32, 64) if d <= max(1, args.graph_iters) and args.steps % d == 0))
    for _ in range(args.warmup):
        st.step()
    st.realign_draws()
torch.cuda.synchronize()
recs = []
for r in range(args.rounds):
    for name, st in steppers.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            st.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert st._graph_pending == 0 and torch.isfinite(st.energy).all()
        rec = {"round": r, "object": name, "graph_mode": st.graph_mode, "steps": args.steps, "batch": B,
               "ms_per_step": 1e3 * dt / args.steps, "evals_per_s": B * args.steps / dt}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
pts1 = steppers["mesh"].cpts.reshape(-1, 3).clone()
query_us["after_run"] = {k: time_query(k, pts1) for k in objects}
d2 = ops.sdf_meshset(pts1, objects["mesh"], B * n)[0]
out = {"hand": args.hand, "batch": B, "n_contact": n, "queries_per_iteration": B * n, "mesh_faces": int(fv.shape[0]),
       "cloud_points": int(cp.shape[0]), "cloud_radius": float(objects["cloud"].radius[0]), "rounds": recs,
       "standalone_query_us": query_us,
       "contact_distance_after_run_median_m": float(d2.sqrt().median())}
for name in steppers:
    ms = sorted(x["ms_per_step"] for x in recs if x["object"] == name)
    out[name] = {"ms_per_step_median": float(np.median(ms)), "ms_per_step_min": ms[0], "ms_per_step_max": ms[-1],
                 "evals_per_s_median": B / (1e-3 * float(np.median(ms))), "energy_mean_final": float(steppers[name].energy.mean())}
out["cloud_over_mesh_ms_per_step"] = out["cloud"]["ms_per_step_median"] / out["mesh"]["ms_per_step_median"]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "rounds"}), flush=True)
