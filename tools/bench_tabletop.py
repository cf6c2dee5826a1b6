"""Cost of the stepper's tabletop mode (E_prior / E_wall: un-fused proposal / accept launches + one gq_tabletop_terms launch
per iteration) beside its default five-term mode, on the scene of BASELINE config 2 (Allegro, one superquadric mesh, 256
grasps, 12 contacts): both steppers replay captured hipGraphs, are warmed up, and are timed alternately over windows of
--steps iterations that end in a device synchronise.  Evidence run, not a test: one JSON line per (round, mode) and a
summary line are appended to --out.

usage: python tools/bench_tabletop.py [--steps 200] [--warmup 24] [--rounds 3] [--w_wall 10] [--w_prior 1] [--out file.jsonl]
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
ap.add_argument("--graph_iters", type=int, default=8, help="iterations per hipGraph of the default mode (tabletop mode: 1)")
ap.add_argument("--w_wall", type=float, default=10.0)
ap.add_argument("--w_prior", type=float, default=1.0)
ap.add_argument("--only", choices=("both", "default", "tabletop"), default="both", help="profiling runs: one mode alone")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "tabletop_bench.jsonl"))
args = ap.parse_args()

from bench import make_initial_state
from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

spec = get_hand_spec(args.hand)
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
hand = ops.HandHandle(spec)
hp, idx = make_initial_state(spec, fv, args.batch_size, args.n_contact, 1000)
modes = {"default": None, "tabletop": {"E_wall": args.w_wall, "E_prior": args.w_prior}}
if args.only != "both":
    modes = {args.only: modes[args.only]}
steppers = {}
for name, w in modes.items():
    st = GraspStepper(hand, ops.MeshSet([fv]), torch.tensor(sp)[None], args.batch_size, args.n_contact, seed=1, weights=w)
    st.reset(hp.cuda(), idx.cuda())
    st.capture(iters=max(d for d in (1, 2, 4, 8, 16, 32, 64) if d <= max(1, args.graph_iters) and args.steps % d == 0))
    for _ in range(args.warmup):
        st.step()
    st.realign_draws()
    steppers[name] = st
torch.cuda.synchronize()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
B = args.batch_size
recs = []
with open(args.out, "a") as f:
    for r in range(args.rounds):
        for name, st in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st.step()
            t_enq = time.perf_counter() - t0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert st._graph_pending == 0 and torch.isfinite(st.energy).all()
            rec = {"round": r, "mode": name, "graph_mode": st.graph_mode, "terms": len(st.term_names), "steps": args.steps,
                   "batch": B, "ms_per_iteration": 1e3 * dt / args.steps, "evals_per_s": B * args.steps / dt,
                   "host_enqueue_fraction": t_enq / dt}
            recs.append(rec)
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
    summ = {"summary": True, "hand": args.hand, "n_contact": args.n_contact, "w_wall": args.w_wall, "w_prior": args.w_prior}
    for name in steppers:
        ms = sorted(x["ms_per_iteration"] for x in recs if x["mode"] == name)
        summ[name] = {"ms_per_iteration_median": float(np.median(ms)), "ms_per_iteration_min": ms[0], "ms_per_iteration_max": ms[-1],
                      "evals_per_s_median": B / (1e-3 * float(np.median(ms)))}
    if "tabletop" in steppers:
        summ["E_wall_mean_final"] = float(steppers["tabletop"].terms[6].mean())
    f.write(json.dumps(summ) + "\n")
    print(json.dumps(summ), flush=True)
