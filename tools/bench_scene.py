"""Cost of the stepper's scene mode (E_scene: un-fused proposal / accept launches + one gq_scene_terms launch per iteration) and
of its approach mode (scene + E_approach: one more gq_approach_terms launch, K = --approach_stations stations over
--approach_distance) beside its default five-term mode and its tabletop mode, on the scene of BASELINE config 2 (Allegro, one superquadric mesh,
256 grasps, 12 contacts).  The obstacles are the ``box`` preset: an open-topped bin of five slabs around the object on an 80^3
grid with 5 mm voxels (ops.SceneSDF.from_meshes).  All steppers replay captured hipGraphs, are warmed up, and are timed
alternately over windows of --steps iterations that end in a device synchronise.  Evidence run, not a test: one JSON line per
(round, mode) and a summary line are appended to --out.  The summary also holds the stand-alone time of 200 gq_scene_terms
launches and of 200 gq_approach_terms launches at K = 1, 4, 8 on the same inputs, beside K x the scene launch's time: what K
separate launches would cost.

usage: python tools/bench_scene.py [--steps 200] [--warmup 24] [--rounds 3] [--w_scene 50] [--scene_margin 0.005]
       [--w_approach 20] [--approach_distance 0.10] [--approach_stations 4] [--only MODE] [--out file.jsonl]
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
ap.add_argument("--graph_iters", type=int, default=8, help="iterations per hipGraph of the default mode (other modes: 1)")
ap.add_argument("--w_scene", type=float, default=50.0)
ap.add_argument("--scene_margin", type=float, default=0.005)
ap.add_argument("--grid", type=int, default=80)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--w_wall", type=float, default=10.0)
ap.add_argument("--w_prior", type=float, default=1.0)
ap.add_argument("--w_approach", type=float, default=20.0)
ap.add_argument("--approach_distance", type=float, default=0.10)
ap.add_argument("--approach_stations", type=int, default=4)
ap.add_argument("--only", choices=("all", "default", "tabletop", "scene", "approach"), default="all", help="profiling runs: one mode alone")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "scene_bench.jsonl"))
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
center = 0.5 * (fv.reshape(-1, 3).min(0) + fv.reshape(-1, 3).max(0))
origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in center]
t0 = time.perf_counter()
scene = ops.SceneSDF.from_meshes(meshes.open_bin(center), origin, (args.grid,) * 3, args.voxel)
torch.cuda.synchronize()
t_setup = time.perf_counter() - t0
modes = {"default": {}, "tabletop": dict(weights={"E_wall": args.w_wall, "E_prior": args.w_prior}),
         "scene": dict(weights={"E_scene": args.w_scene}, scene=scene, scene_margin=args.scene_margin),
         "approach": dict(weights={"E_scene": args.w_scene, "E_approach": args.w_approach}, scene=scene, scene_margin=args.scene_margin,
                          approach_distance=args.approach_distance, approach_stations=args.approach_stations)}
if args.only != "all":
    modes = {args.only: modes[args.only]}
steppers = {}
for name, kw in modes.items():
    st = GraspStepper(hand, ops.MeshSet([fv]), torch.tensor(sp)[None], args.batch_size, args.n_contact, seed=1, **kw)
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
    summ = {"summary": True, "hand": args.hand, "n_contact": args.n_contact, "w_scene": args.w_scene, "scene_margin": args.scene_margin,
            "grid": [args.grid] * 3, "voxel": args.voxel, "scene_setup_s": t_setup, "w_wall": args.w_wall, "w_prior": args.w_prior}
    for name in steppers:
        ms = sorted(x["ms_per_iteration"] for x in recs if x["mode"] == name)
        summ[name] = {"ms_per_iteration_median": float(np.median(ms)), "ms_per_iteration_min": ms[0], "ms_per_iteration_max": ms[-1],
                      "evals_per_s_median": B / (1e-3 * float(np.median(ms)))}

    def launch_us(fn):
        """HIP events around 200 launches (host overhead included), after 20 untimed ones."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(200):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / 200

    if "scene" in steppers:
        st = steppers["scene"]
        summ["E_scene_mean_final"] = float(st.terms[-1].mean())
        # the launch on its own, on the final state
        st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
        summ["scene_launch_us"] = launch_us(lambda: st._eval_scene(st.pose_new, ops._C.stream_ptr()))
    if "approach" in steppers:
        st = steppers["approach"]
        summ.update({"w_approach": args.w_approach, "approach_distance": args.approach_distance,
                     "approach_stations": args.approach_stations, "E_approach_mean_final": float(st.terms[-1].mean())})
        # gq_approach_terms on its own at K = 1, 4, 8, and gq_scene_terms on the same inputs (the approach stepper's own launch, or
        # the scene stepper's at the same pose when --w_scene 0 leaves this one without the term): K x its time is what K
        # separate launches would cost.  The timed launches add into the live wrench / gRt buffers (accumulate = 1, as in an
        # iteration), so the steppers' evaluation buffers are not meaningful afterwards: this is the last thing the tool does.
        st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
        ref = st if st.scene_mode else steppers.get("scene")
        summ["approach_launch"] = {}
        scene_us = None
        if ref is not None:
            if ref is not st:
                ref.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
            scene_us = launch_us(lambda: ref._eval_scene(ref.pose_new, ops._C.stream_ptr()))
            summ["approach_launch"]["scene_launch_us_same_inputs"] = scene_us
        keep = st.approach_stations
        for K in (1, 4, 8):
            st.approach_stations = K
            us = launch_us(lambda: st._eval_approach(st.pose_new, ops._C.stream_ptr()))
            summ["approach_launch"][f"K{K}"] = {"approach_launch_us": us,
                                                "K_scene_launches_us": None if scene_us is None else K * scene_us}
        st.approach_stations = keep
    f.write(json.dumps(summ) + "\n")
    print(json.dumps(summ), flush=True)
