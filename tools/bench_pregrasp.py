"""Timing of the pre-grasp term at BASELINE configs[1]: Allegro, 256 rows, 512 hand surface samples, the ``box`` scene
(an open-topped bin around the object) on an 80^3 grid of 5 mm.  Evidence run, not a test: one JSON record is printed and written
to --out.

  launch     gq_pregrasp_terms alone (energy, gRt and g_theta in one launch) at K = 0 / 4 / 8 stations, against the composed route
             of existing launches on the same inputs: gq_fk_forward at the opened pose without contact queries, gq_scene_terms,
             gq_approach_terms (K > 0) and gq_fk_backward.  HIP events around 200 launches per window, the two routes alternating,
             medians of --rounds windows.  Host enqueue time is inside the windows on both sides.
  iteration  captured graphs in alternating windows of --steps replays: the default five-term stepper, scene + approach, and
             scene + approach + pregrasp; ms per iteration and evaluations per second.

usage: python tools/bench_pregrasp.py [--batch_size 256] [--steps 200] [--warmup 24] [--rounds 3] [--out file.json]
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
ap.add_argument("--hand", default="allegro")
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=24)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--grid", type=int, default=80)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--scene_margin", type=float, default=0.005)
ap.add_argument("--w_scene", type=float, default=50.0)
ap.add_argument("--w_approach", type=float, default=20.0)
ap.add_argument("--w_pregrasp", type=float, default=30.0)
ap.add_argument("--distance", type=float, default=0.10)
ap.add_argument("--stations", type=int, default=4)
ap.add_argument("--opening", type=float, default=0.5)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "pregrasp_bench.json"))
args = ap.parse_args()

from bench import make_initial_state
from graspqp_amd import _C, ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool runs on the GPU"
spec = get_hand_spec(args.hand)
fv = meshes.superquadric(0)
sp = meshes.surface_points(fv, 2500, oversample=4, seed=42)
hand = ops.HandHandle(spec)
B, n = args.batch_size, args.n_contact
hp, idx = make_initial_state(spec, fv, B, n, 1000)
hp, idx = hp.cuda(), idx.cuda()
center = 0.5 * (fv.reshape(-1, 3).min(0) + fv.reshape(-1, 3).max(0))
origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in center]
scene = ops.SceneSDF.from_meshes(meshes.open_bin(center), origin, (args.grid,) * 3, args.voxel)
samples = ops.SurfaceSamples(hand, *meshes.hand_surface_samples(spec, 512))
q_open = ops.default_open_joints(spec, "cuda")
f32, i32, st_ptr = _C.f32, _C.i32, _C.stream_ptr


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


rec = {"pregrasp_bench": True, "hand": args.hand, "rows": B, "n_samples": samples.Ns, "grid": [args.grid] * 3, "voxel": args.voxel,
       "scene": "box", "distance": args.distance, "opening": args.opening, "margin": args.scene_margin, "rounds": args.rounds,
       "launches_per_window": 200, "device": torch.cuda.get_device_name(0)}

# ---- the launch alone --------------------------------------------------------------------------------------------------------
L, J, D = hand.L, hand.J, hp.shape[1]
grids = ops._pregrasp_grids(scene.values, scene.origin, scene.voxel)
axis = (ctypes.c_float * 3)(*(float(a) for a in spec.grasp_axis))
opened = torch.cat([hp[:, :9], (1.0 - args.opening) * hp[:, 9:] + args.opening * q_open[None]], 1).contiguous()
z = lambda *s: torch.zeros(*s, device="cuda")
Rg, LT, e_p, e_s, e_a, g_theta, gRt, wrench, grad = z(B, 9), z(B, L, 12), z(B), z(B), z(B), z(B, J), z(B, 12), z(B, L, 6), z(B, D)
ws, nb = hand.fk_ws(B, hp.device)
_C.call("gq_fk_forward", hand.handle, f32(hp), None, B, 0, f32(Rg), f32(LT), None, None, None, 0.0, None, None, None, None, _C.ptr(ws), nb,
        st_ptr())  # R of the closed pose: an input of the fused launch
Rg_closed = Rg.clone()
rec["launch"] = {}
for K in (0, 4, 8):
    def fused():
        ops._pregrasp_call(hand, grids, args.scene_margin, args.distance, K, args.opening, q_open, hp, samples.points, samples.link,
                           Rg_closed, spec.grasp_axis, None, args.w_pregrasp, e_p, 0, g_theta, gRt)

    def composed():
        s = st_ptr()
        _C.call("gq_fk_forward", hand.handle, f32(opened), None, B, 0, f32(Rg), f32(LT), None, None, None, 0.0, None, None, None, None,
                _C.ptr(ws), nb, s)
        _C.call("gq_scene_terms", ctypes.byref(scene.grid), args.scene_margin, f32(samples.points), i32(samples.link),
                ctypes.c_int64(samples.Ns), L, f32(opened), D, f32(Rg), f32(LT), ctypes.c_int64(B), None, args.w_pregrasp, f32(e_s), 0,
                f32(wrench), f32(gRt), s)
        if K > 0:
            _C.call("gq_approach_terms", ctypes.byref(scene.grid), args.scene_margin, args.distance, K, f32(samples.points),
                    i32(samples.link), ctypes.c_int64(samples.Ns), L, f32(opened), D, f32(Rg), f32(LT), ctypes.c_int64(B),
                    ctypes.cast(axis, ctypes.c_void_p), None, args.w_pregrasp, f32(e_a), 1, f32(wrench), f32(gRt), s)
        _C.call("gq_fk_backward", hand.handle, f32(opened), None, B, 0, f32(Rg), f32(LT), None, None, None, f32(wrench), f32(gRt), None,
                None, f32(grad), None, None, _C.ptr(ws), nb, s)

    r = alternate({"gq_pregrasp_terms": fused, "composed_route": composed}, 200)
    r["launches_in_composed_route"] = 4 if K > 0 else 3
    r["E_pregrasp_mean"] = float(e_p.mean())
    r["rows_with_E_pregrasp"] = int((e_p > 0).sum())
    r["fused_over_composed"] = r["gq_pregrasp_terms"]["median_us"] / r["composed_route"]["median_us"]
    rec["launch"][f"K{K}"] = r
    print(json.dumps({f"K{K}": r}), flush=True)

# ---- the iteration -----------------------------------------------------------------------------------------------------------
corridor = dict(approach_distance=args.distance, approach_stations=args.stations)
modes = {"default": {},
         "scene+approach": dict(weights={"E_scene": args.w_scene, "E_approach": args.w_approach}, scene=scene,
                                scene_margin=args.scene_margin, **corridor),
         "scene+approach+pregrasp": dict(weights={"E_scene": args.w_scene, "E_approach": args.w_approach, "E_pregrasp": args.w_pregrasp},
                                         scene=scene, scene_margin=args.scene_margin, pregrasp_opening=args.opening, **corridor)}
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
rec["iteration"] = {k: {"graph_mode": steppers[k].graph_mode, "terms": len(steppers[k].term_names), "steps_per_window": args.steps,
                        "ms_per_iteration_median": float(np.median(v)), "ms_per_iteration_min": min(v), "ms_per_iteration_max": max(v),
                        "evals_per_s_median": B / (1e-3 * float(np.median(v)))} for k, v in times.items()}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
