"""Cost of the stepper's scene mode (E_scene: un-fused proposal / accept launches + one gq_scene_terms launch per iteration) and
of its approach mode (scene + E_approach: one more gq_approach_terms launch, K = --approach_stations stations over
--approach_distance) beside its default five-term mode and its tabletop mode, on the scene of BASELINE config 2 (Allegro, one superquadric mesh,
256 grasps, 12 contacts).  The obstacles are the ``box`` preset: an open-topped bin of five slabs around the object on an 80^3
grid with 5 mm voxels (ops.SceneSDF.from_meshes).  All steppers replay captured hipGraphs, are warmed up, and are timed
alternately over windows of --steps iterations that end in a device synchronise.  Evidence run, not a test: one JSON line per
(round, mode) and a summary line are appended to --out.  The summary also holds the stand-alone time of 200 gq_scene_terms
launches and of 200 gq_approach_terms launches at K = 1, 4, 8 on the same inputs, beside K x the scene launch's time: what K
separate launches would cost.

--only clutter measures the clutter scenes instead, --n_obj objects x --batch_size rows each: the stand-alone
gq_clutter_terms / gq_clutter_corridor_terms launches beside gq_scene_terms / gq_approach_terms on the same rows with one grid, and
beside --n_obj row-slice launches of the existing entry points (the alternative to the stack); the stepper in scene + approach mode
with an ops.SceneSDFSet and with one ops.SceneSDF; and gq_clutter_compose (--n_obj targets of --grid^3, --n_obj parts of
--part_grid^3, a base of --grid^3) beside ops.SceneSDF.from_meshes of the same scenes.  Everything in windows that alternate,
--rounds of them; the spread of a figure over its windows is its margin.  One JSON line is appended to --out.

usage: python tools/bench_scene.py [--steps 200] [--warmup 24] [--rounds 3] [--w_scene 50] [--scene_margin 0.005]
       [--w_approach 20] [--approach_distance 0.10] [--approach_stations 4] [--only MODE] [--n_obj 8] [--part_grid 48]
       [--out file.jsonl]
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
ap.add_argument("--only", choices=("all", "default", "tabletop", "scene", "approach", "clutter"), default="all",
                help="profiling runs: one mode alone; clutter: the measurements of DESIGN 16")
ap.add_argument("--n_obj", type=int, default=8, help="--only clutter: objects (= grids of the stack)")
ap.add_argument("--part_grid", type=int, default=48, help="--only clutter: nodes per axis of a part grid of the compose measurement")
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


def clutter_bench():
    """--only clutter (module docstring)."""
    G, be, K = args.n_obj, args.batch_size, args.approach_stations
    B, shape = G * be, (args.grid,) * 3
    hpB, idxB = make_initial_state(spec, fv, B, args.n_contact, 1000)
    hpB, idxB = hpB.cuda(), idxB.cuda()
    stack = ops.SceneSDFSet(scene.values[None].repeat(G, 1, 1, 1).contiguous(), scene.origin, scene.voxel)
    surf = torch.tensor(sp)[None].repeat(G, 1, 1)
    kw = dict(weights={"E_scene": args.w_scene, "E_approach": args.w_approach}, scene_margin=args.scene_margin,
              approach_distance=args.approach_distance, approach_stations=K)
    sts = {}
    for name, sc in (("set", stack), ("single", scene)):
        st = GraspStepper(hand, ops.MeshSet([fv] * G), surf, be, args.n_contact, seed=1, scene=sc, **kw)
        st.reset(hpB, idxB)
        st.capture()
        for _ in range(args.warmup):
            st.step()
        st.realign_draws()
        sts[name] = st
    torch.cuda.synchronize()

    def window(fn, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return 1e3 * ev0.elapsed_time(ev1) / n  # us

    def alternate(fns, n, warm=20):
        for fn in fns.values():
            for _ in range(warm):
                fn()
        out = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                out[k].append(window(fn, n))
        return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}

    rec = {"clutter": True, "hand": args.hand, "n_obj": G, "batch_each": be, "rows": B, "grid": list(shape), "voxel": args.voxel,
           "stations": K, "rounds": args.rounds, "lib": os.environ.get("GRASPQP_HIP_LIB", "default build")}
    # the stepper: a window is --steps replays of the captured iteration
    rec["stepper_us_per_iteration"] = alternate({k: st.step for k, st in sts.items()}, args.steps, warm=0)
    assert all(torch.isfinite(st.energy).all() for st in sts.values())
    # the launches on their own, on the final state of the stack's stepper (accumulate = 1 into the live buffers, as in an iteration)
    st, one = sts["set"], sts["single"]
    st.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
    one.evaluate(st.hand_pose.clone(), st.contact_idx.clone())
    ptr, sm, f32 = ops._C.stream_ptr, st.samples, ops._C.f32
    e, wr, gr = torch.empty(B, device="cuda"), torch.zeros(B, st.L, 6, device="cuda"), torch.zeros(B, 12, device="cuda")
    Rg, LT, pose = st.Rg.reshape(B, 9), st.link_T.reshape(B, st.L, 12), st.pose_new

    def sliced(call):
        for g in range(G):
            r = slice(g * be, (g + 1) * be)
            call(grids[g], pose[r], Rg[r], LT[r], e[r], wr[r], gr[r])

    grids = [stack.scene(g).grid for g in range(G)]
    sc_slice = lambda grid, p, R, T, ee, w6, g12: ops._scene_call(grid, args.scene_margin, p, sm.points, sm.link, st.L, R, T, None,
                                                                  args.w_scene, ee, 1, w6, g12)
    ap_slice = lambda grid, p, R, T, ee, w6, g12: ops._approach_call(grid, args.scene_margin, args.approach_distance, K, p, sm.points,
                                                                     sm.link, st.L, R, T, spec.grasp_axis, None, args.w_approach,
                                                                     ee, 1, w6, g12)
    rec["scene_launch"] = alternate({"gq_clutter_terms": lambda: st._launch_scene(pose, None, ptr()),
                                     "gq_scene_terms": lambda: one._launch_scene(one.pose_new, None, ptr()),
                                     f"{G} row-slice gq_scene_terms": lambda: sliced(sc_slice)}, 200)
    rec["corridor_launch"] = alternate({"gq_clutter_corridor_terms": lambda: st._launch_approach(pose, None, ptr()),
                                        "gq_approach_terms": lambda: one._launch_approach(one.pose_new, None, ptr()),
                                        f"{G} row-slice gq_approach_terms": lambda: sliced(ap_slice)}, 200)
    # compose: G targets around the object, G parts (the object's own grid, posed around the bin), the bin as the base
    pn = args.part_grid
    part_origin = [float(c) - 0.5 * args.voxel * (pn - 1) for c in center]
    t0 = time.perf_counter()
    part = ops.SceneSDF.from_meshes([fv], part_origin, (pn,) * 3, args.voxel)
    torch.cuda.synchronize()
    rec["part_grid"], rec["part_setup_s"] = [pn] * 3, time.perf_counter() - t0
    gen = torch.Generator().manual_seed(7)
    T = torch.zeros(G, 3, 4)
    for g in range(G):
        q = torch.nn.functional.normalize(torch.randn(4, generator=gen), dim=0)
        w, x, y, z = (float(v) for v in q)
        T[g, :, :3] = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        T[g, :, 3] = 0.12 * (torch.rand(3, generator=gen) * 2 - 1)
    Td, ex = T.cuda().contiguous(), torch.arange(G, dtype=torch.int32, device="cuda")
    out = ops.SceneSDFSet.empty(G, scene.origin, shape, args.voxel)
    far = 0.5 * args.voxel * (pn - 1) * 0.25
    rec["compose_launch"] = alternate({"gq_clutter_compose": lambda: ops.scene_compose(out, Td, [part] * G, Td, ex, scene, far)}, 50, warm=5)
    rec["compose_nodes"], rec["compose_below_far_fraction"] = int(out.values.numel()), float((out.values < far).float().mean())
    # what a user does today: re-voxelise "bin + every object but g" per target, in the target's frame
    fvt = torch.tensor(fv, dtype=torch.float32)
    binm = [torch.tensor(np.asarray(m), dtype=torch.float32) for m in meshes.open_bin(center)]
    t0 = time.perf_counter()
    for g in range(G):
        Rg_, tg = T[g, :, :3], T[g, :, 3]
        world = binm + [fvt @ T[p, :, :3].T + T[p, :, 3] for p in range(G) if p != g]
        ops.SceneSDF.from_meshes([(m - tg) @ Rg_ for m in world], scene.origin, shape, args.voxel)
    torch.cuda.synchronize()
    rec["from_meshes_same_scenes_s"] = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if args.only == "clutter":
    clutter_bench()
    sys.exit(0)
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
        summ["scene_launch_us"] = launch_us(lambda: st._launch_scene(st.pose_new, None, ops._C.stream_ptr()))
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
            scene_us = launch_us(lambda: ref._launch_scene(ref.pose_new, None, ops._C.stream_ptr()))
            summ["approach_launch"]["scene_launch_us_same_inputs"] = scene_us
        keep = st.approach_stations
        for K in (1, 4, 8):
            st.approach_stations = K
            us = launch_us(lambda: st._launch_approach(st.pose_new, None, ops._C.stream_ptr()))
            summ["approach_launch"][f"K{K}"] = {"approach_launch_us": us,
                                                "K_scene_launches_us": None if scene_us is None else K * scene_us}
        st.approach_stations = keep
    f.write(json.dumps(summ) + "\n")
    print(json.dumps(summ), flush=True)
