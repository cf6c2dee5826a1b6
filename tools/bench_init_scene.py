"""Cost and effect of the scene-aware initialisation (GraspStepper(init_avoid_scene=True)) beside the unscreened one, in
one process: for --n_objects objects x --batch_size rows (1 x 256 = BASELINE configs[1]; M = 100 x batch_size candidates per object)
with a half-space wall, free for x < --wall, on an 80^3 grid of 5 mm voxels, E_scene and E_approach (4 stations over 0.10 m) on,
  fresh_state   of a stepper without and with the switch: windows of --steps calls alternate between the two, --rounds of them, timed
                with HIP events; median with [min, max], and the ratio of the medians;
  iteration     the captured MALA* iteration of the same stepper, --iter_steps replays per window: the screened call's share of a
                600-iteration period is fresh_state / (600 iterations);
  memory        the bytes of the candidate buffers (draws, poses, points, directions, scores), which scale with n_obj M;
  after initialize()   the share of rows with E_scene > 0 and the mean E_scene, without and with the switch;
and, unless --skip_fit, tools/fit_from_depth.py --esdf 0.06 --n_iter 2000 --reset_epochs 600 as a child process without and with
--init_avoid_scene: mean energy and mean E_scene at the end.  Evidence run, not a test: the record is printed and written to --out.

usage: python tools/bench_init_scene.py [--n_objects 1 8] [--batch_size 256] [--steps 10] [--rounds 5] [--skip_fit] [--out file.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--hand", default="allegro")
ap.add_argument("--n_objects", type=int, nargs="+", default=[1, 8])
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--wall", type=float, default=0.12)
ap.add_argument("--margin", type=float, default=0.005)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--iter_steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--fit_n_iter", type=int, default=2000)
ap.add_argument("--fit_reset_epochs", type=int, default=600)
ap.add_argument("--skip_fit", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_scene_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

assert torch.cuda.is_available(), "this tool measures on the GPU"
SHAPE, H, AP_D, AP_K = (80, 80, 80), 0.005, 0.10, 4
WEIGHTS = {"E_scene": 50.0, "E_approach": 20.0}
hand = ops.HandHandle(get_hand_spec(args.hand))
be, n = args.batch_size, args.n_contact
origin = [-0.5 * H * (s - 1) for s in SHAPE]
x = origin[0] + H * torch.arange(SHAPE[0], dtype=torch.float64)
scene = ops.SceneSDF((args.wall - x).float()[:, None, None].expand(SHAPE).contiguous().cuda(), origin, H)


def window(fn, k):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(k):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / k  # us


def alternate(fns, steps, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, steps))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def stepper(fvs, sps, hulls, avoid):
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), be, n, weights=WEIGHTS, seed=1, scene=scene,
                      scene_margin=args.margin, approach_distance=AP_D, approach_stations=AP_K, init_avoid_scene=avoid)
    st.set_hulls(hulls)
    return st


cases = {}
for n_obj in args.n_objects:
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 512, oversample=4, seed=3 + i) for i, f in enumerate(fvs)]
    om = ObjectModel(batch_size_each=be, num_samples=512)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    hulls = om.convex_hulls()
    plain, screened = stepper(fvs, sps, hulls, False), stepper(fvs, sps, hulls, True)
    res = alternate({"fresh_state_unscreened": plain.fresh_state, "fresh_state_screened": screened.fresh_state}, args.steps)
    after = {}
    for name, st in (("unscreened", plain), ("screened", screened)):
        st.initialize()
        e = st.terms[st.term_row("E_scene")]
        after[name] = {"rows_with_E_scene_gt_0": float((e > 0).float().mean()), "E_scene_mean": float(e.mean()),
                       "rows_with_E_approach_gt_0": float((st.terms[st.term_row("E_approach")] > 0).float().mean())}
    after["screened"]["init_feasible"] = screened.init_feasible.tolist()
    screened.capture()
    for _ in range(20):
        screened.step()
    it = [window(screened.step, args.iter_steps) for _ in range(args.rounds)]
    t_it = float(np.median(it))
    M, J = 100 * be, hand.J
    N = n_obj * M
    floats = {"u_face": N, "u_len": 2 * N, "u_pose": 4 * N, "u_joint": J * N, "cand_pose": (9 + J) * N, "cand_points": 3 * N, "cand_dirs": 3 * N,
              "init_workspace": 7 * N + N, "e_scene": N, "e_approach": N, "penalty": N, "select_workspace": N}
    cases[f"{n_obj}x{be}"] = {
        "rows": n_obj * be, "candidates": N, **res,
        "ratio_screened_over_unscreened": res["fresh_state_screened"]["median_us"] / res["fresh_state_unscreened"]["median_us"],
        "iteration": {"median_us": t_it, "min_us": min(it), "max_us": max(it)},
        "screened_share_of_600_iterations": res["fresh_state_screened"]["median_us"] / (600 * t_it),
        "candidate_buffer_bytes": {**{k: 4 * v for k, v in floats.items()}, "total": 4 * sum(floats.values())},
        "after_initialize": after}

fit = None
if not args.skip_fit:
    fit = {}
    tool = os.path.join(ROOT, "tools", "fit_from_depth.py")
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("unscreened", []), ("screened", ["--init_avoid_scene"])):
            out = subprocess.check_output([sys.executable, tool, "--esdf", "0.06", "--n_iter", str(args.fit_n_iter), "--reset_epochs",
                                           str(args.fit_reset_epochs), "--out", os.path.join(tmp, "fit.jsonl"), *extra], timeout=300)
            r = json.loads(out.decode().strip().splitlines()[-1])
            fit[name] = {k: r[k] for k in ("energy_mean", "E_scene_mean", "rows_in_scene", "init_feasible", "n_iter", "reset_epochs", "batch",
                                           "esdf_max_distance", "scene_margin")}
            fit[name]["ms_per_iteration"] = r["ms"]["per_iteration"]

rec = {"init_scene": True, "hand": args.hand, "n_contact": n, "wall_free_for_x_below": args.wall, "margin": args.margin, "grid": list(SHAPE),
       "voxel": H, "approach": {"distance": AP_D, "stations": AP_K}, "weights": WEIGHTS, "steps": args.steps, "rounds": args.rounds,
       "iter_steps": args.iter_steps, "cases": cases, "fit_from_depth_esdf_0.06": fit}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
