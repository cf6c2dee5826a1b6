"""Cost of the grasp-set selection (GraspStepper.select) beside the route a user composes from torch, in one process: for
--n_objects objects x --batch_size rows (1 x 256 = BASELINE configs[1]) next to a half-space wall, free for x < --wall, E_scene and
E_approach on, --iters MALA* iterations from initialize(), K = --k picks at --radius,
  select          GraspStepper.select: the FK forward launch, the prepare launch and the select launch;
  op              ops.grasp_select alone on given Rg / link_T (two launches);
  torch           the composed route: world samples (B,Ns,3) by einsum, torch.cdist per object, then per object a host loop with one
                  device read per pick (argmin of the masked scores, suppression by the matrix row);
  matrix / matrix_torch   ops.grasp_distances, and the einsum + cdist part of the torch route alone.
Windows of --steps calls alternate between the routes, --rounds of them, timed with HIP events around work that ends in a
synchronise; median with [min, max].  The record also counts, for the consumer's rule (the K lowest energies of an object), the rows
that are infeasible or lie within the radius of a better one, and says whether the two routes picked the same rows (they can differ where a
pair sits within fp32 rounding of the radius).  Evidence run, not a test: the record is printed and written to --out.

usage: python tools/bench_select.py [--n_objects 1 8] [--batch_size 256] [--k 32] [--radius 0.01] [--out file.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--hand", default="allegro")
ap.add_argument("--n_objects", type=int, nargs="+", default=[1, 8])
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--radius", type=float, default=0.01)
ap.add_argument("--wall", type=float, default=0.12)
ap.add_argument("--margin", type=float, default=0.005)
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
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
be, n, K, radius = args.batch_size, args.n_contact, args.k, args.radius
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


def torch_matrix(hp, Rg, LT, samples, n_obj):
    """(n_obj,be,be) RMS displacement through the world samples"""
    T = LT.view(hp.shape[0], -1, 3, 4)[:, samples.link.long()]  # (B,Ns,3,4)
    xh = torch.einsum("bsij,sj->bsi", T[..., :3], samples.points) + T[..., 3]
    xw = torch.einsum("bij,bsj->bsi", Rg.view(-1, 3, 3), xh) + hp[:, None, :3]
    flat = xw.reshape(n_obj, be, -1)
    return torch.cdist(flat, flat) / samples.Ns ** 0.5


def torch_select(hp, Rg, LT, samples, n_obj, score, feasible):
    """the rule of gq_grasp_select with a host loop: one device read per pick"""
    d = torch_matrix(hp, Rg, LT, samples, n_obj)
    sel = torch.full((n_obj, K), -1, dtype=torch.int32)
    inf = torch.full_like(score[:be], float("inf"))
    for o in range(n_obj):
        alive = feasible[o * be:(o + 1) * be].clone()
        s = score[o * be:(o + 1) * be]
        for it in range(K):
            masked = torch.where(alive, s, inf)
            pick = int(torch.argmin(masked))  # the read
            if not bool(masked[pick] < float("inf")):
                break
            sel[o, it] = o * be + pick
            alive &= d[o, pick] >= radius
            alive[pick] = False
    return sel


cases = {}
for n_obj in args.n_objects:
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 512, oversample=4, seed=3 + i) for i, f in enumerate(fvs)]
    om = ObjectModel(batch_size_each=be, num_samples=512)
    om.initialize_from_meshes(fvs, surface_points_list=sps)
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), be, n, weights=WEIGHTS, seed=1, scene=scene,
                      scene_margin=args.margin, approach_distance=AP_D, approach_stations=AP_K)
    st.set_hulls(om.convex_hulls())
    st.initialize()
    for _ in range(args.iters):
        st.step()
    got = st.select(K, radius=radius)
    Rg, LT = st._select_fk
    tol = [0.0 if k in ("E_scene", "E_approach") else float("inf") for k in st.term_names]
    feasible = got.feasible.bool()
    ref = torch_select(st.hand_pose, Rg, LT, st.samples, n_obj, st.energy, feasible)
    d_hip = ops.grasp_distances(st.hand_pose, Rg, LT, st.samples, be)
    d_torch = torch_matrix(st.hand_pose, Rg, LT, st.samples, n_obj)
    res = alternate({
        "select": lambda: st.select(K, radius=radius),
        "op": lambda: ops.grasp_select(st.hand_pose, Rg, LT, st.samples, be, st.energy, st.terms, tol, K, radius),
        "torch": lambda: torch_select(st.hand_pose, Rg, LT, st.samples, n_obj, st.energy, feasible),
        "matrix": lambda: ops.grasp_distances(st.hand_pose, Rg, LT, st.samples, be),
        "matrix_torch": lambda: torch_matrix(st.hand_pose, Rg, LT, st.samples, n_obj)}, args.steps)
    sel = got.sel.cpu()
    picked = sel[sel >= 0].long()
    sub = [d_hip[o][sel[o][sel[o] >= 0].long() % be][:, sel[o][sel[o] >= 0].long() % be] for o in range(n_obj)]
    min_d = min((float((m + 10.0 * torch.eye(len(m), device=m.device)).min()) for m in sub if len(m) > 1), default=None)
    # the consumer's rule on the same rows: of the K lowest energies, how many are infeasible or within the radius of a better one
    bad = []
    for o in range(n_obj):
        low = torch.argsort(st.energy[o * be:(o + 1) * be], stable=True)[:K]
        dup = torch.tril((d_hip[o][low][:, low] < radius).to(torch.int32), diagonal=-1).any(1)
        bad.append(int((dup | ~feasible[o * be + low]).sum()))
    cases[f"{n_obj}x{be}"] = {
        "rows": n_obj * be, "n_links": st.L, "n_samples": st.samples.Ns, **res,
        "ratio_torch_over_select": res["torch"]["median_us"] / res["select"]["median_us"],
        "ratio_matrix_torch_over_matrix": res["matrix_torch"]["median_us"] / res["matrix"]["median_us"],
        "n_feasible": got.n_feasible.tolist(), "n_selected": got.n_selected.tolist(), "min_pairwise_d_selected": min_d,
        "lowest_energy_rule_infeasible_or_duplicate": bad,
        "same_rows_as_torch": bool(torch.equal(sel, ref)), "max_abs_matrix_difference_m": float((d_hip - d_torch).abs().max()),
        "energy_of_picks_mean": float(st.energy[picked].mean()) if len(picked) else None}

rec = {"select": True, "hand": args.hand, "n_contact": n, "k": K, "radius": radius, "wall_free_for_x_below": args.wall,
       "margin": args.margin, "weights": WEIGHTS, "iters": args.iters, "steps": args.steps, "rounds": args.rounds, "cases": cases}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
