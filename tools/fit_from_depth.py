"""Depth frames -> scene grid -> target object -> grasp set without a mesh anywhere: the tool renders
--views labelled depth images of a sphere resting on a table from cameras on a ring, fuses
  a scene volume   ops.SceneTSDF.integrate with skip = the sphere's label (the target is no obstacle of its own scene), and
  a target volume  the same frames through ops.keep_label (only the sphere's pixels measure), at a finer voxel about the target,
turns the target volume into an oriented point cloud on the device (SceneTSDF.extract_clouds -> ObjectModel.initialize_from_tsdf),
and runs GraspStepper with E_scene on the scene volume and the extracted cloud as the object.  With --esdf MAX_DISTANCE the stepper reads
the Euclidean distance field of the scene volume instead (SceneTSDF.esdf), which allows a --scene_margin above trunc.  It reports the number of surfels,
With --init_avoid_scene the initial poses and those of every reset are screened against that field; --reset_epochs N
turns the z-score resets of the reference's schedule on (default: none).  The tool also fuses a second scene volume of the same
frames WITHOUT skip, so the target stays in it: the grid of the pre-grasp term, whose station 0 is the opened hand at the
grasp pose (with --esdf that volume's ESDF).  --w_pregrasp W > 0 puts the term into the energy; either way the final grasp set is
evaluated with ops.pregrasp_terms and the mean E_pregrasp and the share of rows with E_pregrasp > 0 are reported.  --select K
--select_radius R ends with GraspStepper.select and appends n_feasible, n_selected, the smallest pairwise distance among the
selected and, for the consumer's rule (the K lowest energies), how many of those rows are infeasible or lie within R of a better one.
It reports the number of surfels,
how far they lie from the true sphere, the mean energy and the mean E_scene before and after --n_iter iterations, and the wall
times of the stages (each closed by a synchronisation).  Evidence run, not a test: one JSON line is printed and appended to --out.

usage: python tools/fit_from_depth.py [--views 8] [--batch_size 64] [--n_iter 400] [--esdf 0.06 --scene_margin 0.03]
       [--init_avoid_scene] [--reset_epochs 600] [--w_pregrasp 30 --pregrasp_opening 0.5 --pregrasp_stations 4]
       [--select 8 --select_radius 0.01] [--out file.jsonl]
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
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--batch_size", type=int, default=64)
ap.add_argument("--n_contact", type=int, default=4)
ap.add_argument("--n_iter", type=int, default=400)
ap.add_argument("--num_samples", type=int, default=512)
ap.add_argument("--min_weight", type=float, default=2.0)
ap.add_argument("--hand", default="allegro")
ap.add_argument("--esdf", type=float, default=None, metavar="MAX_DISTANCE", help="run the stepper on scene.esdf(MAX_DISTANCE)")
ap.add_argument("--scene_margin", type=float, default=0.005)
ap.add_argument("--init_avoid_scene", action="store_true", help="screen the initial and the re-initialised poses against the scene")
ap.add_argument("--reset_epochs", type=int, default=None, help="z-score resets every N iterations (default: no resets)")
ap.add_argument("--w_pregrasp", type=float, default=0.0, help="weight of E_pregrasp (0: evaluated at the end only)")
ap.add_argument("--pregrasp_opening", type=float, default=0.5)
ap.add_argument("--pregrasp_stations", type=int, default=4)
ap.add_argument("--select", type=int, default=0, metavar="K", help="select the K best feasible, distinct grasps at the end (DESIGN 22)")
ap.add_argument("--select_radius", type=float, default=0.01, metavar="R", help="grasps closer than R metres (RMS hand surface) are one grasp")
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "fit_from_depth.jsonl"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper

assert torch.cuda.is_available(), "this tool runs on the GPU"
W, H = args.width, args.height
K = (525.0 * W / 640, 525.0 * W / 640, 0.5 * (W - 1), 0.5 * (H - 1))
RANGE = (0.05, 5.0)
SPHERE = (np.array([0.0, 0.0, 0.05]), 0.05)  # resting on the table z = 0; label 1, the table label 0
LOOK = np.array([0.0, 0.0, 0.05])


def look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32)


def render(T):
    """z-depth and labels (0 table, 1 sphere) from the pose T (3,4)."""
    T = T.astype(np.float64)
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dw = np.stack([(col - K[2]) / K[0], (row - K[3]) / K[1], np.ones_like(col)], -1) @ T[:, :3].T
    o = T[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        sp = -o[2] / dw[..., 2]
        sp = np.where(np.isfinite(sp) & (sp > 0), sp, np.inf)
        a, b, q = (dw * dw).sum(-1), (dw * (o - SPHERE[0])).sum(-1), ((o - SPHERE[0]) ** 2).sum() - SPHERE[1] ** 2
        disc = b * b - a * q
        ss = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / a, np.inf)
    depth = np.minimum(sp, ss)
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32), (ss < sp).astype(np.int32)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.time() - t0)


cams = np.stack([look_at(LOOK + 0.6 * np.array([np.cos(a) * 0.75, np.sin(a) * 0.75, 0.66]), LOOK)
                 for a in np.linspace(0.0, 2 * np.pi, args.views, endpoint=False)])
imgs = [render(T) for T in cams]
depth = torch.as_tensor(np.stack([i[0] for i in imgs])).cuda()
labels = torch.as_tensor(np.stack([i[1] for i in imgs])).cuda()
cam_T = torch.as_tensor(cams).cuda().reshape(args.views, 12).contiguous()

# the surroundings: one world grid of 5 mm voxels, the sphere's rays taken as free
S_SHAPE, S_H, S_TRUNC = (80, 80, 80), 0.005, 0.02
scene = ops.SceneTSDF([-0.5 * S_H * 79, -0.5 * S_H * 79, -0.1], S_SHAPE, S_H, S_TRUNC)
skip = torch.tensor([1], dtype=torch.int32, device="cuda")
# the surroundings AND the target, for the pre-grasp term: the same grid, nothing skipped
whole = ops.SceneTSDF([-0.5 * S_H * 79, -0.5 * S_H * 79, -0.1], S_SHAPE, S_H, S_TRUNC)
# the target: 2.5 mm voxels about the sphere, only its own pixels
T_SHAPE, T_H = (56, 56, 56), 0.0025
target = ops.SceneTSDF([float(c) - 0.5 * T_H * 55 for c in SPHERE[0]], T_SHAPE, T_H, 3 * T_H, n_grids=1)
for t in (scene, target):  # warm-up: the first launch of a kernel loads its code object
    t.integrate(ops.keep_label(depth[:1], labels[:1], 1), K, cam_T[:1], depth_range=RANGE).reset()
_, ms_scene = timed(lambda: scene.integrate(depth, K, cam_T, labels=labels, skip=skip, depth_range=RANGE))
_, ms_whole = timed(lambda: whole.integrate(depth, K, cam_T, labels=labels, depth_range=RANGE))
_, ms_target = timed(lambda: target.integrate(ops.keep_label(depth, labels, 1), K, cam_T, depth_range=RANGE))
target.extract_clouds(args.min_weight)  # warm-up of the three kernels
clouds, ms_extract = timed(lambda: target.extract_clouds(args.min_weight))
p, nrm = (x.double().cpu().numpy() for x in clouds[0])
d = p - SPHERE[0]
radial = np.abs(np.linalg.norm(d, axis=1) - SPHERE[1])
cosang = np.clip((nrm * d).sum(1) / np.linalg.norm(d, axis=1), -1, 1)
angle = np.degrees(np.arccos(cosang))

be, n = args.batch_size, args.n_contact
om = ObjectModel(batch_size_each=be, num_samples=args.num_samples)
_, ms_object = timed(lambda: om.initialize_from_tsdf(target, min_weight=args.min_weight))
weights = {"E_scene": 50.0}
field, ms_esdf = scene.scene, None
if args.esdf is not None:
    scene.esdf(args.esdf)  # warm-up: the output, the workspace and the kernels' code objects
    field, ms_esdf = timed(lambda: scene.esdf(args.esdf))
pre_field = whole.scene if args.esdf is None else whole.esdf(args.esdf)
if args.w_pregrasp > 0:
    weights["E_pregrasp"] = args.w_pregrasp
PG = dict(distance=0.10, stations=args.pregrasp_stations, opening=args.pregrasp_opening)
st = GraspStepper(ops.HandHandle(get_hand_spec(args.hand)), om._cloudset, om.surface_points_each, be, n, seed=1, weights=weights,
                  scene=field, scene_margin=args.scene_margin, init_avoid_scene=args.init_avoid_scene, pregrasp_scene=pre_field,
                  pregrasp_distance=PG["distance"], pregrasp_stations=PG["stations"], pregrasp_opening=PG["opening"])
st.set_hulls(om.convex_hulls())
st.initialize()
names = list(st.term_names)
e0, s0 = st.energy.clone(), st.terms[names.index("E_scene")].clone()
feasible0 = st.init_feasible.tolist() if args.init_avoid_scene else None
st.capture(iters=8)
_, ms_run = timed(lambda: st.run(args.n_iter, reset_epochs=args.reset_epochs))
e1, s1 = st.energy, st.terms[names.index("E_scene")]
assert torch.isfinite(e1).all() and torch.isfinite(st.hand_pose).all()
dis, _ = om.cal_distance(st.cpts)


def pregrasp_of(pose, idx):
    """E_pregrasp (B) of a grasp set through the op, whatever the weight the run had."""
    Rg, LT, _, _, _, ws = ops.fk_contacts(pose, idx, st.hand)
    return ops.pregrasp_terms(pose, st.hand, st.samples, idx, Rg, LT, ws, pre_field, st.hand.spec.grasp_axis, PG["distance"], PG["stations"],
                              PG["opening"], None, args.scene_margin)


p1 = pregrasp_of(st.hand_pose, st.contact_idx)


def selection_record(K, R):
    """GraspStepper.select beside the consumer's rule (the K lowest energies) on the same rows; the objects are looked at one by one"""
    sel = st.select(K, radius=R)
    Rg, LT = st._select_fk
    d = ops.grasp_distances(st.hand_pose, Rg, LT, st.samples, be).cpu()
    feasible, energy, picks = sel.feasible.bool().cpu(), st.energy.cpu(), sel.sel.cpu().long()
    min_d, bad = [], []
    for o in range(d.shape[0]):
        rows = picks[o][picks[o] >= 0] - o * be
        min_d.append(float(d[o][rows][:, rows].clone().fill_diagonal_(float("inf")).min()) if len(rows) > 1 else None)
        low = torch.argsort(energy[o * be:(o + 1) * be], stable=True)[:K]
        bad.append(sum(1 for i, r in enumerate(low.tolist()) if not feasible[o * be + r] or (i > 0 and bool((d[o][r][low[:i]] < R).any()))))
    return {"k": K, "radius": R, "n_feasible": sel.n_feasible.tolist(), "n_selected": sel.n_selected.tolist(),
            "min_pairwise_d_selected": min_d, "lowest_energy_rule_infeasible_or_duplicate": bad}


selected = selection_record(args.select, args.select_radius) if args.select > 0 else None

rec = {"fit_from_depth": True, "hand": args.hand, "views": args.views, "image": [W, H], "batch": be, "n_contact": n, "n_iter": args.n_iter,
       "scene_grid": list(S_SHAPE), "scene_voxel": S_H, "target_grid": list(T_SHAPE), "target_voxel": T_H, "min_weight": args.min_weight,
       "esdf_max_distance": args.esdf, "scene_margin": args.scene_margin, "init_avoid_scene": args.init_avoid_scene,
       "reset_epochs": args.reset_epochs, "init_feasible": feasible0,
       "rows_in_scene": {"before": float((s0 > 0).float().mean()), "after": float((s1 > 0).float().mean())},
       "surfels": int(len(p)), "radius_used": float(om._cloudset.radius[0]),
       "radial_error_mm": {"median": 1e3 * float(np.median(radial)), "max": 1e3 * float(radial.max())},
       "normal_angle_deg": {"median": float(np.median(angle)), "p99": float(np.percentile(angle, 99)), "max": float(angle.max())},
       "energy_mean": {"before": float(e0.mean()), "after": float(e1.mean())},
       "E_scene_mean": {"before": float(s0.mean()), "after": float(s1.mean())},
       "w_pregrasp": args.w_pregrasp, "pregrasp": dict(PG, margin=args.scene_margin, grid="esdf" if args.esdf is not None else "tsdf"),
       "E_pregrasp_mean_after": float(p1.mean()), "rows_with_E_pregrasp_after": float((p1 > 0).float().mean()),
       "contact_distance_mm_mean_abs_after": 1e3 * float(dis.abs().mean()), "select": selected,
       "ms": {"integrate_scene": ms_scene, "integrate_whole_scene": ms_whole, "integrate_target_with_keep_label": ms_target, "extract_clouds": ms_extract,
              "initialize_from_tsdf": ms_object, "esdf": ms_esdf, "run": ms_run, "per_iteration": ms_run / args.n_iter}}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write(json.dumps(rec) + "\n")
print(json.dumps(rec), flush=True)
