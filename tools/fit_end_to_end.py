"""The reference's whole fit.py flow on the bench scene, on the device: initialize_convex_hull (fit.py:315) -> n_iter
MALA* iterations with z-score resets every `reset_epochs` (fit.py:399-458) -> export_poses (.dexgrasp.pt, fit.py:224-300),
then three independent checks of what came out:

  * the final energies re-evaluated through the class surface (HandModel / ObjectModel / calculate_energy: the autograd
    route, separate launches) must equal the stepper's accepted energies;
  * a sample of rows re-evaluated by the CPU oracle (fp64);
  * the exported files reloaded with torch.load(weights_only=True) and assembled the way the reference's consumer does
    (graspqp_isaaclab/.../utils/data.py:105-140).

Evidence run, not a test: writes one JSON record (default gpurun_out/fit_end_to_end.json).

usage: python tools/fit_end_to_end.py [--n_objects 1] [--batch_size 256] [--n_iter 7000] [--out file.json]
       [--w_squeeze 0] [--squeeze_min_travel 5e-3] [--squeeze_damping 1e-3]   (contact closing feasibility, E_squeeze)
       [--hold_mass 0] [--hold_max_force 20] [--hold_tol 0.05]   (payload holding: export only the grasps that carry this mass)
       [--w_reach 0] [--arm arm7|file.urdf] [--arm_tip LINK] [--arm_base X Y Z YAW] [--reach_stations 0]   (arm reachability, E_reach)
       [--w_track 0] [--track_waypoints 8] [--track_updates 3] [--arm_on_track]   (approach tracking, E_track: needs --w_reach > 0 and
                                                                                   --reach_stations >= 1; the path is exported as arm_path)
       [--w_arm 0] [--arm_margin 0] [--arm_sphere_radius 0.05] [--arm_sphere_spacing 0.08]   (arm clearance, E_arm: needs --w_reach > 0)
       [--w_wall 0] [--w_prior 0]   (scripts/fit.py:77-78: tabletop synthesis; the class surface and the oracle then carry
       E_wall / E_prior on the stepper's surface samples, st.samples)
       [--w_scene 0] [--scene_margin 0] [--scene box]   (scene obstacles: the ``box`` preset is an open-topped bin of five slabs
       around the first object, voxelised on an 80^3 grid of 5 mm by ops.SceneSDF.from_meshes; the class surface carries E_scene)
       [--w_approach 0] [--approach_distance 0.10] [--approach_stations 4]   (approach corridor against the same preset; the class
       surface carries E_approach through HandModel.set_approach)
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--hand", default="allegro")
ap.add_argument("--n_objects", type=int, default=1)
ap.add_argument("--batch_size", type=int, default=256)
ap.add_argument("--n_contact", type=int, default=12)
ap.add_argument("--n_iter", type=int, default=7000)
ap.add_argument("--reset_epochs", type=int, default=600)
ap.add_argument("--oracle_rows", type=int, default=6)
ap.add_argument("--w_wall", type=float, default=0.0)
ap.add_argument("--w_prior", type=float, default=0.0)
ap.add_argument("--w_scene", type=float, default=0.0)
ap.add_argument("--scene_margin", type=float, default=0.0)
ap.add_argument("--scene", choices=("box",), default="box")
ap.add_argument("--w_approach", type=float, default=0.0)
ap.add_argument("--approach_distance", type=float, default=0.10)
ap.add_argument("--approach_stations", type=int, default=4)
ap.add_argument("--w_squeeze", type=float, default=0.0)
ap.add_argument("--squeeze_min_travel", type=float, default=5e-3)
ap.add_argument("--squeeze_damping", type=float, default=1e-3)
ap.add_argument("--w_reach", type=float, default=0.0)
ap.add_argument("--arm", default="arm7")  # a preset of graspqp_amd.arm, or a URDF file (then --arm_tip, optionally --arm_base_link)
ap.add_argument("--w_arm", type=float, default=0.0)  # arm clearance: the arm's link spheres on the ``box`` scene
ap.add_argument("--arm_margin", type=float, default=0.0)
ap.add_argument("--arm_sphere_radius", type=float, default=0.05)
ap.add_argument("--arm_sphere_spacing", type=float, default=0.08)
ap.add_argument("--arm_tip", default=None)
ap.add_argument("--arm_base_link", default=None)
ap.add_argument("--arm_base", type=float, nargs=4, default=(-0.45, 0.0, -0.3, 0.0), metavar=("X", "Y", "Z", "YAW"))
ap.add_argument("--reach_stations", type=int, default=0)
ap.add_argument("--reach_distance", type=float, default=0.10)
ap.add_argument("--w_track", type=float, default=0.0)  # approach tracking: one continuous arm path along the retreat line
ap.add_argument("--track_waypoints", type=int, default=8)
ap.add_argument("--track_updates", type=int, default=3)
ap.add_argument("--arm_on_track", action="store_true")  # E_arm at the path's configurations (needs --w_arm and --w_track)
ap.add_argument("--hold_mass", type=float, default=0.0)  # payload holding: > 0 gates the selection on carrying this mass (kg)
ap.add_argument("--hold_max_force", type=float, default=20.0)  # newtons per cone edge
ap.add_argument("--hold_tol", type=float, default=0.05)  # largest unheld share |r| / |w| of a load that still counts as held
ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "fit_end_to_end.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.core.energy import calculate_energy
from graspqp_amd.core.hand_model import HandModel
from graspqp_amd.core.object_model import ObjectModel
from graspqp_amd.export import export_poses
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.metrics import GraspSpanMetricFactory
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

W = {"E_dis": 100.0, "E_fc": 1.0, "E_pen": 100.0, "E_spen": 10.0, "E_joints": 1.0}  # fit.py:51-55
TABLETOP = args.w_wall > 0 or args.w_prior > 0
if TABLETOP:
    W.update({"E_prior": args.w_prior, "E_wall": args.w_wall})  # fit.py:369-370
SCENE = args.w_scene > 0
if SCENE:
    W["E_scene"] = args.w_scene
APPROACH = args.w_approach > 0
if APPROACH:
    W["E_approach"] = args.w_approach
SQUEEZE = args.w_squeeze > 0  # contact closing feasibility (E_squeeze: the reference's E_manipulativity as one launch)
if SQUEEZE:
    W["E_squeeze"] = args.w_squeeze
REACH = args.w_reach > 0  # arm reachability (E_reach: batched wrist IK as one launch)
reach_kw = {}
if REACH:
    from graspqp_amd.arm import arm_from_arg, base_from_arg

    W["E_reach"] = args.w_reach
    reach_kw = dict(arm=arm_from_arg(args.arm, args.arm_tip, args.arm_base_link), arm_base=base_from_arg(args.arm_base),
                    reach_stations=args.reach_stations, reach_distance=args.reach_distance)
ARM = args.w_arm > 0  # arm clearance (E_arm: the arm's collision spheres on the scene grid, one launch after the reach launch)
if ARM:
    if not REACH:
        ap.error("--w_arm needs --w_reach > 0")
    W["E_arm"] = args.w_arm
    reach_kw["arm"] = reach_kw["arm"].with_link_spheres(args.arm_sphere_radius, args.arm_sphere_spacing)
TRACK = args.w_track > 0  # approach tracking (E_track: the straight approach line followed from reach_q[:, K], one launch)
if TRACK:
    if not REACH or args.reach_stations < 1:
        ap.error("--w_track needs --w_reach > 0 and --reach_stations >= 1")
    W["E_track"] = args.w_track
    reach_kw.update(track_waypoints=args.track_waypoints, track_updates=args.track_updates)
if args.arm_on_track:
    if not (TRACK and ARM):
        ap.error("--arm_on_track needs --w_track > 0 and --w_arm > 0")
    reach_kw["arm_on_track"] = True
spec = get_hand_spec(args.hand)
n_obj, be, n = args.n_objects, args.batch_size, args.n_contact
B = n_obj * be
codes = [f"superquadric_{o}" for o in range(n_obj)]
fvs = [meshes.superquadric(o) for o in range(n_obj)]
sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
om = ObjectModel(batch_size_each=be, num_samples=2500)
om.initialize_from_meshes(fvs, codes, surface_points_list=sps)
hand = ops.HandHandle(spec)
weights = {"E_prior": args.w_prior, "E_wall": args.w_wall} if TABLETOP else {}
scene = None
if SCENE or APPROACH or ARM:  # the ``box`` preset: an open-topped bin around the first object
    center = 0.5 * (fvs[0].reshape(-1, 3).min(0) + fvs[0].reshape(-1, 3).max(0))
    scene = ops.SceneSDF.from_meshes(meshes.open_bin(center), [float(c) - 0.5 * 0.005 * 79 for c in center], (80, 80, 80), 0.005)
    if SCENE:
        weights["E_scene"] = args.w_scene
    if APPROACH:
        weights["E_approach"] = args.w_approach
if SQUEEZE:
    weights["E_squeeze"] = args.w_squeeze
if REACH:
    weights["E_reach"] = args.w_reach
if ARM:
    weights["E_arm"] = args.w_arm
    reach_kw.update(arm_scene=scene, arm_margin=args.arm_margin)
if TRACK:
    weights["E_track"] = args.w_track
st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), be, n, seed=1, weights=weights or None, scene=scene,
                  scene_margin=args.scene_margin, approach_distance=args.approach_distance, approach_stations=args.approach_stations,
                  squeeze_min_travel=args.squeeze_min_travel, squeeze_damping=args.squeeze_damping, **reach_kw)
st.set_hulls(om.convex_hulls())
st.initialize()  # on-device initialize_convex_hull + the first evaluation
e0, t0_terms = st.energy.clone(), st.terms.clone()
st.capture(iters=8)
trace = []


def cb(step):
    if step % 500 == 0:
        e = st.energy
        trace.append({"step": int(step), "mean": float(e.mean()), "min": float(e.min()), "max": float(e.max()),
                      "accept": float(st.accept.float().mean())})


torch.cuda.synchronize()
t0 = time.time()
st.run(args.n_iter, reset_epochs=args.reset_epochs, z_score_threshold=1.0, callback=cb)
torch.cuda.synchronize()
dt = time.time() - t0
assert torch.isfinite(st.energy).all() and torch.isfinite(st.hand_pose).all()

# ---- (1) class surface (autograd route, separate launches) on the final state -------------------------------------------
hm = HandModel(spec, "cuda")
hp = st.hand_pose.clone().requires_grad_()
hm.set_parameters(hp, st.contact_idx.clone())
if TABLETOP or SCENE or APPROACH:
    hm.set_surface_points(st.samples.points.cpu().numpy(), st.samples.link.cpu().numpy())
if SCENE or APPROACH:
    hm.set_scene(scene, args.scene_margin)
if APPROACH:
    hm.set_approach(args.approach_distance, args.approach_stations)
if SQUEEZE:
    hm.set_squeeze(args.squeeze_min_travel, args.squeeze_damping)
if REACH:
    hm.set_reach(reach_kw["arm"], reach_kw["arm_base"], args.reach_distance, args.reach_stations)
if ARM:
    hm.set_arm_scene(scene, args.arm_margin)
if TRACK:
    hm.set_track(args.track_waypoints, args.track_updates)
metric = GraspSpanMetricFactory.create(GraspSpanMetricFactory.MetricType.GRASPQP, {"friction": 0.2, "max_limit": 20.0, "n_cone_vecs": 4})
losses = calculate_energy(hm, om, energy_fnc=metric, method="gendexgrasp", svd_gain=0.1,
                          energy_names=(["E_prior", "E_wall"] if TABLETOP else []) + (["E_scene"] if SCENE else []) +
                          (["E_approach"] if APPROACH else []) + (["E_squeeze"] if SQUEEZE else []) +
                          (["E_reach"] if REACH else []) + (["E_arm"] if ARM and not args.arm_on_track else []) +
                          (["E_track"] if TRACK else []))
# (with --arm_on_track E_arm reads the tracked path: the class surface has no such switch, the term is taken from the stepper)
total_cls = sum(W[k] * (losses[k] if k in losses else st.terms[list(st.term_names).index(k)]) for k in W)
rel_cls = ((total_cls.detach() - st.energy).abs() / st.energy.abs().clamp_min(1e-6))

# ---- (2) the CPU oracle (fp64) on a few rows ------------------------------------------------------------------------------
import ref_cpu
from ref_cpu import models as omodels

rows = torch.linspace(0, be - 1, args.oracle_rows).long().tolist()
oh = omodels.OracleHand(spec, torch.float64)
oo = omodels.OracleObject([fvs[0]], [sps[0]], len(rows), torch.float64)
if TABLETOP:
    oh.surface_points, oh.surface_link = st.samples.points.double().cpu().numpy(), st.samples.link.cpu().numpy()
oh.set_parameters(st.hand_pose[rows].double().cpu(), st.contact_idx[rows].cpu())
lo = ref_cpu.calculate_energy(oh, oo, box_form=True)
# every term but E_fc row by row (E_fc's stop rule is batch-global: it is compared on whole batches in tests/)
rel_oracle = {}
names = list(st.term_names)
for k in ("E_dis", "E_pen", "E_spen", "E_joints"):
    got = st.terms[names.index(k)][rows].double().cpu()
    rel_oracle[k] = float(((got - lo[k]).abs() / lo[k].abs().clamp_min(1e-4)).max())
if TABLETOP:
    from ref_cpu import energy as oenergy

    for k, v in oenergy.optional_terms(oh).items():
        got = st.terms[names.index(k)][rows].double().cpu()
        rel_oracle[k] = float(((got - v).abs() / v.abs().clamp_min(1e-4)).max())

# ---- (3) export + reload the way the consumer does ----------------------------------------------------------------------
hold = selection = hold_rec = None
if args.hold_mass > 0:  # can the accepted grasps carry the object, at rest and braking at 3 m/s^2?  Only those are exported.
    from graspqp_amd import ops

    hold = st.hold(ops.hold_loads(args.hold_mass, accelerations=((0, 0, 0), (3, 0, 0), (0, 3, 0))), args.hold_max_force)
    held = hold.resid.amax(1) <= args.hold_tol
    selection = st.select(be, radius=0.0, score=torch.where(held, st.energy, torch.inf))
    hold_rec = {"mass_kg": args.hold_mass, "max_force_N": args.hold_max_force, "tol": args.hold_tol, "rows_held": int(held.sum()),
                "n_selected": selection.n_selected.cpu().tolist(), "E_hold_mean": float(hold.e.mean()),
                "largest_contact_force_N": float(hold.force.norm(dim=-1).max()), "largest_joint_torque_Nm": float(hold.torque.abs().max())}
with tempfile.TemporaryDirectory() as tmp:
    hm.set_parameters(st.hand_pose.clone(), st.contact_idx.clone())
    files = export_poses(hm, st.energy.clone(), om, codes, be, tmp, args.hand, n, "graspqp", suffix="",  # fit.py:521
                         arm_path=st.track_q if TRACK else None, hold=hold, selection=selection)
    data = torch.load(files[0], weights_only=True)
    jn = list(spec.joint_names)
    params = torch.cat([data["parameters"]["root_pose"], torch.stack([data["parameters"][k] for k in jn], -1)], -1)
    vel = torch.stack([data["grasp_velocities_off"][k] + 0.1 * data["grasp_velocities"][k] for k in jn], -1)
    export = {"files": [os.path.relpath(f, tmp) for f in files], "keys": sorted(data), "params_shape": list(params.shape),
              "velocities_finite": bool(torch.isfinite(vel).all()), "quaternion_norm_max_dev": float((params[:, 3:7].norm(dim=-1) - 1).abs().max()),
              "bytes": os.path.getsize(files[0])}

best = torch.topk(-st.energy, min(5, B)).indices
rec = {
    "what": "reference fit.py flow on the device: initialize_convex_hull -> MALA* schedule with z-score resets -> export_poses",
    "hand": args.hand, "n_objects": n_obj, "batch_size": be, "n_contact": n, "n_iter": args.n_iter, "reset_epochs": args.reset_epochs,
    "graph_mode": st.graph_mode, "wall_s": dt, "evals_per_s_including_host_callbacks_and_resets": B * args.n_iter / dt,
    "energy_mean_initial": float(e0.mean()), "energy_mean_final": float(st.energy.mean()), "energy_min_final": float(st.energy.min()),
    "terms_mean_initial": {k: float(t0_terms[i].mean()) for i, k in enumerate(names)},
    "terms_mean_final": {k: float(st.terms[i].mean()) for i, k in enumerate(names)},
    "best_rows": [{"row": int(i), "E": float(st.energy[i]), **{k: float(st.terms[j][i]) for j, k in enumerate(names)}} for i in best],
    "trace": trace,
    "check_class_surface_rel_err": {"median": float(rel_cls.median()), "max": float(rel_cls.max())},
    "check_oracle_fp64_rel_err_max_over_rows": rel_oracle, "oracle_rows": rows,
    "export": export,
}
if hold_rec is not None:
    rec["hold"] = hold_rec
assert rec["energy_mean_final"] < rec["energy_mean_initial"]
assert rec["check_class_surface_rel_err"]["median"] < 1e-4
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(rec, open(args.out, "w"), indent=1)
print(json.dumps({k: rec[k] for k in ("wall_s", "energy_mean_initial", "energy_mean_final", "energy_min_final",
                                      "check_class_surface_rel_err", "check_oracle_fp64_rel_err_max_over_rows", "export")}))
