"""Finger closing measured on the device -> profiles/close_bench.json (one JSON object).

  launch   gq_close_fingers replayed from a captured graph at 256 and 2 048 rows, S = 8 and 32, Allegro with 512 surface samples, on
           a sphere grid the opened hand closes onto.  Next to it, in the same call, the route COMPOSED from existing ops: per round
           one FK forward (ops.fk_contacts), the samples moved by torch, ops.scene_distance, a torch per-link minimum
           (scatter_reduce), the touch / stop masks and the clamped update -- S + 1 rounds.  Both are replayed from a graph where
           they capture; --calls replays per window, the two routes alternating, medians of --rounds windows.
  stepper  GraspStepper.close() end to end (host time per call, the device drained) at 1 x 256 and 8 x 256 rows.
  grasps   a 256-row run of --iterations iterations, with and without E_squeeze: the share of rows with >= 2 and >= 3 touching links
           after close(), the mean overshoot max(-phi, 0) of the touching links, and hold() on the ideal contacts beside
           hold(closed=) on the contacts that exist."""
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
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rows", default="256,2048")
ap.add_argument("--iterations", type=int, default=300)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "close_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops
from graspqp_amd.hands import get_hand_spec
from graspqp_amd.stepper import GraspStepper
from graspqp_amd.utils import meshes

spec = get_hand_spec("allegro")
hand = ops.HandHandle(spec)
pts, lnk = meshes.hand_surface_samples(spec, 512)
samples = ops.SurfaceSamples(hand, pts, lnk)
L, JA = hand.L, hand.J
TOUCH = 5e-4
step_np = ops.close_default_step(spec)
step = torch.from_numpy(step_np).cuda()
masks = ops.close_stop_masks(hand)
mask_bits = torch.tensor([[(int(m) >> l) & 1 for l in range(L)] for m in ops.close_stop_masks_host(spec)], dtype=torch.bool).cuda()
lo, hi = torch.tensor(np.asarray(spec.joints_lower, np.float32)).cuda(), torch.tensor(np.asarray(spec.joints_upper, np.float32)).cuda()


def window(fn, n_calls):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n_calls):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / n_calls  # us


def captured(fn, what):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g):
            fn()
    except Exception as ex:  # noqa: BLE001 -- recorded, the eager route is timed instead
        print(f"[bench_close] {what} does not capture ({type(ex).__name__}); timed eagerly", flush=True)
        torch.cuda.synchronize()
        return None
    return g.replay


def sphere_grid(radius=0.04, n=64, h=0.005):
    o = -0.5 * (n - 1) * h
    ax = o + h * torch.arange(n, dtype=torch.float64)
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    return ops.SceneSDF((x.norm(dim=-1) - radius).float().cuda(), [o, o, o], h)


rec = {"close_bench": True, "hand": "allegro", "n_samples": 512, "touch": TOUCH, "rounds": args.rounds, "calls_per_window": args.calls,
       "device": torch.cuda.get_device_name(0), "launch": {}}
grid = sphere_grid()
grids = ops._pregrasp_grids(grid.values, grid.origin, grid.voxel)
gen = torch.Generator().manual_seed(0)
for B in map(int, args.rows.split(",")):
    # the opened hand with the sphere in front of the palm: the fingers close onto it
    th0 = torch.tensor(np.asarray(spec.joints_lower, np.float32) + 0.1 * (np.asarray(spec.joints_upper, np.float32) - np.asarray(spec.joints_lower, np.float32)))
    hp = torch.cat([torch.zeros(B, 3), torch.randn(B, 6, generator=gen), th0[None] + 0.02 * torch.randn(B, JA, generator=gen)], 1).float().cuda()
    idx = torch.zeros(B, 1, dtype=torch.long, device="cuda")
    Rg = ops.fk_contacts(hp, idx, hand)[0].contiguous()
    axis = torch.tensor(np.asarray(spec.grasp_axis, np.float32)).cuda()
    hp[:, :3] = -(Rg @ axis) * 0.11 + 0.004 * torch.randn(B, 3, generator=gen).cuda()  # the palm 11 cm from the centre, facing it
    v = (0.5 + 0.5 * torch.rand(B, JA, generator=gen)).cuda()
    for S in (8, 32):
        out = ops._close_outputs(hp, L)

        def fused():
            ops._close_call(hand, grids, samples.points, samples.link, hp, Rg, v, S, step, TOUCH, masks, *out)

        link = samples.link.long()

        def composed():
            u = v / step
            delta = step * (u / u.abs().amax(1, keepdim=True))
            theta = hp[:, 9:].clone()
            touched = torch.zeros(B, L, dtype=torch.bool, device="cuda")
            tstep = torch.full((B, L), -1, dtype=torch.int32, device="cuda")
            for s in range(S + 1):
                pose = torch.cat([hp[:, :9], theta], 1)
                R, LT = ops.fk_contacts(pose, idx, hand)[:2]
                T = LT[:, link]  # (B,Ns,3,4)
                xh = (T[..., :3] @ samples.points[None, :, :, None]).squeeze(-1) + T[..., 3]
                x = xh @ R.transpose(1, 2) + hp[:, None, :3]
                phi = ops.scene_distance(x, grid)  # +inf outside the volume
                m = torch.full((B, L), float("inf"), device="cuda").scatter_reduce(1, link[None].expand(B, -1), phi, "amin")
                new = ~touched & (m <= TOUCH)
                tstep = torch.where(new, s, tstep)
                touched = touched | new
                stopped = (touched[:, None, :] & mask_bits[None]).any(-1)
                if s < S:
                    theta = torch.where(stopped, theta, torch.minimum(torch.maximum(theta + delta, lo), hi))
            return theta, tstep, m

        fused()
        th_c, ts_c, m_c = composed()
        torch.cuda.synchronize()
        agree = {"touch_step_equal_share": float((out[1] == ts_c).float().mean()), "theta_max_abs": float((out[0] - th_c).abs().max()),
                 "rows_with_2_touching": float(((out[1] >= 0).sum(1) >= 2).float().mean())}
        fns = {"gq_close_fingers": captured(fused, "the launch") or fused}
        cg = captured(composed, "the composed route")
        fns["composed_route"] = cg or composed
        for fn in fns.values():
            for _ in range(3):
                fn()
        t = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                t[key].append(window(fn, args.calls if key == "gq_close_fingers" else max(args.calls // 10, 3)))
        r_ = {key: {"median_us": float(np.median(x)), "min_us": min(x), "max_us": max(x)} for key, x in t.items()}
        r_.update({"rows": B, "steps": S, "composed_mode": "graph" if cg else "eager", "agreement": agree,
                   "us_per_row": r_["gq_close_fingers"]["median_us"] / B,
                   "launch_over_composed": r_["gq_close_fingers"]["median_us"] / r_["composed_route"]["median_us"]})
        rec["launch"][f"{B}xS{S}"] = r_
        print(json.dumps({f"{B}xS{S}": r_}), flush=True)


# ---- GraspStepper.close() end to end, and what closing finds on finished grasps ----------------------------------------------------
def stepper(n_obj, weights=None):
    fvs = [meshes.superquadric(o) for o in range(n_obj)]
    sps = [meshes.surface_points(f, 2500, oversample=4, seed=42) for f in fvs]
    st = GraspStepper(hand, ops.MeshSet(fvs), torch.tensor(np.stack(sps)), 256, 4, seed=3, weights=weights)
    c = np.concatenate([f.reshape(-1, 3) for f in fvs]).mean(0)
    origin = [float(x) - 0.1575 for x in c]
    stack = ops.SceneSDFSet(torch.stack([ops.SceneSDF.from_meshes([fv], origin, (64, 64, 64), 0.005).values for fv in fvs]), origin, 0.005)
    g2 = torch.Generator().manual_seed(1)
    hp = torch.cat([0.12 * torch.nn.functional.normalize(torch.randn(st.B, 3, generator=g2), dim=-1), torch.randn(st.B, 6, generator=g2),
                    torch.tensor(spec.default_state)[None] + 0.1 * torch.randn(st.B, spec.n_dofs, generator=g2)], 1).float().cuda()
    st.reset(hp, torch.randint(spec.n_contact_candidates, (st.B, 4), generator=g2).cuda())
    return st, stack


rec["stepper_close"] = {}
for n_obj in (1, 8):
    st, stack = stepper(n_obj)
    for _ in range(5):
        c = st.close(stack)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(20):
            c = st.close(stack)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0) / 20)
    rec["stepper_close"][f"{n_obj}x256"] = {"rows": st.B, "steps": 32, "ms_per_call_median": float(np.median(ts)), "ms_per_call_min": min(ts),
                                            "ms_per_call_max": max(ts)}
    print(json.dumps({"stepper_close": rec["stepper_close"]}), flush=True)
    del st

rec["grasps"] = {}
loads = ops.hold_loads(0.2)
for name, w in (("without_E_squeeze", None), ("with_E_squeeze", {"E_squeeze": 10.0})):
    st, stack = stepper(1, w)
    for _ in range(args.iterations):
        st.step()
    st.flush()
    c = st.close(stack)
    ideal = st.hold(loads, 10.0)
    e_c, resid_c, _ = st.hold(loads, 10.0, closed=c, contacts=8)
    n_t = c.touched.sum(1)
    over = torch.where(c.touched, (-c.phi).clamp_min(0), torch.zeros_like(c.phi))
    rec["grasps"][name] = {"rows": st.B, "iterations": args.iterations, "share_2_touching": float((n_t >= 2).float().mean()),
                           "share_3_touching": float((n_t >= 3).float().mean()), "mean_touching_links": float(n_t.float().mean()),
                           "mean_overshoot_m": float(over.sum() / c.touched.sum().clamp_min(1)),
                           "max_overshoot_m": float(over.max()), "hold_resid_ideal_median": float(ideal.resid.amax(1).median()),
                           "hold_resid_closed_median": float(resid_c.amax(1).median()),
                           "rows_holding_ideal": float((ideal.resid.amax(1) <= 0.05).float().mean()),
                           "rows_holding_closed": float((resid_c.amax(1) <= 0.05).float().mean())}
    print(json.dumps({"grasps": rec["grasps"]}), flush=True)
    del st
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
