"""Cost of the Euclidean distance field of fused TSDF volumes on the device (ops.SceneTSDF.esdf, gq_esdf): grids of
--grid^3 nodes at --voxel (the shape of tools/bench_tsdf.py and bench_surfel.py), fused from four frames of the plane-and-sphere
scene with trunc 2 cm, then for 1 and --n_obj grids and every window R of --windows (max_distance = R voxel)
  esdf       the eight launches into buffers that exist, captured in a hipGraph;
and beside it, in the same run, the sibling launches it sits between on the stack of --n_obj grids,
  integrate  gq_tsdf_integrate of one frame (V = 1),
  surfels    gq_tsdf_surfels (three launches),
each captured too.  Windows of --steps replays alternate between the variants, --rounds of them, timed with HIP events: median with
[min, max]; the spread over the windows is the margin.  As context only, scipy.ndimage.distance_transform_edt of one grid's
occupancy on the host (voxel centres, not crossing points, no clamp: another problem, and another processor).  The tool derives
the bytes the eight passes move (19 words per node) and the rate that gives.  Evidence run, not a test: the record is printed and
written to --out.

usage: python tools/bench_esdf.py [--grid 80] [--voxel 0.005] [--n_obj 8] [--windows 8 20] [--steps 100] [--rounds 5] [--out file.json]
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
ap.add_argument("--grid", type=int, default=80)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--n_obj", type=int, default=8)
ap.add_argument("--windows", type=int, nargs="+", default=[8, 20])
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--trunc", type=float, default=0.02)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esdf_bench.json"))
args = ap.parse_args()

from graspqp_amd import ops

assert torch.cuda.is_available(), "this tool measures on the GPU"
W, H = args.width, args.height
K = (525.0 * W / 640, 525.0 * W / 640, 0.5 * (W - 1), 0.5 * (H - 1))
RANGE, TRUNC = (0.05, 5.0), args.trunc
CENTRE = np.array([0.0, 0.0, 0.15])
SPHERE = (np.array([0.02, -0.01, 0.08]), 0.08)


def look_at(eye, target):
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    return np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1).astype(np.float32)


def render(T):
    """z-depth of the plane z = 0 and the sphere from the pose T (3,4)."""
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
    return np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)


V = 4
cams = np.stack([look_at(CENTRE + 0.7 * np.array([np.cos(a) * 0.8, np.sin(a) * 0.8, 0.6]), CENTRE)
                 for a in np.linspace(0.0, 2 * np.pi, V, endpoint=False)])
depth = torch.as_tensor(np.stack([render(T) for T in cams])).cuda()
cam_T = torch.as_tensor(cams).cuda().reshape(V, 12).contiguous()


def window(fn, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    torch.cuda.synchronize()
    return 1e3 * ev0.elapsed_time(ev1) / n  # us


def alternate(fns, steps, warm=20):
    for fn in fns.values():
        for _ in range(min(warm, steps)):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, steps))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def graphed(fn):
    fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    torch.cuda.synchronize()
    return g.replay


def volume(G):
    shape = (args.grid,) * 3
    origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in CENTRE]
    gen = torch.Generator().manual_seed(G)
    tT = torch.zeros(G, 3, 4)
    tT[:, :, :3] = torch.eye(3)
    tT[:, :, 3] = 0.03 * (torch.rand(G, 3, generator=gen) * 2 - 1)
    tT = tT.cuda().reshape(G, 12).contiguous()
    t = ops.SceneTSDF(origin, shape, args.voxel, TRUNC, n_grids=G)
    t.integrate(depth, K, cam_T, target_T=tT, depth_range=RANGE)
    return t, tT


fns, keep, stats = {}, [], {}
for G in sorted({1, args.n_obj}):
    t, tT = volume(G)
    keep.append(t)
    for R in args.windows:
        out = ops.SceneSDFSet.empty(G, t.origin, t.shape, t.voxel)
        keep.append(out)  # the graph holds the addresses of out and of its workspace, not the objects: they must outlive it
        fns[f"esdf_{G}x{args.grid}^3_R{R}"] = graphed(lambda t=t, R=R, out=out: t.esdf(R * args.voxel, out=out))
        v = out.values
        stats[f"{G}x{args.grid}^3_R{R}"] = {"window_used": int(np.ceil(float(np.float32(R * args.voxel)) / float(np.float32(args.voxel)))),
                                            "in_band": float((t.values.abs() < TRUNC).float().mean()),
                                            "clamped_at_max_distance": float((v.abs() >= np.float32(R * args.voxel)).float().mean())}
    if G == args.n_obj:
        one = t  # the siblings run on the full stack; a further frame moves D, which the timing does not mind
        fns["integrate_V1"] = graphed(lambda: one.integrate(depth[:1], K, cam_T[:1], target_T=tT, depth_range=RANGE))
        one.surfels(1)
        count = torch.empty(G, 2, dtype=torch.int32, device="cuda")
        ops._Eager.tsdf_surfels(one._stack, one._weight, list(one.origin), one.voxel, [], 1.0, one.trunc, None, None, count, one._surfel_workspace())
        cap = int(count[:, 0].max())
        buf = one.surfels(cap)
        fns["surfels"] = graphed(lambda: one.surfels(cap, out=buf))
res = alternate(fns, args.steps)

# context only: the host's voxel-centre transform of one grid
host_ms = None
try:
    from scipy.ndimage import distance_transform_edt

    occ = (keep[0].values[0] < 0).cpu().numpy()
    t0 = time.time()
    d_out, d_in = distance_transform_edt(~occ), distance_transform_edt(occ)
    host_ms = 1e3 * (time.time() - t0)
except ImportError:
    pass

nodes = args.grid ** 3
words = 19  # per node: seed 2 x 3, envelope 2 x 3, the two envelopes with a second input 3 + 4
for k, r in res.items():
    if k.startswith("esdf_"):
        G = int(k.split("_")[1].split("x")[0])
        r["passes_bytes"] = words * 4 * nodes * G
        r["passes_TBps"] = r["passes_bytes"] / r["median_us"] * 1e-6
rec = {"esdf": True, "grid": [args.grid] * 3, "voxel": args.voxel, "trunc": TRUNC, "views_fused": V, "steps": args.steps, "rounds": args.rounds,
       "windows": args.windows, "n_obj": args.n_obj, "hbm_peak_TBps": 8.0, "hbm_achievable_TBps": 6.3, "volumes": stats, "cases": res,
       "host_scipy_distance_transform_edt_1_grid_ms": host_ms}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print(json.dumps(rec), flush=True)
