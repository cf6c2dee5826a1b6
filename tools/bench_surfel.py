"""Cost of turning fused TSDF volumes into oriented point clouds on the device (ops.SceneTSDF.surfels, gq_tsdf_surfels):
--n_obj grids of --grid^3 nodes at --voxel (the shape of tools/bench_tsdf.py), fused from four frames of the plane-and-sphere
scene, then
  surfels        the three launches (count per tile, scan per grid, emit) into buffers that exist, captured in a hipGraph;
  count_only     the counting call alone (two launches), what extract_clouds runs before its one read of the count;
  eager_call     the same call launched from Python, host work included;
  extract_clouds the counting call, the read of the count, and the call of exactly that size (one synchronisation);
  torch_ops      the same rule written in plain torch ops on the device (masks, nonzero, gathers): what a user writes without
                 these kernels.  torch.nonzero synchronises, so this one cannot be captured and is timed as it is called.
Windows of --steps calls alternate between the variants, --rounds of them, timed with HIP events; the spread over the windows is
the margin.  The count pass reads D and W once (8 bytes per node); the tool derives its achieved bytes/s.  Before timing, the
torch restatement is compared with the kernels (the count exactly, the surfels row by row, sorted into the kernels' order, at 1e-5 m).  Evidence run, not a test: one
JSON line is printed and appended to --out.

usage: python tools/bench_surfel.py [--grid 80] [--voxel 0.005] [--n_obj 8] [--steps 200] [--rounds 5] [--out file.jsonl]
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
ap.add_argument("--grid", type=int, default=80)
ap.add_argument("--voxel", type=float, default=0.005)
ap.add_argument("--n_obj", type=int, default=8)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--trunc", type=float, default=0.02)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "surfel_bench.jsonl"))
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


def shift(A, off):
    """out[n] = A[n + off] on the last three axes, NaN where n + off leaves the grid."""
    out = torch.full_like(A, float("nan"))
    src, dst = [slice(None)], [slice(None)]
    for o, n in zip(off, A.shape[1:]):
        lo, hi = max(0, -o), min(n, n - o)
        dst.append(slice(lo, hi)), src.append(slice(lo + o, hi + o))
    out[tuple(dst)] = A[tuple(src)]
    return out


def torch_rule(values, weight, origin, voxel, trunc, min_weight):
    """The contract of gq_tsdf_surfels in torch ops -> per axis (grid and node indices of a, positions, normals)."""
    seen = torch.isfinite(values) & (weight >= min_weight)
    D = torch.where(seen, values, torch.full_like(values, float("nan")))
    grad = []
    for c in range(3):
        e = [int(a == c) for a in range(3)]
        hi, lo = shift(D, e), shift(D, [-x for x in e])
        a, b = ~torch.isnan(lo), ~torch.isnan(hi)
        d = torch.where(a & b, 0.5 * (hi - lo), torch.where(b, hi - D, torch.where(a, D - lo, torch.zeros_like(D))))
        d = torch.where(seen, d, torch.full_like(D, float("nan")))
        u, v = [x for x in range(3) if x != c]
        num, den = torch.zeros_like(D), torch.zeros_like(D)
        for du in (-1, 0, 1):
            for dv in (-1, 0, 1):
                off = [0, 0, 0]
                off[u], off[v] = du, dv
                dm = shift(d, off)
                ok = ~torch.isnan(dm)
                w = float((2 - abs(du)) * (2 - abs(dv)))
                num = num + torch.where(ok, w * dm, torch.zeros_like(dm))
                den = den + ok * w
        grad.append(num / den.clamp_min(1.0))
    grad = torch.stack(grad, -1)
    out = []
    for c in range(3):
        e = [int(a == c) for a in range(3)]
        Db = shift(D, e)
        cross = (D.abs() < trunc) & (Db.abs() < trunc) & ((D >= 0) != (Db >= 0))
        idx = cross.nonzero()  # (n,4): grid, i, j, k -- synchronises
        ib = idx.clone()
        ib[:, 1 + c] += 1
        Da, Dbv = D[tuple(idx.T)], D[tuple(ib.T)]
        t = Da / (Da - Dbv)
        P = torch.tensor(origin, device=values.device) + voxel * idx[:, 1:].float()
        P[:, c] += t * voxel
        n = (1 - t)[:, None] * grad[tuple(idx.T)] + t[:, None] * grad[tuple(ib.T)]
        n2 = (n * n).sum(-1, keepdim=True)
        fall = torch.zeros_like(n)
        fall[:, c] = torch.sign(Dbv - Da)
        out.append((idx, P, torch.where(n2 > 1e-20, n / n2.clamp_min(1e-30).sqrt(), fall)))
    return out


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
    for k, fn in fns.items():
        for _ in range(min(warm, steps[k])):
            fn()
    out = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            out[k].append(window(fn, steps[k]))
    return {k: {"median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def graphed(fn):
    fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    torch.cuda.synchronize()
    return g.replay


G = args.n_obj
shape = (args.grid,) * 3
origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in CENTRE]
gen = torch.Generator().manual_seed(G)
tT = torch.zeros(G, 3, 4)
tT[:, :, :3] = torch.eye(3)
tT[:, :, 3] = 0.03 * (torch.rand(G, 3, generator=gen) * 2 - 1)
t = ops.SceneTSDF(origin, shape, args.voxel, TRUNC, n_grids=G)
t.integrate(depth, K, cam_T, target_T=tT.cuda().reshape(G, 12).contiguous(), depth_range=RANGE)
nodes = t._stack.numel()
count = torch.empty(G, 2, dtype=torch.int32, device="cuda")
count_only = lambda: ops._Eager.tsdf_surfels(t._stack, t._weight, list(t.origin), t.voxel, [], 1.0, t.trunc, None, None, count,
                                             t._surfel_workspace())
count_only()
found = count[:, 0].cpu().tolist()
cap = max(found)
out = t.surfels(cap)
full = lambda: t.surfels(cap, out=out)
plain = lambda: torch_rule(t._stack, t._weight, list(t.origin), t.voxel, t.trunc, 1.0)

# the restatement computes what the kernels compute: the count per grid, and every surfel
ref = plain()
torch.cuda.synchronize()
ref_n = sum(torch.bincount(idx[:, 0], minlength=G) for idx, _, _ in ref).cpu().tolist()
assert ref_n == found, (ref_n, found)
# the restatement's order is (axis, grid, node); the kernels' is (grid, tile of 4 x 4 x 16 nodes, node in the tile, axis)
tiles = [-(-n // d) for n, d in zip(shape, (4, 4, 16))]
keys = []
for c, (idx, _, _) in enumerate(ref):
    g, i, j, k = idx.T
    tile = ((i // 4) * tiles[1] + j // 4) * tiles[2] + k // 16
    keys.append((((g * (tiles[0] * tiles[1] * tiles[2]) + tile) * 256 + ((i % 4) * 4 + j % 4) * 16 + k % 16) * 3 + c))
order = torch.cat(keys).argsort()
Pr, Nr = torch.cat([x[1] for x in ref])[order], torch.cat([x[2] for x in ref])[order]
Pk, Nk = (torch.cat([o[g, :found[g]] for g in range(G)]) for o in out[:2])
worst_p, worst_n = float((Pk - Pr).abs().max()), float((Nk - Nr).abs().max())
assert worst_p < 1e-5 and worst_n < 1e-3, (worst_p, worst_n)

fns = {"surfels": graphed(full), "count_only": graphed(count_only), "eager_call": full, "extract_clouds": t.extract_clouds, "torch_ops": plain}
slow = max(args.steps // 20, 2)
res = alternate(fns, {"surfels": args.steps, "count_only": args.steps, "eager_call": args.steps, "extract_clouds": slow, "torch_ops": slow})
us = res["count_only"]["median_us"]
rec = {"surfel": True, "n_grids": G, "grid": list(shape), "voxel": args.voxel, "trunc": TRUNC, "views_fused": V, "steps": args.steps,
       "rounds": args.rounds, "nodes": nodes, "surfels_per_grid": found, "capacity": cap, "count_pass_bytes": 8 * nodes,
       "count_only_TBps": 8 * nodes / us * 1e-6, "hbm_peak_TBps": 8.0, "hbm_achievable_TBps": 6.3,
       "torch_ops_max_position_diff_m": worst_p, "torch_ops_max_normal_diff": worst_n,
       "torch_over_surfels": res["torch_ops"]["median_us"] / res["surfels"]["median_us"], "cases": res}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write(json.dumps(rec) + "\n")
print(json.dumps(rec), flush=True)
