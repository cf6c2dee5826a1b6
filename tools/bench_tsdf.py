"""Cost of fusing depth frames into scene grids on the device (ops.SceneTSDF.integrate, gq_tsdf_integrate): V frames of
--width x --height pixels of a plane-and-sphere scene, from cameras on a ring, into 1 and --n_obj grids of --grid^3 nodes at
--voxel, for V = 1, 4, 8, beside two alternatives on the same inputs:
  (a) V launches of one view each (the grid traffic is paid V times);
  (b) the same rule written in plain torch ops on the device, one view after the other: what a user writes without this kernel.
Every variant is captured in a hipGraph (one replay = one fusion of V frames from a fresh volume's memory, no host work between
the launches), warmed up, and timed with HIP events around windows of --steps replays that alternate between the variants,
--rounds of them; the spread of a figure over its windows is its margin.  The eager call, host work included, is timed the same
way.  From the 16 bytes per node of grid traffic (D and W, read and written) the tool derives the achieved bytes/s of the single
launch, to be read beside the 8.0 TB/s peak (6.3 TB/s achievable) of the HBM and the rates of the caches a stack of this size
stays in.  Before timing, (b) is compared with the kernel (weight exactly, values at 1e-5).  Evidence run, not a test: one JSON
line is printed and appended to --out.

usage: python tools/bench_tsdf.py [--grid 80] [--voxel 0.005] [--n_obj 8] [--width 640] [--height 480] [--steps 200] [--rounds 5]
       [--out file.jsonl]
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
ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "tsdf_bench.jsonl"))
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
    """z-depth of the plane z = 0 and the sphere from the pose T (3,4), and the labels (0 plane, 1 sphere)."""
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


V_MAX = 8
cams = np.stack([look_at(CENTRE + 0.7 * np.array([np.cos(a) * 0.8, np.sin(a) * 0.8, 0.6]), CENTRE)
                 for a in np.linspace(0.0, 2 * np.pi, V_MAX, endpoint=False)])
imgs = [render(T) for T in cams]
depth = torch.as_tensor(np.stack([i[0] for i in imgs])).cuda()
labels = torch.as_tensor(np.stack([i[1] for i in imgs])).cuda()
cam_T = torch.as_tensor(cams).cuda().reshape(V_MAX, 12).contiguous()


def torch_rule(values, weight, origin, voxel, target_T, d, lab, T, skip):
    """The rule of gq_tsdf_integrate in plain torch ops, one view after the other, in place on (G,nx,ny,nz) tensors."""
    G, nx, ny, nz = values.shape
    ax = [origin[a] + voxel * torch.arange(n, device=values.device, dtype=torch.float32) for a, n in enumerate((nx, ny, nz))]
    xf = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1)  # (nx,ny,nz,3)
    Tg = target_T.reshape(G, 3, 4)
    xw = torch.einsum("gab,xyzb->gxyza", Tg[:, :, :3], xf) + Tg[:, None, None, None, :, 3]
    for v in range(d.shape[0]):
        Tc = T[v].reshape(3, 4)
        xc = (xw - Tc[:, 3]) @ Tc[:, :3]
        z = xc[..., 2]
        front = z >= RANGE[0]
        zs = torch.where(front, z, torch.ones_like(z))
        u, w = K[0] * xc[..., 0] / zs + K[2], K[1] * xc[..., 1] / zs + K[3]
        inimg = front & (u >= -0.5) & (u < W - 0.5) & (w >= -0.5) & (w < H - 0.5)
        pix = torch.where(inimg, torch.floor(w + 0.5) * W + torch.floor(u + 0.5), torch.zeros_like(u)).long()
        dd = d[v].reshape(-1)[pix]
        valid = inimg & (dd >= RANGE[0]) & (dd <= RANGE[1])
        carve = valid & (lab[v].reshape(-1)[pix] == skip[:, None, None, None]) & (skip[:, None, None, None] >= 0)
        sdf = dd - z
        upd = valid & (carve | (sdf >= -TRUNC))
        s = torch.where(carve, torch.full_like(sdf, TRUNC), sdf.clamp(max=TRUNC))
        values.copy_(torch.where(upd, (weight * values + s) / (weight + 1.0), values))
        weight.copy_(torch.where(upd, (weight + 1.0).clamp(max=64.0), weight))


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


def graphed(fn):
    fn()  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    torch.cuda.synchronize()
    return g.replay


rec = {"tsdf": True, "grid": [args.grid] * 3, "voxel": args.voxel, "image": [W, H], "trunc": TRUNC, "steps": args.steps,
       "rounds": args.rounds, "bytes_per_node": 16, "hbm_peak_TBps": 8.0, "hbm_achievable_TBps": 6.3, "cases": {}}
shape = (args.grid,) * 3
origin = [float(c) - 0.5 * args.voxel * (args.grid - 1) for c in CENTRE]
for G in (1, args.n_obj):
    gen = torch.Generator().manual_seed(G)
    tT = torch.zeros(G, 3, 4)
    tT[:, :, :3] = torch.eye(3)
    tT[:, :, 3] = 0.03 * (torch.rand(G, 3, generator=gen) * 2 - 1)
    tT = tT.cuda().reshape(G, 12).contiguous()
    skip = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    skip[0] = 1
    t = ops.SceneTSDF(origin, shape, args.voxel, TRUNC, n_grids=G)
    nodes = t._stack.numel()
    for V in (1, 4, 8):
        d, lab, T = depth[:V].contiguous(), labels[:V].contiguous(), cam_T[:V].contiguous()
        one = lambda: t.integrate(d, K, T, labels=lab, target_T=tT, skip=skip, depth_range=RANGE)
        views = [(d[v:v + 1], lab[v:v + 1], T[v:v + 1]) for v in range(V)]

        def per_view():
            for dv, lv, Tv in views:
                t.integrate(dv, K, Tv, labels=lv, target_T=tT, skip=skip, depth_range=RANGE)

        ref = (torch.empty_like(t._stack), torch.empty_like(t._stack))
        plain = lambda: torch_rule(ref[0], ref[1], list(t.origin), t.voxel, tT, d, lab, T, skip)
        # (b) computes what the kernel computes
        t.reset(), ref[0].fill_(t.unknown), ref[1].zero_()
        one(), plain()
        torch.cuda.synchronize()
        same_w = float((t._weight == ref[1]).float().mean())
        close = float(((t._stack - ref[0]).abs() <= 1e-5).float().mean())
        seen = float((t._weight > 0).float().mean())
        assert same_w > 0.99 and close > 0.99, (same_w, close)  # fp32 against fp32: a pixel or band decision may fall the other way
        fns = {"one_launch": graphed(one), "per_view_launches": graphed(per_view), "torch_ops": graphed(plain), "eager_call": one}
        res = alternate(fns, args.steps)
        us = res["one_launch"]["median_us"]
        res.update({"nodes": nodes, "views": V, "seen_fraction": seen, "torch_ops_weight_equal_fraction": same_w,
                    "torch_ops_values_close_fraction": close, "grid_bytes": 16 * nodes, "one_launch_grid_TBps": 16 * nodes / us * 1e-6,
                    "per_view_over_one": res["per_view_launches"]["median_us"] / us, "torch_over_one": res["torch_ops"]["median_us"] / us})
        rec["cases"][f"G{G}_V{V}"] = res
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    f.write(json.dumps(rec) + "\n")
print(json.dumps(rec), flush=True)
