#!/usr/bin/env python3
"""Timing of the exact grasp-quality metrics (csrc/exact.hip) against the reference's CPU path.

  - ScipyLsqSolver.solve on (B, 12, 6, nz): the Euclidean metric's problems through the solver class;
  - ops.span_exact (F built on the device, one block per row) at 256 and 8192 rows, k = 4 and 8, Euclidean and overall;
  - the reference-equivalent CPU path (scipy.optimize.lsq_linear once per problem, its default method, as
    metrics/solver/scipy_solver.py does) on a small sample, reported per grasp.
Device times: CUDA events around `reps` launches after `warmup` launches, median of `trials`.  One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from graspqp_amd import ops  # noqa: E402
from graspqp_amd.metrics import ScipyLsqSolver  # noqa: E402


def contacts(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g), dim=-1)
    cp = d * (0.05 + 0.01 * torch.randn(B, n, 1, generator=g))
    cn = torch.nn.functional.normalize(d + 0.3 * torch.randn(B, n, 3, generator=g), dim=-1)
    cog = 0.005 * torch.randn(B, 3, generator=g)
    return cp.cuda(), cn.cuda(), cog.cuda()


def grasp_matrix(cp, cn, cog, k, mu=0.2, tw=5.0):
    """F (B,6,n k) of the friction-cone metric (reference span.py:25-38,167-205), fp32 torch"""
    B, n, _ = cn.shape
    b1 = torch.full((B, n, 3), 3 ** -0.5)
    dot = (b1 * cn).sum(-1) / (cn.norm(dim=-1) + 1e-6)
    b1[..., 1] -= 2 * (dot > 0.9).float()
    t1 = torch.linalg.cross(cn, b1)
    t2 = torch.linalg.cross(cn, t1)
    c = (1 - mu ** 2) ** 0.5
    if k == 4:
        dirs = [mu * t1 + c * cn, mu * t2 + c * cn, -mu * t1 + c * cn, -mu * t2 + c * cn]
    else:
        dirs = [mu * (np.cos(2 * np.pi / k * i) * t1 + np.sin(2 * np.pi / k * i) * t2) + c * cn for i in range(k)]
    f = torch.stack(dirs, -2).flatten(-3, -2) / k
    r = (cp - cog.unsqueeze(1)).repeat_interleave(k, dim=-2)
    return torch.cat([f, torch.linalg.cross(r, f) * tw], -1).mT.contiguous()


def time_gpu(fn, warmup, reps, trials):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--cpu-grasps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    n = a.n
    for k in (4, 8):
        for B in (256, 8192):
            cp, cn, cog = contacts(B, n, B + k)
            for nb, lo, hi in ((12, 0.0, 50.0), (1, 1.0, 21.0)):
                fn = lambda: ops.span_exact(cp, cn, cog, k, 0.2, 5.0, nb, lo, hi)
                med, mn, mx = time_gpu(fn, a.warmup, a.reps, a.trials)
                st = fn()[3]
                rows.append(dict(case="span_exact", metric="euclidean" if nb == 12 else "overall", rows=B, n=n, k=k,
                                 ms_median=med, ms_min=mn, ms_max=mx, max_status=int(st.max()),
                                 mean_status=float(st.float().mean()), min_status=int(st.min())))
        # the solver class on the Euclidean problems of 256 grasps
        B = 256
        F = torch.randn(B, 6, n * k, device="cuda") * 0.1
        A = F.unsqueeze(1).expand(-1, 12, -1, -1).contiguous()
        eye = torch.eye(6, device="cuda")
        bb = torch.cat([eye, -eye]).unsqueeze(0).expand(B, -1, -1).contiguous()
        s = ScipyLsqSolver.from_mat(A, bb)
        med, mn, mx = time_gpu(lambda: s.solve(A, bb, min_bound=0.0, max_bound=50.0), a.warmup, a.reps, a.trials)
        rows.append(dict(case="ScipyLsqSolver.solve", shape=[B, 12, 6, n * k], ms_median=med, ms_min=mn, ms_max=mx))
        # reference-equivalent CPU path: lsq_linear per problem (its default method), a few grasps
        from scipy.optimize import lsq_linear

        cp, cn, cog = contacts(a.cpu_grasps, n, 7 + k)
        Fc = grasp_matrix(cp.cpu(), cn.cpu(), cog.cpu(), k).double().numpy()
        basis = np.concatenate([np.eye(6), -np.eye(6)])
        t0 = time.perf_counter()
        for r in range(Fc.shape[0]):
            for i in range(12):
                lsq_linear(Fc[r], basis[i], bounds=(0.0, 50.0))
        per = (time.perf_counter() - t0) / Fc.shape[0]
        rows.append(dict(case="reference_cpu_lsq_linear", metric="euclidean", n=n, k=k, grasps=Fc.shape[0],
                         s_per_grasp=per, s_256_grasps=256 * per))
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
