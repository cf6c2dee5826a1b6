#!/usr/bin/env python3
"""Generate tests/golden/span_euclid_n{12,16}_k{4,8}.npz by RUNNING the reference's Euclidean span metric.

The reference's ``EucledianFrictionConeSpanMetric`` with its ``ScipyLsqSolver`` (metrics/ops/span.py:125-231,
metrics/solver/scipy_solver.py) is driven through ``SpanMetricWrapper`` directly -- not through the factory, whose
GRASPQP_EUCLIDIAN_SCIPY branch nests n_cone_vecs where from_dim ignores it (registry.py:120-131), so that k = 8 is
honoured.  Stored per fixture: the inputs, F, svd, the reference's per-basis values (its default ``trf`` solver) and E,
and fp64 ``lsq_linear(method="bvls")`` values on the same F, the exact yardstick (``trf`` sometimes stops at its
iteration cap).  Same switches as tools/make_golden.py: GRASPQP_REFERENCE, GRASPQP_GOLDEN_OUT.
"""
import os
import sys

import numpy as np
import torch
from scipy.optimize import lsq_linear

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

MAX_LIMIT = 50.0  # span.py:28 default, the Euclidean metric's upper bound


def bvls_values(F):
    """(B,12) fp64 exact values of the 12 basis problems on each F (6,nz), bounds [0, MAX_LIMIT]."""
    F = F.astype(np.float64)
    eye = np.eye(6)
    basis = np.concatenate([eye, -eye])
    out = np.zeros((F.shape[0], 12))
    for r in range(F.shape[0]):
        for i in range(12):
            out[r, i] = lsq_linear(F[r], basis[i], bounds=(0.0, MAX_LIMIT), method="bvls").cost
    return out


def gen_euclid(scipy_solver, span_mod, registry):
    for n, k, B, seed in ((12, 4, 8, 10), (12, 8, 8, 11), (16, 4, 8, 12), (16, 8, 8, 13)):
        torch.manual_seed(seed)
        # contacts roughly on a 5 cm object, normals roughly outward + noise (as tools/make_golden.py::gen_span)
        d = torch.nn.functional.normalize(torch.randn(B, n, 3), dim=-1)
        pts = d * (0.05 + 0.01 * torch.randn(B, n, 1))
        nrm = torch.nn.functional.normalize(d + 0.3 * torch.randn(B, n, 3), dim=-1)
        cog = 0.005 * torch.randn(B, 3)
        fn = registry.SpanMetricWrapper(span_mod.EucledianFrictionConeSpanMetric,
                                        metric_kwargs={"solver_cls": scipy_solver.ScipyLsqSolver, "friction": 0.2,
                                                       "n_cone_vecs": k})
        e, x = fn(contact_pts=pts, contact_normals=nrm, sdf=None, cog=cog, with_solution=True, svd_gain=0.1)
        F = fn.metric._cache["F"]
        values = fn.metric._cache["results"][0]
        svd = (torch.linalg.svdvals(F)).prod(-1) ** (1 / 6)
        exact = bvls_values(F.numpy())
        path = os.path.join(make_golden.OUT, f"span_euclid_n{n}_k{k}.npz")
        np.savez(path, **make_golden.to_np(dict(
            contact_pts=pts, contact_normals=nrm, cog=cog, F=F, svd=svd, values_ref=values, e_ref=e, x_sum_ref=x,
            values_bvls=exact, friction=0.2, max_limit=MAX_LIMIT, n_cone_vecs=k, svd_gain=0.1, values_gain=2.0)))
        print(f"euclid n={n} k={k}: max |trf - bvls| {np.abs(values.numpy() - exact).max():.2e}  -> {path}")


def main():
    os.makedirs(make_golden.OUT, exist_ok=True)
    scipy_solver, registry = make_golden.ref_metrics()
    span_mod = sys.modules["graspqp.metrics.ops.span"]
    gen_euclid(scipy_solver, span_mod, registry)


if __name__ == "__main__":
    main()
