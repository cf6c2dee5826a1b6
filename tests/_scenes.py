"""Shared synthetic inputs of the CPU and GPU tests (plain torch, no product / oracle imports)."""
import torch


def hetero_contacts(B, n, seed, dtype=torch.float64):
    """Heterogeneous batch of contact sets (points (B,n,3), object normals (B,n,3), cog (B,3)): contacts on spheres of
    different radii, from well spread (easy rows: the force-closure QP converges in a few iterations) to bunched on one
    side of the object (hard rows: far from force closure, slow PDIPM convergence)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(B, n, 3, generator=g, dtype=torch.float64), dim=-1)
    bunch = torch.rand(B, 1, 1, generator=g, dtype=torch.float64) ** 2  # 0 = spread, 1 = all contacts on one side
    pole = torch.nn.functional.normalize(torch.randn(B, 1, 3, generator=g, dtype=torch.float64), dim=-1)
    d = torch.nn.functional.normalize(d + 3.0 * bunch * pole, dim=-1)
    pts = d * (0.03 + 0.05 * torch.rand(B, 1, 1, generator=g, dtype=torch.float64))
    nrm = torch.nn.functional.normalize(-d + 0.3 * torch.randn(B, n, 3, generator=g, dtype=torch.float64), dim=-1)
    cog = 0.005 * torch.randn(B, 3, generator=g, dtype=torch.float64)
    return pts.to(dtype), nrm.to(dtype), cog.to(dtype)


def _fp32_exact(*ts):
    """Round to fp32 and back: the fp64 oracle then solves exactly the problem the fp32 kernels receive."""
    return tuple(t.float().double() for t in ts)


def spd_box_qp(B, nz, seed, cond=(1e1, 1e4)):
    """Dense box QPs  min 1/2 x'Qx + p'x, lower <= x <= upper  (fp64 values exactly representable in fp32).

    Q = V diag(ev) V' with random orthogonal V and eigenvalues log-spaced over [1, c], c drawn log-uniformly from ``cond``
    per row; p = -Q x_u for an unconstrained optimum x_u ~ N(0, 1.5^2), and per-row asymmetric bounds lower in
    [-1.5, -0.3], upper in [0.3, 1.5], so that at the optimum some bounds are active and some are not."""
    g = torch.Generator().manual_seed(seed)
    dt = torch.float64
    V, _ = torch.linalg.qr(torch.randn(B, nz, nz, generator=g, dtype=dt))
    lc = torch.log10(torch.tensor(cond, dtype=dt))
    c = 10 ** (lc[0] + (lc[1] - lc[0]) * torch.rand(B, generator=g, dtype=dt))
    ev = c[:, None] ** torch.linspace(0.0, 1.0, nz, dtype=dt)[None]
    Q = (V * ev[:, None, :]) @ V.transpose(1, 2)
    Q = 0.5 * (Q + Q.transpose(1, 2))
    p = -(Q @ (1.5 * torch.randn(B, nz, 1, generator=g, dtype=dt))).squeeze(-1)
    lower = -(0.3 + 1.2 * torch.rand(B, nz, generator=g, dtype=dt))
    upper = 0.3 + 1.2 * torch.rand(B, nz, generator=g, dtype=dt)
    return _fp32_exact(Q, p, lower, upper)


def lsq_box_problem(B, m, nz, seed, lower=1.0, upper=21.0):
    """Least-squares box QPs  min 1/2 |A x - b|^2 (+ ridge), lower <= x <= upper  with A (B, m, nz), b (B, m) != 0.

    b = A x_t for a target x_t drawn uniformly over the box widened by 10 % on either side ([-5, 5] for boxes wider than
    100), plus noise: some coordinates of the optimum sit on a bound, the rest inside (fp32-exact fp64 values)."""
    g = torch.Generator().manual_seed(seed)
    dt = torch.float64
    # |A|_2^2 ~ 0.1 .. 4: with the solver's ridge 1e-4, cond(A'A + 1e-4 I) ~ 1e3 .. 4e4 (a grasp matrix: ~ 1e3 .. 1e4)
    s = (0.3 + 0.7 * torch.rand(B, 1, 1, generator=g, dtype=dt)) / nz**0.5
    A = torch.randn(B, m, nz, generator=g, dtype=dt) * s
    lo, up = (lower, upper) if upper - lower <= 100.0 else (-5.0, 5.0)
    w = up - lo
    xt = lo - 0.1 * w + 1.2 * w * torch.rand(B, nz, 1, generator=g, dtype=dt)
    b = (A @ xt).squeeze(-1) + 0.1 * torch.randn(B, m, generator=g, dtype=dt)
    return _fp32_exact(A, b)
