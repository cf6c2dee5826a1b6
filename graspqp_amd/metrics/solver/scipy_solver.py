"""HIP-backed drop-in for reference ``graspqp/metrics/solver/scipy_solver.py`` (ScipyLsqSolver).

The reference calls ``scipy.optimize.lsq_linear`` once per problem on the CPU; here every problem of the batch is solved
to optimality on the device by one launch of the exact bounded-least-squares kernel (csrc/exact.hip, BVLS in fp64).
Same constructor / ``from_mat`` / ``build_solver`` / ``to`` / ``solve`` surface and the same (value, x) shapes; value is
scipy's ``res.cost`` = 1/2 |A x - b|^2.  Nothing here is differentiable, as in the reference (its values come from numpy).

Deliberately NOT a subclass of ``SQPLsqSolver``: the span metrics tell the two apart by class, and the PDIPM routes
(``_require_hip_solver``, the fused loop) must not accept this one.
"""

import torch

from ... import ops


class ScipyLsqSolver:
    def __init__(self):
        self.last_status = None  # (B...) int32 of the last solve: solves used, -1 iteration cap, -2 non-finite input

    @classmethod
    def from_mat(cls, A, b, step_size=0.15, solver_kwargs={}):
        solver = cls()
        solver.build_solver_from_mat(A, b, step_size=step_size, solver_kwargs=solver_kwargs)
        return solver

    def build_solver_from_mat(self, A, b, step_size=0.15, solver_kwargs={}):
        if A.ndim == 2:
            A = A.unsqueeze(0)
        if b.ndim == 1:
            b = b.unsqueeze(0)
        batch_size = A.shape[0] * A.shape[1] if A.ndim == 4 else A.shape[0]
        self.build_solver(A.shape[-1], b.shape[-1], batch_size, device=A.device, step_size=step_size,
                          solver_kwargs=solver_kwargs)

    def to(self, device):
        self._device = device

    def build_solver(self, num_wrenches, wrench_dim, batch_size=1, step_size=0.15, device="cuda", solver_kwargs={}):
        self._num_wrenches, self._wrench_dim = num_wrenches, wrench_dim
        self._batch_size, self._device, self._step_size = batch_size, device, step_size

    def __call__(self, A, b, **kwargs):
        return self.solve(A, b, **kwargs)

    def solve(self, A, b, reg=0.0, init=None, min_bound=-1e4, max_bound=1e4, return_solution=False, verbose=False):
        """min 1/2 |A x - b|^2 s.t. min_bound <= x <= max_bound for every problem, exactly (scipy_solver.py:61-131).
        ``reg`` and ``init`` are accepted and ignored, as in the reference (lsq_linear never sees them)."""
        batch_shape = (A.shape[0],)
        if A.ndim == 4:
            batch_shape = A.shape[0], A.shape[1]
            if b.shape[0] != A.shape[0]:
                b = b.expand(A.shape[0], -1, -1)
            A = A.flatten(0, 1)
            b = b.flatten(0, 1)
        if b.shape[0] != A.shape[0]:
            b = b.expand(A.shape[0], -1)
        nw = A.shape[-1]
        # the reference builds its bound vectors in A's dtype before handing them to scipy
        dt = A.dtype if A.dtype in (torch.float32, torch.float64) else torch.float32
        lo = float(torch.tensor(float(min_bound), dtype=dt))
        hi = float(torch.tensor(float(max_bound), dtype=dt))
        x, value, status = ops.lsq_box_exact(A, b, lo, hi)
        device = getattr(self, "_device", A.device)
        x = x.to(device=device, dtype=A.dtype).view(*batch_shape, nw)
        value = value.to(device=device, dtype=A.dtype).view(*batch_shape)
        self.last_status = status.view(*batch_shape)
        if return_solution:
            return value, x
        return value
