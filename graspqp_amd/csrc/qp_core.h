// Device building blocks of the batched box QP, one problem per wavefront:
//
//   min 1/2 x'Qx + p'x   s.t.  lower <= x <= upper          (G = [I; -I], h = [upper; -lower])
//
// qpth's PDIPM as driven by the reference (metrics/solver/qp_solver.py:8,101-126; algorithm restated in
// oracle/ref_cpu/qp.py::pdipm_forward_box).
//
// GqChol: dense Q of nz <= 64 variables entirely in registers.  Lane i owns variable i: row i of the (symmetric) KKT
// matrix lives in NZ VGPRs of lane i, vectors are one VGPR per lane.  The reduced KKT system (Q + diag(d_u + d_l)) dx =
// rhs is factored by a right-looking Cholesky whose pivot row is broadcast with v_readlane (no LDS): after the
// factorisation register k of lane i holds L[max(i,k)][min(i,k)], so both triangular solves are broadcast + masked FMA
// sweeps as well.
#pragma once
#include "common.h"

#define GQ_INF GQ_INF_F

template <int NZ>
struct GqChol {
  // in: a[k] = M[lane][k] (full symmetric row).  out: symmetric-L storage + dinv = 1/L[lane][lane].
  static __device__ __forceinline__ void factor(float (&a)[NZ], float& dinv, int lane) {
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      const float piv = gq_readlane(a[j], j);
      const float r = 1.0f / sqrtf(piv);  // wave-uniform
      const float lij = a[j] * r;
      // lanes > j: eliminate with L_ij; lane j: scale its own row by r (a - (1-r) a = r a); lanes < j: untouched
      const float mult = (lane > j) ? lij * r : ((lane == j) ? (1.0f - r) : 0.0f);
      a[j] = (lane > j) ? lij : a[j];
      dinv = (lane == j) ? r : dinv;
#pragma unroll
      for (int k = j + 1; k < NZ; ++k) {
        const float ajk = gq_readlane(a[k], j);  // pivot row entry M'[j][k], uniform
        a[k] = fmaf(-mult, ajk, a[k]);
      }
    }
  }
  // solve (L L') x = b, b/x one value per lane
  static __device__ __forceinline__ float solve(const float (&a)[NZ], float dinv, int lane, float b) {
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      const float yj = gq_readlane(b * dinv, j);
      const float m = (lane > j) ? a[j] : 0.0f;
      b = fmaf(-m, yj, b);
    }
    float y = b * dinv;
#pragma unroll
    for (int i = NZ - 1; i >= 0; --i) {
      const float xi = gq_readlane(y * dinv, i);
      const float m = (lane < i) ? a[i] : 0.0f;
      y = fmaf(-m, xi, y);
    }
    return y * dinv;
  }
  // M = Q + diag(dd) into a[]
  static __device__ __forceinline__ void form(float (&a)[NZ], const float (&q)[NZ], float dd, int lane) {
#pragma unroll
    for (int k = 0; k < NZ; ++k) a[k] = q[k] + ((lane == k) ? dd : 0.0f);
  }
  // y_lane = sum_k q[k] * x_k
  static __device__ __forceinline__ float matvec(const float (&q)[NZ], float x) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NZ; ++k) acc = fmaf(q[k], gq_readlane(x, k), acc);
    return acc;
  }
};

// qpth solve_kkt on the reduced system (see oracle _solve_kkt_box)
template <int NZ>
__device__ __forceinline__ void gq_kkt_solve(const float (&a)[NZ], float dinv, int lane, float du, float dl, float rx,
                                             float rsu, float rsl, float rzu, float rzl, float& dx, float& dsu,
                                             float& dsl, float& dzu, float& dzl) {
  const float tu = du * rzu - rsu, tl = dl * rzl - rsl;
  const float rhs = -rx - (tu - tl);
  dx = GqChol<NZ>::solve(a, dinv, lane, rhs);
  dzu = du * (dx + rzu) - rsu;
  dzl = dl * (-dx + rzl) - rsl;
  dsu = (-rsu - dzu) / du;
  dsl = (-rsl - dzl) / dl;
}

// qpth get_step for one (v, dv) pair per lane and bound side; caller reduces with NaN-propagating min
__device__ __forceinline__ float gq_step_ratio(float v, float dv) {
  const float a = -v / dv;
  return (dv > 0.0f) ? GQ_INF : a;
}

// Register-resident solver (NC = 1) of the shared backward row (qp_kernels.h): the lane's row of Q and of the factor of
// Q + diag(lam).  Rows of lanes >= nz are identity rows, so the padding decouples from the live block.
template <int NZ>
struct GqRegChol {
  float q[NZ];  // row `lane` of Q
  float a[NZ];  // factor of Q + diag(lam), GqChol storage
  float dinv = 1.0f;
  int lane;

  // row `lane` of this problem's Q (B, nz, nz); rows and columns past nz are those of the identity
  __device__ __forceinline__ void load(const float* Q, int row, int nz, int ln) {
    lane = ln;
#pragma unroll
    for (int k = 0; k < NZ; ++k)
      q[k] = (lane < nz && k < nz) ? Q[((size_t)row * nz + lane) * nz + k] : ((lane == k) ? 1.0f : 0.0f);
  }
  __device__ __forceinline__ void factor(const float (&lam)[1], const bool (&)[1]) {
    GqChol<NZ>::form(a, q, lam[0], lane);
    GqChol<NZ>::factor(a, dinv, lane);
  }
  __device__ __forceinline__ void solve(const float (&rhs)[1], float (&dx)[1]) const {
    dx[0] = GqChol<NZ>::solve(a, dinv, lane, rhs[0]);
  }
};

// ---- qpth's batch-global stop rule and per-row selection: the stop, select and fc energy kernels.  The fused
// force-closure step (fcstep_dev.h) keeps inline copies: through these helpers its timed kernels compile differently.
// The sequential decision after iteration it, from that iteration's batch aggregates: did any row improve its best
// residual, the largest running best residual, the smallest mu (NaN-propagating, like torch).  not_improved carries the
// count of iterations without improvement from one call to the next.
__device__ __forceinline__ bool gq_qp_stop_now(int it, bool improved, float max_best, float min_mu, float eps, int lim,
                                               int& not_improved) {
  not_improved = (it == 0) ? 0 : (improved ? 0 : not_improved + 1);
  return (not_improved == lim) || (max_best < eps) || (min_mu > 1e32f);
}
// kstar = [last iteration whose record counts, qpth-style iteration count]
__device__ __forceinline__ void gq_qp_write_kstar(int* kstar, int32_t* n_iter, int stop_at) {
  kstar[0] = stop_at;
  kstar[1] = stop_at + 1;
  if (n_iter) *n_iter = stop_at + 1;
}
// Best iterate of one row among iterations 0..ks (qpth returns the per-row best, not the last; a NaN never becomes best):
// the row's residuals are fetched together (lane it holds iteration it), then scanned from registers.
__device__ __forceinline__ int gq_qp_best_iter(const float* resid, int row, int max_iter, int ks, int lane) {
  const float mine = (lane < max_iter && lane < 64) ? resid[(size_t)row * max_iter + lane] : 0.0f;
  float bst = 0.0f;
  int bi = 0;
  for (int it = 0; it <= ks; ++it) {
    const float rs = it < 64 ? gq_readlane(mine, it) : resid[(size_t)row * max_iter + it];
    if (it == 0 || rs < bst) {
      bst = rs;
      bi = it;
    }
  }
  return bi;
}
