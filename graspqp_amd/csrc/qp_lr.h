// Box-QP whose Hessian is low rank plus ridge: Q = A'A + ridge*I with A (m x nz), m <= 8 -- the force-closure QP
// (m = 6 wrench rows, nz = contacts x cone edges).  One problem per wavefront, lane k owns column(s) k, k+64.
//
// Every interior-point iteration has to solve (Q + diag(d_u + d_l)) dx = rhs.  With Lam = ridge + d_u + d_l
// (diagonal) the matrix is Lam + A'A, so by the Woodbury identity
//     dx = Lam^-1 (rhs - A' y),    (I_m + A Lam^-1 A') y = A Lam^-1 rhs,
// i.e. an m x m SPD system instead of an nz x nz one.  Lam spans ~1e-4 .. 1e8 late in the iteration, so the small
// system and the final difference are formed in fp64 (cond(I + A Lam^-1 A') ~ 1e5; in fp32 the subtraction
// rhs - A'y would lose everything for the free variables); everything else stays fp32.  Cross-lane sums use the
// DPP row_shr/row_bcast network (common.h), no LDS.  GqLr is a solver of the shared PDIPM loop and backward row
// (qp_kernels.h).
#pragma once
#include "qp_kernels.h"

template <int M>
struct GqSmall {
  static constexpr int T = M * (M + 1) / 2;
  // in-place Cholesky of the packed lower triangle (idx(i,j) = i(i+1)/2 + j); the diagonal slots receive 1 / L_ii
  static __device__ __forceinline__ void factor(double (&G)[T]) {
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double s = G[i * (i + 1) / 2 + j];
#pragma unroll
        for (int t = 0; t < j; ++t) s -= G[i * (i + 1) / 2 + t] * G[j * (j + 1) / 2 + t];
        if (i == j) G[i * (i + 1) / 2 + j] = gq_rsq_d(s);
        else G[i * (i + 1) / 2 + j] = s * G[j * (j + 1) / 2 + j];
      }
    }
  }
  static __device__ __forceinline__ void solve(const double (&L)[T], double (&v)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int t = 0; t < i; ++t) v[i] -= L[i * (i + 1) / 2 + t] * v[t];
      v[i] *= L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
#pragma unroll
      for (int t = i + 1; t < M; ++t) v[i] -= L[t * (t + 1) / 2 + i] * v[t];
      v[i] *= L[i * (i + 1) / 2 + i];
    }
  }
};

template <int M, int NC>
struct GqLr {
  static constexpr int T = M * (M + 1) / 2;
  float a[NC][M];   // my columns of A
  double il[NC];    // 1 / Lam of my columns (0 for dead columns)
  double L[T];      // Cholesky factor of I + A Lam^-1 A'
  float ridge;

  __device__ __forceinline__ void factor(const float (&lam)[NC], const bool (&live)[NC]) {
    double part[T];
#pragma unroll
    for (int i = 0; i < T; ++i) part[i] = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      il[c] = live[c] ? gq_rcp_d((double)lam[c]) : 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const double ai = (double)a[c][i] * il[c];
#pragma unroll
        for (int j = 0; j <= i; ++j) part[i * (i + 1) / 2 + j] += ai * (double)a[c][j];
      }
    }
    gq_wave_sums_d<T>(part);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[i * (i + 1) / 2 + j] = part[i * (i + 1) / 2 + j] + (i == j ? 1.0 : 0.0);
    GqSmall<M>::factor(L);
  }
  // dx = (Lam + A'A)^-1 rhs
  __device__ __forceinline__ void solve(const float (&rhs)[NC], float (&dx)[NC]) const {
    double v[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) s += (double)a[c][i] * ((double)rhs[c] * il[c]);
      v[i] = s;
    }
    gq_wave_sums_d<M>(v);
    GqSmall<M>::solve(L, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double num = (double)rhs[c];
#pragma unroll
      for (int i = 0; i < M; ++i) num -= (double)a[c][i] * v[i];
      dx[c] = (float)(num * il[c]);
    }
  }
  // Q x = A'(A x) + ridge x
  __device__ __forceinline__ void matvec(const float (&x)[NC], float (&out)[NC]) const {
    float ax[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < NC; ++c) s = fmaf(a[c][i], x[c], s);
      ax[i] = s;
    }
    gq_wave_sums_f<M>(ax);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      float s = ridge * x[c];
#pragma unroll
      for (int i = 0; i < M; ++i) s = fmaf(a[c][i], ax[i], s);
      out[c] = s;
    }
  }
};

template <int M, int NC>
__global__ __launch_bounds__(GQ_WAVE) void gq_qp_lr_iter_kernel(GqQpArgs g) {
  const int row = blockIdx.x;
  const int lane = gq_lane();
  const int nz = g.nz;
  GqLr<M, NC> S;
  S.ridge = g.ridge;
  bool live[NC];
  float p[NC], hu[NC], hl[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + GQ_WAVE * c;
    live[c] = k < nz;
    p[c] = 0.0f;
#pragma unroll
    for (int r = 0; r < M; ++r) S.a[c][r] = (live[c] && r < g.m) ? g.A[((size_t)row * g.m + r) * nz + k] : 0.0f;
    if (g.b != nullptr) {
#pragma unroll
      for (int r = 0; r < M; ++r)
        if (r < g.m) p[c] = fmaf(-S.a[c][r], g.b[(size_t)row * g.m + r], p[c]);
    }
    const float up = live[c] ? (g.upper ? g.upper[(size_t)row * nz + k] : g.upper_s) : 1.0f;
    const float lo = live[c] ? (g.lower ? g.lower[(size_t)row * nz + k] : g.lower_s) : -1.0f;
    hu[c] = up;
    hl[c] = -lo;
  }
  gq_qp_lr_iterate(g, row, lane, S, live, p, hu, hl);
}

template <int M, int NC>
__global__ __launch_bounds__(GQ_WAVE) void gq_qp_lr_bwd_kernel(GqQpBwdArgs g) {
  const int row = blockIdx.x;
  const int lane = gq_lane();
  GqLr<M, NC> S;
  S.ridge = g.ridge;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + GQ_WAVE * c;
#pragma unroll
    for (int r = 0; r < M; ++r) S.a[c][r] = (k < g.nz && r < g.m) ? g.A[((size_t)row * g.m + r) * g.nz + k] : 0.0f;
  }
  gq_qp_bwd_row<NC>(g, S, row, lane);
}
