// Exact bounded least squares for small problems: min 1/2 |A x - b|^2 s.t. lo <= x <= hi, A (m, nz), m <= 8, nz <= 128,
// scalar bounds.  One wavefront per problem, fp64 throughout.
//
// Method: BVLS (Stark & Parker 1995, the two-sided Lawson-Hanson active set behind scipy's lsq_linear(method="bvls")).
//   - column i lives in lane i % 64, slot i / 64 (A's columns in registers, rows padded with zeros to MR);
//   - every variable is FREE, at LOWER, at UPPER, or at REST (x = 0 strictly inside the box: the start point when
//     lo < 0 < hi, which it only leaves for the free set);
//   - outer iteration: gradient w = A'(b - A x) lane-parallel, the most violating variable by a wave arg-max (ties go
//     to the smallest index), which joins the free set;
//   - inner iteration: least squares on the free columns (modified Gram-Schmidt, twice, in fp64), then the step
//     length back to feasibility as in Lawson-Hanson; a variable that reaches its bound leaves the free set.
//   - the free columns are kept linearly independent (a new column whose Gram-Schmidt residual is below 1e-10 of its
//     norm is refused), so the free set never exceeds rank A <= m <= 8 and the solve is a <= 8 x 8 system.  A new
//     column whose least-squares value moves the wrong way (round-off) is refused as well; refused columns stay out
//     until x changes.  This is what makes zero / duplicate columns and rank-deficient A safe.
// The free-set solve is uniform across the wave: every lane computes it redundantly from a per-wave LDS block (same
// addresses in every lane = broadcasts), so no lane waits on another and nothing is indexed dynamically in registers.
// Reductions are fixed DPP / butterfly trees: bitwise reproducible.
#pragma once
#include "common.h"
#include "wave.h"

#define GQ_EX_NC 2    // columns per lane: nz <= 128
#define GQ_EX_MAXF 8  // free columns at most (rank A <= m <= 8)

enum { GQ_EX_FREE = 0, GQ_EX_LOW = 1, GQ_EX_UP = 2, GQ_EX_REST = 3, GQ_EX_DEAD = 4 };

struct GqExLds {              // per-wavefront scratch of the free-set solve
  double col[GQ_EX_MAXF][8];  // free columns (rows padded with zeros)
  double q[GQ_EX_MAXF][8];    // orthonormal basis of the free columns
  double rr[GQ_EX_MAXF][GQ_EX_MAXF];  // R of the Gram-Schmidt factorisation, rr[t][s], t <= s
  double y[GQ_EX_MAXF], z[GQ_EX_MAXF], xf[GQ_EX_MAXF];
  double b[8], rhs[8];  // right-hand side; right-hand side of the free-set problem
  int idx[GQ_EX_MAXF];
};

__device__ __forceinline__ double gq_ex_readlane_d(double v, int l) {
  const GqD2 s = gq_split_d(v);
  return gq_join_d(__builtin_amdgcn_readlane(s.lo, l), __builtin_amdgcn_readlane(s.hi, l));
}
__device__ __forceinline__ double gq_ex_wave_sum_d(double v) {  // fixed butterfly: every lane holds the same sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, GQ_WAVE);
  return v;
}
__device__ __forceinline__ double gq_ex_wave_max_d(double v) {  // exact, order-independent
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, GQ_WAVE));
  return v;
}

// least squares on the k free columns against L->rhs: z (LDS) = argmin |C z - rhs|.  Returns false if the LAST column's
// Gram-Schmidt residual is below 1e-10 of its norm (it depends on the others).
template <int MR>
__device__ __forceinline__ bool gq_ex_free_solve(GqExLds* L, int k) {
  bool ok = true;
#pragma unroll 1
  for (int s = 0; s < k; ++s) {  // Gram-Schmidt in place in LDS: q[s] <- col[s], orthogonalised against q[0..s)
    double n0 = 0.0;
#pragma unroll
    for (int r = 0; r < MR; ++r) {
      const double v = L->col[s][r];
      L->q[s][r] = v;
      n0 = fma(v, v, n0);
    }
#pragma unroll 1
    for (int t = 0; t < s; ++t) L->rr[t][s] = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {  // MGS with one re-orthogonalisation
#pragma unroll 1
      for (int t = 0; t < s; ++t) {
        double d = 0.0;
#pragma unroll
        for (int r = 0; r < MR; ++r) d = fma(L->q[t][r], L->q[s][r], d);
#pragma unroll
        for (int r = 0; r < MR; ++r) L->q[s][r] = fma(-d, L->q[t][r], L->q[s][r]);
        L->rr[t][s] += d;
      }
    }
    double n1 = 0.0;
#pragma unroll
    for (int r = 0; r < MR; ++r) n1 = fma(L->q[s][r], L->q[s][r], n1);
    const double nrm = sqrt(n1);
    if (s == k - 1 && !(n1 > 1e-20 * n0)) ok = false;
    const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
#pragma unroll
    for (int r = 0; r < MR; ++r) L->q[s][r] *= inv;
    L->rr[s][s] = nrm;
  }
#pragma unroll 1
  for (int s = 0; s < k; ++s) {
    double d = 0.0;
#pragma unroll
    for (int r = 0; r < MR; ++r) d = fma(L->q[s][r], L->rhs[r], d);
    L->y[s] = d;
  }
  #pragma unroll 1
  for (int s = k - 1; s >= 0; --s) {
    double t = L->y[s];
    #pragma unroll 1
    for (int u = s + 1; u < k; ++u) t = fma(-L->rr[s][u], L->z[u], t);
    const double d = L->rr[s][s];
    L->z[s] = d > 0.0 ? t / d : 0.0;
  }
  return ok;
}

// r = A x summed over the wave (every lane holds the sum); skip_free: leave the free columns out.
template <int MR, typename TA>
__device__ __forceinline__ void gq_ex_partial(const TA (&a)[GQ_EX_NC][MR], const double (&x)[GQ_EX_NC],
                                              const int (&st)[GQ_EX_NC], bool skip_free, double (&r)[MR]) {
#pragma unroll
  for (int q = 0; q < MR; ++q) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < GQ_EX_NC; ++c)
      if (!(skip_free && st[c] == GQ_EX_FREE)) s = fma((double)a[c][q], x[c], s);
    r[q] = s;
  }
#pragma unroll
  for (int q = 0; q < MR; ++q) r[q] = gq_ex_wave_sum_d(r[q]);
}

struct GqExResult {
  double cost;
  int status;  // iterations (free-set solves) used, -1 if the cap was hit
};

// BVLS on one wavefront.  a: this lane's columns (TA = float when the input is fp32: exact, half the registers) (rows >= m and columns >= nz zero), L->b: the right-hand side (set by
// the caller), x: out, this lane's columns.  lo <= hi finite.  Every inner solve counts as one iteration against
// max_iter.
template <int MR, typename TA>
__device__ __forceinline__ GqExResult gq_bvls_wave(const TA (&a)[GQ_EX_NC][MR], double lo, double hi, int nz,
                                                   int max_iter, GqExLds* L, double (&x)[GQ_EX_NC]) {
  const int lane = gq_lane();
  int st[GQ_EX_NC];
  bool blk[GQ_EX_NC];
  double anrm2 = 0.0;
#pragma unroll
  for (int c = 0; c < GQ_EX_NC; ++c) {
    const int i = lane + GQ_WAVE * c;
    blk[c] = false;
    if (i >= nz) {
      st[c] = GQ_EX_DEAD;
      x[c] = 0.0;
    } else if (lo <= 0.0 && 0.0 <= hi) {
      x[c] = 0.0;
      st[c] = lo == 0.0 ? GQ_EX_LOW : (hi == 0.0 ? GQ_EX_UP : GQ_EX_REST);
    } else if (lo > 0.0) {
      x[c] = lo;
      st[c] = GQ_EX_LOW;
    } else {
      x[c] = hi;
      st[c] = GQ_EX_UP;
    }
#pragma unroll
    for (int q = 0; q < MR; ++q) anrm2 = fma((double)a[c][q], (double)a[c][q], anrm2);
  }
  anrm2 = gq_ex_wave_sum_d(anrm2);
  double bnrm2 = 0.0;
#pragma unroll
  for (int q = 0; q < MR; ++q) bnrm2 = fma(L->b[q], L->b[q], bnrm2);
  const double an = sqrt(anrm2), bn = sqrt(bnrm2), sq = sqrt((double)nz);
  const bool movable = hi > lo;
  int k = 0, it = 0;
  bool capped = false;
  double cost = 0.0;
  for (;;) {
    // residual and gradient at the current point (the free variables sit at their least-squares optimum)
    double r[MR];
    gq_ex_partial<MR, TA>(a, x, st, false, r);
    cost = 0.0;
#pragma unroll
    for (int q = 0; q < MR; ++q) {
      r[q] = L->b[q] - r[q];
      cost = fma(r[q], r[q], cost);
    }
    if (!movable || capped) break;
    double w[GQ_EX_NC];
    double xi = 0.0;
#pragma unroll
    for (int c = 0; c < GQ_EX_NC; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < MR; ++q) s = fma((double)a[c][q], r[q], s);
      w[c] = s;
      xi = fmax(xi, fabs(x[c]));
      blk[c] = false;
    }
    xi = gq_ex_wave_max_d(xi);
    // KKT tolerance: a few hundred ulps of the gradient's magnitude
    const double tol = 1e-13 * an * (bn + an * sq * xi) + 1e-300;
    bool advanced = false;
    while (!advanced) {
      double sc[GQ_EX_NC];
#pragma unroll
      for (int c = 0; c < GQ_EX_NC; ++c) {
        sc[c] = st[c] == GQ_EX_LOW ? w[c] : st[c] == GQ_EX_UP ? -w[c] : st[c] == GQ_EX_REST ? fabs(w[c]) : -1.0;
        if (blk[c]) sc[c] = -1.0;
      }
      const double mx = gq_ex_wave_max_d(fmax(sc[0], sc[1]));
      if (!(mx > tol)) break;  // KKT conditions hold: optimal
      const unsigned long long m0 = __ballot(sc[0] == mx), m1 = __ballot(sc[1] == mx);
      const int j = m0 ? (__ffsll((long long)m0) - 1) : (GQ_WAVE + __ffsll((long long)m1) - 1);
      const int jl = j & (GQ_WAVE - 1), jc = j >> 6;
      if (k >= GQ_EX_MAXF || k >= MR) {  // cannot happen with independent free columns; never grow past the rank
        if (lane == jl) {
          if (jc) blk[1] = true;
          else blk[0] = true;
        }
        continue;
      }
      // the new column and its current value, broadcast from its lane
      const int from = __builtin_amdgcn_readlane(jc ? st[1] : st[0], jl);
      const double xj = gq_ex_readlane_d(jc ? x[1] : x[0], jl);
#pragma unroll
      for (int q = 0; q < MR; ++q) L->col[k][q] = gq_ex_readlane_d((double)(jc ? a[1][q] : a[0][q]), jl);
      L->idx[k] = j;
      L->xf[k] = xj;
      if (lane == jl) {
        if (jc) st[1] = GQ_EX_FREE;
        else st[0] = GQ_EX_FREE;
      }
      ++k;
      bool first = true;
      for (;;) {  // inner loop: least squares on the free set, step back to feasibility
        if (it >= max_iter) {
          capped = true;
          break;
        }
        ++it;
        {
          double rhs[MR];
          gq_ex_partial<MR, TA>(a, x, st, true, rhs);
#pragma unroll
          for (int q = 0; q < MR; ++q) L->rhs[q] = L->b[q] - rhs[q];
        }
        const bool indep = gq_ex_free_solve<MR>(L, k);
        if (first) {
          const double zj = L->z[k - 1];
          const bool wrong = (from == GQ_EX_LOW && !(zj > xj)) || (from == GQ_EX_UP && !(zj < xj)) || !(zj == zj);
          if (!indep || wrong) {  // refuse the column: back to where it was, out of the selection until x changes
            --k;
            if (lane == jl) {
              if (jc) {
                st[1] = from;
                blk[1] = true;
              } else {
                st[0] = from;
                blk[0] = true;
              }
            }
            break;
          }
          first = false;
        }
        double alpha = 1.0;
        int hit = -1;
        #pragma unroll 1
        for (int s = 0; s < k; ++s) {
          const double zs = L->z[s], xs = L->xf[s];
          double as = 2.0;
          if (zs < lo) as = (lo - xs) / (zs - xs);
          else if (zs > hi) as = (hi - xs) / (zs - xs);
          if (as < alpha) {
            alpha = as;
            hit = s;
          }
        }
        if (hit < 0) {
          #pragma unroll 1
          for (int s = 0; s < k; ++s) L->xf[s] = L->z[s];
          advanced = true;
          break;
        }
        alpha = fmax(alpha, 0.0);
        // move, then every free variable at (or, by round-off, past) a bound leaves the free set
        int kk = 0;
        #pragma unroll 1
        for (int s = 0; s < k; ++s) {
          const double xs = fma(alpha, L->z[s] - L->xf[s], L->xf[s]);
          const int js = L->idx[s];
          int to = -1;
          if (s == hit) to = L->z[s] < lo ? GQ_EX_LOW : GQ_EX_UP;
          else if (xs <= lo) to = GQ_EX_LOW;
          else if (xs >= hi) to = GQ_EX_UP;
          if (to >= 0) {
            if (lane == (js & (GQ_WAVE - 1))) {
              const double v = to == GQ_EX_LOW ? lo : hi;
              if (js >> 6) {
                x[1] = v;
                st[1] = to;
              } else {
                x[0] = v;
                st[0] = to;
              }
            }
          } else {
            L->idx[kk] = js;
            L->xf[kk] = xs;
#pragma unroll
            for (int q = 0; q < 8; ++q) L->col[kk][q] = L->col[s][q];
            ++kk;
          }
        }
        k = kk;
        advanced = true;  // x moved: the refused columns may be tried again
        if (k == 0) break;
      }
      if (capped) advanced = true;
      // the free variables' values back into their lanes
      #pragma unroll 1
      for (int s = 0; s < k; ++s) {
        const int js = L->idx[s];
        const double v = L->xf[s];
        if (lane == (js & (GQ_WAVE - 1))) {
          if (js >> 6) x[1] = v;
          else x[0] = v;
        }
      }
    }
    if (!advanced) break;
  }
  GqExResult res;
  res.cost = 0.5 * cost;
  res.status = capped ? -1 : it;
  return res;
}
