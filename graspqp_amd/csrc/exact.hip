// Exact grasp-quality evaluation: batched bounded least squares solved to optimality (BVLS, exact_dev.h) and the fused
// span metrics on top of it.  Replaces scipy.optimize.lsq_linear in metrics/solver/scipy_solver.py:61-131 and the
// GRASPQP_SCIPY / GRASPQP_EUCLIDIAN_SCIPY metrics of metrics/ops/registry.py:108-131 (span.py:94-231,313-415).
#include <math.h>

#include "common.h"
#include "exact_dev.h"
#include "fc_dev.h"

#define GQ_EX_WAVES 4  // problems (wavefronts) per block of gq_lsq_exact_kernel

__device__ __forceinline__ bool gq_ex_finite(double v) { return v - v == 0.0; }

template <typename T>
__global__ __launch_bounds__(GQ_EX_WAVES * GQ_WAVE) void gq_lsq_exact_kernel(const T* __restrict__ A,
                                                                             const T* __restrict__ b, int64_t B, int m,
                                                                             int nz, double lo, double hi, int max_iter,
                                                                             T* __restrict__ x, T* __restrict__ cost,
                                                                             int32_t* __restrict__ status) {
  __shared__ GqExLds lds[GQ_EX_WAVES];
  const int wv = threadIdx.x >> 6, lane = gq_lane();
  const int64_t row = (int64_t)blockIdx.x * GQ_EX_WAVES + wv;
  if (row >= B) return;  // whole wavefront: no block barrier below
  const T* Ar = A + row * m * nz;
  double a[GQ_EX_NC][8];  // fp64 registers for either input type (fewer VGPRs than float storage converted on use)
  double xv[GQ_EX_NC];
  GqExLds* L = &lds[wv];
  bool fin = true;
#pragma unroll
  for (int c = 0; c < GQ_EX_NC; ++c) {
    const int i = lane + GQ_WAVE * c;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[c][q] = (i < nz && q < m) ? (double)Ar[(size_t)q * nz + i] : 0.0;
      fin = fin && gq_ex_finite((double)a[c][q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double bq = q < m ? (double)b[row * m + q] : 0.0;
    L->b[q] = bq;
    fin = fin && gq_ex_finite(bq);
  }
  T* xr = x + row * nz;
  if (__ballot(!fin)) {  // non-finite inputs: NaN value and x, status -2
    for (int i = lane; i < nz; i += GQ_WAVE) xr[i] = (T)NAN;
    if (lane == 0) {
      cost[row] = (T)NAN;
      status[row] = -2;
    }
    return;
  }
  const GqExResult res = gq_bvls_wave<8, double>(a, lo, hi, nz, max_iter, L, xv);
#pragma unroll
  for (int c = 0; c < GQ_EX_NC; ++c) {
    const int i = lane + GQ_WAVE * c;
    if (i < nz) xr[i] = (T)xv[c];
  }
  if (lane == 0) {
    cost[row] = (T)res.cost;
    status[row] = res.status;
  }
}

// One block per row, one wavefront per basis problem.  The grasp matrix F (6 x nz) is built once per row into LDS with
// the loop's cone construction (gq_cone_column), every wavefront then solves its basis problem on it:
//   NB = 1:  b = 0 (span.py:313-415), NB = 12: b = +e_i (i < 6) / -e_(i-6) (span.py:94-231).
// Wavefront 0 also writes svd = det(F F')^(1/12) = (prod sigma)^(1/6), as the loop's fcstep_dev.h does.
template <int NB>
__global__ __launch_bounds__(NB * GQ_WAVE) void gq_span_exact_kernel(const float* __restrict__ cp,
                                                                     const float* __restrict__ cn,
                                                                     const float* __restrict__ cog, int n, int k, float mu,
                                                                     float tw, double lo, double hi, int max_iter,
                                                                     float* __restrict__ value, float* __restrict__ x_sum,
                                                                     float* __restrict__ svd, int32_t* __restrict__ status) {
  __shared__ float sF[6 * 128];
  __shared__ GqExLds lds[NB];
  const int64_t row = blockIdx.x;
  const int wv = threadIdx.x >> 6, lane = gq_lane();
  const int nz = n * k;
  const float* cpr = cp + row * n * 3;
  const float* cnr = cn + row * n * 3;
  const float* cgr = cog + row * 3;
  for (int i = threadIdx.x; i < nz; i += NB * GQ_WAVE) {
    const GqCone cone = gq_cone_column(cpr, cnr, cgr, i / k, i % k, k, mu, tw);
    sF[0 * nz + i] = cone.f.x;
    sF[1 * nz + i] = cone.f.y;
    sF[2 * nz + i] = cone.f.z;
    sF[3 * nz + i] = cone.tau.x;
    sF[4 * nz + i] = cone.tau.y;
    sF[5 * nz + i] = cone.tau.z;
  }
  __syncthreads();
  float a[GQ_EX_NC][6];
  double xv[GQ_EX_NC];
  bool fin = true;
#pragma unroll
  for (int c = 0; c < GQ_EX_NC; ++c) {
    const int i = lane + GQ_WAVE * c;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      a[c][q] = i < nz ? sF[q * nz + i] : 0.0f;
      fin = fin && gq_ex_finite((double)a[c][q]);
    }
  }
  const size_t sb = (size_t)row * NB + wv;
  const bool bad = __ballot(!fin) != 0;
  if (wv == 0) {
    double part[21];
#pragma unroll
    for (int t = 0; t < 21; ++t) part[t] = 0.0;
#pragma unroll
    for (int c = 0; c < GQ_EX_NC; ++c)
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) part[p * (p + 1) / 2 + q] = fma((double)a[c][p], (double)a[c][q], part[p * (p + 1) / 2 + q]);
    gq_wave_sums_d<21>(part);
    double Lm[21], inv[6];
    const bool ok = gq_chol6(part, Lm, inv);
    double lp = 1.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) lp *= Lm[t * (t + 1) / 2 + t];
    if (lane == 0) svd[row] = bad ? NAN : (ok ? powf((float)lp, 1.0f / 6.0f) : 0.0f);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) lds[wv].b[q] = NB == 1 ? 0.0 : (q == wv % 6 ? (wv < 6 ? 1.0 : -1.0) : 0.0);
  float* xs = x_sum ? x_sum + sb * n : nullptr;
  if (bad) {
    for (int c = lane; xs && c < n; c += GQ_WAVE) xs[c] = NAN;
    if (lane == 0) {
      value[sb] = NAN;
      status[sb] = -2;
    }
    return;
  }
  const GqExResult res = gq_bvls_wave<6, float>(a, lo, hi, nz, max_iter, &lds[wv], xv);
  if (lane == 0) {
    value[sb] = (float)res.cost;
    status[sb] = res.status;
  }
  if (xs) {  // per-contact force sums: x staged in this wavefront's LDS block (its solve is finished)
    double* buf = &lds[wv].col[0][0];  // 128 doubles: col + q
#pragma unroll
    for (int c = 0; c < GQ_EX_NC; ++c) {
      const int i = lane + GQ_WAVE * c;
      if (i < nz) buf[i] = xv[c];
    }
    gq_wave_sync();
    for (int c = lane; c < n; c += GQ_WAVE) {
      double s = 0.0;
      for (int e = 0; e < k; ++e) s += buf[c * k + e];
      xs[c] = (float)s;
    }
  }
}

extern "C" {

int gq_lsq_exact_check(int64_t batch, int m, int nz, double lower, double upper, int max_iter) {
  GQ_REQUIRE(batch >= 0 && batch <= ((int64_t)1 << 33), "lsq_exact: bad arguments (batch %lld)", (long long)batch);
  GQ_REQUIRE(m >= 1 && m <= 8, "lsq_exact: bad arguments: m = %d rows, 1 <= m <= 8 supported", m);
  GQ_REQUIRE(nz >= 1 && nz <= 128, "lsq_exact: bad arguments: nz = %d columns, 1 <= nz <= 128 supported", nz);
  GQ_REQUIRE(isfinite(lower) && isfinite(upper), "lsq_exact: bad arguments: bounds must be finite (got %g, %g)", lower, upper);
  GQ_REQUIRE(lower <= upper, "lsq_exact: bad arguments: lower %g > upper %g", lower, upper);
  GQ_REQUIRE(max_iter >= 0, "lsq_exact: bad arguments: max_iter %d < 0", max_iter);
  return GQ_OK;
}

int gq_lsq_exact_forward(const void* A, const void* b, int fp64, int64_t batch, int m, int nz, double lower,
                         double upper, int max_iter, void* x, void* cost, int32_t* status, void* stream) {
  const int rc = gq_lsq_exact_check(batch, m, nz, lower, upper, max_iter);
  if (rc) return rc;
  if (batch == 0) return GQ_OK;
  GQ_REQUIRE(A && b && x && cost && status, "lsq_exact: null pointer");
  const dim3 grid((unsigned)((batch + GQ_EX_WAVES - 1) / GQ_EX_WAVES));
  hipStream_t s = (hipStream_t)stream;
  if (fp64)
    gq_lsq_exact_kernel<double><<<grid, GQ_EX_WAVES * GQ_WAVE, 0, s>>>(
        (const double*)A, (const double*)b, batch, m, nz, lower, upper, max_iter, (double*)x, (double*)cost, status);
  else
    gq_lsq_exact_kernel<float><<<grid, GQ_EX_WAVES * GQ_WAVE, 0, s>>>(
        (const float*)A, (const float*)b, batch, m, nz, lower, upper, max_iter, (float*)x, (float*)cost, status);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_span_exact_check(int64_t batch, int n_contact, int n_cone, int n_basis, double lower, double upper,
                        int max_iter) {
  GQ_REQUIRE(n_contact >= 1 && n_cone >= 1 && (int64_t)n_contact * n_cone <= 128,
             "span_exact: bad arguments: n_contact %d x n_cone %d must be 1..128 columns", n_contact, n_cone);
  GQ_REQUIRE(n_basis == 1 || n_basis == 12, "span_exact: bad arguments: n_basis %d (1: overall, 12: Euclidean)", n_basis);
  GQ_REQUIRE(batch >= 0 && batch <= 0x7fffffff, "span_exact: bad arguments (batch %lld)", (long long)batch);
  return gq_lsq_exact_check(batch, 6, n_contact * n_cone, lower, upper, max_iter);
}

int gq_span_exact_forward(const float* contact_pts, const float* contact_normals, const float* cog, int64_t batch,
                          int n_contact, int n_cone, float friction, float torque_weight, int n_basis, double lower,
                          double upper, int max_iter, float* value, float* x_sum, float* svd, int32_t* status,
                          void* stream) {
  const int rc = gq_span_exact_check(batch, n_contact, n_cone, n_basis, lower, upper, max_iter);
  if (rc) return rc;
  if (batch == 0) return GQ_OK;
  GQ_REQUIRE(contact_pts && contact_normals && cog && value && svd && status, "span_exact: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_basis == 1)
    gq_span_exact_kernel<1><<<(unsigned)batch, GQ_WAVE, 0, s>>>(contact_pts, contact_normals, cog, n_contact, n_cone,
                                                                friction, torque_weight, lower, upper, max_iter, value,
                                                                x_sum, svd, status);
  else
    gq_span_exact_kernel<12><<<(unsigned)batch, 12 * GQ_WAVE, 0, s>>>(contact_pts, contact_normals, cog, n_contact,
                                                                      n_cone, friction, torque_weight, lower, upper,
                                                                      max_iter, value, x_sum, svd, status);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
