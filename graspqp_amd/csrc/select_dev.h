// Per-row bodies of the grasp-set selection (select.hip): the world transform of a link, the feasibility gate, the squared RMS
// displacement of the hand surface between two rows, and what a thread of the select block does with the rows it owns.  A
// thread of a block of T threads owns the rows tid, tid + T, ... of its object; the block only takes a minimum of 64-bit keys
// and a sum of counts over the threads.  The keys are totally ordered and carry the row, and the distance of a pair is ONE
// serial sum over the links in ascending order, so nothing depends on T or on the order of a reduction.
// tests/select_host.cpp runs these bodies for a serially emulated block on the host (behind tests/host_shim.h) and compares
// with a numpy fp64 oracle.
//
// Layouts: link_T (L,12) = [A | b] row-major 3x4 per link (x_h = A p + b, scene_row_dev.h), Rg (9) row-major,
// world transforms W (L,12) = [Rg A | Rg b + t], link moments (L,10) = n, c (3), Cxx Cxy Cxz Cyy Cyz Czz of the CENTRED
// second moment sum (p - c)(p - c)'.
//
// Every product-sum below is an explicit fmaf and contraction is off, so a host compiler with -ffp-contract=off gives the bits
// of the device.
#pragma once
#ifndef GQ_SCENE_HOST_BUILD
#include "common.h"
#endif
#include "init_select_dev.h"  // gq_sel_fill_key: (order-preserving bits of the score, row)

#define GQ_GS_MAX_TERMS 16
#define GQ_GS_NO_KEY (~0ull)  // above the key of every finite score: not feasible, picked or suppressed
#define GQ_GS_MOM 10

// W = [Rg A | Rg b + t] of one link
__device__ __forceinline__ void gq_gs_world(const float* Rg, const float* t, const float* T, float* W) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) {
    const float a = Rg[r * 3], b = Rg[r * 3 + 1], c = Rg[r * 3 + 2];
    for (int k = 0; k < 3; ++k) W[r * 4 + k] = fmaf(a, T[k], fmaf(b, T[4 + k], c * T[8 + k]));
    W[r * 4 + 3] = fmaf(a, T[3], fmaf(b, T[7], c * T[11])) + t[r];
  }
}

// row b is feasible iff its score is finite and every gated term (tol < +inf) is <= its tolerance; a NaN term under a gate
// fails the comparison, a term with tol = +inf is not read
__device__ __forceinline__ bool gq_gs_feasible(const float* score, const float* terms, int n_terms, size_t B, size_t b,
                                               const float* tol) {
  const float s = score[b];
  bool ok = s - s == 0.0f;  // finite
  for (int t = 0; t < n_terms; ++t)
    if (tol[t] < GQ_INF_F) ok = ok && terms[(size_t)t * B + b] <= tol[t];
  return ok;
}

// one row u of dA against the centred second moment: u C u' >= 0 in exact arithmetic, clamped so that rounding cannot
// make it negative
__device__ __forceinline__ float gq_gs_quad(float x, float y, float z, const float* C) {
#pragma clang fp contract(off)
  const float d = fmaf(C[0], x * x, fmaf(C[3], y * y, C[5] * (z * z)));
  const float o = fmaf(C[1], x * y, fmaf(C[2], x * z, C[4] * (y * z)));
  return fmaxf(fmaf(2.0f, o, d), 0.0f);
}

// d^2 = (1/Ns) sum over the hand-surface samples of |x_w,i(s) - x_w,j(s)|^2 in closed form: per link
// n |dA c + db|^2 + tr(dA C dA'), summed serially over the links in ascending order.  A link without samples adds an exact 0,
// whatever its transforms hold.  The loop has no branch and loads link l + 1 of Wi (global memory in the kernels; Wj and the
// moments sit in LDS there) while link l is summed, so the round trip of a link hides behind the sums of the one before.
__device__ __forceinline__ float gq_gs_dist2(const float* Wi, const float* Wj, const float* mom, int L, float inv_ns) {
#pragma clang fp contract(off)
  float sum = 0.0f;
  float a[12], next[12];
  for (int k = 0; k < 12; ++k) a[k] = Wi[k];
  for (int l = 0; l < L; ++l) {
    const float* an = Wi + (size_t)(l + 1 < L ? l + 1 : l) * 12;
    for (int k = 0; k < 12; ++k) next[k] = an[k];
    const float* m = mom + (size_t)l * GQ_GS_MOM;
    const float* b = Wj + (size_t)l * 12;
    float link = 0.0f, v2 = 0.0f;
    for (int r = 0; r < 3; ++r) {
      const float x = a[r * 4] - b[r * 4], y = a[r * 4 + 1] - b[r * 4 + 1], z = a[r * 4 + 2] - b[r * 4 + 2];
      const float v = fmaf(x, m[1], fmaf(y, m[2], fmaf(z, m[3], a[r * 4 + 3] - b[r * 4 + 3])));
      v2 = fmaf(v, v, v2);
      link += gq_gs_quad(x, y, z, m + 4);
    }
    sum += m[0] > 0.0f ? fmaf(m[0], v2, link) : 0.0f;
    for (int k = 0; k < 12; ++k) a[k] = next[k];
  }
  return sum * inv_ns;
}

// First pass of thread tid over the keys of its object: -> its smallest key and how many of its rows are feasible
__device__ __forceinline__ unsigned long long gq_gs_first_thread(const unsigned long long* key, int be, int tid, int T, int* count) {
  unsigned long long best = GQ_GS_NO_KEY;
  int c = 0;
  for (int r = tid; r < be; r += T) {
    const unsigned long long k = key[r];
    if (k == GQ_GS_NO_KEY) continue;
    ++c;
    best = k < best ? k : best;
  }
  *count = c;
  return best;
}

// Thread tid after the pick of row `pick` with world transforms Wp: the pick leaves, every remaining row closer than the radius
// (d^2 < r2, strict) leaves too; -> the smallest key among the thread's rows that stay.  r2 = 0 suppresses nothing and reads
// no transform.
__device__ __forceinline__ unsigned long long gq_gs_suppress_thread(unsigned long long* key, const float* W, int be, int tid, int T,
                                                                    int pick, const float* Wp, const float* mom, int L,
                                                                    float inv_ns, float r2) {
  unsigned long long best = GQ_GS_NO_KEY;
  for (int r = tid; r < be; r += T) {
    const unsigned long long k = key[r];
    if (k == GQ_GS_NO_KEY) continue;
    if (r == pick || (r2 > 0.0f && gq_gs_dist2(W + (size_t)r * L * 12, Wp, mom, L, inv_ns) < r2)) {
      key[r] = GQ_GS_NO_KEY;
      continue;
    }
    best = k < best ? k : best;
  }
  return best;
}
