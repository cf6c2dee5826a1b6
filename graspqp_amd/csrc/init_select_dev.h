// Per-candidate bodies of gq_init_select_kernel (init.hip): which hull candidates are collision-free, the farthest-point
// sampling among those, and the fill of the remaining slots by ascending penalty.  A thread of a block of T threads owns the
// candidates tid, tid + T, ...; what a thread does with them is here, what the block does with the threads' results (a maximum
// or a minimum of 64-bit keys, a sum, a minimum) is in the kernel.  The keys are totally ordered and carry the index, so the
// result does not depend on T or on the order of the reduction.  tests/init_select_host.cpp runs these bodies for a serially
// emulated block on the host (behind tests/host_shim.h) and compares with a numpy oracle.
//
// The running distances `dist` (M floats per object) double as the state of a candidate in phase 1:
//   dist >= 0 (or +inf)   in A and not yet picked
//   GQ_SEL_OUT (-1)       not in A (infeasible), or picked
#pragma once
#ifndef GQ_SCENE_HOST_BUILD
#include "common.h"
#endif

#define GQ_SEL_OUT (-1.0f)
#define GQ_SEL_NO_FPS_KEY 0ull             // below every key of a candidate in A (index < 2^30 -> low word > 0)
#define GQ_SEL_NO_FILL_KEY (~0ull)         // above every fill key (index < 2^30)

// squared distance of farthest-point sampling: the one expression of gq_init_fps_kernel and gq_init_select_kernel
__device__ __forceinline__ float gq_fps_dist2(float px, float py, float pz, float cx, float cy, float cz) {
  const float dx = px - cx, dy = py - cy, dz = pz - cz;
  return dx * dx + dy * dy + dz * dz;
}

// key = (distance bits, ~index): the maximum picks the largest distance and, among equals, the smallest index
__device__ __forceinline__ unsigned long long gq_fps_key(float d, int i) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
}
__device__ __forceinline__ int gq_fps_key_index(unsigned long long key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

// m is in A iff penalty <= tol: false for NaN, true for -0.0 at tol = 0
__device__ __forceinline__ bool gq_sel_feasible(float penalty, float tol) { return penalty <= tol; }

// key = (order-preserving bits of the penalty, index): the minimum picks the smallest penalty and, among equals, the smallest
// index; every NaN sorts after +inf
__device__ __forceinline__ unsigned long long gq_sel_fill_key(float penalty, int i) {
  unsigned u = __float_as_uint(penalty);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (penalty != penalty) u = 0xffffffffu;
  return ((unsigned long long)u << 32) | (unsigned long long)(unsigned)i;
}
__device__ __forceinline__ int gq_sel_fill_key_index(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }

// Set-up pass of thread tid: dist = +inf inside A, GQ_SEL_OUT outside; -> the thread's share of |A| and its smallest member
// (M when it has none)
__device__ __forceinline__ void gq_sel_init_thread(const float* penalty, float* dist, int M, float tol, int tid, int T, int* count,
                                                   int* first) {
  int c = 0, f = M;
  for (int i = tid; i < M; i += T) {
    const bool in = gq_sel_feasible(penalty[i], tol);
    dist[i] = in ? GQ_INF_F : GQ_SEL_OUT;
    if (in) {
      ++c;
      f = i < f ? i : f;
    }
  }
  *count = c;
  *first = f;
}

// Phase 1, thread tid after the pick of `cur` at (cx,cy,cz): cur leaves A, every other member of A gets
// dist = min(dist, |P - P[cur]|^2); -> the thread's largest key (GQ_SEL_NO_FPS_KEY when none of its candidates is in A)
__device__ __forceinline__ unsigned long long gq_sel_fps_thread(const float* P, float* dist, int M, int tid, int T, int cur, float cx,
                                                                float cy, float cz) {
  unsigned long long best = GQ_SEL_NO_FPS_KEY;
  for (int i = tid; i < M; i += T) {
    const float old = dist[i];
    if (old < 0.0f) continue;
    if (i == cur) {
      dist[i] = GQ_SEL_OUT;
      continue;
    }
    const float d = fminf(old, gq_fps_dist2(P[(size_t)i * 3], P[(size_t)i * 3 + 1], P[(size_t)i * 3 + 2], cx, cy, cz));
    dist[i] = d;
    const unsigned long long key = gq_fps_key(d, i);
    best = key > best ? key : best;
  }
  return best;
}

// Phase 2, thread tid: the smallest fill key above `last` among its candidates outside A (`any_last` = 0: no fill yet, every
// key qualifies); -> GQ_SEL_NO_FILL_KEY when there is none
__device__ __forceinline__ unsigned long long gq_sel_fill_thread(const float* penalty, int M, float tol, int tid, int T,
                                                                 int any_last, unsigned long long last) {
  unsigned long long best = GQ_SEL_NO_FILL_KEY;
  for (int i = tid; i < M; i += T) {
    const float p = penalty[i];
    if (gq_sel_feasible(p, tol)) continue;
    const unsigned long long key = gq_sel_fill_key(p, i);
    if (any_last && key <= last) continue;
    best = key < best ? key : best;
  }
  return best;
}
