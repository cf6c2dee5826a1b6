// The row frame of the hand-surface terms: what gq_tabletop_kernel (tabletop.hip), gq_scene_row (scene_row_dev.h), gq_approach_row
// (approach_row_dev.h) and gq_pregrasp_row (pregrasp.hip) have in common.  One block of GQ_ROW_WAVES wavefronts per row; wavefront w
// takes the 64-sample chunks w, w+8, ..., lane = sample; for every link met in a chunk the N masked values of the lanes are summed
// over the wavefront by the DPP network and added to the accumulators that lane l keeps for link l; the wavefronts' partial sums
// meet in LDS and wavefront 0 folds them in wavefront order.  No atomics: the order of every sum depends only on the order of the
// samples.  N = 4 for the table plane (S_l, n_l), 6 for the grid terms (sum g_h, sum x_h x g_h).
//
// Every piece is the text the four bodies used to carry, moved: no operation was re-associated or hoisted, and the six kernels that
// inline the bodies are instruction for instruction what they were.  That is why four of the pieces are macros (below, at
// GQ_ROW_LINK_SUMS).  The __shared__ arrays stay declared in the bodies (the LDS layout is theirs), and so does the sample prefetch
// (l = sample_link[s], p = samples[3s..]): as a function, in either form tried, it costs gq_scene_kernel two VGPRs and with them an
// occupancy step.
#pragma once
#include "common.h"

#define GQ_ROW_MAX_LINKS 64  // lane l of a wavefront owns link l
#define GQ_ROW_WAVES 8       // 512 default samples: one 64-sample chunk per wavefront

// accumulate: a plain rounded add of the finished value (no contraction with the product that made it), so that adding to
// a buffer gives the bits of buffer + (the overwriting launch's value)
__device__ __forceinline__ void gq_row_store(float* p, float v, int accumulate) {
#pragma clang fp contract(off)
  *p = accumulate ? *p + v : v;
}

// x_h = T p for a link transform [A | b], 3x4 row-major at T[0..11]
__device__ __forceinline__ gq3 gq_row_point(const float* T, gq3 p) {
  return gq_mk(fmaf(T[0], p.x, fmaf(T[1], p.y, fmaf(T[2], p.z, T[3]))),
               fmaf(T[4], p.x, fmaf(T[5], p.y, fmaf(T[6], p.z, T[7]))),
               fmaf(T[8], p.x, fmaf(T[9], p.y, fmaf(T[10], p.z, T[11]))));
}

// One chunk: the lane's sample rides on link l (-1: none) and holds v[N]; lane k adds the wavefront's sum over link k to acc[N] and
// runs SEEN (`seen = 1`: the wavefront met the link, active or not; empty for a body that keeps no flags).  This, GQ_ROW_WAVE_PARTIALS,
// GQ_ROW_FOLD and GQ_ROW_GRT are text, not functions: as __forceinline__ functions they give the six kernels another instruction
// stream (the same figures and the same additions), as text the kernels are instruction for instruction what they were.
#define GQ_ROW_LINK_SUMS(N, l, L, lane, v, acc, SEEN)                                                     \
  for (int k_ = 0; k_ < (L); ++k_) {                                                                      \
    const bool mine_ = (l) == k_;                                                                         \
    if (__ballot(mine_) == 0ull) continue; /* wave-uniform */                                             \
    float r_[N];                                                                                          \
    _Pragma("unroll") for (int q_ = 0; q_ < (N); ++q_) r_[q_] = gq_dpp_sum(mine_ ? (v)[q_] : 0.0f);       \
    if ((lane) == k_) {                                                                                   \
      _Pragma("unroll") for (int q_ = 0; q_ < (N); ++q_) (acc)[q_] += r_[q_];                             \
      SEEN;                                                                                               \
    }                                                                                                     \
  }

// The wavefront's energy and K (nine per-lane accumulators over the lane's chunks) to LDS; e becomes the wavefront's sum
#define GQ_ROW_WAVE_PARTIALS(e, K, lane, wv, s_e, s_K)                                                    \
  {                                                                                                       \
    (e) = gq_dpp_sum(e);                                                                                  \
    float Kw_ = 0.0f; /* lane q < 9 of the wavefront keeps the wavefront's K[q] */                        \
    _Pragma("unroll") for (int q_ = 0; q_ < 9; ++q_) {                                                    \
      const float kq_ = gq_dpp_sum((K)[q_]);                                                              \
      if ((lane) == q_) Kw_ = kq_;                                                                        \
    }                                                                                                     \
    if ((lane) == 0) (s_e)[wv] = (e);                                                                     \
    if ((lane) < 9) (s_K)[wv][lane] = Kw_;                                                                \
  }

// Lane l folds link l over the wavefronts, in wavefront order, into tot[N]; `present`: whether any wavefront met a sample of the link
#define GQ_ROW_FOLD(N, s_part, s_seen, lane, tot, present)                                                \
  for (int w_ = 0; w_ < GQ_ROW_WAVES; ++w_) {                                                             \
    _Pragma("unroll") for (int q_ = 0; q_ < (N); ++q_) (tot)[q_] += (s_part)[w_][lane][q_];               \
    (present) |= (s_seen)[w_][lane];                                                                      \
  }

// ... for a body that keeps no flags (gq_pregrasp_row: its link sums go to LDS, not to a wrench that may be left alone)
#define GQ_ROW_FOLD_SUMS(N, s_part, lane, tot)                                                            \
  for (int w_ = 0; w_ < GQ_ROW_WAVES; ++w_) {                                                             \
    _Pragma("unroll") for (int q_ = 0; q_ < (N); ++q_) (tot)[q_] += (s_part)[w_][lane][q_];               \
  }

// gRt of the row by wavefront 0, from the folded link sums (tot[0..2] = sum g_h of link `lane`; lanes >= L hold zeros) and the
// wavefronts' K: lanes 0..2 hold gsum = -sum g_h, lanes 3..11 K, row-major, folded over the wavefronts in wavefront order
#define GQ_ROW_GRT(gRt, row, tot, s_K, lane, up, accumulate)                                              \
  {                                                                                                       \
    const float Fx_ = gq_dpp_sum((tot)[0]), Fy_ = gq_dpp_sum((tot)[1]), Fz_ = gq_dpp_sum((tot)[2]);       \
    if ((gRt) && (lane) < 12) {                                                                           \
      float val_ = (lane) == 0 ? -Fx_ : ((lane) == 1 ? -Fy_ : -Fz_);                                      \
      if ((lane) >= 3) {                                                                                  \
        val_ = 0.0f;                                                                                      \
        for (int w_ = 0; w_ < GQ_ROW_WAVES; ++w_) val_ += (s_K)[w_][(lane) - 3];                          \
      }                                                                                                   \
      gq_row_store((gRt) + (row) * 12 + (lane), (up) * val_, accumulate);                                 \
    }                                                                                                     \
  }

// The row's energy from the wavefronts' sums: a fixed pairwise tree
__device__ __forceinline__ float gq_row_energy(const float* s_e) {
  return ((s_e[0] + s_e[1]) + (s_e[2] + s_e[3])) + ((s_e[4] + s_e[5]) + (s_e[6] + s_e[7]));
}
