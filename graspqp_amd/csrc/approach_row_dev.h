// The row body of the approach term's fused launch (approach.hip has the derivation and the shape of the block): everything one
// block of eight wavefronts does for one row, as ONE function that takes the grid by reference.  gq_approach_kernel
// (approach.hip) calls it with the launch's one grid; gq_clutter_corridor_kernel (clutter.hip) with the grid of the row's
// object.  Nothing else differs between the two launches, so row b's numbers are bit for bit the same at the same grid.
#pragma once
#include "approach_dev.h"

#define GQ_AP_MAX_LINKS 64     // lane l of a wavefront owns link l
#define GQ_AP_WAVES 8          // 512 default samples: one 64-sample chunk per wavefront
#define GQ_AP_MAX_STATIONS 32

struct GqApproachArgs {
  gqSceneGrid grid;
  const float* samples;        // (Ns,3) link frame
  const int32_t* sample_link;  // (Ns)
  const float* hand_pose;      // (B,D)
  const float* Rg;             // (B,9)
  const float* link_T;         // (B,L,12)
  const float* up_approach;    // (B) or null
  int Ns, L, D, K;
  float margin, w_approach, distance;
  float ax, ay, az;  // approach axis, hand frame
  int accumulate;
  float* e_approach;  // (B) or null
  float* wrench;      // (B,L,6) or null
  float* gRt;         // (B,12) or null
};

// accumulate: a plain rounded add of the finished value (no contraction with the product that made it), so that adding to
// a buffer gives the bits of buffer + (the overwriting launch's value)
__device__ __forceinline__ void gq_ap_store(float* p, float v, int accumulate) {
#pragma clang fp contract(off)
  *p = accumulate ? *p + v : v;
}

// row = blockIdx.x; `grid` is the grid this row reads (g.grid itself in the single-grid launch)
__device__ __forceinline__ void gq_approach_row(const GqApproachArgs& g, const gqSceneGrid& grid) {
  __shared__ float s_T[GQ_AP_MAX_LINKS * 12];
  __shared__ float s_part[GQ_AP_WAVES][GQ_AP_MAX_LINKS][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ int s_seen[GQ_AP_WAVES][GQ_AP_MAX_LINKS];       // the wavefront met a sample of the link (active or not)
  __shared__ float s_K[GQ_AP_WAVES][9];
  __shared__ float s_e[GQ_AP_WAVES];
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L, nK = g.K;
  for (int i = tid; i < L * 12; i += GQ_AP_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
  const float* R = g.Rg + row * 9;
  const gq3 r1 = gq_mk(R[0], R[1], R[2]), r2 = gq_mk(R[3], R[4], R[5]), r3 = gq_mk(R[6], R[7], R[8]);
  const float* tp = g.hand_pose + row * g.D;
  const gq3 t = gq_mk(tp[0], tp[1], tp[2]);
  const gq3 a = gq_mk(g.ax, g.ay, g.az);
  // the first chunk's samples do not depend on the staged transforms: loaded before the barrier
  const int chunks = (g.Ns + GQ_WAVE - 1) / GQ_WAVE;
  int s = wv * GQ_WAVE + lane;
  int l = -1;
  gq3 p = gq_mk(0, 0, 0);
  if (wv < chunks && s < g.Ns) {
    l = g.sample_link[s];
    p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
  }
  __syncthreads();
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float K[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float e = 0.0f;
  int seen = 0;
  for (int c = wv; c < chunks; c += GQ_AP_WAVES) {
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if ((unsigned)l < (unsigned)L) {
      const float* T = s_T + l * 12;
      const gq3 xh = gq_mk(fmaf(T[0], p.x, fmaf(T[1], p.y, fmaf(T[2], p.z, T[3]))),
                           fmaf(T[4], p.x, fmaf(T[5], p.y, fmaf(T[6], p.z, T[7]))),
                           fmaf(T[8], p.x, fmaf(T[9], p.y, fmaf(T[10], p.z, T[11]))));
      gq3 G = gq_mk(0, 0, 0);  // sum of g_h over the stations of this sample
      gq_approach_stations(grid, xh, a, r1, r2, r3, t, g.distance, nK, g.margin, e, G, K);
      const gq3 m = gq_cross(xh, G);
      v[0] = G.x, v[1] = G.y, v[2] = G.z, v[3] = m.x, v[4] = m.y, v[5] = m.z;
    } else {
      l = -1;  // a link id outside the hand (refused by ops.SurfaceSamples): the sample is ignored
    }
    for (int k = 0; k < L; ++k) {
      const bool mine = l == k;
      if (__ballot(mine) == 0ull) continue;  // wave-uniform
      float r[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) r[q] = gq_dpp_sum(mine ? v[q] : 0.0f);
      if (lane == k) {
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[q] += r[q];
        seen = 1;
      }
    }
    s += GQ_AP_WAVES * GQ_WAVE;
    l = -1;
    if (c + GQ_AP_WAVES < chunks && s < g.Ns) {
      l = g.sample_link[s];
      p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
    }
  }
  e = gq_dpp_sum(e);
  float Kw = 0.0f;  // lane q < 9 of the wavefront keeps the wavefront's K[q]
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    const float kq = gq_dpp_sum(K[q]);
    if (lane == q) Kw = kq;
  }
  if (lane == 0) s_e[wv] = e;
  if (lane < 9) s_K[wv][lane] = Kw;
  if (lane < L) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s_part[wv][lane][q] = acc[q];
    s_seen[wv][lane] = seen;
  }
  __syncthreads();
  if (wv != 0) return;
  // wavefront 0: lane l folds link l over the wavefronts, in wavefront order
  const float invK = 1.0f / (float)nK;
  const float up = (g.up_approach ? g.up_approach[row] : g.w_approach) * invK;
  float tot[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (lane < L) {
    int present = 0;
    for (int w = 0; w < GQ_AP_WAVES; ++w) {
#pragma unroll
      for (int q = 0; q < 6; ++q) tot[q] += s_part[w][lane][q];
      present |= s_seen[w][lane];
    }
    if (g.wrench && (present || !g.accumulate)) {  // links without samples: zero (overwrite) or left alone (accumulate)
      float* w6 = g.wrench + (row * L + lane) * 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) gq_ap_store(w6 + q, up * tot[q], g.accumulate);
    }
  }
  // row sums over the links (lanes >= L hold zeros)
  const float Fx = gq_dpp_sum(tot[0]), Fy = gq_dpp_sum(tot[1]), Fz = gq_dpp_sum(tot[2]);
  if (g.gRt && lane < 12) {
    // lanes 0..2: gsum = -sum g_h; lanes 3..11: K9, row-major, folded over the wavefronts in wavefront order
    float val = lane == 0 ? -Fx : (lane == 1 ? -Fy : -Fz);
    if (lane >= 3) {
      val = 0.0f;
      for (int w = 0; w < GQ_AP_WAVES; ++w) val += s_K[w][lane - 3];
    }
    gq_ap_store(g.gRt + row * 12 + lane, up * val, g.accumulate);
  }
  if (lane == 0 && g.e_approach)
    g.e_approach[row] = (((s_e[0] + s_e[1]) + (s_e[2] + s_e[3])) + ((s_e[4] + s_e[5]) + (s_e[6] + s_e[7]))) * invK;
}
