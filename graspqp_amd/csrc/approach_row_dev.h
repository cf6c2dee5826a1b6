// The row body of the approach term's fused launch (approach.hip has the derivation and the shape of the block): everything one
// block of eight wavefronts does for one row, as ONE function that takes the grid by reference.  gq_approach_kernel
// (approach.hip) calls it with the launch's one grid; gq_clutter_corridor_kernel (clutter.hip) with the grid of the row's
// object.  Nothing else differs between the two launches, so row b's numbers are bit for bit the same at the same grid.
#pragma once
#include "approach_dev.h"
#include "sample_row_dev.h"  // the row frame the four hand-surface terms share

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

// the arguments of a launch, checked by the caller, as the kernels take them; `grid` is the launch's grid or grid 0 of its stack
static inline GqApproachArgs gq_approach_args(const gqSceneGrid& grid, float margin, float distance, int n_stations,
                                              const float* samples, const int32_t* sample_link, int64_t n_samples, int n_links,
                                              const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                                              const float* grasp_axis, const float* up_approach, float w_approach,
                                              float* e_approach, int accumulate, float* link_wrench, float* gRt) {
  GqApproachArgs a{};
  a.grid = grid;
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.link_T = link_T;
  a.up_approach = up_approach;
  a.Ns = (int)n_samples, a.L = n_links, a.D = pose_dim, a.K = n_stations;
  a.margin = margin, a.w_approach = w_approach, a.distance = distance;
  a.ax = grasp_axis[0], a.ay = grasp_axis[1], a.az = grasp_axis[2];
  a.accumulate = accumulate != 0;
  a.e_approach = e_approach, a.wrench = link_wrench, a.gRt = gRt;
  return a;
}

// row = blockIdx.x; `grid` is the grid this row reads (g.grid itself in the single-grid launch)
__device__ __forceinline__ void gq_approach_row(const GqApproachArgs& g, const gqSceneGrid& grid) {
  __shared__ float s_T[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_part[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ int s_seen[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS];       // the wavefront met a sample of the link (active or not)
  __shared__ float s_K[GQ_ROW_WAVES][9];
  __shared__ float s_e[GQ_ROW_WAVES];
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L, nK = g.K;
  for (int i = tid; i < L * 12; i += GQ_ROW_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
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
  for (int c = wv; c < chunks; c += GQ_ROW_WAVES) {
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if ((unsigned)l < (unsigned)L) {
      const gq3 xh = gq_row_point(s_T + l * 12, p);
      gq3 G = gq_mk(0, 0, 0);  // sum of g_h over the stations of this sample
      gq_approach_stations(grid, xh, a, r1, r2, r3, t, g.distance, nK, g.margin, e, G, K);
      const gq3 m = gq_cross(xh, G);
      v[0] = G.x, v[1] = G.y, v[2] = G.z, v[3] = m.x, v[4] = m.y, v[5] = m.z;
    } else {
      l = -1;  // a link id outside the hand (refused by ops.SurfaceSamples): the sample is ignored
    }
    GQ_ROW_LINK_SUMS(6, l, L, lane, v, acc, seen = 1)
    s += GQ_ROW_WAVES * GQ_WAVE;
    l = -1;
    if (c + GQ_ROW_WAVES < chunks && s < g.Ns) {
      l = g.sample_link[s];
      p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
    }
  }
  GQ_ROW_WAVE_PARTIALS(e, K, lane, wv, s_e, s_K)
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
    GQ_ROW_FOLD(6, s_part, s_seen, lane, tot, present)
    if (g.wrench && (present || !g.accumulate)) {  // links without samples: zero (overwrite) or left alone (accumulate)
      float* w6 = g.wrench + (row * L + lane) * 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) gq_row_store(w6 + q, up * tot[q], g.accumulate);
    }
  }
  GQ_ROW_GRT(g.gRt, row, tot, s_K, lane, up, g.accumulate)  // K is K9 here: g_h (x) the shifted point
  if (lane == 0 && g.e_approach) g.e_approach[row] = gq_row_energy(s_e) * invK;
}
