// The row body of the lift term's launch (lift.hip has the derivation): everything one block of eight wavefronts does for one row,
// as gq_approach_row does it (approach_row_dev.h), with two additions.  The hand's stations carry the lift h_k u in their
// translation, and after its hand chunks a wavefront takes the 64-point chunks w, w+8, ... of the held object's points, which feed
// the row's energy, the object's share of it and K9 -- no per-link sums: no joint moves the object.
#pragma once
#include "lift_dev.h"
#include "sample_row_dev.h"  // the row frame of the hand-surface terms

#define GQ_LIFT_MAX_STATIONS 32

struct GqLiftArgs {
  gqSceneGrid grid;             // grid 0 of the stack
  const float* samples;         // (Ns,3) link frame
  const int32_t* sample_link;   // (Ns)
  const float* hand_pose;       // (B,D)
  const float* Rg;              // (B,9)
  const float* link_T;          // (B,L,12)
  const float* object_points;   // (n_obj,M,3) object frame, or null with M = 0
  const float* up_lift;         // (B) or null
  int Ns, L, D, K, M;
  int rows_per_grid, batch_each;
  float margin, object_margin, w_lift, height, retreat;
  float ax, ay, az;  // approach axis, hand frame
  float ux, uy, uz;  // lift direction, object frame
  int accumulate;
  float* e_lift;    // (B) or null
  float* e_object;  // (B) or null
  float* wrench;    // (B,L,6) or null
  float* gRt;       // (B,12) or null
};

// row = blockIdx.x; `grid` is the grid this row reads
__device__ __forceinline__ void gq_lift_row(const GqLiftArgs& g, const gqSceneGrid& grid) {
  __shared__ float s_T[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_part[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ int s_seen[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS];       // the wavefront met a sample of the link (active or not)
  __shared__ float s_K[GQ_ROW_WAVES][9];
  __shared__ float s_e[GQ_ROW_WAVES];
  __shared__ float s_eo[GQ_ROW_WAVES];  // the object's share of s_e
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L, nK = g.K;
  for (int i = tid; i < L * 12; i += GQ_ROW_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
  const float* R = g.Rg + row * 9;
  const gq3 r1 = gq_mk(R[0], R[1], R[2]), r2 = gq_mk(R[3], R[4], R[5]), r3 = gq_mk(R[6], R[7], R[8]);
  const float* tp = g.hand_pose + row * g.D;
  const gq3 t = gq_mk(tp[0], tp[1], tp[2]);
  const gq3 a = gq_mk(g.ax, g.ay, g.az), u = gq_mk(g.ux, g.uy, g.uz);
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
      gq_lift_hand_stations(grid, xh, a, r1, r2, r3, t, u, g.height, g.retreat, nK, g.margin, e, G, K);
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
  // the held object: points j = 64 c + lane of object row / batch_each, chunks w, w+8, ...; j < M <= 2^24 and
  // (row / batch_each) < n_obj, so the largest float read is n_obj M 3 - 1
  float eo = 0.0f;
  if (g.M > 0) {
    const gq3 Ra = gq_lift_world_axis(a, r1, r2, r3);
    const float* op = g.object_points + (row / (size_t)g.batch_each) * (size_t)g.M * 3;
    const int ochunks = (g.M + GQ_WAVE - 1) / GQ_WAVE;
    for (int c = wv; c < ochunks; c += GQ_ROW_WAVES) {
      const int j = c * GQ_WAVE + lane;
      if (j < g.M) {
        const gq3 q = gq_mk(op[(size_t)j * 3], op[(size_t)j * 3 + 1], op[(size_t)j * 3 + 2]);
        gq_lift_object_stations(grid, q, a, Ra, r1, r2, r3, u, g.height, g.retreat, nK, g.object_margin, eo, K);
      }
    }
    e += eo;
  }
  GQ_ROW_WAVE_PARTIALS(e, K, lane, wv, s_e, s_K)
  eo = gq_dpp_sum(eo);
  if (lane == 0) s_eo[wv] = eo;
  if (lane < L) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s_part[wv][lane][q] = acc[q];
    s_seen[wv][lane] = seen;
  }
  __syncthreads();
  if (wv != 0) return;
  // wavefront 0: lane l folds link l over the wavefronts, in wavefront order
  const float invK = 1.0f / (float)nK;
  const float up = (g.up_lift ? g.up_lift[row] : g.w_lift) * invK;
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
  GQ_ROW_GRT(g.gRt, row, tot, s_K, lane, up, g.accumulate)  // K is K9: g_h (x) the shifted point / the object's -d_k a
  if (lane == 0 && g.e_lift) g.e_lift[row] = gq_row_energy(s_e) * invK;
  if (lane == 0 && g.e_object) g.e_object[row] = gq_row_energy(s_eo) * invK;
}
