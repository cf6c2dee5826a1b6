// The row body of the scene term's fused launch (scene.hip has the derivation and the shape of the block): everything one block
// of eight wavefronts does for one row, as ONE function that takes the grid by reference.  gq_scene_kernel (scene.hip) calls it
// with the launch's one grid; gq_clutter_kernel (clutter.hip) with the grid of the row's object.  Nothing else differs between
// the two launches, so row b's numbers are bit for bit the same at the same grid.
#pragma once
#include "sample_row_dev.h"  // the row frame the four hand-surface terms share
#include "scene_dev.h"

struct GqSceneArgs {
  gqSceneGrid grid;
  const float* samples;        // (Ns,3) link frame
  const int32_t* sample_link;  // (Ns)
  const float* hand_pose;      // (B,D)
  const float* Rg;             // (B,9)
  const float* link_T;         // (B,L,12)
  const float* up_scene;       // (B) or null
  int Ns, L, D;
  float margin, w_scene;
  int accumulate;
  float* e_scene;  // (B) or null
  float* wrench;   // (B,L,6) or null
  float* gRt;      // (B,12) or null
};

// the arguments of a launch, checked by the caller, as the kernels take them; `grid` is the launch's grid or grid 0 of its stack
static inline GqSceneArgs gq_scene_args(const gqSceneGrid& grid, float margin, const float* samples, const int32_t* sample_link,
                                        int64_t n_samples, int n_links, const float* hand_pose, int pose_dim, const float* Rg,
                                        const float* link_T, const float* up_scene, float w_scene, float* e_scene, int accumulate,
                                        float* link_wrench, float* gRt) {
  GqSceneArgs a{};
  a.grid = grid;
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.link_T = link_T;
  a.up_scene = up_scene;
  a.Ns = (int)n_samples, a.L = n_links, a.D = pose_dim;
  a.margin = margin, a.w_scene = w_scene;
  a.accumulate = accumulate != 0;
  a.e_scene = e_scene, a.wrench = link_wrench, a.gRt = gRt;
  return a;
}

// row = blockIdx.x; `grid` is the grid this row reads (g.grid itself in the single-grid launch)
__device__ __forceinline__ void gq_scene_row(const GqSceneArgs& g, const gqSceneGrid& grid) {
  __shared__ float s_T[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_part[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ int s_seen[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS];       // the wavefront met a sample of the link (active or not)
  __shared__ float s_K[GQ_ROW_WAVES][9];
  __shared__ float s_e[GQ_ROW_WAVES];
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L;
  for (int i = tid; i < L * 12; i += GQ_ROW_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
  const float* R = g.Rg + row * 9;
  const gq3 r1 = gq_mk(R[0], R[1], R[2]), r2 = gq_mk(R[3], R[4], R[5]), r3 = gq_mk(R[6], R[7], R[8]);
  const float* tp = g.hand_pose + row * g.D;
  const gq3 t = gq_mk(tp[0], tp[1], tp[2]);
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
      const gq3 xw = gq_mk(gq_dot(r1, xh) + t.x, gq_dot(r2, xh) + t.y, gq_dot(r3, xh) + t.z);
      float phi = GQ_INF_F;
      gq3 gp = gq_mk(0, 0, 0);
      const int where = gq_scene_sample(grid, xw, phi, gp);
      if (where == GQ_SCENE_NONFINITE) phi = gp.x = gp.y = gp.z = __builtin_nanf("");  // the row's energy and gradient: NaN
      if (where != GQ_SCENE_OUTSIDE && !(phi >= g.margin)) {
        e += g.margin - phi;
        // g_h = R' (-grad phi), the upstream factor follows at the fold
        const gq3 gh = gq_mk(-fmaf(r1.x, gp.x, fmaf(r2.x, gp.y, r3.x * gp.z)), -fmaf(r1.y, gp.x, fmaf(r2.y, gp.y, r3.y * gp.z)),
                             -fmaf(r1.z, gp.x, fmaf(r2.z, gp.y, r3.z * gp.z)));
        const gq3 m = gq_cross(xh, gh);
        v[0] = gh.x, v[1] = gh.y, v[2] = gh.z, v[3] = m.x, v[4] = m.y, v[5] = m.z;
        K[0] = fmaf(gh.x, xh.x, K[0]), K[1] = fmaf(gh.x, xh.y, K[1]), K[2] = fmaf(gh.x, xh.z, K[2]);
        K[3] = fmaf(gh.y, xh.x, K[3]), K[4] = fmaf(gh.y, xh.y, K[4]), K[5] = fmaf(gh.y, xh.z, K[5]);
        K[6] = fmaf(gh.z, xh.x, K[6]), K[7] = fmaf(gh.z, xh.y, K[7]), K[8] = fmaf(gh.z, xh.z, K[8]);
      }
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
  const float up = g.up_scene ? g.up_scene[row] : g.w_scene;
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
  GQ_ROW_GRT(g.gRt, row, tot, s_K, lane, up, g.accumulate)
  if (lane == 0 && g.e_scene) g.e_scene[row] = gq_row_energy(s_e);
}
