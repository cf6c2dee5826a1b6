// Scene obstacles for the MALA* stepper: the hand's surface samples must stay outside a signed-distance grid of the
// surroundings (an ESDF / TSDF volume, positive outside the obstacles), as ONE launch of its own:
//
//   E_scene = sum_s max(margin - phi(x_w(s)), 0)          x_h = T_link p (hand frame), x_w = R x_h + t
//
// with phi the trilinear interpolant of the grid (scene_dev.h); a sample outside the volume is in free space.  The launch
// also emits the gradient in the form gq_fk_backward takes (include/graspqp_hip.h): link wrenches (f, m about the hand
// origin, hand frame) and gRt = [gsum(3), K(9)] with grad_t = -R gsum and grad_R = R K.  A sample with phi < margin pulls
// with g_w = -up grad phi(x_w), g_h = R' g_w.  Unlike the table plane (tabletop.hip) every sample has its own force, so
// per link six numbers are reduced, and nine more for K:
//
//   f_l = sum g_h        m_l = sum x_h x g_h        gsum = -sum_l f_l        K = sum g_h (x) x_h
//
// One block of eight wavefronts per row, as gq_tabletop_kernel: the link transforms of the row are staged in LDS while the
// first samples are in flight; wavefront w takes the 64-sample chunks w, w+8, ...: lane = sample.  Per sample the
// transform, the cell, the 8 node loads (issued together), then value and gradient.  For every link met in the chunk the
// six masked values are summed over the wavefront by the DPP network and added to the accumulators that lane l keeps for
// link l; K stays in nine per-lane accumulators over the lane's chunks and is folded once at the end.  The upstream factor
// multiplies the finished sums.  The eight wavefronts' partial sums are folded in wavefront order, link l by lane l of
// wavefront 0.  No atomics: the order of every sum depends only on the order of the samples, so results are bitwise
// reproducible run to run.
#include "scene_dev.h"

#define GQ_SC_MAX_LINKS 64  // lane l of a wavefront owns link l
#define GQ_SC_WAVES 8       // 512 default samples: one 64-sample chunk per wavefront

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

// accumulate: a plain rounded add of the finished value (no contraction with the product that made it), so that adding to
// a buffer gives the bits of buffer + (the overwriting launch's value)
__device__ __forceinline__ void gq_sc_store(float* p, float v, int accumulate) {
#pragma clang fp contract(off)
  *p = accumulate ? *p + v : v;
}

__global__ __launch_bounds__(GQ_SC_WAVES * GQ_WAVE) void gq_scene_kernel(const GqSceneArgs g) {
  __shared__ float s_T[GQ_SC_MAX_LINKS * 12];
  __shared__ float s_part[GQ_SC_WAVES][GQ_SC_MAX_LINKS][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ int s_seen[GQ_SC_WAVES][GQ_SC_MAX_LINKS];       // the wavefront met a sample of the link (active or not)
  __shared__ float s_K[GQ_SC_WAVES][9];
  __shared__ float s_e[GQ_SC_WAVES];
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L;
  for (int i = tid; i < L * 12; i += GQ_SC_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
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
  for (int c = wv; c < chunks; c += GQ_SC_WAVES) {
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if ((unsigned)l < (unsigned)L) {
      const float* T = s_T + l * 12;
      const gq3 xh = gq_mk(fmaf(T[0], p.x, fmaf(T[1], p.y, fmaf(T[2], p.z, T[3]))),
                           fmaf(T[4], p.x, fmaf(T[5], p.y, fmaf(T[6], p.z, T[7]))),
                           fmaf(T[8], p.x, fmaf(T[9], p.y, fmaf(T[10], p.z, T[11]))));
      const gq3 xw = gq_mk(gq_dot(r1, xh) + t.x, gq_dot(r2, xh) + t.y, gq_dot(r3, xh) + t.z);
      float phi = GQ_INF_F;
      gq3 gp = gq_mk(0, 0, 0);
      const int where = gq_scene_sample(g.grid, xw, phi, gp);
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
    s += GQ_SC_WAVES * GQ_WAVE;
    l = -1;
    if (c + GQ_SC_WAVES < chunks && s < g.Ns) {
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
  const float up = g.up_scene ? g.up_scene[row] : g.w_scene;
  float tot[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (lane < L) {
    int present = 0;
    for (int w = 0; w < GQ_SC_WAVES; ++w) {
#pragma unroll
      for (int q = 0; q < 6; ++q) tot[q] += s_part[w][lane][q];
      present |= s_seen[w][lane];
    }
    if (g.wrench && (present || !g.accumulate)) {  // links without samples: zero (overwrite) or left alone (accumulate)
      float* w6 = g.wrench + (row * L + lane) * 6;
#pragma unroll
      for (int q = 0; q < 6; ++q) gq_sc_store(w6 + q, up * tot[q], g.accumulate);
    }
  }
  // row sums over the links (lanes >= L hold zeros)
  const float Fx = gq_dpp_sum(tot[0]), Fy = gq_dpp_sum(tot[1]), Fz = gq_dpp_sum(tot[2]);
  if (g.gRt && lane < 12) {
    // lanes 0..2: gsum = -sum g_h; lanes 3..11: K, row-major, folded over the wavefronts in wavefront order
    float val = lane == 0 ? -Fx : (lane == 1 ? -Fy : -Fz);
    if (lane >= 3) {
      val = 0.0f;
      for (int w = 0; w < GQ_SC_WAVES; ++w) val += s_K[w][lane - 3];
    }
    gq_sc_store(g.gRt + row * 12 + lane, up * val, g.accumulate);
  }
  if (lane == 0 && g.e_scene)
    g.e_scene[row] = ((s_e[0] + s_e[1]) + (s_e[2] + s_e[3])) + ((s_e[4] + s_e[5]) + (s_e[6] + s_e[7]));
}

// one query per lane: the differentiable building block for arbitrary world points
__global__ __launch_bounds__(256) void gq_scene_query_kernel(const gqSceneGrid grid, const float* __restrict__ points, int64_t N,
                                                             float* __restrict__ phi, float* __restrict__ grad,
                                                             uint8_t* __restrict__ inside) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const gq3 x = gq_mk(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]);
  float f = GQ_INF_F;  // outside the volume: free space
  gq3 gp = gq_mk(0, 0, 0);
  const int where = gq_scene_sample(grid, x, f, gp);
  if (where == GQ_SCENE_NONFINITE) f = gp.x = gp.y = gp.z = __builtin_nanf("");
  phi[i] = f;
  if (grad) grad[i * 3] = gp.x, grad[i * 3 + 1] = gp.y, grad[i * 3 + 2] = gp.z;
  if (inside) inside[i] = where == GQ_SCENE_INSIDE;
}

// total[row] += w_scene E_scene[row]: the FK backward's row total holds the five terms of its own tail
__global__ __launch_bounds__(256) void gq_scene_total_kernel(float* __restrict__ total, const float* __restrict__ e_scene,
                                                             float w_scene, int64_t B) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < B) total[row] += w_scene * e_scene[row];
}

static int gq_scene_check_grid(const gqSceneGrid* grid) {
  GQ_REQUIRE(grid, "scene: grid is NULL");
  GQ_REQUIRE(grid->values, "scene: grid values is NULL");
  GQ_REQUIRE(grid->nx >= 2, "scene: grid nx must be >= 2, got %d", grid->nx);
  GQ_REQUIRE(grid->ny >= 2, "scene: grid ny must be >= 2, got %d", grid->ny);
  GQ_REQUIRE(grid->nz >= 2, "scene: grid nz must be >= 2, got %d", grid->nz);
  GQ_REQUIRE((long long)grid->nx * grid->ny <= (1ll << 28) && (long long)grid->nx * grid->ny * grid->nz <= (1ll << 28),
             "scene: grid nx*ny*nz must be <= 2^28 nodes, got %d x %d x %d", grid->nx, grid->ny, grid->nz);
  GQ_REQUIRE(grid->voxel > 0.0f && grid->voxel < GQ_INF_F, "scene: grid voxel must be finite and > 0, got %g", (double)grid->voxel);
  for (int a = 0; a < 3; ++a)
    GQ_REQUIRE(grid->origin[a] > -GQ_INF_F && grid->origin[a] < GQ_INF_F, "scene: grid origin[%d] must be finite, got %g", a,
               (double)grid->origin[a]);
  return GQ_OK;
}

int gq_scene_check(const gqSceneGrid* grid, int64_t batch, int n_links, int64_t n_samples) {
  const int rc = gq_scene_check_grid(grid);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "scene: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(n_links > 0 && n_links <= GQ_SC_MAX_LINKS, "scene: n_links must be in 1..%d, got %d", GQ_SC_MAX_LINKS, n_links);
  GQ_REQUIRE(n_samples > 0 && n_samples <= (1ll << 24), "scene: n_samples must be in 1..2^24, got %lld", (long long)n_samples);
  return GQ_OK;
}

int gq_scene_terms(const gqSceneGrid* grid, float margin, const float* samples, const int32_t* sample_link, int64_t n_samples,
                   int n_links, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, int64_t batch,
                   const float* up_scene, float w_scene, float* e_scene, int accumulate, float* link_wrench, float* gRt,
                   void* stream) {
  const int rc = gq_scene_check(grid, batch, n_links, n_samples);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "scene: bad arguments");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "scene: margin must be finite and >= 0, got %g", (double)margin);
  GqSceneArgs a{};
  a.grid = *grid;
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.link_T = link_T;
  a.up_scene = up_scene;
  a.Ns = (int)n_samples, a.L = n_links, a.D = pose_dim;
  a.margin = margin, a.w_scene = w_scene;
  a.accumulate = accumulate != 0;
  a.e_scene = e_scene, a.wrench = link_wrench, a.gRt = gRt;
  hipLaunchKernelGGL(gq_scene_kernel, dim3((unsigned)batch), dim3(GQ_SC_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_scene_query(const gqSceneGrid* grid, const float* points, int64_t n_points, float* phi, float* grad, uint8_t* inside,
                   void* stream) {
  const int rc = gq_scene_check_grid(grid);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(n_points >= 0 && n_points <= (1ll << 31) * 255, "scene: n_points must be in 0..255*2^31, got %lld", (long long)n_points);
  if (n_points == 0) return GQ_OK;
  GQ_REQUIRE(points && phi, "scene: points / phi is NULL");
  hipLaunchKernelGGL(gq_scene_query_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *grid,
                     points, n_points, phi, grad, inside);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_scene_total(float* total, const float* e_scene, float w_scene, int64_t batch, void* stream) {
  GQ_REQUIRE(total && e_scene && batch > 0 && batch <= 0x7fffffffll, "scene_total: bad arguments");
  hipLaunchKernelGGL(gq_scene_total_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total,
                     e_scene, w_scene, batch);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
