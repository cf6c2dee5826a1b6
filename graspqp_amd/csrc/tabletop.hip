// Tabletop terms of the reference's energy (core/energy.py:68-78) for the MALA* stepper, as ONE launch of their own:
//
//   E_prior = 1 - (R grasp_axis) . (0,0,-1) = 1 + (R grasp_axis)_z          the grasp axis should point down
//   E_wall  = sum_s max(table_z - x_w(s).z, 0)                              hand surface samples below the table plane
//
// with x_h = T_link p (hand frame), x_w = R x_h + t.  The launch also emits the gradient in the form gq_fk_backward takes
// (include/graspqp_hip.h): link wrenches (f, m about the hand origin, hand frame), gRt = [gsum(3), K(9)] with
// grad_t = -R gsum and grad_R = R K, and a direct g_R for E_prior.  Every sample below the plane pulls with the SAME
// hand-frame force g_h = R' (0,0,-up) = -up r3 (r3 = third row of R), so per link only the count n_l and the sum
// S_l = sum x_h of its samples below the plane are reduced:
//
//   f_l = n_l g_h        m_l = S_l x g_h        gsum = -(sum_l n_l) g_h        K = g_h (x) (sum_l S_l)
//
// (K is the transpose of the penetration case, pen_dev.h: there the point rides on the object, here on the hand.)
//
// One block of eight wavefronts per row.  The link transforms of the row are staged in LDS while the samples are in flight;
// wavefront w takes the 64-sample chunks w, w+8, ...: lane = sample, and for every link met in the chunk the four masked
// values are summed over the wavefront by the DPP network and added to the accumulators that lane l keeps for link l.  The
// eight wavefronts' partial sums are then folded in wavefront order.  No atomics: the order of every sum depends only on
// the order of the samples, so results are bitwise reproducible run to run.  The samples may come in any order (the sums,
// and so the last bits, follow it); sorted by link a chunk meets two or three links instead of all of them.
#include "sample_row_dev.h"  // the row frame the four hand-surface terms share

struct GqTabletopArgs {
  const float* samples;        // (Ns,3) link frame
  const int32_t* sample_link;  // (Ns)
  const float* hand_pose;      // (B,D)
  const float* Rg;             // (B,9)
  const float* link_T;         // (B,L,12)
  const float* up_wall;        // (B) or null
  const float* up_prior;       // (B) or null
  int Ns, L, D;
  float ax, ay, az;  // grasp axis, hand frame
  float table_z, w_wall, w_prior;
  int accumulate;
  float* e_wall;   // (B) or null
  float* e_prior;  // (B) or null
  float* wrench;   // (B,L,6) or null
  float* gRt;      // (B,12) or null
  float* g_R;      // (B,9) or null
};

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_tabletop_kernel(const GqTabletopArgs g) {
  __shared__ float s_T[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_part[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS][4];  // per wavefront and link: S_l (3), n_l
  __shared__ int s_seen[GQ_ROW_WAVES][GQ_ROW_MAX_LINKS];       // the wavefront met a sample of the link (on either side)
  __shared__ float s_e[GQ_ROW_WAVES];
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const int L = g.L;
  for (int i = tid; i < L * 12; i += GQ_ROW_WAVES * GQ_WAVE) s_T[i] = g.link_T[row * L * 12 + i];
  const float* R = g.Rg + row * 9;
  const gq3 r3 = gq_mk(R[6], R[7], R[8]);  // x_w.z = r3 . x_h + t.z
  const float tz = g.hand_pose[row * g.D + 2];
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
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float e = 0.0f;
  int seen = 0;
  for (int c = wv; c < chunks; c += GQ_ROW_WAVES) {
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if ((unsigned)l < (unsigned)L) {
      const gq3 xh = gq_row_point(s_T + l * 12, p);
      const float z = gq_dot(r3, xh) + tz;
      if (!(z >= g.table_z)) {  // a NaN height counts as below: E_wall of the row is NaN, as in the reference
        v[0] = xh.x, v[1] = xh.y, v[2] = xh.z, v[3] = 1.0f;
        e += g.table_z - z;
      }
    } else {
      l = -1;  // a link id outside the hand (refused by ops.SurfaceSamples): the sample is ignored
    }
    GQ_ROW_LINK_SUMS(4, l, L, lane, v, acc, seen = 1)
    s += GQ_ROW_WAVES * GQ_WAVE;
    l = -1;
    if (c + GQ_ROW_WAVES < chunks && s < g.Ns) {
      l = g.sample_link[s];
      p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
    }
  }
  e = gq_dpp_sum(e);
  if (lane == 0) s_e[wv] = e;
  if (lane < L) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s_part[wv][lane][q] = acc[q];
    s_seen[wv][lane] = seen;
  }
  __syncthreads();
  if (wv != 0) return;
  // wavefront 0: lane l folds link l over the wavefronts, in wavefront order
  const float up_w = g.up_wall ? g.up_wall[row] : g.w_wall;
  const gq3 gh = (-up_w) * r3;  // d E_wall / d x_h of a sample below the plane, times the upstream factor
  float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (lane < L) {
    int present = 0;
    GQ_ROW_FOLD(4, s_part, s_seen, lane, tot, present)
    if (g.wrench && (present || !g.accumulate)) {  // links without samples: zero (overwrite) or left alone (accumulate)
      const gq3 f = tot[3] * gh;
      const gq3 m = gq_cross(gq_mk(tot[0], tot[1], tot[2]), gh);
      float* w6 = g.wrench + (row * L + lane) * 6;
      gq_row_store(w6 + 0, f.x, g.accumulate);
      gq_row_store(w6 + 1, f.y, g.accumulate);
      gq_row_store(w6 + 2, f.z, g.accumulate);
      gq_row_store(w6 + 3, m.x, g.accumulate);
      gq_row_store(w6 + 4, m.y, g.accumulate);
      gq_row_store(w6 + 5, m.z, g.accumulate);
    }
  }
  // row sums over the links (lanes >= L hold zeros)
  const float Sx = gq_dpp_sum(tot[0]), Sy = gq_dpp_sum(tot[1]), Sz = gq_dpp_sum(tot[2]), N = gq_dpp_sum(tot[3]);
  const float up_p = g.up_prior ? g.up_prior[row] : g.w_prior;
  if (g.gRt && lane < 12) {
    // lanes 0..2: gsum = -sum g_h; lanes 3..11: K = g_h (x) sum x_h, row-major (selects, not indexed arrays: no scratch)
    const int a = lane < 3 ? lane : (lane - 3) / 3, j = (lane - 3) % 3;
    const float gha = a == 0 ? gh.x : (a == 1 ? gh.y : gh.z);
    const float Sj = j == 0 ? Sx : (j == 1 ? Sy : Sz);
    gq_row_store(g.gRt + row * 12 + lane, lane < 3 ? -N * gha : gha * Sj, g.accumulate);
  }
  if (g.g_R && lane < 9) {  // E_prior = 1 + sum_j R[2][j] a_j
    const float aj = lane == 6 ? g.ax : (lane == 7 ? g.ay : g.az);
    gq_row_store(g.g_R + row * 9 + lane, lane >= 6 ? up_p * aj : 0.0f, g.accumulate);
  }
  if (lane == 0) {
    if (g.e_wall) g.e_wall[row] = gq_row_energy(s_e);
    if (g.e_prior) g.e_prior[row] = 1.0f + fmaf(r3.x, g.ax, fmaf(r3.y, g.ay, r3.z * g.az));
  }
}

// total[row] += w_prior E_prior[row] + w_wall E_wall[row]: the FK backward's row total holds the five terms of its own tail
__global__ __launch_bounds__(256) void gq_tabletop_total_kernel(float* __restrict__ total, const float* __restrict__ e_prior,
                                                                const float* __restrict__ e_wall, float w_prior, float w_wall,
                                                                int64_t B) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < B) total[row] += w_prior * e_prior[row] + w_wall * e_wall[row];
}

int gq_tabletop_check(int64_t batch, int n_links, int64_t n_samples) {
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "tabletop: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(n_links > 0 && n_links <= GQ_ROW_MAX_LINKS, "tabletop: n_links must be in 1..%d, got %d", GQ_ROW_MAX_LINKS, n_links);
  GQ_REQUIRE(n_samples > 0 && n_samples <= (1ll << 24), "tabletop: n_samples must be in 1..2^24, got %lld", (long long)n_samples);
  return GQ_OK;
}

int gq_tabletop_terms(const float* samples, const int32_t* sample_link, int64_t n_samples, int n_links, const float* hand_pose,
                      int pose_dim, const float* Rg, const float* link_T, int64_t batch, const float* grasp_axis, float table_z,
                      const float* up_wall, float w_wall, const float* up_prior, float w_prior, float* e_wall, float* e_prior,
                      int accumulate, float* link_wrench, float* gRt, float* g_R, void* stream) {
  const int rc = gq_tabletop_check(batch, n_links, n_samples);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && grasp_axis && pose_dim >= 9, "tabletop: bad arguments");
  GqTabletopArgs a{};
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.link_T = link_T;
  a.up_wall = up_wall, a.up_prior = up_prior;
  a.Ns = (int)n_samples, a.L = n_links, a.D = pose_dim;
  a.ax = grasp_axis[0], a.ay = grasp_axis[1], a.az = grasp_axis[2];
  a.table_z = table_z, a.w_wall = w_wall, a.w_prior = w_prior;
  a.accumulate = accumulate != 0;
  a.e_wall = e_wall, a.e_prior = e_prior, a.wrench = link_wrench, a.gRt = gRt, a.g_R = g_R;
  hipLaunchKernelGGL(gq_tabletop_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_tabletop_total(float* total, const float* e_prior, float w_prior, const float* e_wall, float w_wall, int64_t batch,
                      void* stream) {
  GQ_REQUIRE(total && e_prior && e_wall && batch > 0 && batch <= 0x7fffffffll, "tabletop_total: bad arguments");
  hipLaunchKernelGGL(gq_tabletop_total_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total,
                     e_prior, e_wall, w_prior, w_wall, batch);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
