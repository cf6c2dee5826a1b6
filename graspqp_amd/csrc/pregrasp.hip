// Pre-grasp clearance for the MALA* stepper: the hand travels its approach corridor OPEN and closes at the end, so the opened
// hand must be free of the grid at every station of the corridor, the grasp pose (d = 0) included -- as ONE launch that does the
// opened kinematics, the stations and the joint gradient of the row (include/graspqp_hip.h, "pre-grasp clearance"):
//
//   theta_o = (1 - alpha) theta + alpha q_o     x_h = T_l(theta_o) p     y_k = x_h - d_k a     x_w^k = R y_k + t
//   d_k = D k / K, k = 0..K                     E_pregrasp = 1/(K+1) sum_k sum_s max(margin - phi(x_w^k), 0)
//
// One block of eight wavefronts per row, shaped like gq_approach_row (approach_row_dev.h):
//   head      wavefront 0 forms theta_o and walks the tree level by level into LDS, lane = joint node, then lane = link: the walk
//             of gq_fk_forward_row (kin.hip) without contacts, spheres or the proposal.  The hand tables a lane needs are
//             requested before anything else.  Every wavefront has its first chunk of samples in flight meanwhile.  One barrier.
//   stations  lane = sample, x_h once per sample, the stations an inner loop of the lane (gq_pregrasp_stations, pregrasp_dev.h);
//             per-link DPP reductions once per chunk; per-wavefront partials to LDS.  One barrier.
//   tail      wavefront 0: links over the wavefronts in wavefront order; links -> nodes -> parents, deepest level first (lane j
//             holds the six components of node j); tau_j = a_j . (m_j - o_j x f_j) (revolute) or a_j . f_j (prismatic) with the
//             opened frames still in LDS; C' tau for a coupled hand; g_theta = (1 - alpha) up C' tau.
// The root pose of the opened hand is the closed hand's, so gRt is the layout gq_approach_terms emits and the FK backward of the
// closed hand takes it as it is; g_theta is that launch's direct joint gradient.  No second FK forward, no second FK backward.
//
// One kernel for a single grid and a stack: the row picks its grid by gq_stack_grid, a single grid is the stack of one.
// No atomics, every sum in a fixed order: bitwise reproducible run to run.
#include "approach_row_dev.h"  // gq_approach_check's station limit; the row frame (sample_row_dev.h)
#include "kin_dev.h"
#include "pregrasp_dev.h"

struct GqPregraspArgs {
  gqHand h;
  gqSceneGrid grid;  // grid 0 of the stack
  int rows_per_grid;
  const float* samples;        // (Ns,3) link frame
  const int32_t* sample_link;  // (Ns)
  const float* hand_pose;      // (B,D), D = 9 + JA
  const float* Rg;             // (B,9)
  const float* open_joints;    // (JA)
  const float* up_pregrasp;    // (B) or null
  int Ns, D, K;
  float margin, w_pregrasp, distance, opening;
  float ax, ay, az;  // approach axis, hand frame
  int accumulate;     // bit 0: add to gRt, bit 1: add to g_theta
  float* e_pregrasp;  // (B) or null
  float* g_theta;     // (B,JA) or null
  float* gRt;         // (B,12) or null
};

// row = blockIdx.x; `grid` is the grid this row reads
__device__ __forceinline__ void gq_pregrasp_row(const GqPregraspArgs& g, const gqSceneGrid& grid) {
  __shared__ float sW[64 * 12];   // node frames at the opened joints
  __shared__ float sT[64 * 12];   // link transforms at the opened joints
  __shared__ float sAw[64 * 3];   // joint axes in the hand frame
  __shared__ float sTh[64];       // coupled hands: the opened actuated joints (head), the tree torques (tail)
  __shared__ int sLN[64];         // link -> node
  __shared__ int sCh[64];         // child lists
  __shared__ float s_part[GQ_ROW_WAVES][64][6];  // per wavefront and link: sum g_h (3), sum x_h x g_h (3), up = 1
  __shared__ float s_K[GQ_ROW_WAVES][9];
  __shared__ float s_e[GQ_ROW_WAVES];
  __shared__ float sWr[64 * 6];   // link wrenches of the row
  __shared__ float sNF[64 * 6];   // node wrenches of the row
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const gqHand& h = g.h;
  const int L = h.L, J = h.J, JA = h.JA, nK = g.K;
  // ---- head ------------------------------------------------------------------------------------------------------------
  // wavefront 0: the constant hand tables of this lane (its joint node, its link, its child-list entry) and the row's joints
  int parent = -1, depth = -1, ntype = 0, lnode = -1, ch0 = 0, ch1 = 0, child = 0;
  GqT pre = gq_t_identity(), loff = gq_t_identity();
  gq3 axj = gq_mk(0, 0, 0);
  float th = 0.0f, qo = 0.0f, c0 = 0.0f;
  const float* hp = g.hand_pose + row * g.D;
  if (wv == 0) {
    if (lane < J) {
      parent = h.node_parent[lane];
      depth = h.node_depth[lane];
      ntype = h.node_type[lane];
      ch0 = h.child_off[lane];
      ch1 = h.child_off[lane + 1];
      pre = gq_t_load(h.node_pre + lane * 12);
      axj = gq_mk(h.node_axis[lane * 3], h.node_axis[lane * 3 + 1], h.node_axis[lane * 3 + 2]);
      if (h.coup) c0 = h.coup0[lane];
    }
    if (lane < h.child_off[J]) child = h.child_idx[lane];  // J - (number of roots) entries; first needed after the walk
    if (lane < L) {
      lnode = h.link_node[lane];
      loff = gq_t_load(h.link_offset + lane * 12);
    }
    if (lane < JA) {
      th = hp[9 + lane];
      qo = g.open_joints[lane];
    }
  }
  const float* R = g.Rg + row * 9;
  const gq3 r1 = gq_mk(R[0], R[1], R[2]), r2 = gq_mk(R[3], R[4], R[5]), r3 = gq_mk(R[6], R[7], R[8]);
  const gq3 t = gq_mk(hp[0], hp[1], hp[2]);
  const gq3 a = gq_mk(g.ax, g.ay, g.az);
  // the first chunk's samples do not depend on the kinematics: in flight while wavefront 0 walks the tree
  const int chunks = (g.Ns + GQ_WAVE - 1) / GQ_WAVE;
  int s = wv * GQ_WAVE + lane;
  int l = -1;
  gq3 p = gq_mk(0, 0, 0);
  if (wv < chunks && s < g.Ns) {
    l = g.sample_link[s];
    p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
  }
  if (wv == 0) {
    if (lane < L) sLN[lane] = lnode;
    float q = gq_pregrasp_open(th, qo, g.opening);  // lanes < JA
    if (h.coup) {  // coupled hand: theta_tree = C theta_o + c0, as gq_fk_forward
      sTh[lane] = q;
      gq_wave_sync();
      q = c0;
      if (lane < J)
        for (int k = 0; k < JA; ++k) q = fmaf(h.coup[lane * JA + k], sTh[k], q);
    }
    GqT A = gq_t_identity();
    if (lane < J) {
      A = gq_t_mul(pre, gq_joint_motion(ntype, axj, q));
      if (parent < 0) gq_t_store(sW + lane * 12, A);
    }
    gq_wave_sync();
    for (int d = 1; d <= h.max_depth; ++d) {  // level by level down the tree
      if (depth == d) {
        A = gq_t_mul(gq_t_load(sW + parent * 12), A);
        gq_t_store(sW + lane * 12, A);
      }
      gq_wave_sync();
    }
    if (lane < J) {
      const gq3 aw = gq_t_rot(A, axj);
      sAw[lane * 3] = aw.x, sAw[lane * 3 + 1] = aw.y, sAw[lane * 3 + 2] = aw.z;
    }
    if (lane < L) {
      GqT T = loff;
      if (lnode >= 0) T = gq_t_mul(gq_t_load(sW + lnode * 12), T);
      gq_t_store(sT + lane * 12, T);
    }
    sCh[lane] = child;
  }
  __syncthreads();
  // ---- stations: gq_approach_row's loop on the opened transforms ------------------------------------------------------------
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float K[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float e = 0.0f;
  for (int c = wv; c < chunks; c += GQ_ROW_WAVES) {
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if ((unsigned)l < (unsigned)L) {
      const gq3 xh = gq_pregrasp_point(sT + l * 12, p);
      gq3 G = gq_mk(0, 0, 0);  // sum of g_h over the stations of this sample
      gq_pregrasp_stations(grid, xh, a, r1, r2, r3, t, g.distance, nK, g.margin, e, G, K);
      const gq3 m = gq_pregrasp_moment(xh, G);
      v[0] = G.x, v[1] = G.y, v[2] = G.z, v[3] = m.x, v[4] = m.y, v[5] = m.z;
    } else {
      l = -1;  // a link id outside the hand (refused by ops.SurfaceSamples): the sample is ignored
    }
    GQ_ROW_LINK_SUMS(6, l, L, lane, v, acc, )
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
  }
  __syncthreads();
  if (wv != 0) return;
  // ---- tail, wavefront 0 ----------------------------------------------------------------------------------------------------
  // 1. lane l folds link l over the wavefronts, in wavefront order
  const float invK = 1.0f / (float)(nK + 1);
  const float up = (g.up_pregrasp ? g.up_pregrasp[row] : g.w_pregrasp) * invK;
  float tot[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (lane < L) {
    GQ_ROW_FOLD_SUMS(6, s_part, lane, tot)
#pragma unroll
    for (int q = 0; q < 6; ++q) sWr[lane * 6 + q] = tot[q];
  }
  GQ_ROW_GRT(g.gRt, row, tot, s_K, lane, up, g.accumulate & 1)
  if (lane == 0 && g.e_pregrasp)  // the energy is a value, not a gradient: always overwritten
    g.e_pregrasp[row] = gq_row_energy(s_e) * invK;
  if (!g.g_theta) return;
  // 2. links -> nodes, then children into parents, deepest level first: lane j holds the six components of node j
  gq_wave_sync();
  float nf[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (lane < J) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      nf[k] = gq_pregrasp_fold_links(lane, k, sLN, L, sWr);
      sNF[lane * 6 + k] = nf[k];
    }
  }
  gq_wave_sync();
  for (int d = h.max_depth - 1; d >= 0; --d) {
    if (depth == d) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        nf[k] = gq_pregrasp_fold_children(nf[k], k, sCh, ch0, ch1, sNF);
        sNF[lane * 6 + k] = nf[k];
      }
    }
    gq_wave_sync();
  }
  // 3. the joint torques at the opened frames, C' for a coupled hand
  float tau = 0.0f;
  if (lane < J)
    tau = gq_pregrasp_torque(ntype, gq_mk(sAw[lane * 3], sAw[lane * 3 + 1], sAw[lane * 3 + 2]),
                             gq_mk(sW[lane * 12 + 3], sW[lane * 12 + 7], sW[lane * 12 + 11]), gq_mk(nf[0], nf[1], nf[2]),
                             gq_mk(nf[3], nf[4], nf[5]));
  if (h.coup) {
    sTh[lane] = tau;
    gq_wave_sync();
    tau = 0.0f;
    if (lane < JA)
      for (int j = 0; j < J; ++j) tau = fmaf(h.coup[j * JA + lane], sTh[j], tau);
  }
  // 4. d theta_o / d theta = 1 - alpha
  if (lane < JA) gq_row_store(g.g_theta + row * JA + lane, (1.0f - g.opening) * (up * tau), g.accumulate & 2);
}

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_pregrasp_kernel(const GqPregraspArgs g) {
  const gqSceneGrid grid = gq_stack_grid(g.grid, blockIdx.x / (unsigned)g.rows_per_grid);
  gq_pregrasp_row(g, grid);
}

int gq_pregrasp_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_links, int64_t n_samples,
                      float distance, int n_stations, const float* grasp_axis, float opening) {
  GQ_REQUIRE(rows_per_grid >= 1 && rows_per_grid <= 0x7fffffffll, "pregrasp: rows_per_grid must be in 1..2^31-1, got %lld",
             (long long)rows_per_grid);
  if (gq_clutter_check(grids, batch, (int)rows_per_grid, n_links, n_samples) != GQ_OK) return gq_retell("pregrasp", "grids");
  GQ_REQUIRE(n_stations >= 0 && n_stations <= GQ_AP_MAX_STATIONS, "pregrasp: n_stations must be in 0..%d, got %d", GQ_AP_MAX_STATIONS,
             n_stations);
  const gqSceneGrid first = gq_stack_grid(grids);
  // the corridor: gq_approach_check's rules, but d = 0 is a station here, so n_stations = 0 is the one station d = 0
  if (gq_approach_check(&first, batch, n_links, n_samples, distance, n_stations < 1 ? 1 : n_stations, grasp_axis) != GQ_OK)
    return gq_retell("pregrasp", "corridor");
  GQ_REQUIRE(opening >= 0.0f && opening <= 1.0f, "pregrasp: opening must be in [0, 1], got %g", (double)opening);
  return GQ_OK;
}

int gq_pregrasp_terms(const gqHand* h, const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float distance,
                      int n_stations, float opening, const float* open_joints, const float* samples, const int32_t* sample_link,
                      int64_t n_samples, const float* hand_pose, int pose_dim, const float* Rg, int64_t batch,
                      const float* grasp_axis, const float* up_pregrasp, float w_pregrasp, float* e_pregrasp, int accumulate,
                      float* g_theta, float* gRt, void* stream) {
  GQ_REQUIRE(h, "pregrasp: hand is NULL");
  GQ_REQUIRE(h->J >= 1 && h->J <= 64 && h->L >= 1 && h->L <= 64 && h->JA >= 1 && h->JA <= 64,
             "pregrasp: the hand must have at most 64 joints and 64 links, got J=%d L=%d JA=%d", h->J, h->L, h->JA);
  const int rc = gq_pregrasp_check(grids, batch, rows_per_grid, h->L, n_samples, distance, n_stations, grasp_axis, opening);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && open_joints, "pregrasp: bad arguments");
  GQ_REQUIRE(pose_dim == 9 + h->JA, "pregrasp: pose_dim must be 9 + the hand's actuated joints = %d, got %d", 9 + h->JA, pose_dim);
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "pregrasp: margin must be finite and >= 0, got %g", (double)margin);
  GqPregraspArgs a{};
  a.h = *h;
  a.grid = gq_stack_grid(grids);
  a.rows_per_grid = (int)rows_per_grid;
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.open_joints = open_joints;
  a.up_pregrasp = up_pregrasp;
  a.Ns = (int)n_samples, a.D = pose_dim, a.K = n_stations;
  a.margin = margin, a.w_pregrasp = w_pregrasp, a.distance = distance, a.opening = opening;
  a.ax = grasp_axis[0], a.ay = grasp_axis[1], a.az = grasp_axis[2];
  a.accumulate = accumulate & 3;  // bit 0: gRt, bit 1: g_theta
  a.e_pregrasp = e_pregrasp, a.g_theta = g_theta, a.gRt = gRt;
  hipLaunchKernelGGL(gq_pregrasp_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
