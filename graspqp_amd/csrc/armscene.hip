// E_arm: where does the arm configuration of the reach term put the arm?  The arm's collision spheres on the scene grid, at the
// winner's joints of every station, as ONE launch after gq_reach_terms and before gq_fk_backward (include/graspqp_hip.h, "arm
// clearance", has the term and its gradient).
//
// One block per row, one wavefront per station (K + 1 <= 4), lane = collision sphere (Ns <= 64):
//
//   head     lanes 0..7 form the joint transforms pre_j m_j(q_j) of the station's joints (reach_q, an input) and hand them over in
//            LDS; lane j multiplies base X_0 ... X_j left to right and leaves the link frame W_j in LDS.  The spheres of the lanes
//            are in flight meanwhile.
//   spheres  x_s = W_l c_s, the hinge on the row's grid by gq_scene_sample, and the lane's eight scalars [l_s >= j] f_s . col_j(x_s);
//            eight wave sums (a fixed tree, the same bits on every lane) give g_q = dE_k/dq.  The hinges go to LDS.
//   solve    lanes 0..7 form the columns of J = [J_v ; rho J_w] at the hand root, zero for a joint on a limit; every lane forms
//            J g_q and J J' in fp64, joints ascending, and solves the damped 6 x 6 system by an unrolled Cholesky in fp64.  Lane 0
//            adds the hinges, spheres ascending.
//   tail     one barrier; thread 0 folds the stations in ascending order into the mean and into gRt, in the layout and signs of
//            gq_reach_terms.
// No atomics, no block waits for another, every sum in a fixed order, no array indexed at run time in registers: bitwise
// reproducible, graph-capturable, no scratch.
#include "armscene_dev.h"
#include "wave.h"

struct GqArmSceneArgs {
  gqArm arm;
  gqSceneGrid grid;  // grid 0 of the stack
  int rows_per_grid;
  const int32_t* sphere_link;  // (Ns)
  const float* sphere_centre;  // (Ns,3) link frame
  const float* sphere_radius;  // (Ns)
  const float *Rg, *base_T, *reach_q, *up;
  int64_t batch_each;
  gq3 axis;
  float margin, lambda, rho, D, w;
  int Ns, K, accumulate;
  float *e, *gRt;
};

#define GQ_ARM_WAVES (GQ_REACH_MAX_STATIONS + 1)

__global__ __launch_bounds__(GQ_ARM_WAVES* GQ_WAVE) void gq_arm_kernel(const GqArmSceneArgs g) {
  __shared__ float sX[GQ_ARM_WAVES][GQ_REACH_MAX_JOINTS * 12];  // joint transforms
  __shared__ float sW[GQ_ARM_WAVES][GQ_REACH_MAX_JOINTS * 12];  // link frames
  __shared__ float sC[GQ_ARM_WAVES][GQ_REACH_MAX_JOINTS * 6];   // columns of J
  __shared__ float sH[GQ_ARM_WAVES][GQ_ARM_MAX_SPHERES];        // hinges
  __shared__ float sY[GQ_ARM_WAVES][8];                         // per station: y / 2 (6), E_k
  const int lane = gq_lane(), k = threadIdx.x / GQ_WAVE;        // the block has K + 1 wavefronts
  const size_t row = blockIdx.x;
  const int N = g.arm.N, K = g.K;
  const gqSceneGrid grid = gq_stack_grid(g.grid, row / (size_t)g.rows_per_grid);

  // the lane's sphere: independent of the kinematics, requested first
  int l = -1;
  gq3 ctr = gq_mk(0.0f, 0.0f, 0.0f);
  float rad = 0.0f;
  if (lane < g.Ns) {
    l = g.sphere_link[lane];
    ctr = gq_mk(g.sphere_centre[lane * 3], g.sphere_centre[lane * 3 + 1], g.sphere_centre[lane * 3 + 2]);
    rad = g.sphere_radius[lane];
  }
  // ---- head: the link frames of the station ------------------------------------------------------------------------------------
  GqRT base, tool;
  const float* bt = g.base_T + (size_t)((int64_t)row / g.batch_each) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) base.m[i] = bt[i], tool.m[i] = g.arm.tool[i];
  int type = 0;
  gq3 ax = gq_mk(0.0f, 0.0f, 0.0f);
  float q = 0.0f, lo = 0.0f, hi = 0.0f;
  if (lane < GQ_REACH_MAX_JOINTS) {
    GqRT pre;
#pragma unroll
    for (int i = 0; i < 12; ++i) pre.m[i] = g.arm.pre[lane * 12 + i];
    type = g.arm.type[lane];
    ax = gq_mk(g.arm.axis[lane * 3], g.arm.axis[lane * 3 + 1], g.arm.axis[lane * 3 + 2]);
    lo = g.arm.lower[lane], hi = g.arm.upper[lane];
    if (lane < N) q = g.reach_q[(row * (size_t)(K + 1) + k) * N + lane];
    const GqRT X = gq_reach_joint(pre, type, ax, q);
#pragma unroll
    for (int i = 0; i < 12; ++i) sX[k][lane * 12 + i] = X.m[i];
  }
  gq_wave_sync();
  GqRT W = base;
  if (lane < GQ_REACH_MAX_JOINTS) {
    W = gq_arm_chain(base, sX[k], lane);
#pragma unroll
    for (int i = 0; i < 12; ++i) sW[k][lane * 12 + i] = W.m[i];
  }
  gq_wave_sync();
  // ---- spheres -----------------------------------------------------------------------------------------------------------------
  float h = 0.0f;
  float gq[GQ_REACH_MAX_JOINTS] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if ((unsigned)l < (unsigned)N) {  // a link outside the arm (refused by ops.ArmSpec) is ignored
    const gq3 x = gq_arm_point(sW[k] + l * 12, ctr);
    gq3 f;
    h = gq_arm_hinge(grid, x, g.margin, rad, f);
    if (g.gRt) gq_arm_joint_terms(l, x, f, sW[k], g.arm.type, g.arm.axis, gq);
  }
  sH[k][lane] = h;
  float half_y[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (g.gRt) {
    gq_wave_sums_f<GQ_REACH_MAX_JOINTS>(gq);
    // ---- solve: y = (J J' + lambda I)^-1 J g_q ---------------------------------------------------------------------------------
    if (lane < GQ_REACH_MAX_JOINTS) {
      GqRT W7;
#pragma unroll
      for (int i = 0; i < 12; ++i) W7.m[i] = sW[k][(GQ_REACH_MAX_JOINTS - 1) * 12 + i];
      const GqRT T = gq_reach_mul(W7, tool);  // the padding joints are identities: frame 7 is the last joint's
      float c[6];
      gq_arm_col(type, W, ax, gq_mk(T.m[3], T.m[7], T.m[11]), g.rho, q, lo, hi, c);
#pragma unroll
      for (int i = 0; i < 6; ++i) sC[k][lane * 6 + i] = c[i];
    }
    gq_wave_sync();
    double A[21], b[6], y[6];
    gq_arm_normal(sC[k], gq, A, b);
    gq_arm_solve6(A, (double)g.lambda, b, y);
#pragma unroll
    for (int i = 0; i < 6; ++i) half_y[i] = 0.5f * (float)y[i];  // gq_reach_grad_add doubles its operand
  } else {
    gq_wave_sync();
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) sY[k][i] = half_y[i];
    sY[k][6] = gq_arm_station_sum(sH[k], g.Ns);
  }
  __syncthreads();
  // ---- tail: the stations in ascending order -----------------------------------------------------------------------------------
  if (threadIdx.x != 0) return;
  const float inv = 1.0f / (float)(K + 1);
  float esum = 0.0f;
  for (int kk = 0; kk <= K; ++kk) esum += sY[kk][6];
  if (g.e) g.e[row] = esum * inv;
  if (!g.gRt) return;
  float R[9], gRt[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, tau_h[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = g.Rg[row * 9 + i];
  const float cu = (g.up ? g.up[row] * g.w : g.w) * inv;
  for (int kk = 0; kk <= K; ++kk) gq_reach_grad_add(R, sY[kk], cu, g.rho, gq_reach_station(g.D, kk, K), g.axis, gRt, tau_h);
  gq_reach_grad_close(tau_h, gRt);
  float* o = g.gRt + row * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) o[i] = g.accumulate ? o[i] + gRt[i] : gRt[i];
}

static bool gq_arm_finite(float v) { return v > -GQ_INF_F && v < GQ_INF_F; }

extern "C" {

int gq_arm_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_joints, int n_spheres, float margin,
                 float damping, float rot_scale, float distance, int n_stations, const float* grasp_axis) {
  GQ_REQUIRE(rows_per_grid >= 1 && rows_per_grid <= 0x7fffffffll, "arm: rows_per_grid must be in 1..2^31-1, got %lld",
             (long long)rows_per_grid);
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "arm: batch must be in 1..2^31-1, got %lld", (long long)batch);
  // grids == NULL: the parameters alone, before a scene exists (gq_arm_terms refuses a NULL stack itself)
  if (grids && gq_clutter_check(grids, batch, (int)rows_per_grid, 1, 1) != GQ_OK) return gq_retell("arm", "grids");
  GQ_REQUIRE(n_joints >= 1 && n_joints <= GQ_REACH_MAX_JOINTS, "arm: n_joints must be in 1..%d, got %d", GQ_REACH_MAX_JOINTS, n_joints);
  GQ_REQUIRE(n_spheres >= 1 && n_spheres <= GQ_ARM_MAX_SPHERES, "arm: n_spheres must be in 1..%d, got %d", GQ_ARM_MAX_SPHERES,
             n_spheres);
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "arm: margin must be finite and >= 0, got %g", (double)margin);
  GQ_REQUIRE(damping > 0.0f && damping < GQ_INF_F, "arm: damping must be finite and > 0, got %g", (double)damping);
  GQ_REQUIRE(rot_scale > 0.0f && rot_scale < GQ_INF_F, "arm: rot_scale must be finite and > 0, got %g", (double)rot_scale);
  GQ_REQUIRE(n_stations >= 0 && n_stations <= GQ_REACH_MAX_STATIONS, "arm: n_stations must be in 0..%d, got %d", GQ_REACH_MAX_STATIONS,
             n_stations);
  GQ_REQUIRE(n_stations == 0 || (distance > 0.0f && distance < GQ_INF_F), "arm: distance must be finite and > 0, got %g",
             (double)distance);
  GQ_REQUIRE(grasp_axis, "arm: grasp_axis is NULL");
  for (int i = 0; i < 3; ++i) GQ_REQUIRE(gq_arm_finite(grasp_axis[i]), "arm: grasp_axis[%d] must be finite", i);
  GQ_REQUIRE(grasp_axis[0] != 0.0f || grasp_axis[1] != 0.0f || grasp_axis[2] != 0.0f, "arm: grasp_axis must not be all zero");
  return GQ_OK;
}

int gq_arm_terms(const gqArm* arm, const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float damping, float rot_scale,
                 const int32_t* sphere_link, const float* sphere_centre, const float* sphere_radius, int n_spheres,
                 const float* hand_pose, int pose_dim, const float* Rg, int64_t batch, const float* base_T, int64_t n_obj,
                 int64_t batch_each, const float* grasp_axis, float distance, int n_stations, const float* reach_q, const float* up,
                 float w, float* e_arm, int accumulate, float* gRt, void* stream) {
  GQ_REQUIRE(arm, "arm: arm is NULL");
  GQ_REQUIRE(grids, "arm: grids is NULL");
  const int rc = gq_arm_check(grids, batch, rows_per_grid, arm->N, n_spheres, margin, damping, rot_scale, distance, n_stations, grasp_axis);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(sphere_link && sphere_centre && sphere_radius, "arm: the sphere arrays must not be NULL");
  GQ_REQUIRE(hand_pose && Rg && base_T && pose_dim >= 9, "arm: bad arguments");
  GQ_REQUIRE(reach_q, "arm: reach_q is NULL");
  GQ_REQUIRE(n_obj >= 1 && batch_each >= 1 && n_obj * batch_each == batch,
             "arm: base_T has %lld transforms for %lld rows each, the batch is %lld", (long long)n_obj, (long long)batch_each,
             (long long)batch);
  GqArmSceneArgs a{};
  a.arm = *arm;
  a.grid = gq_stack_grid(grids);
  a.rows_per_grid = (int)rows_per_grid;
  a.sphere_link = sphere_link, a.sphere_centre = sphere_centre, a.sphere_radius = sphere_radius;
  a.Rg = Rg, a.base_T = base_T, a.reach_q = reach_q, a.up = up;
  a.batch_each = batch_each;
  a.axis = gq3{grasp_axis[0], grasp_axis[1], grasp_axis[2]};
  a.margin = margin, a.lambda = damping, a.rho = rot_scale, a.D = n_stations > 0 ? distance : 0.0f, a.w = w;
  a.Ns = n_spheres, a.K = n_stations, a.accumulate = accumulate != 0;
  a.e = e_arm, a.gRt = gRt;
  hipLaunchKernelGGL(gq_arm_kernel, dim3((unsigned)batch), dim3((n_stations + 1) * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
