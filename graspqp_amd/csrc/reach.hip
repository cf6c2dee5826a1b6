// E_reach: can the arm bring the hand to this pose, and to the stations of its retreat?  Batched damped-least-squares wrist IK as ONE
// launch (include/graspqp_hip.h, "arm reachability", has the iteration and the formulas).
//
// A row has (K + 1) stations x S seeds independent IK problems.  Eight lanes make a problem: lane j of the group is joint j of the
// arm, so a wavefront runs eight problems and the block of a row, up to four wavefronts, runs them all side by side.  Per update:
//
//   1. lane j forms its joint transform; an inclusive scan over the group (three DPP row shifts of twelve values, a product each)
//      leaves base -> joint j in lane j; the last lane's is handed to the group and gives the hand-root pose on every lane
//   2. the six error entries (log map) on every lane; lane j's column of J = [J_v ; rho J_w]
//   3. the 21 entries of the lower triangle of J J' summed over the group (quad_perm xor 1, xor 2, row_half_mirror: every stage
//      adds a pair symmetrically, so the eight lanes hold the same bits)
//   4. the 6 x 6 Cholesky and both substitutions unrolled in registers, on every lane of the group; dq_j = c_j . y, the group's
//      largest |dq| for the step cap, the clamp to the joint's limits
//
// After M updates one more FK gives e and E = |e|^2.  The problems leave E, e and q in LDS; one thread picks the winner of every
// station (lowest seed on a tie), forms the mean and the gradient in the gRt layout; the winners' joints are written side by side.
// No atomics, no block waits for another, every sum in a fixed order, no array indexed at run time: bitwise reproducible,
// graph-capturable, no scratch.  Joint state is never carried from one launch to the next: the term is a pure function of the pose.
#include "reach_lanes.h"
#include "setup.h"

#include <memory>

struct GqReachArgs {
  gqArm arm;
  const float *hand_pose, *Rg, *base_T, *up;
  int pose_dim;
  int64_t batch_each;
  gq3 axis;
  float D, lambda, rho, w;
  int K, M, accumulate;
  float *e, *q, *gRt;
  int32_t* seed;
};

__global__ __launch_bounds__(GQ_REACH_MAX_PROBLEMS* GQ_REACH_MAX_JOINTS) void gq_reach_kernel(const GqReachArgs g) {
  __shared__ float s_E[GQ_REACH_MAX_PROBLEMS], s_e[GQ_REACH_MAX_PROBLEMS * 6], s_q[GQ_REACH_MAX_PROBLEMS * GQ_REACH_MAX_JOINTS];
  __shared__ int s_best[GQ_REACH_MAX_STATIONS + 1];
  const int tid = threadIdx.x, j = tid & (GQ_REACH_MAX_JOINTS - 1), grp = tid >> 3;
  const int S = g.arm.S, N = g.arm.N, K = g.K, P = (K + 1) * S;
  const int p = grp < P ? grp : P - 1;  // the idle groups of the last wavefront shadow the last problem and write nothing
  const int k = p / S, sd = p - k * S;
  const size_t row = blockIdx.x;

  GqRT base, tool, pre;
  float R[9];
  const float* bt = g.base_T + (size_t)((int64_t)row / g.batch_each) * 12;
#pragma unroll
  for (int i = 0; i < 12; ++i) base.m[i] = bt[i], tool.m[i] = g.arm.tool[i], pre.m[i] = g.arm.pre[j * 12 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = g.Rg[row * 9 + i];
  const float* hp = g.hand_pose + row * (size_t)g.pose_dim;
  const gq3 t = gq_mk(hp[0], hp[1], hp[2]);
  const gq3 ax = gq_mk(g.arm.axis[j * 3], g.arm.axis[j * 3 + 1], g.arm.axis[j * 3 + 2]);
  const int type = g.arm.type[j];
  const float lo = g.arm.lower[j], hi = g.arm.upper[j];
  const float d = gq_reach_station(g.D, k, K);
  const gq3 ps = gq_reach_target(R, t, g.axis, d);

  float q = g.arm.seeds[sd * GQ_REACH_MAX_JOINTS + j];
  float e[6];
  for (int it = 0;; ++it) {
    GqRT W;
    const GqRT T = gq_reach_fk(base, pre, tool, type, ax, q, j, W);
    gq_reach_err(R, ps, T, g.rho, e);
    if (it >= g.M) break;
    float c[6], A[21], y[6];
    gq_reach_col(type, W, ax, gq_mk(T.m[3], T.m[7], T.m[11]), g.rho, c);
    gq_reach_gram(c, A);
#pragma unroll
    for (int i = 0; i < 21; ++i) A[i] = gq_reach_group_sum(A[i]);
    gq_reach_solve6(A, g.lambda, e, y);
    const float dq = gq_reach_dq(c, y);
    q = gq_reach_step(q, dq, gq_reach_group_max(fabsf(dq)), lo, hi);
  }
  if (grp < P) {
    s_q[p * GQ_REACH_MAX_JOINTS + j] = q;
    if (j < 6) {
      float ej = e[0];
#pragma unroll
      for (int i = 1; i < 6; ++i) ej = j == i ? e[i] : ej;
      s_e[p * 6 + j] = ej;
    }
    if (j == 0) s_E[p] = gq_reach_energy(e);
  }
  __syncthreads();

  if (tid == 0) {  // winners, mean and gradient: stations ascending
    float esum = 0.0f, gRt[12] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, tau_h[3] = {0.0f, 0.0f, 0.0f};
    const float inv = 1.0f / (float)(K + 1);
    const float cu = (g.up ? g.up[row] * g.w : g.w) * inv;
    for (int kk = 0; kk <= K; ++kk) {
      const int best = gq_reach_pick(s_E + kk * S, S);
      s_best[kk] = best;
      if (g.seed) g.seed[row * (size_t)(K + 1) + kk] = best;
      esum += s_E[kk * S + best];
      if (g.gRt) gq_reach_grad_add(R, s_e + (kk * S + best) * 6, cu, g.rho, gq_reach_station(g.D, kk, K), g.axis, gRt, tau_h);
    }
    if (g.e) g.e[row] = esum * inv;
    if (g.gRt) {
      gq_reach_grad_close(tau_h, gRt);
      float* o = g.gRt + row * 12;
#pragma unroll
      for (int i = 0; i < 12; ++i) o[i] = g.accumulate ? o[i] + gRt[i] : gRt[i];
    }
  }
  if (g.q) {
    __syncthreads();
    if (grp <= K && j < N) g.q[(row * (size_t)(K + 1) + grp) * N + j] = s_q[(grp * S + s_best[grp]) * GQ_REACH_MAX_JOINTS + j];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct GqArmObject : gqArm {
  GqOwner mem;
};

static bool gq_reach_finite(float v) { return v > -GQ_INF_F && v < GQ_INF_F; }

extern "C" {

int gq_arm_create(const gqArmDesc* d, gqArm** out) {
  GQ_REQUIRE(d && out, "arm_create: null");
  const int N = d->n_joints, S = d->n_seeds;
  GQ_REQUIRE(N >= 1 && N <= GQ_REACH_MAX_JOINTS, "arm_create: n_joints must be in 1..%d, got %d", GQ_REACH_MAX_JOINTS, N);
  GQ_REQUIRE(S >= 1 && S <= GQ_REACH_MAX_SEEDS, "arm_create: n_seeds must be in 1..%d, got %d", GQ_REACH_MAX_SEEDS, S);
  GQ_REQUIRE(d->joint_type && d->joint_T && d->joint_axis && d->lower && d->upper && d->tool_T && d->seeds, "arm_create: null array");
  int32_t type[8] = {0};
  float pre[8 * 12], axis[8 * 3] = {0}, lower[8] = {0}, upper[8] = {0}, seeds[GQ_REACH_MAX_SEEDS * 8] = {0};
  for (int j = 0; j < 8; ++j)
    for (int i = 0; i < 12; ++i) pre[j * 12 + i] = (i == 0 || i == 5 || i == 10) ? 1.0f : 0.0f;
  for (int j = 0; j < N; ++j) {
    GQ_REQUIRE(d->joint_type[j] == 1 || d->joint_type[j] == 2, "arm_create: joint_type[%d] must be 1 (revolute) or 2 (prismatic)", j);
    type[j] = d->joint_type[j];
    for (int i = 0; i < 12; ++i) {
      GQ_REQUIRE(gq_reach_finite(d->joint_T[j * 12 + i]), "arm_create: joint_T[%d] is not finite", j);
      pre[j * 12 + i] = d->joint_T[j * 12 + i];
    }
    const float* a = d->joint_axis + j * 3;
    const double n2 = (double)a[0] * a[0] + (double)a[1] * a[1] + (double)a[2] * a[2];
    GQ_REQUIRE(n2 > 0.999 && n2 < 1.001, "arm_create: joint_axis[%d] must be a unit vector", j);
    for (int i = 0; i < 3; ++i) axis[j * 3 + i] = a[i];
    GQ_REQUIRE(gq_reach_finite(d->lower[j]) && gq_reach_finite(d->upper[j]) && d->lower[j] < d->upper[j],
               "arm_create: limits of joint %d must be finite with lower < upper", j);
    lower[j] = d->lower[j], upper[j] = d->upper[j];
    for (int s = 0; s < S; ++s) {
      const float v = d->seeds[s * N + j];
      GQ_REQUIRE(v >= lower[j] && v <= upper[j], "arm_create: seed %d of joint %d lies outside its limits", s, j);
      seeds[s * 8 + j] = v;
    }
  }
  for (int i = 0; i < 12; ++i) GQ_REQUIRE(gq_reach_finite(d->tool_T[i]), "arm_create: tool_T is not finite");
  auto a = std::make_unique<GqArmObject>();
  GqOwner& mem = a->mem;
  a->N = N, a->S = S;
  a->type = mem.upload((const int32_t*)type, 8);
  a->pre = mem.upload((const float*)pre, 8 * 12);
  a->axis = mem.upload((const float*)axis, 8 * 3);
  a->lower = mem.upload((const float*)lower, 8);
  a->upper = mem.upload((const float*)upper, 8);
  a->tool = mem.upload(d->tool_T, 12);
  a->seeds = mem.upload((const float*)seeds, (size_t)S * 8);
  if (mem.rc) return mem.rc;
  *out = a.release();
  return GQ_OK;
}

int gq_arm_destroy(gqArm* a) {
  delete static_cast<GqArmObject*>(a);
  return GQ_OK;
}

int gq_reach_check(int n_joints, int n_seeds, float distance, int n_stations, int n_iterations, float damping, float rot_scale,
                   const float* grasp_axis) {
  GQ_REQUIRE(n_joints >= 1 && n_joints <= GQ_REACH_MAX_JOINTS, "reach: n_joints must be in 1..%d, got %d", GQ_REACH_MAX_JOINTS, n_joints);
  GQ_REQUIRE(n_seeds >= 1 && n_seeds <= GQ_REACH_MAX_SEEDS, "reach: n_seeds must be in 1..%d, got %d", GQ_REACH_MAX_SEEDS, n_seeds);
  GQ_REQUIRE(n_stations >= 0 && n_stations <= GQ_REACH_MAX_STATIONS, "reach: n_stations must be in 0..%d, got %d",
             GQ_REACH_MAX_STATIONS, n_stations);
  GQ_REQUIRE(n_stations == 0 || (distance > 0.0f && distance < GQ_INF_F), "reach: distance must be finite and > 0, got %g",
             (double)distance);
  GQ_REQUIRE(n_iterations >= 0 && n_iterations <= 4096, "reach: n_iterations must be in 0..4096, got %d", n_iterations);
  GQ_REQUIRE(damping > 0.0f && damping < GQ_INF_F, "reach: damping must be finite and > 0, got %g", (double)damping);
  GQ_REQUIRE(rot_scale > 0.0f && rot_scale < GQ_INF_F, "reach: rot_scale must be finite and > 0, got %g", (double)rot_scale);
  GQ_REQUIRE(grasp_axis, "reach: grasp_axis is NULL");
  for (int i = 0; i < 3; ++i) GQ_REQUIRE(gq_reach_finite(grasp_axis[i]), "reach: grasp_axis[%d] must be finite", i);
  GQ_REQUIRE(grasp_axis[0] != 0.0f || grasp_axis[1] != 0.0f || grasp_axis[2] != 0.0f, "reach: grasp_axis must not be all zero");
  return GQ_OK;
}

int gq_reach_terms(const gqArm* arm, const float* hand_pose, int pose_dim, const float* Rg, int64_t batch, const float* base_T,
                   int64_t n_obj, int64_t batch_each, const float* grasp_axis, float distance, int n_stations, int n_iterations,
                   float damping, float rot_scale, const float* up, float w, float* e_reach, float* reach_q, int32_t* reach_seed,
                   int accumulate, float* gRt, void* stream) {
  GQ_REQUIRE(arm, "reach: arm is NULL");
  const int rc = gq_reach_check(arm->N, arm->S, distance, n_stations, n_iterations, damping, rot_scale, grasp_axis);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "reach: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(hand_pose && Rg && base_T && pose_dim >= 9, "reach: bad arguments");
  GQ_REQUIRE(n_obj >= 1 && batch_each >= 1 && n_obj * batch_each == batch,
             "reach: base_T has %lld transforms for %lld rows each, the batch is %lld", (long long)n_obj, (long long)batch_each,
             (long long)batch);
  GqReachArgs a{};
  a.arm = *arm;
  a.hand_pose = hand_pose, a.Rg = Rg, a.base_T = base_T, a.up = up;
  a.pose_dim = pose_dim, a.batch_each = batch_each;
  a.axis = gq3{grasp_axis[0], grasp_axis[1], grasp_axis[2]};
  a.D = n_stations > 0 ? distance : 0.0f, a.lambda = damping, a.rho = rot_scale, a.w = w;
  a.K = n_stations, a.M = n_iterations, a.accumulate = accumulate != 0;
  a.e = e_reach, a.q = reach_q, a.gRt = gRt, a.seed = reach_seed;
  const int lanes = (n_stations + 1) * arm->S * GQ_REACH_MAX_JOINTS;
  const int block = (lanes + GQ_WAVE - 1) / GQ_WAVE * GQ_WAVE;
  hipLaunchKernelGGL(gq_reach_kernel, dim3((unsigned)batch), dim3(block), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
