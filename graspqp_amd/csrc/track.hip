// E_track: can the arm FOLLOW the straight approach line from the pre-grasp configuration to the grasp?  Damped-least-squares
// tracking of T + 1 waypoints, each warm-started from the one before, as ONE launch (include/graspqp_hip.h, "approach tracking", has
// the iteration and the formulas).
//
// Eight lanes make a row: lane j of the group is joint j of the arm, so a wavefront carries eight rows and a block is one wavefront.
// The kernel is a dependent chain of (T + 1)(U + 1) FK passes per row: latency-bound, so the wavefronts are spread over the CUs, one
// per block.  T and U are launch-uniform: the loops do not diverge, and a row needs no other row -- no LDS, no barrier.  Per update
// the group runs exactly the reach term's update (reach_lanes.h, reach_dev.h): the scan of the joint transforms, the error with the
// log map, the lane's column of J, the 21 group sums of J J', the unrolled 6 x 6 Cholesky, the capped and clamped step.  After U
// updates one more FK gives e_i; every lane of the group holds the same e_i and keeps the same running sums (mean, worst waypoint,
// largest joint move, gradient) in registers, and lane 0 writes them; lanes j < N write q_i at every waypoint.
// The idle groups of the last wavefront shadow the last row and write nothing.  No atomics, every sum in a fixed order, no array
// indexed at run time: bitwise reproducible, graph-capturable, no scratch.
#include "reach_lanes.h"
#include "track_dev.h"

struct GqTrackArgs {
  gqArm arm;
  const float *hand_pose, *Rg, *base_T, *up, *q_start;
  int pose_dim;
  int64_t batch, batch_each, q_stride;
  gq3 axis;
  float D, lambda, rho, w;
  int T, U, K, accumulate;
  float *e, *q, *worst, *step, *station_q, *gRt;
};

__global__ __launch_bounds__(GQ_WAVE) void gq_track_kernel(const GqTrackArgs g) {
  const int tid = threadIdx.x, j = tid & (GQ_REACH_MAX_JOINTS - 1), grp = tid >> 3;
  const int N = g.arm.N, T = g.T, U = g.U, K = g.K;
  const int64_t r = (int64_t)blockIdx.x * GQ_TRACK_ROWS_PER_WAVE + grp;
  const bool live = r < g.batch;  // the idle groups of the last wavefront shadow the last row and write nothing
  const size_t row = (size_t)(live ? r : g.batch - 1);

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
  const float inv = 1.0f / (float)(T + 1);
  const float cu = (g.up ? g.up[row] * g.w : g.w) * inv;
  const bool grad = g.gRt != nullptr;

  float q = j < N ? g.q_start[row * (size_t)g.q_stride + j] : 0.0f;
  GqTrackAcc acc;
  gq_track_acc_init(acc);
  for (int i = 0; i <= T; ++i) {
    const float d = gq_track_dist(g.D, i, T);
    const gq3 ps = gq_reach_target(R, t, g.axis, d);
    const float q_prev = q;
    float e[6];
    for (int it = 0;; ++it) {
      GqRT W;
      const GqRT Tee = gq_reach_fk(base, pre, tool, type, ax, q, j, W);
      gq_reach_err(R, ps, Tee, g.rho, e);
      if (it >= U) break;
      float c[6], A[21], y[6];
      gq_reach_col(type, W, ax, gq_mk(Tee.m[3], Tee.m[7], Tee.m[11]), g.rho, c);
      gq_reach_gram(c, A);
#pragma unroll
      for (int s = 0; s < 21; ++s) A[s] = gq_reach_group_sum(A[s]);
      gq_reach_solve6(A, g.lambda, e, y);
      const float dq = gq_reach_dq(c, y);
      q = gq_reach_step(q, dq, gq_reach_group_max(fabsf(dq)), lo, hi);
    }
    gq_track_acc_add(acc, R, e, gq_reach_group_max(fabsf(q - q_prev)), cu, g.rho, d, g.axis, grad);
    if (live && j < N) {
      if (g.q) g.q[(row * (size_t)(T + 1) + i) * N + j] = q;
      if (g.station_q) {
        const int k = gq_track_station(i, T, K);
        if (k >= 0) g.station_q[(row * (size_t)(K + 1) + k) * N + j] = q;
      }
    }
  }
  if (!live || j != 0) return;
  if (g.e) g.e[row] = acc.esum * inv;
  if (g.worst) g.worst[row] = acc.worst;
  if (g.step) g.step[row] = acc.step;
  if (grad) {
    gq_reach_grad_close(acc.tau_h, acc.gRt);
    float* o = g.gRt + row * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = g.accumulate ? o[i] + acc.gRt[i] : acc.gRt[i];
  }
}

static bool gq_track_finite(float v) { return v > -GQ_INF_F && v < GQ_INF_F; }

extern "C" {

int gq_track_check(int n_joints, float distance, int n_waypoints, int n_updates, float damping, float rot_scale, int n_stations,
                   int with_station_q, const float* grasp_axis) {
  GQ_REQUIRE(n_joints >= 1 && n_joints <= GQ_REACH_MAX_JOINTS, "track: n_joints must be in 1..%d, got %d", GQ_REACH_MAX_JOINTS, n_joints);
  GQ_REQUIRE(n_waypoints >= 1 && n_waypoints <= GQ_TRACK_MAX_WAYPOINTS, "track: n_waypoints must be in 1..%d, got %d",
             GQ_TRACK_MAX_WAYPOINTS, n_waypoints);
  GQ_REQUIRE(n_updates >= 1 && n_updates <= GQ_TRACK_MAX_UPDATES, "track: n_updates must be in 1..%d, got %d", GQ_TRACK_MAX_UPDATES,
             n_updates);
  GQ_REQUIRE(distance > 0.0f && distance < GQ_INF_F, "track: distance must be finite and > 0, got %g", (double)distance);
  GQ_REQUIRE(damping > 0.0f && damping < GQ_INF_F, "track: damping must be finite and > 0, got %g", (double)damping);
  GQ_REQUIRE(rot_scale > 0.0f && rot_scale < GQ_INF_F, "track: rot_scale must be finite and > 0, got %g", (double)rot_scale);
  GQ_REQUIRE(n_stations >= 0 && n_stations <= GQ_REACH_MAX_STATIONS, "track: n_stations must be in 0..%d, got %d", GQ_REACH_MAX_STATIONS,
             n_stations);
  GQ_REQUIRE(!with_station_q || (n_stations >= 1 && n_waypoints % n_stations == 0),
             "track: track_station_q needs n_stations >= 1 that divides n_waypoints, got n_stations %d, n_waypoints %d", n_stations,
             n_waypoints);
  GQ_REQUIRE(grasp_axis, "track: grasp_axis is NULL");
  for (int i = 0; i < 3; ++i) GQ_REQUIRE(gq_track_finite(grasp_axis[i]), "track: grasp_axis[%d] must be finite", i);
  GQ_REQUIRE(grasp_axis[0] != 0.0f || grasp_axis[1] != 0.0f || grasp_axis[2] != 0.0f, "track: grasp_axis must not be all zero");
  return GQ_OK;
}

int gq_track_terms(const gqArm* arm, const float* hand_pose, int pose_dim, const float* Rg, int64_t batch, const float* base_T,
                   int64_t n_obj, int64_t batch_each, const float* grasp_axis, float distance, int n_waypoints, int n_updates,
                   float damping, float rot_scale, const float* q_start, int64_t q_start_stride, int n_stations, const float* up,
                   float w, float* e_track, float* track_q, float* track_worst, float* track_step, float* track_station_q,
                   int accumulate, float* gRt, void* stream) {
  GQ_REQUIRE(arm, "track: arm is NULL");
  const int rc = gq_track_check(arm->N, distance, n_waypoints, n_updates, damping, rot_scale, n_stations, track_station_q != nullptr,
                                grasp_axis);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "track: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(hand_pose && Rg && base_T && pose_dim >= 9, "track: bad arguments");
  GQ_REQUIRE(q_start, "track: q_start is NULL");
  GQ_REQUIRE(q_start_stride >= arm->N, "track: q_start_stride must be at least n_joints = %d floats, got %lld", arm->N,
             (long long)q_start_stride);
  GQ_REQUIRE(n_obj >= 1 && batch_each >= 1 && n_obj * batch_each == batch,
             "track: base_T has %lld transforms for %lld rows each, the batch is %lld", (long long)n_obj, (long long)batch_each,
             (long long)batch);
  GqTrackArgs a{};
  a.arm = *arm;
  a.hand_pose = hand_pose, a.Rg = Rg, a.base_T = base_T, a.up = up, a.q_start = q_start;
  a.pose_dim = pose_dim, a.batch = batch, a.batch_each = batch_each, a.q_stride = q_start_stride;
  a.axis = gq3{grasp_axis[0], grasp_axis[1], grasp_axis[2]};
  a.D = distance, a.lambda = damping, a.rho = rot_scale, a.w = w;
  a.T = n_waypoints, a.U = n_updates, a.K = n_stations, a.accumulate = accumulate != 0;
  a.e = e_track, a.q = track_q, a.worst = track_worst, a.step = track_step, a.station_q = track_station_q, a.gRt = gRt;
  const int64_t blocks = (batch + GQ_TRACK_ROWS_PER_WAVE - 1) / GQ_TRACK_ROWS_PER_WAVE;
  hipLaunchKernelGGL(gq_track_kernel, dim3((unsigned)blocks), dim3(GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
