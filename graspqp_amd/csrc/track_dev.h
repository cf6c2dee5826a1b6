// Device bodies of the approach tracking term (include/graspqp_hip.h, "approach tracking"): what gq_track_kernel (track.hip) does
// per row beyond the reach term's update (reach_dev.h): the distance of a waypoint, the station a waypoint stands for, and the
// running sums of a row (mean, worst waypoint, largest joint move, the gradient in the gRt layout), as plain functions of their
// operands.  tests/track_body_host.cpp compiles them for the host and walks the lane groups serially in the kernel's order.
//
// The gradient is the partial derivative with respect to the targets with every q_i held fixed.  It is the gradient of the
// converged path energy where every waypoint has reached a fixed point with no joint on a limit (there J'e_i = 0, E_i is
// stationary in q_i and the warm start drops out); it is an approximation at finite U, with a clamped joint, and in the two-cycle
// past the outer boundary of a revolute arm.
#pragma once
#include "reach_dev.h"

#define GQ_TRACK_MAX_WAYPOINTS 64  // T: waypoints beyond the first
#define GQ_TRACK_MAX_UPDATES 16    // U: updates per waypoint
#define GQ_TRACK_ROWS_PER_WAVE 8   // eight lanes per row, eight rows per wavefront

// d_i = D (T - i) / T: waypoint 0 is the retreated pose (the reach term's station K), waypoint T the grasp pose
__device__ __forceinline__ float gq_track_dist(float D, int i, int T) { return D * (float)(T - i) / (float)T; }

// The station of reach_q's layout that waypoint i stands for: k with i = T (K - k) / K, or -1 (K must divide T; K = 0: none)
__device__ __forceinline__ int gq_track_station(int i, int T, int K) {
  if (K < 1) return -1;
  const int per = T / K;
  return i % per == 0 ? K - i / per : -1;
}

struct GqTrackAcc {  // the running sums of a row, waypoints ascending
  float esum, worst, step;
  float gRt[12], tau_h[3];
};

__device__ __forceinline__ void gq_track_acc_init(GqTrackAcc& a) {
  a.esum = a.worst = a.step = 0.0f;
#pragma unroll
  for (int i = 0; i < 12; ++i) a.gRt[i] = 0.0f;
  a.tau_h[0] = a.tau_h[1] = a.tau_h[2] = 0.0f;
}

// waypoint i has ended with the error e at the distance d; `move` is the largest |q_i,j - q_{i-1},j| of the row's joints
__device__ __forceinline__ void gq_track_acc_add(GqTrackAcc& a, const float* R, const float (&e)[6], float move, float cu, float rho,
                                                 float d, gq3 axis, bool grad) {
  const float E = gq_reach_energy(e);
  a.esum += E;
  a.worst = fmaxf(a.worst, E);
  a.step = fmaxf(a.step, move);
  if (grad) gq_reach_grad_add(R, e, cu, rho, d, axis, a.gRt, a.tau_h);
}
