// Decision bodies of finger closing (include/graspqp_hip.h, "finger closing"): what gq_close_kernel (close.hip) decides per joint
// and per link, as plain functions of their operands.  tests/close_body_host.cpp compiles them for the host (behind
// tests/host_shim.h) and holds them against the fp64 oracle.  Only math.h and stdint.h are needed: nothing here rounds but the one
// division pair of gq_close_delta and the one addition of gq_close_update.
#pragma once
#include <math.h>
#include <stdint.h>

#define GQ_CLOSE_MAX_STEPS 64
#define GQ_CLOSE_NONE 0x7fffffff  // the sample index of "no sample": behind every real index at equal phi

// One fold step of m = max_a |u_a|, NaN-propagating: the fold is associative and commutative, so the order of the lanes cannot
// matter.  acc starts at 0.
__device__ __forceinline__ float gq_close_umax(float acc, float u) {
  const float a = fabsf(u);
  if (acc != acc) return acc;
  if (a != a) return a;
  return a > acc ? a : acc;
}

// u_a = v_a / step_a: the command in units of the joint's step
__device__ __forceinline__ float gq_close_units(float v, float step) { return v / step; }

// Delta_a = step_a (u_a / m).  m = 0, inf or NaN (some u_a not finite): the row does not move.  u_a / m is exactly +-1 for the
// fastest joint, so it moves exactly its step.
__device__ __forceinline__ float gq_close_delta(float u, float step, float m) {
  if (!(m > 0.0f && m < __builtin_inff())) return 0.0f;
  return step * (u / m);
}

// The (phi, index) key: a before b when its phi is smaller, at equal phi when its sample index is lower.  -0 == +0 compare equal,
// so the index decides between them; a NaN phi never gets here.  "No sample" is (+inf, GQ_CLOSE_NONE).
__device__ __forceinline__ bool gq_close_key_less(float phi_a, int idx_a, float phi_b, int idx_b) {
  return phi_a < phi_b || (phi_a == phi_b && idx_a < idx_b);
}

// A link touches when its smallest phi is at or under the tolerance (false for "no sample": +inf)
__device__ __forceinline__ bool gq_close_touches(float m_l, float touch) { return m_l <= touch; }

// The stop mask: joint a stands still when a touched link (bit l of `touched`) lies in joint_links[a]
__device__ __forceinline__ bool gq_close_stopped(uint64_t touched, uint64_t joint_links) { return (touched & joint_links) != 0; }

// The clamped update: a stopped joint and a joint without a command keep their bits, every other one takes its step and is clamped
__device__ __forceinline__ float gq_close_update(float theta, float delta, float lower, float upper, bool stopped) {
  if (stopped || delta == 0.0f) return theta;
  return fminf(fmaxf(theta + delta, lower), upper);
}

// x_w = R x_h + t with r1..r3 the rows of R: gq_pregrasp_stations' expression (gq3 / gq_mk: common.h or tests/host_shim.h)
__device__ __forceinline__ gq3 gq_close_world(gq3 r1, gq3 r2, gq3 r3, gq3 t, gq3 y) {
  return gq_mk(fmaf(r1.x, y.x, fmaf(r1.y, y.y, r1.z * y.z)) + t.x, fmaf(r2.x, y.x, fmaf(r2.y, y.y, r2.z * y.z)) + t.y,
               fmaf(r3.x, y.x, fmaf(r3.y, y.y, r3.z * y.z)) + t.z);
}
