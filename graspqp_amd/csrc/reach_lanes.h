// The lane-group helpers of the arm kernels: eight lanes make an IK problem, lane j of the group is joint j of the arm, two groups
// share a DPP row of 16.  gq_reach_kernel (reach.hip) and gq_track_kernel (track.hip) both walk their problems through these; the
// per-joint and per-problem arithmetic they call is in reach_dev.h.  Device only (DPP row operations).
#pragma once
#include "reach_dev.h"
#include "wave.h"

// value of the lane `d` places below in the row of 16; the first d lanes of a row keep their own (no lane of a group that uses the
// shifted value -- j >= d -- sits there)
template <int CTRL>
__device__ __forceinline__ float gq_reach_shr(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ void gq_reach_scan_step(GqRT& X, bool take) {
  GqRT Y;
#pragma unroll
  for (int i = 0; i < 12; ++i) Y.m[i] = gq_reach_shr<CTRL>(X.m[i]);
  const GqRT Z = gq_reach_mul(Y, X);
#pragma unroll
  for (int i = 0; i < 12; ++i) X.m[i] = take ? Z.m[i] : X.m[i];
}
__device__ __forceinline__ float gq_reach_group_sum(float t) {
  t += gq_dpp_all_f<0xb1>(t);   // quad_perm [1,0,3,2]
  t += gq_dpp_all_f<0x4e>(t);   // quad_perm [2,3,0,1]
  t += gq_dpp_all_f<0x141>(t);  // row_half_mirror: lane j <-> 7 - j of the group
  return t;
}
__device__ __forceinline__ float gq_reach_group_max(float t) {
  t = fmaxf(t, gq_dpp_all_f<0xb1>(t));
  t = fmaxf(t, gq_dpp_all_f<0x4e>(t));
  t = fmaxf(t, gq_dpp_all_f<0x141>(t));
  return t;
}

// base -> hand root for the group's joints q (lane j holds q_j); W is base -> joint j on lane j
__device__ __forceinline__ GqRT gq_reach_fk(const GqRT& base, const GqRT& pre, const GqRT& tool, int type, gq3 ax, float q, int j,
                                            GqRT& W) {
  GqRT X = gq_reach_joint(pre, type, ax, q);
  gq_reach_scan_step<0x111>(X, j >= 1);  // row_shr:1
  gq_reach_scan_step<0x112>(X, j >= 2);  // row_shr:2
  gq_reach_scan_step<0x114>(X, j >= 4);  // row_shr:4
  W = gq_reach_mul(base, X);
  GqRT W7;
#pragma unroll
  for (int i = 0; i < 12; ++i) W7.m[i] = __shfl(W.m[i], GQ_REACH_MAX_JOINTS - 1, GQ_REACH_MAX_JOINTS);
  return gq_reach_mul(W7, tool);
}
