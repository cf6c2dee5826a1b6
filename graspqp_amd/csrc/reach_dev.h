// Device bodies of the reach term (include/graspqp_hip.h, "arm reachability"): what gq_reach_kernel (reach.hip) does per joint of
// an IK problem (joint transform, product of two transforms, Jacobian column, products of J J', the joint step) and per problem (the
// pose error with the log map, the damped 6 x 6 solve), and the tail of a row (winner per station, mean, gradient in the gRt layout),
// as plain functions of their operands.  tests/reach_body_host.cpp compiles them for the host and walks the lane groups of a row
// through them serially in the kernel's order.  Only gq3 / gq_mk are needed.
#pragma once
#ifndef GQ_SCENE_HOST_BUILD
#include "common.h"
#endif

#define GQ_REACH_MAX_JOINTS 8     // joints of the arm = lanes of a problem's group
#define GQ_REACH_MAX_SEEDS 8
#define GQ_REACH_MAX_STATIONS 3   // stations beyond the grasp pose
#define GQ_REACH_MAX_PROBLEMS ((GQ_REACH_MAX_STATIONS + 1) * GQ_REACH_MAX_SEEDS)
#define GQ_REACH_STEP_CAP 0.5f    // largest joint step of one update
#define GQ_REACH_LOG_SERIES 1e-6f // below this |vee| the log map takes its series

// The arm as the kernel takes it: a table of device pointers, every per-joint array padded to eight joints (type 0, identity
// transform, limits 0) so that lane j of a group loads entry j without a test.
struct gqArm {
  int N, S;
  const int32_t* type;  // (8) 1 revolute, 2 prismatic, 0 beyond N
  const float* pre;     // (8,12) fixed transform parent -> joint frame
  const float* axis;    // (8,3) unit, joint frame
  const float* lower;   // (8)
  const float* upper;   // (8)
  const float* tool;    // (12) flange -> hand root
  const float* seeds;   // (S,8)
};

struct GqRT {  // 3x4 row-major [A | b]
  float m[12];
};

// a * b for two rigid transforms
__device__ __forceinline__ GqRT gq_reach_mul(const GqRT& a, const GqRT& b) {
  GqRT c;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      c.m[r * 4 + k] = fmaf(a.m[r * 4], b.m[k], fmaf(a.m[r * 4 + 1], b.m[4 + k], a.m[r * 4 + 2] * b.m[8 + k]));
    c.m[r * 4 + 3] = fmaf(a.m[r * 4], b.m[3], fmaf(a.m[r * 4 + 1], b.m[7], fmaf(a.m[r * 4 + 2], b.m[11], a.m[r * 4 + 3])));
  }
  return c;
}

// pre * motion(q): the joint's frame in its parent's, after the joint has moved by q about / along its unit axis (Rodrigues for a
// revolute joint, a shift for a prismatic one, nothing for the padding lanes)
__device__ __forceinline__ GqRT gq_reach_joint(const GqRT& pre, int type, gq3 a, float q) {
  GqRT mo = {{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}};
  if (type == 1) {
    const float s = sinf(q), c = cosf(q), v = 1.0f - c;
    mo.m[0] = fmaf(v, a.x * a.x, c), mo.m[1] = fmaf(v, a.x * a.y, -s * a.z), mo.m[2] = fmaf(v, a.x * a.z, s * a.y);
    mo.m[4] = fmaf(v, a.x * a.y, s * a.z), mo.m[5] = fmaf(v, a.y * a.y, c), mo.m[6] = fmaf(v, a.y * a.z, -s * a.x);
    mo.m[8] = fmaf(v, a.x * a.z, -s * a.y), mo.m[9] = fmaf(v, a.y * a.z, s * a.x), mo.m[10] = fmaf(v, a.z * a.z, c);
  } else if (type == 2) {
    mo.m[3] = q * a.x, mo.m[7] = q * a.y, mo.m[11] = q * a.z;
  }
  return gq_reach_mul(pre, mo);
}

// Target of station k: R* = R, p* = t - d_k R a with d_k = D k / K (0 for K = 0), the direction convention of gq_approach_terms
__device__ __forceinline__ float gq_reach_station(float D, int k, int K) { return K > 0 ? D * (float)k / (float)K : 0.0f; }
__device__ __forceinline__ gq3 gq_reach_target(const float* R, gq3 t, gq3 a, float d) {
  const gq3 Ra = gq_mk(fmaf(R[0], a.x, fmaf(R[1], a.y, R[2] * a.z)), fmaf(R[3], a.x, fmaf(R[4], a.y, R[5] * a.z)),
                       fmaf(R[6], a.x, fmaf(R[7], a.y, R[8] * a.z)));
  return gq_mk(fmaf(-d, Ra.x, t.x), fmaf(-d, Ra.y, t.y), fmaf(-d, Ra.z, t.z));
}

// e = [p* - p ; rho log(R* R')] for the hand-root pose T = [R | p]; the log map takes its angle from atan2(|vee|, (trace - 1) / 2)
// and the series 1 + |vee|^2 / 6 of angle / |vee| below GQ_REACH_LOG_SERIES
__device__ __forceinline__ void gq_reach_err(const float* Rs, gq3 ps, const GqRT& T, float rho, float (&e)[6]) {
  e[0] = ps.x - T.m[3], e[1] = ps.y - T.m[7], e[2] = ps.z - T.m[11];
  // E = R* R'  (E[a][b] = sum_c R*[a][c] R[b][c])
  const float* m = T.m;
  const float E00 = fmaf(Rs[0], m[0], fmaf(Rs[1], m[1], Rs[2] * m[2])), E11 = fmaf(Rs[3], m[4], fmaf(Rs[4], m[5], Rs[5] * m[6]));
  const float E22 = fmaf(Rs[6], m[8], fmaf(Rs[7], m[9], Rs[8] * m[10]));
  const float E01 = fmaf(Rs[0], m[4], fmaf(Rs[1], m[5], Rs[2] * m[6])), E10 = fmaf(Rs[3], m[0], fmaf(Rs[4], m[1], Rs[5] * m[2]));
  const float E02 = fmaf(Rs[0], m[8], fmaf(Rs[1], m[9], Rs[2] * m[10])), E20 = fmaf(Rs[6], m[0], fmaf(Rs[7], m[1], Rs[8] * m[2]));
  const float E12 = fmaf(Rs[3], m[8], fmaf(Rs[4], m[9], Rs[5] * m[10])), E21 = fmaf(Rs[6], m[4], fmaf(Rs[7], m[5], Rs[8] * m[6]));
  const float vx = 0.5f * (E21 - E12), vy = 0.5f * (E02 - E20), vz = 0.5f * (E10 - E01);
  const float s2 = fmaf(vx, vx, fmaf(vy, vy, vz * vz)), s = sqrtf(s2);
  const float c = 0.5f * (E00 + E11 + E22 - 1.0f);
  const float f = rho * (s < GQ_REACH_LOG_SERIES ? fmaf(s2, 1.0f / 6.0f, 1.0f) : atan2f(s, c) / s);
  e[3] = f * vx, e[4] = f * vy, e[5] = f * vz;
}

// Column of J = [J_v ; rho J_w] for the joint whose frame is W (in the frame the row lives in): revolute a x (p_ee - o) and rho a,
// prismatic a and 0, padding lane 0.  a = W's rotation applied to the joint's axis, o = W's origin.
__device__ __forceinline__ void gq_reach_col(int type, const GqRT& W, gq3 ax, gq3 pee, float rho, float (&c)[6]) {
  const gq3 a = gq_mk(fmaf(W.m[0], ax.x, fmaf(W.m[1], ax.y, W.m[2] * ax.z)), fmaf(W.m[4], ax.x, fmaf(W.m[5], ax.y, W.m[6] * ax.z)),
                      fmaf(W.m[8], ax.x, fmaf(W.m[9], ax.y, W.m[10] * ax.z)));
  const gq3 r = gq_mk(pee.x - W.m[3], pee.y - W.m[7], pee.z - W.m[11]);
  if (type == 1) {
    c[0] = a.y * r.z - a.z * r.y, c[1] = a.z * r.x - a.x * r.z, c[2] = a.x * r.y - a.y * r.x;
    c[3] = rho * a.x, c[4] = rho * a.y, c[5] = rho * a.z;
  } else if (type == 2) {
    c[0] = a.x, c[1] = a.y, c[2] = a.z, c[3] = c[4] = c[5] = 0.0f;
  } else {
    c[0] = c[1] = c[2] = c[3] = c[4] = c[5] = 0.0f;
  }
}

// The joint's share of the lower triangle of J J', packed row by row: g[i (i + 1) / 2 + k] = c_i c_k, k <= i
__device__ __forceinline__ void gq_reach_gram(const float (&c)[6], float (&g)[21]) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = 0; k <= i; ++k) g[i * (i + 1) / 2 + k] = c[i] * c[k];
}

// y = (A + lambda I)^-1 e by Cholesky, A the packed lower triangle of J J'.  Unrolled: every index is a constant.  fp32: a
// backward-stable factorisation solves a matrix within about eps |A| = 6e-8 x 8 m^2 of the given one, 0.5 % of the default damping;
// the fixed point of the iteration (e = 0, or J'e = 0 out of range) does not depend on the solve, and E is stationary in q there.
__device__ __forceinline__ void gq_reach_solve6(const float (&A)[21], float lambda, const float (&e)[6], float (&y)[6]) {
  float L[21], dinv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      float s = A[i * (i + 1) / 2 + k] + (i == k ? lambda : 0.0f);
#pragma unroll
      for (int q = 0; q < k; ++q) s = fmaf(-L[i * (i + 1) / 2 + q], L[k * (k + 1) / 2 + q], s);
      if (i == k) {
        L[i * (i + 1) / 2 + i] = sqrtf(s);
        dinv[i] = 1.0f / L[i * (i + 1) / 2 + i];
      } else {
        L[i * (i + 1) / 2 + k] = s * dinv[k];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // L z = e
    float s = e[i];
#pragma unroll
    for (int q = 0; q < i; ++q) s = fmaf(-L[i * (i + 1) / 2 + q], y[q], s);
    y[i] = s * dinv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L' y = z
    float s = y[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) s = fmaf(-L[q * (q + 1) / 2 + i], y[q], s);
    y[i] = s * dinv[i];
  }
}

// dq_j = c_j . y
__device__ __forceinline__ float gq_reach_dq(const float (&c)[6], const float (&y)[6]) {
  return fmaf(c[0], y[0], fmaf(c[1], y[1], fmaf(c[2], y[2], fmaf(c[3], y[3], fmaf(c[4], y[4], c[5] * y[5])))));
}

// q <- clamp(q + dq scaled so that the group's largest |dq| is at most the step cap, lower, upper)
__device__ __forceinline__ float gq_reach_step(float q, float dq, float max_abs, float lo, float hi) {
  if (max_abs > GQ_REACH_STEP_CAP) dq *= GQ_REACH_STEP_CAP / max_abs;
  return fminf(fmaxf(q + dq, lo), hi);
}

__device__ __forceinline__ float gq_reach_energy(const float (&e)[6]) {
  return fmaf(e[0], e[0], fmaf(e[1], e[1], fmaf(e[2], e[2], fmaf(e[3], e[3], fmaf(e[4], e[4], e[5] * e[5])))));
}

// Winner of a station among the S seeds at E[0..S): the smallest value, the lowest index on a tie (a NaN never wins over seed 0's)
__device__ __forceinline__ int gq_reach_pick(const float* E, int S) {
  int best = 0;
  for (int s = 1; s < S; ++s)
    if (E[s] < E[best]) best = s;
  return best;
}

// One station's share of the row gradient in the gRt layout, [gsum(3), K9(9)] with grad_t = -R gsum and grad_R = R K9.  With the
// row factor c = w up / (K + 1): g_p = 2 c e_p pulls on p* = t - d R a, the torque tau = 2 c rho e_w (e_w = rho log) turns R* = R:
//   gsum -= R' g_p      K9 += (R' g_p) (x) (-d a)      tau_h += R' tau     (gq_reach_grad_close adds hat(tau_h) / 2 to K9 once)
__device__ __forceinline__ void gq_reach_grad_add(const float* R, const float* e, float c, float rho, float d, gq3 a, float (&gRt)[12],
                                                  float (&tau_h)[3]) {
  const float c2 = 2.0f * c, cr = 2.0f * c * rho;
  const gq3 gp = gq_mk(c2 * e[0], c2 * e[1], c2 * e[2]), tq = gq_mk(cr * e[3], cr * e[4], cr * e[5]);
  const float gh[3] = {fmaf(R[0], gp.x, fmaf(R[3], gp.y, R[6] * gp.z)), fmaf(R[1], gp.x, fmaf(R[4], gp.y, R[7] * gp.z)),
                       fmaf(R[2], gp.x, fmaf(R[5], gp.y, R[8] * gp.z))};
  const float y[3] = {-d * a.x, -d * a.y, -d * a.z};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gRt[i] -= gh[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) gRt[3 + i * 3 + k] = fmaf(gh[i], y[k], gRt[3 + i * 3 + k]);
  }
  tau_h[0] += fmaf(R[0], tq.x, fmaf(R[3], tq.y, R[6] * tq.z));
  tau_h[1] += fmaf(R[1], tq.x, fmaf(R[4], tq.y, R[7] * tq.z));
  tau_h[2] += fmaf(R[2], tq.x, fmaf(R[5], tq.y, R[8] * tq.z));
}
// K9 += hat(tau_h) / 2: R K9 then holds tau^ R / 2, the matrix whose pairing with a rotation d^ R of R is tau . d
__device__ __forceinline__ void gq_reach_grad_close(const float (&tau_h)[3], float (&gRt)[12]) {
  const float hx = 0.5f * tau_h[0], hy = 0.5f * tau_h[1], hz = 0.5f * tau_h[2];
  gRt[3 + 1] -= hz, gRt[3 + 2] += hy;
  gRt[3 + 3] += hz, gRt[3 + 5] -= hx;
  gRt[3 + 6] -= hy, gRt[3 + 7] += hx;
}
