// Device bodies of the arm clearance term (include/graspqp_hip.h, "arm clearance"): what gq_arm_kernel (armscene.hip) does per
// joint of a station (the chain of link frames, the Jacobian column with a joint on a limit frozen), per collision sphere (its
// world point, the hinge on the scene grid, its share of dE/dq) and per station (J g_q and J J' in fp64, the damped 6 x 6 solve in
// fp64), as plain functions of their operands.  The joint transform, the product of two transforms and the Jacobian column are
// the reach term's (reach_dev.h), the field is gq_scene_sample (scene_dev.h).  tests/armscene_body_host.cpp compiles them for the
// host and walks the stations of a row through them serially in the kernel's order.
#pragma once
#include "reach_dev.h"
#include "scene_dev.h"

#define GQ_ARM_MAX_SPHERES 64  // collision spheres of the arm = lanes of a station's wavefront

// W_j = base X_0 X_1 ... X_j, multiplied left to right; X (8,12) are the joint transforms pre_i m_i(q_i) of the station
__device__ __forceinline__ GqRT gq_arm_chain(const GqRT& base, const float* X, int j) {
  GqRT W = base;
  for (int i = 0; i <= j; ++i) {
    GqRT Xi;
#pragma unroll
    for (int e = 0; e < 12; ++e) Xi.m[e] = X[i * 12 + e];
    W = gq_reach_mul(W, Xi);
  }
  return W;
}

// x = W c for a link frame W (12 floats, row-major [A | b]) and a centre c in the link frame
__device__ __forceinline__ gq3 gq_arm_point(const float* W, gq3 c) {
  return gq_mk(fmaf(W[0], c.x, fmaf(W[1], c.y, fmaf(W[2], c.z, W[3]))), fmaf(W[4], c.x, fmaf(W[5], c.y, fmaf(W[6], c.z, W[7]))),
               fmaf(W[8], c.x, fmaf(W[9], c.y, fmaf(W[10], c.z, W[11]))));
}

// h = max((margin + r) - phi(x), 0) inside the grid's volume, 0 outside it or at a non-finite point; f = -grad phi where h > 0,
// else 0.  The rules and the numbers are gq_scene_sample's.
__device__ __forceinline__ float gq_arm_hinge(const gqSceneGrid& grid, gq3 x, float margin, float r, gq3& f) {
  float phi = 0.0f;
  gq3 grad = gq_mk(0.0f, 0.0f, 0.0f);
  f = gq_mk(0.0f, 0.0f, 0.0f);
  if (gq_scene_sample(grid, x, phi, grad) != GQ_SCENE_INSIDE) return 0.0f;
  const float h = (margin + r) - phi;
  if (!(h > 0.0f)) return 0.0f;
  f = gq_mk(-grad.x, -grad.y, -grad.z);
  return h;
}

// The sphere's share of dE/dq: g[j] = [l >= j] f . col_j(x), col_j(x) = z_j x (x - o_j) for a revolute joint, z_j for a prismatic
// one, 0 for the padding joints: the first three entries of the reach term's column taken at x.  W (8,12) are the link frames.
__device__ __forceinline__ void gq_arm_joint_terms(int l, gq3 x, gq3 f, const float* W, const int32_t* type, const float* axis,
                                                   float (&g)[GQ_REACH_MAX_JOINTS]) {
#pragma unroll
  for (int j = 0; j < GQ_REACH_MAX_JOINTS; ++j) {
    GqRT Wj;
#pragma unroll
    for (int e = 0; e < 12; ++e) Wj.m[e] = W[j * 12 + e];
    float c[6];
    gq_reach_col(type[j], Wj, gq_mk(axis[j * 3], axis[j * 3 + 1], axis[j * 3 + 2]), x, 1.0f, c);
    const float d = fmaf(f.x, c[0], fmaf(f.y, c[1], f.z * c[2]));
    g[j] = l >= j ? d : 0.0f;
  }
}

// Column j of J = [J_v ; rho J_w] at the hand root, zero for a joint ON a limit (free: lower < q < upper on the float32 numbers)
__device__ __forceinline__ void gq_arm_col(int type, const GqRT& W, gq3 ax, gq3 pee, float rho, float q, float lo, float hi,
                                           float (&c)[6]) {
  gq_reach_col(type, W, ax, pee, rho, c);
  if (!(lo < q && q < hi)) c[0] = c[1] = c[2] = c[3] = c[4] = c[5] = 0.0f;
}

// b = J g_q and the packed lower triangle A of J J' in fp64, joints ascending; C (8,6) are the columns (zero where frozen or padding,
// so that a frozen joint's g_q drops out of b)
__device__ __forceinline__ void gq_arm_normal(const float* C, const float (&gq)[GQ_REACH_MAX_JOINTS], double (&A)[21], double (&b)[6]) {
#pragma unroll
  for (int i = 0; i < 21; ++i) A[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) b[i] = 0.0;
#pragma unroll
  for (int j = 0; j < GQ_REACH_MAX_JOINTS; ++j) {
    double c[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = (double)C[j * 6 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      b[i] = fma(c[i], (double)gq[j], b[i]);
#pragma unroll
      for (int k = 0; k <= i; ++k) A[i * (i + 1) / 2 + k] = fma(c[i], c[k], A[i * (i + 1) / 2 + k]);
    }
  }
}

// y = (A + lambda I)^-1 b by Cholesky in fp64, A the packed lower triangle; unrolled: every index is a constant.  ONE solve per
// station whose result is the gradient itself, at a damping far below the reach iteration's: |A| / lambda reaches 8e6, beyond fp32.
__device__ __forceinline__ void gq_arm_solve6(const double (&A)[21], double lambda, const double (&b)[6], double (&y)[6]) {
  double L[21], dinv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k <= i; ++k) {
      double s = A[i * (i + 1) / 2 + k] + (i == k ? lambda : 0.0);
#pragma unroll
      for (int q = 0; q < k; ++q) s = fma(-L[i * (i + 1) / 2 + q], L[k * (k + 1) / 2 + q], s);
      if (i == k) {
        L[i * (i + 1) / 2 + i] = sqrt(s);
        dinv[i] = 1.0 / L[i * (i + 1) / 2 + i];
      } else {
        L[i * (i + 1) / 2 + k] = s * dinv[k];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // L z = b
    double s = b[i];
#pragma unroll
    for (int q = 0; q < i; ++q) s = fma(-L[i * (i + 1) / 2 + q], y[q], s);
    y[i] = s * dinv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L' y = z
    double s = y[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) s = fma(-L[q * (q + 1) / 2 + i], y[q], s);
    y[i] = s * dinv[i];
  }
}

// E_k = sum of the hinges of the station, spheres ascending
__device__ __forceinline__ float gq_arm_station_sum(const float* h, int ns) {
  float e = 0.0f;
  for (int s = 0; s < ns; ++s) e += h[s];
  return e;
}
