// Device bodies of the squeeze term (include/graspqp_hip.h, "contact closing feasibility"): what gq_squeeze_kernel (squeeze.hip)
// does per (contact, joint), per entry of the normal matrix, per column of its Cholesky factor and per joint of the kinematic
// Hessian walk, as plain functions of their operands.  tests/squeeze_body_host.cpp compiles them for the host and walks one row
// through them serially in the kernel's order.  Only gq3 / gq_mk are needed: the small vector products are written out here.
// The Jacobian column and the Hessian branches restate gq_jacobian_kernel<false> and gq_contact_jacobian_bwd_kernel of export.hip
// term for term (those kernels keep their own text, so their code objects do not change).
#pragma once
#ifndef GQ_SCENE_HOST_BUILD
#include "common.h"
#endif

#define GQ_SQ_MAX 64        // most actuated joints, tree joints and contacts of a row
#define GQ_SQ_EPS 1e-8f     // |distance| = sqrt(dist_sq + eps), as the contact branch takes it

__device__ __forceinline__ gq3 gq_sq_cross(gq3 a, gq3 b) {
  return gq_mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ gq3 gq_sq_sub(gq3 a, gq3 b) { return gq_mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ float gq_sq_dot(gq3 a, gq3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }

// Row stride of the normal matrix in LDS: odd, so the lanes of a column walk hit different banks
#define gq_squeeze_ld(JA) ((JA) | 1)

// Column of the linear contact Jacobian for tree joint j and the contact at x (hand frame): a x (x - p) for a revolute joint
// (type 1) on the path base -> contact, a for a prismatic one, 0 off the path.  a, p: axis and origin of the joint, hand frame.
__device__ __forceinline__ gq3 gq_squeeze_col(int type, bool on_path, gq3 a, gq3 p, gq3 x) {
  if (!on_path) return gq_mk(0.0f, 0.0f, 0.0f);
  return type == 1 ? gq_sq_cross(a, gq_sq_sub(x, p)) : a;
}

// The contact's travel s = max(sqrt(dist_sq + eps), tau) and its motion d = n s (world frame); n = outward object normal.
__device__ __forceinline__ gq3 gq_squeeze_dir(float dist_sq, gq3 n, float tau, float& s, bool& free_travel) {
  const float dist = sqrtf(dist_sq + GQ_SQ_EPS);
  free_travel = dist > tau;  // false at the clamp: no gradient to the contact point
  s = free_travel ? dist : tau;
  return gq_mk(n.x * s, n.y * s, n.z * s);
}

// d_h = R' d, R row-major at R[0..8]
__device__ __forceinline__ gq3 gq_squeeze_to_hand(const float* R, gq3 d) {
  return gq_mk(fmaf(R[0], d.x, fmaf(R[3], d.y, R[6] * d.z)), fmaf(R[1], d.x, fmaf(R[4], d.y, R[7] * d.z)),
               fmaf(R[2], d.x, fmaf(R[5], d.y, R[8] * d.z)));
}
// R v
__device__ __forceinline__ gq3 gq_squeeze_to_world(const float* R, gq3 v) {
  return gq_mk(fmaf(R[0], v.x, fmaf(R[1], v.y, R[2] * v.z)), fmaf(R[3], v.x, fmaf(R[4], v.y, R[5] * v.z)),
               fmaf(R[6], v.x, fmaf(R[7], v.y, R[8] * v.z)));
}

// One contact's share of (J'J)[i][j] and of (J'd_h)[j], in fp64 on exact products of the fp32 columns
__device__ __forceinline__ double gq_squeeze_gram(gq3 ci, gq3 cj) {
  return (double)ci.x * (double)cj.x + (double)ci.y * (double)cj.y + (double)ci.z * (double)cj.z;
}

// Left-looking Cholesky, entry (i, k), i >= k, of column k: A[i][k] - sum_{j<k} L[i][j] L[k][j] in ascending j.  The columns
// before k hold L already.  The caller takes the square root of entry (k, k) and divides the entries below it by that root.
__device__ __forceinline__ double gq_squeeze_chol_dot(const double* A, int LD, int i, int k) {
  double s = A[(size_t)i * LD + k];
  for (int j = 0; j < k; ++j) s -= A[(size_t)i * LD + j] * A[(size_t)k * LD + j];
  return s;
}

// Substitution step k as the owner of entry i sees it: entry k becomes the solution value y_k (the caller passes
// y_k = b_k * (1 / L[k][k]), the reciprocal taken once per row of the factor), the entries still open lose their share coef * y_k (forward: coef = L[i][k], i > k; backward: L[k][i], i < k)
__device__ __forceinline__ double gq_squeeze_sub(double b, double coef, double yk) { return b - coef * yk; }

// Residual of one contact: r = J theta - d_h, from the three row sums ee = J theta
__device__ __forceinline__ gq3 gq_squeeze_resid(gq3 ee, gq3 dh) { return gq_sq_sub(ee, dh); }

// Joint k's share of sum_j G_ij . dJ_ij/dtheta_k for the contact at x, G_ij = theta_j v - u_j r (the rank-two dE/dJ, never
// stored), with the kinematic Hessian in closed form.  The walk goes from the node `start` the contact's link rides on towards
// the base (parent[]); joint k is on that path.  type / a3 / p3: joint types, axes and origins (hand frame) of all tree joints;
// tt / ut: theta and u spread to the tree joints.  For another joint j on the path:
//   j below k (passed not yet set): everything below k turns about a_k (revolute k): dJ = a_k x J_ij; prismatic k: 0
//   j == k, revolute:               dJ = a_k x (a_k x (x - p_k))
//   j above k:                      only x moves, by a_k x (x - p_k) (revolute k) or a_k: dJ = a_j x dx for a revolute j, else 0
__device__ __forceinline__ float gq_squeeze_hess(int k, int start, const int* parent, const int* type, const float* a3,
                                                 const float* p3, gq3 x, gq3 v, gq3 r, const float* tt, const float* ut) {
  const int tk = type[k];
  const gq3 ak = gq_mk(a3[k * 3], a3[k * 3 + 1], a3[k * 3 + 2]), pk = gq_mk(p3[k * 3], p3[k * 3 + 1], p3[k * 3 + 2]);
  float acc = 0.0f;
  bool passed = false;
  for (int j = start; j >= 0; j = parent[j]) {
    const gq3 aj = gq_mk(a3[j * 3], a3[j * 3 + 1], a3[j * 3 + 2]), pj = gq_mk(p3[j * 3], p3[j * 3 + 1], p3[j * 3 + 2]);
    const float tj = tt[j], uj = ut[j];
    const gq3 G = gq_mk(fmaf(tj, v.x, -(uj * r.x)), fmaf(tj, v.y, -(uj * r.y)), fmaf(tj, v.z, -(uj * r.z)));
    const bool jrev = type[j] == 1;
    gq3 dJ = gq_mk(0.0f, 0.0f, 0.0f);
    if (j == k) {
      passed = true;
      if (jrev) dJ = gq_sq_cross(aj, gq_sq_cross(aj, gq_sq_sub(x, pj)));
    } else if (!passed) {
      if (tk == 1) dJ = gq_sq_cross(ak, jrev ? gq_sq_cross(aj, gq_sq_sub(x, pj)) : aj);
    } else {
      if (jrev) dJ = gq_sq_cross(aj, tk == 1 ? gq_sq_cross(ak, gq_sq_sub(x, pk)) : ak);
    }
    acc += gq_sq_dot(G, dJ);
  }
  return acc;
}

// dE/dp of one contact: (n . R(-v)) [s > tau] (p - closest) / sqrt(dist_sq + eps); the normals are constants
__device__ __forceinline__ gq3 gq_squeeze_gp(const float* R, gq3 n, gq3 v, bool free_travel, float dist_sq, gq3 p, gq3 closest) {
  if (!free_travel) return gq_mk(0.0f, 0.0f, 0.0f);
  const gq3 gw = gq_squeeze_to_world(R, gq_mk(-v.x, -v.y, -v.z));
  const float k = gq_sq_dot(n, gw) / sqrtf(dist_sq + GQ_SQ_EPS);
  return gq_mk(k * (p.x - closest.x), k * (p.y - closest.y), k * (p.z - closest.z));
}
