// Device bodies of the pre-grasp term (include/graspqp_hip.h, "pre-grasp clearance"): what gq_pregrasp_kernel (pregrasp.hip) does
// per joint, per hand surface sample and per node of the tree, as plain functions of their operands.  tests/pregrasp_body_host.cpp
// compiles them for the host (as scene_dev.h's and approach_dev.h's bodies) and walks a block through them serially.  Only gq3 /
// gq_mk and scene_dev.h are needed: every product is written out, every fmaf is where the source says so.
#pragma once
#include "scene_dev.h"

// The opened joint value theta_o = (1 - alpha) theta + alpha q_o.  alpha = 0 gives theta and alpha = 1 gives q_o, both exactly.
__device__ __forceinline__ float gq_pregrasp_open(float theta, float q_open, float alpha) {
  return fmaf(alpha, q_open, (1.0f - alpha) * theta);
}

// The stations of ONE hand surface sample.  x_h: the sample in the hand frame at the opened joints; a: approach axis (hand frame);
// r1..r3: rows of R; t: translation.  For k = 0..n_stations in ascending order: d_k = distance k / n_stations (d_0 = 0, also for
// n_stations = 0, where it is the only station), y_k = x_h - d_k a, x_w = R y_k + t, phi by gq_scene_sample.  An active station
// (inside the volume and phi < margin, or a non-finite point: NaN) adds margin - phi to e, g_h = R' (-grad phi) to G and
// g_h (x) y_k to K9 (row-major).  Stations k >= 1 are gq_approach_stations' expressions term for term.  The upstream factor and
// 1/(n_stations + 1) are the caller's, at the fold.
__device__ __forceinline__ void gq_pregrasp_stations(const gqSceneGrid& grid, gq3 xh, gq3 a, gq3 r1, gq3 r2, gq3 r3, gq3 t,
                                                     float distance, int n_stations, float margin, float& e, gq3& G, float* K9) {
  const float fK = (float)n_stations;
  for (int k = 0; k <= n_stations; ++k) {
    const float d = k == 0 ? 0.0f : distance * (float)k / fK;
    const gq3 y = gq_mk(fmaf(-d, a.x, xh.x), fmaf(-d, a.y, xh.y), fmaf(-d, a.z, xh.z));
    const gq3 xw = gq_mk(fmaf(r1.x, y.x, fmaf(r1.y, y.y, r1.z * y.z)) + t.x, fmaf(r2.x, y.x, fmaf(r2.y, y.y, r2.z * y.z)) + t.y,
                         fmaf(r3.x, y.x, fmaf(r3.y, y.y, r3.z * y.z)) + t.z);
    float phi = GQ_INF_F;
    gq3 gp = gq_mk(0, 0, 0);
    const int where = gq_scene_sample(grid, xw, phi, gp);
    if (where == GQ_SCENE_NONFINITE) phi = gp.x = gp.y = gp.z = __builtin_nanf("");  // the row's energy and gradient: NaN
    if (where != GQ_SCENE_OUTSIDE && !(phi >= margin)) {
      e += margin - phi;
      const gq3 gh = gq_mk(-fmaf(r1.x, gp.x, fmaf(r2.x, gp.y, r3.x * gp.z)), -fmaf(r1.y, gp.x, fmaf(r2.y, gp.y, r3.y * gp.z)),
                           -fmaf(r1.z, gp.x, fmaf(r2.z, gp.y, r3.z * gp.z)));
      G.x += gh.x, G.y += gh.y, G.z += gh.z;
      K9[0] = fmaf(gh.x, y.x, K9[0]), K9[1] = fmaf(gh.x, y.y, K9[1]), K9[2] = fmaf(gh.x, y.z, K9[2]);
      K9[3] = fmaf(gh.y, y.x, K9[3]), K9[4] = fmaf(gh.y, y.y, K9[4]), K9[5] = fmaf(gh.y, y.z, K9[5]);
      K9[6] = fmaf(gh.z, y.x, K9[6]), K9[7] = fmaf(gh.z, y.y, K9[7]), K9[8] = fmaf(gh.z, y.z, K9[8]);
    }
  }
}

// x_h = T p for a 3x4 row-major [R|t] at T[0..11]
__device__ __forceinline__ gq3 gq_pregrasp_point(const float* T, gq3 p) {
  return gq_mk(fmaf(T[0], p.x, fmaf(T[1], p.y, fmaf(T[2], p.z, T[3]))), fmaf(T[4], p.x, fmaf(T[5], p.y, fmaf(T[6], p.z, T[7]))),
               fmaf(T[8], p.x, fmaf(T[9], p.y, fmaf(T[10], p.z, T[11]))));
}

// The moment of the sample's pull about the hand origin: x_h x G
__device__ __forceinline__ gq3 gq_pregrasp_moment(gq3 xh, gq3 G) {
  return gq_mk(xh.y * G.z - xh.z * G.y, xh.z * G.x - xh.x * G.z, xh.x * G.y - xh.y * G.x);
}

// Fold task (node j, component k): the sum, in link order, of component k of the wrenches of the links that ride on node j.
// link_node (L): link -> node, -1 for a link fixed to the hand's base (it moves with no joint); wrench (L,6).
__device__ __forceinline__ float gq_pregrasp_fold_links(int j, int k, const int* link_node, int L, const float* wrench) {
  float nf = 0.0f;
  for (int l = 0; l < L; ++l)
    if (link_node[l] == j) nf += wrench[l * 6 + k];
  return nf;
}

// ... and one level of the tree sweep for the same task: `own` plus component k of the children child_idx[c0..c1) of node j, in
// list order.  node_wrench (J,6) holds the finished sums of every deeper level.
__device__ __forceinline__ float gq_pregrasp_fold_children(float own, int k, const int* child_idx, int c0, int c1,
                                                           const float* node_wrench) {
  for (int c = c0; c < c1; ++c) own += node_wrench[child_idx[c] * 6 + k];
  return own;
}

// Joint torque of node j from its folded wrench (f, m about the hand origin): a . (m - o x f) for a revolute joint (type 1),
// a . f for a prismatic one; a = the joint axis and o = the joint origin, both in the hand frame at the opened joints.
__device__ __forceinline__ float gq_pregrasp_torque(int type, gq3 a, gq3 o, gq3 f, gq3 m) {
  if (type != 1) return fmaf(a.x, f.x, fmaf(a.y, f.y, a.z * f.z));
  const gq3 c = gq_mk(o.y * f.z - o.z * f.y, o.z * f.x - o.x * f.z, o.x * f.y - o.y * f.x);
  const gq3 r = gq_mk(m.x - c.x, m.y - c.y, m.z - c.z);
  return fmaf(a.x, r.x, fmaf(a.y, r.y, a.z * r.z));
}
