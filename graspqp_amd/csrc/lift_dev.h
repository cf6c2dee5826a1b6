// Device bodies of the lift term (include/graspqp_hip.h, "lift clearance"): the stations of ONE hand surface sample and of ONE
// point of the held object along the straight carry c = H u - D R a.  gq_lift_row (lift_row_dev.h) calls them once per sample /
// point; tests/lift_body_host.cpp compiles them for the host, as approach_dev.h's body.
//
// Station k = 1..K, ascending: d_k = D k / K, h_k = H k / K, both written as approach_dev.h writes its d.
//   hand    y_k = x_h - d_k a (hand frame), x_w^k = R y_k + t_k with t_k = fmaf(h_k, u, t) per axis: the approach body with the
//           translation moved up.  With H = 0 the fmaf returns t and every operation is gq_approach_stations', in its order.
//   object  x^{j,k} = p_j + h_k u - d_k R a, two fmaf per axis (the lift inside).  R a is formed once by the caller.
// phi by gq_scene_sample, unchanged.  The upstream factor and 1/K are the caller's, at the fold.
#pragma once
#include "scene_dev.h"

// x_h: the sample in the hand frame; a: approach axis (hand frame); r1..r3: rows of R; t: translation; u: lift direction (world).
// An active station (inside the volume, phi < margin, or a non-finite point: NaN) adds margin - phi to e, g_h = R' (-grad phi) to
// G and g_h (x) y_k to K9 (row-major): the world shift h_k u depends on nothing, so it adds nothing.
__device__ __forceinline__ void gq_lift_hand_stations(const gqSceneGrid& grid, gq3 xh, gq3 a, gq3 r1, gq3 r2, gq3 r3, gq3 t, gq3 u,
                                                      float height, float distance, int n_stations, float margin, float& e, gq3& G,
                                                      float* K9) {
  const float fK = (float)n_stations;
  for (int k = 1; k <= n_stations; ++k) {
    const float d = distance * (float)k / fK;
    const float h = height * (float)k / fK;
    const gq3 tk = gq_mk(fmaf(h, u.x, t.x), fmaf(h, u.y, t.y), fmaf(h, u.z, t.z));
    const gq3 y = gq_mk(fmaf(-d, a.x, xh.x), fmaf(-d, a.y, xh.y), fmaf(-d, a.z, xh.z));
    const gq3 xw = gq_mk(fmaf(r1.x, y.x, fmaf(r1.y, y.y, r1.z * y.z)) + tk.x, fmaf(r2.x, y.x, fmaf(r2.y, y.y, r2.z * y.z)) + tk.y,
                         fmaf(r3.x, y.x, fmaf(r3.y, y.y, r3.z * y.z)) + tk.z);
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

// R a, the approach direction in the world: what the object is drawn back along
__device__ __forceinline__ gq3 gq_lift_world_axis(gq3 a, gq3 r1, gq3 r2, gq3 r3) {
  return gq_mk(fmaf(r1.x, a.x, fmaf(r1.y, a.y, r1.z * a.z)), fmaf(r2.x, a.x, fmaf(r2.y, a.y, r2.z * a.z)),
               fmaf(r3.x, a.x, fmaf(r3.y, a.y, r3.z * a.z)));
}

// p: the object point (object frame = the grid's frame); Ra = gq_lift_world_axis.  An active station adds margin - phi to e (the
// caller feeds the row's energy and the object's share from it) and g_h (x) (-d_k a) to K9, nothing else: the translation does not
// move the object (no gsum) and no joint does (no wrench).  With D = 0 the added products are zeros: a value and no gradient.
__device__ __forceinline__ void gq_lift_object_stations(const gqSceneGrid& grid, gq3 p, gq3 a, gq3 Ra, gq3 r1, gq3 r2, gq3 r3, gq3 u,
                                                        float height, float distance, int n_stations, float margin, float& e,
                                                        float* K9) {
  const float fK = (float)n_stations;
  for (int k = 1; k <= n_stations; ++k) {
    const float d = distance * (float)k / fK;
    const float h = height * (float)k / fK;
    const gq3 x = gq_mk(fmaf(-d, Ra.x, fmaf(h, u.x, p.x)), fmaf(-d, Ra.y, fmaf(h, u.y, p.y)), fmaf(-d, Ra.z, fmaf(h, u.z, p.z)));
    float phi = GQ_INF_F;
    gq3 gp = gq_mk(0, 0, 0);
    const int where = gq_scene_sample(grid, x, phi, gp);
    if (where == GQ_SCENE_NONFINITE) phi = gp.x = gp.y = gp.z = __builtin_nanf("");
    if (where != GQ_SCENE_OUTSIDE && !(phi >= margin)) {
      e += margin - phi;
      const gq3 gh = gq_mk(-fmaf(r1.x, gp.x, fmaf(r2.x, gp.y, r3.x * gp.z)), -fmaf(r1.y, gp.x, fmaf(r2.y, gp.y, r3.y * gp.z)),
                           -fmaf(r1.z, gp.x, fmaf(r2.z, gp.y, r3.z * gp.z)));
      const gq3 y = gq_mk(-d * a.x, -d * a.y, -d * a.z);
      K9[0] = fmaf(gh.x, y.x, K9[0]), K9[1] = fmaf(gh.x, y.y, K9[1]), K9[2] = fmaf(gh.x, y.z, K9[2]);
      K9[3] = fmaf(gh.y, y.x, K9[3]), K9[4] = fmaf(gh.y, y.y, K9[4]), K9[5] = fmaf(gh.y, y.z, K9[5]);
      K9[6] = fmaf(gh.z, y.x, K9[6]), K9[7] = fmaf(gh.z, y.y, K9[7]), K9[8] = fmaf(gh.z, y.z, K9[8]);
    }
  }
}
