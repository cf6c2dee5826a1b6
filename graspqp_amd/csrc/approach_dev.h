// Device body of the approach term (include/graspqp_hip.h, "approach clearance"): the stations of ONE hand surface sample.
// gq_approach_kernel calls it once per sample; tests/approach_body_host.cpp compiles it for the host, as scene_dev.h's body.
//
// Two forms of the same loop, the same bits at the same inputs (tests/test_approach_body_host.py builds both):
//  - the default calls gq_scene_sample (scene_dev.h) once per station: it locates, loads and interpolates in one body, so a lane
//    waits for a station's gathers before it can address the next;
//  - with -DGQ_APPROACH_ROTATED (a variant build: GQ_EXTRA_FLAGS / GQ_OUT_DIR of build.sh) the same steps are three pieces --
//    gq_ap_locate (the tests and the cell, by gq_finite and scene_dev.h's own gq_scene_axis_in / gq_scene_axis), gq_ap_load
//    (the 8 nodes) and gq_ap_interp (the fmaf chains of gq_scene_sample, copied term for term) -- and the loop is rotated: the
//    loads of station k + 1 are issued before station k's are interpolated and consumed.  DESIGN 15 has both code objects'
//    figures and the launch times.
#pragma once
#include "scene_dev.h"

#ifdef GQ_APPROACH_ROTATED
struct GqApCell {
  const float* v;    // first node of the cell; only meaningful when where == GQ_SCENE_INSIDE
  float fx, fy, fz;  // weights
  int where;
};
struct GqApNodes {
  float v000, v001, v010, v011, v100, v101, v110, v111;
};

// the order of gq_scene_sample: finiteness, the exact range test, then floor / clamp / conversion; nothing is loaded here
__device__ __forceinline__ GqApCell gq_ap_locate(const gqSceneGrid& g, gq3 x) {
  GqApCell c;
  c.v = g.values, c.fx = c.fy = c.fz = 0.0f;
  if (!(gq_finite(x.x) && gq_finite(x.y) && gq_finite(x.z))) {
    c.where = GQ_SCENE_NONFINITE;
    return c;
  }
  if (!(gq_scene_axis_in(x.x, g.origin[0], g.voxel, g.nx) && gq_scene_axis_in(x.y, g.origin[1], g.voxel, g.ny) &&
        gq_scene_axis_in(x.z, g.origin[2], g.voxel, g.nz))) {
    c.where = GQ_SCENE_OUTSIDE;
    return c;
  }
  const float ux = (x.x - g.origin[0]) / g.voxel, uy = (x.y - g.origin[1]) / g.voxel, uz = (x.z - g.origin[2]) / g.voxel;
  const int ix = gq_scene_axis(ux, g.nx, c.fx), iy = gq_scene_axis(uy, g.ny, c.fy), iz = gq_scene_axis(uz, g.nz, c.fz);
  c.v = g.values + ((ix * g.ny + iy) * g.nz + iz);  // 0 <= ix <= nx-2 etc.: the largest index read is nx ny nz - 1
  c.where = GQ_SCENE_INSIDE;
  return c;
}

// the 8 nodes of the cell, issued together; a point that is not inside the volume loads nothing
__device__ __forceinline__ void gq_ap_load(const gqSceneGrid& g, const GqApCell& c, GqApNodes& n) {
  if (c.where != GQ_SCENE_INSIDE) return;
  const int sy = g.nz, sx = g.ny * g.nz;
  const float* v = c.v;
  n.v000 = v[0], n.v001 = v[1], n.v010 = v[sy], n.v011 = v[sy + 1];
  n.v100 = v[sx], n.v101 = v[sx + 1], n.v110 = v[sx + sy], n.v111 = v[sx + sy + 1];
}

// value and gradient of the trilinear interpolant: gq_scene_sample's expressions
__device__ __forceinline__ void gq_ap_interp(const gqSceneGrid& g, const GqApCell& c, const GqApNodes& n, float& phi, gq3& grad) {
  const float fx = c.fx, fy = c.fy, fz = c.fz;
  const float d00 = n.v001 - n.v000, d01 = n.v011 - n.v010, d10 = n.v101 - n.v100, d11 = n.v111 - n.v110;  // along z
  const float c00 = fmaf(fz, d00, n.v000), c01 = fmaf(fz, d01, n.v010), c10 = fmaf(fz, d10, n.v100), c11 = fmaf(fz, d11, n.v110);
  const float e0 = c01 - c00, e1 = c11 - c10;  // along y, at x = 0 / 1
  const float c0 = fmaf(fy, e0, c00), c1 = fmaf(fy, e1, c10);
  phi = fmaf(fx, c1 - c0, c0);
  const float dz0 = fmaf(fy, d01 - d00, d00), dz1 = fmaf(fy, d11 - d10, d10);
  grad = gq_mk((c1 - c0) / g.voxel, fmaf(fx, e1 - e0, e0) / g.voxel, fmaf(fx, dz1 - dz0, dz0) / g.voxel);
}

// station k of the sample: y = x_h - d_k a (hand frame), x_w = R y + t
__device__ __forceinline__ gq3 gq_ap_station(gq3 xh, gq3 a, float distance, int k, float fK, gq3 r1, gq3 r2, gq3 r3, gq3 t, gq3& y) {
  const float d = distance * (float)k / fK;
  y = gq_mk(fmaf(-d, a.x, xh.x), fmaf(-d, a.y, xh.y), fmaf(-d, a.z, xh.z));
  return gq_mk(fmaf(r1.x, y.x, fmaf(r1.y, y.y, r1.z * y.z)) + t.x, fmaf(r2.x, y.x, fmaf(r2.y, y.y, r2.z * y.z)) + t.y,
               fmaf(r3.x, y.x, fmaf(r3.y, y.y, r3.z * y.z)) + t.z);
}

#endif

// x_h: the sample in the hand frame; a: approach axis (hand frame); r1..r3: rows of R; t: translation.  For k = 1..n_stations in
// ascending order: d_k = distance k / n_stations, y_k = x_h - d_k a, x_w = R y_k + t, phi by gq_scene_sample; an active station
// (inside the volume, phi < margin, or a non-finite point: NaN) adds margin - phi to e, g_h = R' (-grad phi) to G and
// g_h (x) y_k to K9 (row-major).  The upstream factor and 1/n_stations are the caller's, at the fold.
#ifndef GQ_APPROACH_ROTATED
__device__ __forceinline__ void gq_approach_stations(const gqSceneGrid& grid, gq3 xh, gq3 a, gq3 r1, gq3 r2, gq3 r3, gq3 t,
                                                     float distance, int n_stations, float margin, float& e, gq3& G, float* K9) {
  const float fK = (float)n_stations;
  for (int k = 1; k <= n_stations; ++k) {
    const float d = distance * (float)k / fK;
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
#else
__device__ __forceinline__ void gq_approach_stations(const gqSceneGrid& grid, gq3 xh, gq3 a, gq3 r1, gq3 r2, gq3 r3, gq3 t,
                                                     float distance, int n_stations, float margin, float& e, gq3& G, float* K9) {
  const float fK = (float)n_stations;
  gq3 y_next;
  GqApCell c_next = gq_ap_locate(grid, gq_ap_station(xh, a, distance, 1, fK, r1, r2, r3, t, y_next));
  GqApNodes n_next = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  gq_ap_load(grid, c_next, n_next);
  for (int k = 1; k <= n_stations; ++k) {
    const gq3 y = y_next;
    const GqApCell c = c_next;
    const GqApNodes n = n_next;
    if (k < n_stations) {  // station k + 1: located and its loads issued before station k's are used
      c_next = gq_ap_locate(grid, gq_ap_station(xh, a, distance, k + 1, fK, r1, r2, r3, t, y_next));
      gq_ap_load(grid, c_next, n_next);
    }
    float phi = GQ_INF_F;
    gq3 gp = gq_mk(0, 0, 0);
    if (c.where == GQ_SCENE_INSIDE) gq_ap_interp(grid, c, n, phi, gp);
    if (c.where == GQ_SCENE_NONFINITE) phi = gp.x = gp.y = gp.z = __builtin_nanf("");  // the row's energy and gradient: NaN
    if (c.where != GQ_SCENE_OUTSIDE && !(phi >= margin)) {
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
#endif
