// Device body of the scene term (include/graspqp_hip.h, "scene obstacles"): cell, weights, value and gradient of the
// trilinear interpolant of a signed-distance grid at one world point.  gq_scene_kernel (one block per row, lane = hand
// surface sample) and gq_scene_query_kernel (lane = query point) both call gq_scene_sample, with explicit fmaf, so the two
// routes agree bit for bit on the same point.
#pragma once
#include "grid_stack.h"  // gq_finite; common.h unless tests/scene_body_host.cpp compiles this body for the host (GQ_SCENE_HOST_BUILD)

enum { GQ_SCENE_OUTSIDE = 0, GQ_SCENE_INSIDE = 1, GQ_SCENE_NONFINITE = 2 };

// The range test 0 <= u <= n - 1 of one axis, made on exact quantities: in float the difference x - origin rounds, and a
// point one ulp beyond the last node plane would pass as u = n - 1.  x >= origin is exact as it stands; x - origin and
// h (n - 1) are exact in double (24-bit operands, n - 1 < 2^28).  False for a NaN.
__device__ __forceinline__ bool gq_scene_axis_in(float x, float o, float h, int n) {
  return x >= o && (double)x - (double)o <= (double)h * (double)(n - 1);
}

// Cell index along one axis.  The point has passed the range test (so `u` is finite and in [0, n - 1] up to one rounding):
// floor, then the clamp to [0, n - 2] IN FLOAT, then the conversion -- the int never comes from a value outside the grid.
// The second clamp, on the int, matters only for n > 2^24, where (float)(n - 2) may round up.
__device__ __forceinline__ int gq_scene_axis(float u, int n, float& f) {
  const float c = fmaxf(fminf(floorf(u), (float)(n - 2)), 0.0f);
  const int i = min((int)c, n - 2);
  f = u - (float)i;  // in [0,1] (up to one rounding above 1 on the last plane); exact for n <= 2^24 (Sterbenz, or u < 1)
  return i;
}

// phi and grad phi of the grid at x.  -> GQ_SCENE_INSIDE (phi / grad written), GQ_SCENE_OUTSIDE (free space; nothing is
// loaded, phi / grad untouched) or GQ_SCENE_NONFINITE (x has a NaN or inf coordinate; nothing is loaded).
// The tests come first and are written positively: a NaN fails every comparison and so never reaches the conversion.
__device__ __forceinline__ int gq_scene_sample(const gqSceneGrid& g, gq3 x, float& phi, gq3& grad) {
  if (!(gq_finite(x.x) && gq_finite(x.y) && gq_finite(x.z))) return GQ_SCENE_NONFINITE;
  if (!(gq_scene_axis_in(x.x, g.origin[0], g.voxel, g.nx) && gq_scene_axis_in(x.y, g.origin[1], g.voxel, g.ny) &&
        gq_scene_axis_in(x.z, g.origin[2], g.voxel, g.nz)))
    return GQ_SCENE_OUTSIDE;
  // inside: 0 <= x - origin <= h (n - 1), so u is finite, >= 0 and at most one rounding above n - 1
  const float ux = (x.x - g.origin[0]) / g.voxel, uy = (x.y - g.origin[1]) / g.voxel, uz = (x.z - g.origin[2]) / g.voxel;
  float fx, fy, fz;
  const int ix = gq_scene_axis(ux, g.nx, fx), iy = gq_scene_axis(uy, g.ny, fy), iz = gq_scene_axis(uz, g.nz, fz);
  // 0 <= ix <= nx-2 etc., nx ny nz <= 2^28: the largest index below, base + sx + sy + 1, is nx ny nz - 1
  const int sy = g.nz, sx = g.ny * g.nz;
  const float* v = g.values + ((ix * g.ny + iy) * g.nz + iz);
  // the 8 nodes of the cell, issued together before any is used
  const float v000 = v[0], v001 = v[1], v010 = v[sy], v011 = v[sy + 1];
  const float v100 = v[sx], v101 = v[sx + 1], v110 = v[sx + sy], v111 = v[sx + sy + 1];
  const float d00 = v001 - v000, d01 = v011 - v010, d10 = v101 - v100, d11 = v111 - v110;  // along z
  const float c00 = fmaf(fz, d00, v000), c01 = fmaf(fz, d01, v010), c10 = fmaf(fz, d10, v100), c11 = fmaf(fz, d11, v110);
  const float e0 = c01 - c00, e1 = c11 - c10;  // along y, at x = 0 / 1
  const float c0 = fmaf(fy, e0, c00), c1 = fmaf(fy, e1, c10);
  phi = fmaf(fx, c1 - c0, c0);
  const float dz0 = fmaf(fy, d01 - d00, d00), dz1 = fmaf(fy, d11 - d10, d10);
  grad = gq_mk((c1 - c0) / g.voxel, fmaf(fx, e1 - e0, e0) / g.voxel, fmaf(fx, dz1 - dz0, dz0) / g.voxel);
  return GQ_SCENE_INSIDE;
}
