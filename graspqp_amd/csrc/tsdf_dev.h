// Device body of the TSDF integration (include/graspqp_hip.h, "scenes from depth images"): ONE node of one grid of the stack,
// carried through every view of a batch of depth frames.  gq_tsdf_integrate_kernel (tsdf.hip) calls it; tests/
// tsdf_body_host.cpp compiles it for the host, as clutter_dev.h's body.
//
// The node's running truncated signed distance D and weight W stay in registers; views ascending, per view:
//   x_w = R_g x_f + t_g (gq_clutter_world; x_w = x_f without target poses)      x_c = R_c' (x_w - t_c) (gq_clutter_to_part)
//   z = x_c.z >= depth_min, else the view is skipped (before any division)
//   u = fx x_c.x / z + cx, v = fy x_c.y / z + cy; in the image iff -0.5 <= u < W - 0.5 and -0.5 <= v < H - 0.5, tested on the
//   floats; col = floor(u + 0.5), row = floor(v + 0.5); d = depth[view][row][col], valid iff depth_min <= d <= depth_max
//   s = trunc if the pixel carries the grid's skipped label; else sdf = d - z, skipped if sdf < -trunc, s = min(sdf, trunc)
//   D = (W D + s) / (W + 1)      W = min(W + 1, max_weight)
// Every range test is written positively and precedes the conversion and the load: a NaN fails it and never becomes an index.
#pragma once
#include "clutter_dev.h"

// x_f of gq_clutter_world, for a stack without target poses
__device__ __forceinline__ gq3 gq_tsdf_frame(const gqSceneGrid& out, float fi, float fj, float fk) {
  return gq_mk(fmaf(out.voxel, fi, out.origin[0]), fmaf(out.voxel, fj, out.origin[1]), fmaf(out.voxel, fk, out.origin[2]));
}

// Pixel index along one axis of a coordinate that has passed -0.5 <= u < n - 0.5.  u + 0.5 is then in [0, n] -- n itself only
// when the sum rounds up from just below it (n = 1: 0.5 - 2^-25 + 0.5 = 1.0f) -- so the conversion is of an in-range value, and
// the clamp on the int keeps that one rounding inside the image.
__device__ __forceinline__ int gq_tsdf_pixel(float u, int n) { return min((int)floorf(u + 0.5f), n - 1); }

// One view's update of (D, W) of the node at the finite world position xw.  skip < 0: no label is skipped; c.labels may be null.
__device__ __forceinline__ void gq_tsdf_view(const gqDepthViews& c, int view, gq3 xw, int skip, float trunc, float max_weight, float& D,
                                             float& W) {
  const gq3 xc = gq_clutter_to_part(c.cam_T + 12 * (size_t)view, xw);
  if (!(gq_finite(xc.x) && gq_finite(xc.y) && gq_finite(xc.z))) {
    D = __builtin_nanf("");  // sticky: every later mean keeps it; the weight is left alone
    return;
  }
  const float z = xc.z;
  if (!(z >= c.depth_min)) return;  // behind the camera or too close; depth_min > 0, so z divides safely below
  const float u = fmaf(c.fx, xc.x / z, c.cx), v = fmaf(c.fy, xc.y / z, c.cy);
  if (!(u >= -0.5f && u < (float)c.width - 0.5f && v >= -0.5f && v < (float)c.height - 0.5f)) return;  // also +-inf
  const int col = gq_tsdf_pixel(u, c.width), row = gq_tsdf_pixel(v, c.height);
  // 0 <= col < width, 0 <= row < height, view < n_views: the largest index is n_views height width - 1 (<= 2^32: size_t)
  const size_t pix = ((size_t)view * (size_t)c.height + (size_t)row) * (size_t)c.width + (size_t)col;
  const float d = c.depth[pix];
  if (!(d >= c.depth_min && d <= c.depth_max)) return;  // 0, negative, NaN, +inf: no measurement
  float s = trunc;  // the skipped label: the whole ray through the pixel is free
  if (!(c.labels && skip >= 0 && c.labels[pix] == skip)) {
    const float sdf = d - z;
    if (sdf < -trunc) return;  // behind the surface by more than the band: occluded
    s = fminf(sdf, trunc);
  }
  D = fmaf(W, D, s) / (W + 1.0f);
  W = fminf(W + 1.0f, max_weight);
}

// (D, W) of node (i,j,k) of the grid whose pose is Tg (null: the grid's frame is the world) after every view, ascending.
// A non-finite x_w makes D NaN and leaves W alone.
__device__ __forceinline__ void gq_tsdf_node(const gqSceneGrid& out, const float* Tg, int i, int j, int k, const gqDepthViews& c, int skip,
                                             float trunc, float max_weight, float& D, float& W) {
  const gq3 xw = Tg ? gq_clutter_world(out, Tg, (float)i, (float)j, (float)k) : gq_tsdf_frame(out, (float)i, (float)j, (float)k);
  if (!(gq_finite(xw.x) && gq_finite(xw.y) && gq_finite(xw.z))) {
    D = __builtin_nanf("");
    return;
  }
  for (int view = 0; view < c.n_views; ++view) gq_tsdf_view(c, view, xw, skip, trunc, max_weight, D, W);
}
