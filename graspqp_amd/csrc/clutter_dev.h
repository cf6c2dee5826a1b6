// Device body of the compose kernel (include/graspqp_hip.h, "clutter scenes"): ONE output node of one target grid, and the
// conservative test by which a block leaves out a part that none of its nodes can reach.  gq_clutter_compose_kernel
// (clutter.hip) calls both; tests/clutter_body_host.cpp compiles them for the host, as scene_dev.h's body.
//
// Poses are 12 floats, row-major [R|t]: R[a][b] = T[4a + b], t[a] = T[4a + 3], used as given (not re-orthonormalised).
//   x_f = origin + h (i,j,k)   one fmaf per axis
//   x_w = R_g x_f + t_g        fmaf chain, t innermost
//   q_p = R_p' (x_w - t_p)     the part-frame point
// phi = min(far, base(x_w) if inside, phi_p(q_p) if inside, p ascending, p != exclude), every phi by gq_scene_sample; a
// non-finite x_w or q_p, or a NaN among the sampled values, makes the node NaN.
#pragma once
#include "scene_dev.h"

#define GQ_CL_MAX_PARTS 32  // a block is a tile of one grid: GQ_CL_TX/TY/TZ and its decode are grid_stack.h's

__device__ __forceinline__ gq3 gq_clutter_world(const gqSceneGrid& out, const float* Tg, float fi, float fj, float fk) {
  const gq3 xf = gq_mk(fmaf(out.voxel, fi, out.origin[0]), fmaf(out.voxel, fj, out.origin[1]), fmaf(out.voxel, fk, out.origin[2]));
  return gq_mk(fmaf(Tg[0], xf.x, fmaf(Tg[1], xf.y, fmaf(Tg[2], xf.z, Tg[3]))),
               fmaf(Tg[4], xf.x, fmaf(Tg[5], xf.y, fmaf(Tg[6], xf.z, Tg[7]))),
               fmaf(Tg[8], xf.x, fmaf(Tg[9], xf.y, fmaf(Tg[10], xf.z, Tg[11]))));
}

__device__ __forceinline__ gq3 gq_clutter_to_part(const float* Tp, gq3 xw) {
  const gq3 d = gq_mk(xw.x - Tp[3], xw.y - Tp[7], xw.z - Tp[11]);
  return gq_mk(fmaf(Tp[0], d.x, fmaf(Tp[4], d.y, Tp[8] * d.z)), fmaf(Tp[1], d.x, fmaf(Tp[5], d.y, Tp[9] * d.z)),
               fmaf(Tp[2], d.x, fmaf(Tp[6], d.y, Tp[10] * d.z)));
}

// True only if NO node of the tile whose first node is (i0,j0,k0) can lie in the part's volume: the tile (unclipped, a box in
// the target frame) is mapped to the part frame by M = R_p' R_g, its exact axis-aligned bounds there are centre +- |M| half,
// and they are tested against the volume box with a slack far above the rounding of the per-node chain (1e-5 of a bound S on
// every intermediate magnitude; the chain's error is a few 6e-8 S).  Holds for any matrices, orthonormal or not.  Anything
// non-finite or huge answers false: those nodes take the per-node path, which makes them NaN.
__device__ __forceinline__ bool gq_clutter_culled(const gqSceneGrid& out, const float* Tg, int i0, int j0, int k0,
                                                  const gqSceneGrid& part, const float* Tp) {
  const float half[3] = {0.5f * out.voxel * (float)(GQ_CL_TX - 1), 0.5f * out.voxel * (float)(GQ_CL_TY - 1),
                         0.5f * out.voxel * (float)(GQ_CL_TZ - 1)};
  const float cf[3] = {fmaf(out.voxel, (float)i0, out.origin[0]) + half[0], fmaf(out.voxel, (float)j0, out.origin[1]) + half[1],
                       fmaf(out.voxel, (float)k0, out.origin[2]) + half[2]};
  float d[3], sumRg = 0.0f, sumRp = 0.0f, sumT = 0.0f;
  for (int a = 0; a < 3; ++a) {
    d[a] = fmaf(Tg[4 * a], cf[0], fmaf(Tg[4 * a + 1], cf[1], fmaf(Tg[4 * a + 2], cf[2], Tg[4 * a + 3]))) - Tp[4 * a + 3];
    sumT += fabsf(Tg[4 * a + 3]) + fabsf(Tp[4 * a + 3]);
    for (int b = 0; b < 3; ++b) sumRg += fabsf(Tg[4 * a + b]), sumRp += fabsf(Tp[4 * a + b]);
  }
  const float reach = fmaxf(fmaxf(fabsf(cf[0]), fabsf(cf[1])), fabsf(cf[2])) + half[2];  // half[2] is the largest
  const float S = (sumT + sumRg * reach) * fmaxf(sumRp, 1.0f);
  if (!(S < 1e30f)) return false;  // also a NaN
  const float slack = 1e-5f * S;
  const int n[3] = {part.nx, part.ny, part.nz};
  bool culled = false;
  for (int a = 0; a < 3; ++a) {
    const float c = fmaf(Tp[a], d[0], fmaf(Tp[4 + a], d[1], Tp[8 + a] * d[2]));
    float dev = slack;
    for (int b = 0; b < 3; ++b) {
      const float m = fmaf(Tp[a], Tg[b], fmaf(Tp[4 + a], Tg[4 + b], Tp[8 + a] * Tg[8 + b]));
      dev = fmaf(fabsf(m), half[b], dev);
    }
    if (!(fabsf(c) + dev < 1e30f)) return false;
    const float lo = part.origin[a], hi = fmaf(part.voxel, (float)(n[a] - 1), part.origin[a]);
    culled = culled || c - dev > hi || c + dev < lo;
  }
  return culled;
}

// phi of node (i,j,k) of the target grid whose pose is Tg.  live: bit p set = part p is sampled (the block's cull cleared the
// others).  exclude outside 0..n_parts-1 leaves no part out.  base may be null.
__device__ __forceinline__ float gq_clutter_node(const gqSceneGrid& out, const float* Tg, int i, int j, int k, const gqSceneGrid* parts,
                                                 int n_parts, const float* part_T, int exclude, unsigned live, const gqSceneGrid* base,
                                                 float far) {
  const gq3 xw = gq_clutter_world(out, Tg, (float)i, (float)j, (float)k);
  if (!(gq_finite(xw.x) && gq_finite(xw.y) && gq_finite(xw.z))) return __builtin_nanf("");
  float m = far;
  bool bad = false;
  gq3 unused = gq_mk(0, 0, 0);
  if (base) {
    float phi = GQ_INF_F;
    if (gq_scene_sample(*base, xw, phi, unused) == GQ_SCENE_INSIDE) {
      bad = bad || phi != phi;
      m = phi < m ? phi : m;
    }
  }
  for (int p = 0; p < n_parts; ++p) {
    if (p == exclude || !((live >> p) & 1u)) continue;
    float phi = GQ_INF_F;
    const int where = gq_scene_sample(parts[p], gq_clutter_to_part(part_T + 12 * p, xw), phi, unused);
    if (where == GQ_SCENE_NONFINITE) bad = true;
    if (where == GQ_SCENE_INSIDE) {
      bad = bad || phi != phi;
      m = phi < m ? phi : m;
    }
  }
  return bad ? __builtin_nanf("") : m;
}
