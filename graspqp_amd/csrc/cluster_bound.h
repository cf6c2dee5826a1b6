// The bound of the pruned cluster search (sdf_dev.h: gq_sdf_wave_query), both halves in one place: how gq_meshset_create orders
// a mesh's faces along the Morton curve and boxes every 64 of them (host, set-up time), and the lower bound the query wavefronts
// evaluate from such a box (device, per step).  Nothing here needs the HIP runtime, so a host compiler accepts the file as it
// is: tests/cluster_bound_host.cpp builds it with sanitizers and tests/test_cluster_bound_host.py checks the one property the
// search relies on -- 0.9999 x the fp32 lower bound never exceeds the exact distance to a face of the cluster.
// The includer provides (common.h does; the host program defines its own): __device__, __forceinline__, float4, gq3, gq_mk.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

// ---- Morton order of a mesh's faces ------------------------------------------------------------------------------------
static inline uint32_t gq_spread10(uint32_t v) {
  v &= 0x3ff;
  v = (v | (v << 16)) & 0x030000ff;
  v = (v | (v << 8)) & 0x0300f00f;
  v = (v | (v << 4)) & 0x030c30c3;
  v = (v | (v << 2)) & 0x09249249;
  return v;
}

// box (lo.xyz, 0, hi.xyz, 0) of the faces perm[a..b)
static inline void gq_box_of(const float* fv, const int32_t* perm, int64_t a, int64_t b, float* out8) {
  float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
  for (int64_t i = a; i < b; ++i) {
    const float* v = fv + (int64_t)perm[i] * 9;
    for (int k = 0; k < 9; ++k) {
      const int c = k % 3;
      lo[c] = v[k] < lo[c] ? v[k] : lo[c];
      hi[c] = v[k] > hi[c] ? v[k] : hi[c];
    }
  }
  out8[0] = lo[0]; out8[1] = lo[1]; out8[2] = lo[2]; out8[3] = 0.0f;
  out8[4] = hi[0]; out8[5] = hi[1]; out8[6] = hi[2]; out8[7] = 0.0f;
}

// perm[begin..end) = the faces begin .. end-1 ordered along the 30-bit Morton curve of their centroids inside `box`
// (gq_box_of layout); faces with equal codes keep their index order
static inline void gq_morton_order(const float* fv, int32_t* perm, int64_t begin, int64_t end, const float* box) {
  std::vector<std::pair<uint32_t, int32_t>> keys;
  keys.reserve(end - begin);
  for (int64_t i = begin; i < end; ++i) {
    const float* v = fv + i * 9;
    uint32_t code = 0;
    for (int c = 0; c < 3; ++c) {
      const float ctr = (v[c] + v[3 + c] + v[6 + c]) * (1.0f / 3.0f);
      const float ext = box[4 + c] - box[c];
      float t = ext > 0.0f ? (ctr - box[c]) / ext : 0.0f;
      t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
      code |= gq_spread10((uint32_t)(t * 1023.0f)) << c;
    }
    keys.emplace_back(code, (int32_t)i);
  }
  std::stable_sort(keys.begin(), keys.end());
  for (int64_t i = begin; i < end; ++i) perm[i] = keys[i - begin].second;
}

// Bound of a 64-face cluster: an oriented box, 16 floats = [centre.xyz, h_u][u.xyz, h_v][v.xyz, h_n][n.xyz, 0].
// n = area-weighted mean normal of the patch, u = principal direction of its vertices in the plane orthogonal to n,
// v = n x u.  A Morton patch of a surface mesh is nearly planar, so the box is ~1 mm thick along n and hugs the patch
// laterally -- for a query point several centimetres away the neighbouring patches are only millimetres farther than
// the nearest one, and an axis-aligned box around a tilted patch is too loose to tell them apart.
static void gq_cluster_bound(const float* fv, const int32_t* perm, int64_t a, int64_t b, float* out16) {
  double n[3] = {0, 0, 0}, c0[3] = {0, 0, 0};
  for (int64_t i = a; i < b; ++i) {
    const float* v = fv + (int64_t)perm[i] * 9;
    const double e1[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
    const double e2[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
    n[0] += e1[1] * e2[2] - e1[2] * e2[1];
    n[1] += e1[2] * e2[0] - e1[0] * e2[2];
    n[2] += e1[0] * e2[1] - e1[1] * e2[0];
    for (int k = 0; k < 9; ++k) c0[k % 3] += v[k];
  }
  const double cnt = 3.0 * (double)(b - a);
  for (int k = 0; k < 3; ++k) c0[k] /= cnt;
  double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (len > 1e-30) {
    for (int k = 0; k < 3; ++k) n[k] /= len;
  } else {
    n[0] = 0; n[1] = 0; n[2] = 1;
  }
  // t1 orthogonal to n (drop the smallest component), t2 = n x t1
  double t1[3], t2[3];
  {
    const int m = (std::fabs(n[0]) <= std::fabs(n[1]) && std::fabs(n[0]) <= std::fabs(n[2])) ? 0
                  : (std::fabs(n[1]) <= std::fabs(n[2]) ? 1 : 2);
    double e[3] = {0, 0, 0};
    e[m] = 1.0;
    const double d = n[m];
    for (int k = 0; k < 3; ++k) t1[k] = e[k] - d * n[k];
    const double l = std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
    for (int k = 0; k < 3; ++k) t1[k] /= l;
    t2[0] = n[1] * t1[2] - n[2] * t1[1];
    t2[1] = n[2] * t1[0] - n[0] * t1[2];
    t2[2] = n[0] * t1[1] - n[1] * t1[0];
  }
  double cxx = 0, cxy = 0, cyy = 0;
  for (int64_t i = a; i < b; ++i) {
    const float* v = fv + (int64_t)perm[i] * 9;
    for (int c = 0; c < 3; ++c) {
      const double q[3] = {v[c * 3] - c0[0], v[c * 3 + 1] - c0[1], v[c * 3 + 2] - c0[2]};
      const double x = q[0] * t1[0] + q[1] * t1[1] + q[2] * t1[2], y = q[0] * t2[0] + q[1] * t2[1] + q[2] * t2[2];
      cxx += x * x;
      cxy += x * y;
      cyy += y * y;
    }
  }
  const double th = 0.5 * std::atan2(2.0 * cxy, cxx - cyy);
  float ax[3][3];  // u, v, n rounded to fp32 (the extents below are taken along the ROUNDED axes)
  for (int k = 0; k < 3; ++k) {
    ax[0][k] = (float)(std::cos(th) * t1[k] + std::sin(th) * t2[k]);
    ax[1][k] = (float)(-std::sin(th) * t1[k] + std::cos(th) * t2[k]);
    ax[2][k] = (float)n[k];
  }
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, mag = 0.0;
  for (int64_t i = a; i < b; ++i) {
    const float* v = fv + (int64_t)perm[i] * 9;
    for (int c = 0; c < 3; ++c) {
      const double q[3] = {v[c * 3] - c0[0], v[c * 3 + 1] - c0[1], v[c * 3 + 2] - c0[2]};
      for (int k = 0; k < 3; ++k) {
        const double s = q[0] * ax[k][0] + q[1] * ax[k][1] + q[2] * ax[k][2];
        lo[k] = s < lo[k] ? s : lo[k];
        hi[k] = s > hi[k] ? s : hi[k];
      }
      const double m = std::fabs((double)v[c * 3]) + std::fabs((double)v[c * 3 + 1]) + std::fabs((double)v[c * 3 + 2]);
      mag = m > mag ? m : mag;
    }
  }
  double ctr[3] = {c0[0], c0[1], c0[2]};
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 3; ++j) ctr[j] += 0.5 * (lo[k] + hi[k]) * ax[k][j];
  const double pad = 1e-6 * mag + 1e-12;  // fp32 evaluation on the device + rounding of the centre
  for (int k = 0; k < 3; ++k) {
    out16[k] = (float)ctr[k];
    out16[4 + k] = ax[0][k];
    out16[8 + k] = ax[1][k];
    out16[12 + k] = ax[2][k];
  }
  out16[3] = (float)(0.5 * (hi[0] - lo[0]) + pad);
  out16[7] = (float)(0.5 * (hi[1] - lo[1]) + pad);
  out16[11] = (float)(0.5 * (hi[2] - lo[2]) + pad);
  out16[15] = 0.0f;
}

// ---- the device side ---------------------------------------------------------------------------------------------------
// lower bound of the squared distance from p to any face of a cluster (oriented box of gq_cluster_bound)
__device__ __forceinline__ float gq_cluster_lb(const float* __restrict__ r, gq3 p) {
  const float4 c = *reinterpret_cast<const float4*>(r), u = *reinterpret_cast<const float4*>(r + 4),
               v = *reinterpret_cast<const float4*>(r + 8), n = *reinterpret_cast<const float4*>(r + 12);
  const gq3 d = gq_mk(p.x - c.x, p.y - c.y, p.z - c.z);
  const float eu = fmaxf(fabsf(fmaf(d.x, u.x, fmaf(d.y, u.y, d.z * u.z))) - c.w, 0.0f);
  const float ev = fmaxf(fabsf(fmaf(d.x, v.x, fmaf(d.y, v.y, d.z * v.z))) - u.w, 0.0f);
  const float en = fmaxf(fabsf(fmaf(d.x, n.x, fmaf(d.y, n.y, d.z * n.z))) - v.w, 0.0f);
  return fmaf(eu, eu, fmaf(ev, ev, en * en));
}
// the same bound from a box already in registers (gq_sdf_wave_prefetch)
__device__ __forceinline__ float gq_cluster_lb4(const float4 (&r)[4], gq3 p) {
  const gq3 d = gq_mk(p.x - r[0].x, p.y - r[0].y, p.z - r[0].z);
  const float eu = fmaxf(fabsf(fmaf(d.x, r[1].x, fmaf(d.y, r[1].y, d.z * r[1].z))) - r[0].w, 0.0f);
  const float ev = fmaxf(fabsf(fmaf(d.x, r[2].x, fmaf(d.y, r[2].y, d.z * r[2].z))) - r[1].w, 0.0f);
  const float en = fmaxf(fabsf(fmaf(d.x, r[3].x, fmaf(d.y, r[3].y, d.z * r[3].z))) - r[2].w, 0.0f);
  return fmaf(eu, eu, fmaf(ev, ev, en * en));
}
