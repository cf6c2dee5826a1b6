// Device body of the TSDF surfel extraction (include/graspqp_hip.h, "target objects from depth images"): the zero level set of
// ONE grid of a fused stack as an oriented point cloud.  The kernels of surfel.hip call it on a tile in LDS; tests/
// surfel_body_host.cpp compiles it for the host, as tsdf_dev.h's body.
//
// A block is a tile of GQ_CL_TX x GQ_CL_TY x GQ_CL_TZ nodes (grid_stack.h), thread tid = (li GQ_CL_TY + lj) GQ_CL_TZ + lk owns node
// a = tile origin + (li,lj,lk) and its three edges to b = a + e_c.  The tile holds D with a halo of -1 .. +2 nodes on every axis, NaN where
// the node is not observed (outside the grid, D not finite, W < min_weight), so `observed` is v == v from then on.
//   crossing: a and b in the region, both observed, (D_a >= 0) != (D_b >= 0), |D_a| < trunc and |D_b| < trunc   (exact tests)
//   t = D_a / (D_a - D_b) in [0,1]      p = x_a + t voxel e_c, x_a = fmaf(voxel, (i,j,k), origin)
//   d_c(m) = (D(m+e_c) - D(m-e_c)) / 2, one-sided where only one neighbour is observed, 0 where neither is
//   g_c(n) = sum w d_c(m) / sum w over the observed m of the 3 x 3 neighbourhood of n transverse to c, w = (1,2,1) x (1,2,1)
//   n = normalize((1 - t) g(a) + t g(b)); e_c sign(D_b - D_a) unless |.|^2 > 1e-20
// D is positive in free space, so the gradient points outward.  Every index is formed after its range test.
#pragma once
#include "clutter_dev.h"

#define GQ_SF_LO 1  // halo below the tile
#define GQ_SF_HI 2  // halo above it
#define GQ_SF_NX (GQ_CL_TX + GQ_SF_LO + GQ_SF_HI)
#define GQ_SF_NY (GQ_CL_TY + GQ_SF_LO + GQ_SF_HI)
#define GQ_SF_NZ (GQ_CL_TZ + GQ_SF_LO + GQ_SF_HI)
#define GQ_SF_TILE (GQ_SF_NX * GQ_SF_NY * GQ_SF_NZ)
#define GQ_SF_THREADS GQ_CL_THREADS
#define GQ_SF_MIN_NORM2 1e-20f

// what a launch reads of one grid: `values` / `weight` are THIS grid's (weight null: every node observed)
struct gqSurfelGrid {
  gqSceneGrid grid;
  const float* weight;
  float min_weight, trunc;
  int region[6];  // i0 i1 j0 j1 k0 k1, half-open, inside the grid
};
// grid g's view of a launch whose `first` is grid 0's: values and weight advance by the nodes of a grid (g < n_grids)
__device__ __forceinline__ gqSurfelGrid gq_surfel_of(const gqSurfelGrid& first, size_t g) {
  gqSurfelGrid s = first;
  s.grid = gq_stack_grid(first.grid, g);
  if (s.weight) s.weight = gq_stack_plane(first.weight, gq_stack_nodes(first.grid), g);
  return s;
}

// offset in the tile of the node at (li,lj,lk) relative to the tile's first node; each in -GQ_SF_LO .. T + GQ_SF_HI - 1
__device__ __forceinline__ int gq_surfel_at(int li, int lj, int lk) {
  return ((li + GQ_SF_LO) * GQ_SF_NY + (lj + GQ_SF_LO)) * GQ_SF_NZ + (lk + GQ_SF_LO);
}
__device__ __forceinline__ int gq_surfel_stride(int c) { return c == 0 ? GQ_SF_NY * GQ_SF_NZ : c == 1 ? GQ_SF_NZ : 1; }
__device__ __forceinline__ bool gq_surfel_seen(float v) { return v == v; }

// D of node (i,j,k) if it is observed, else NaN.  The range test precedes the index; nx ny nz <= 2^28.
__device__ __forceinline__ float gq_surfel_node(const gqSurfelGrid& s, int i, int j, int k) {
  if (!(i >= 0 && i < s.grid.nx && j >= 0 && j < s.grid.ny && k >= 0 && k < s.grid.nz)) return __builtin_nanf("");
  const size_t node = ((size_t)i * (size_t)s.grid.ny + (size_t)j) * (size_t)s.grid.nz + (size_t)k;
  const float D = s.grid.values[node];
  bool seen = gq_finite(D);
  if (s.weight) seen = seen && s.weight[node] >= s.min_weight;  // false for a NaN weight
  return seen ? D : __builtin_nanf("");
}

// Number of tile entries with every local coordinate in -lo .. T + hi - 1, and the e-th of them filled (e < that number).
__device__ __forceinline__ int gq_surfel_entries(int lo, int hi) {
  return (GQ_CL_TX + lo + hi) * (GQ_CL_TY + lo + hi) * (GQ_CL_TZ + lo + hi);
}
__device__ __forceinline__ void gq_surfel_fill(const gqSurfelGrid& s, int i0, int j0, int k0, int lo, int hi, int e, float* tile) {
  const int nz = GQ_CL_TZ + lo + hi, ny = GQ_CL_TY + lo + hi;
  const int lk = e % nz - lo, lj = (e / nz) % ny - lo, li = e / (nz * ny) - lo;
  tile[gq_surfel_at(li, lj, lk)] = gq_surfel_node(s, i0 + li, j0 + lj, k0 + lk);
}

// Bit c set: the edge from the thread's node along axis c is a crossing.  Reads the tile at local 0 .. T on every axis.
__device__ __forceinline__ unsigned gq_surfel_flags(const gqSurfelGrid& s, const float* tile, int i0, int j0, int k0, int tid) {
  int li, lj, lk;
  gq_tile_local(tid, li, lj, lk);
  const int n[3] = {i0 + li, j0 + lj, k0 + lk};
  const int* r = s.region;
  if (!(n[0] >= r[0] && n[0] < r[1] && n[1] >= r[2] && n[1] < r[3] && n[2] >= r[4] && n[2] < r[5])) return 0u;
  const int at = gq_surfel_at(li, lj, lk);
  const float Da = tile[at];
  if (!(gq_surfel_seen(Da) && fabsf(Da) < s.trunc)) return 0u;
  unsigned flags = 0u;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!(n[c] + 1 < r[2 * c + 1])) continue;  // b outside the region
    const float Db = tile[at + gq_surfel_stride(c)];
    if (gq_surfel_seen(Db) && fabsf(Db) < s.trunc && ((Da >= 0.0f) != (Db >= 0.0f))) flags |= 1u << c;
  }
  return flags;
}

// d_c of the observed node at tile offset m (sc = the stride of c)
__device__ __forceinline__ float gq_surfel_diff(const float* tile, int m, int sc) {
  const float lo = tile[m - sc], hi = tile[m + sc];
  const bool a = gq_surfel_seen(lo), b = gq_surfel_seen(hi);
  if (a && b) return 0.5f * (hi - lo);
  if (b) return hi - tile[m];
  if (a) return tile[m] - lo;
  return 0.0f;
}

// g of the observed node at tile offset n: per axis c the (1,2,1) x (1,2,1) mean of d_c over the observed nodes of the plane
// through n transverse to c, the lower of the two other axes outermost.  The weight of n itself is 4, so the sum is >= 4.
__device__ __forceinline__ gq3 gq_surfel_grad(const float* tile, int n) {
  float g[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = gq_surfel_stride(c), su = gq_surfel_stride(c == 0 ? 1 : 0), sv = gq_surfel_stride(c == 2 ? 1 : 2);
    float num = 0.0f, den = 0.0f;
    for (int du = -1; du <= 1; ++du)
      for (int dv = -1; dv <= 1; ++dv) {
        const int m = n + du * su + dv * sv;
        if (!gq_surfel_seen(tile[m])) continue;
        const float w = (float)((2 - (du < 0 ? -du : du)) * (2 - (dv < 0 ? -dv : dv)));
        num = fmaf(w, gq_surfel_diff(tile, m, sc), num);
        den += w;
      }
    g[c] = num / den;
  }
  return gq_mk(g[0], g[1], g[2]);
}

// Position and unit outward normal of the crossing along axis c of the thread's node (bit c of gq_surfel_flags is set).
__device__ __forceinline__ void gq_surfel_emit(const gqSurfelGrid& s, const float* tile, int i0, int j0, int k0, int tid, int c, float* p,
                                               float* nrm) {
  int li, lj, lk;
  gq_tile_local(tid, li, lj, lk);
  const int a = gq_surfel_at(li, lj, lk), b = a + gq_surfel_stride(c);
  const float Da = tile[a], Db = tile[b];
  const float t = Da / (Da - Db);  // the signs differ: the denominator is not 0, t is in [0,1]
  p[0] = fmaf(s.grid.voxel, (float)(i0 + li), s.grid.origin[0]);  // x_a, the chain of gq_clutter_world's x_f
  p[1] = fmaf(s.grid.voxel, (float)(j0 + lj), s.grid.origin[1]);
  p[2] = fmaf(s.grid.voxel, (float)(k0 + lk), s.grid.origin[2]);
  p[c] = fmaf(t, s.grid.voxel, p[c]);
  const gq3 ga = gq_surfel_grad(tile, a), gb = gq_surfel_grad(tile, b);
  const float u = 1.0f - t;
  const gq3 v = gq_mk(fmaf(t, gb.x, u * ga.x), fmaf(t, gb.y, u * ga.y), fmaf(t, gb.z, u * ga.z));
  const float n2 = fmaf(v.x, v.x, fmaf(v.y, v.y, v.z * v.z));
  if (n2 > GQ_SF_MIN_NORM2) {
    const float inv = 1.0f / sqrtf(n2);
    nrm[0] = v.x * inv, nrm[1] = v.y * inv, nrm[2] = v.z * inv;
  } else {  // also a NaN: the count never depends on this decision
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    nrm[c] = Db > Da ? 1.0f : -1.0f;
  }
}
