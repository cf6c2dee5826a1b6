// Device bodies of the Euclidean distance field of a TSDF stack (include/graspqp_hip.h, "Euclidean distance field from a fused
// TSDF"): the tile geometry of a pass and, per output node, the seed, the envelope and the finish.  The kernels of edt.hip call
// them on a tile in LDS; tests/esdf_body_host.cpp compiles them for the host, as surfel_dev.h's body.
//
// A pass works on lines of L nodes along its axis.  One grid is seen as (n_outer, L, n_inner) nodes, the line in the middle:
//   x: (1, nx, ny nz)      y: (nx, ny, nz)      z: (nx ny, nz, 1)
// A tile is GQ_EDT_LINES whole lines.  INNER tiles (x, y) take lines that are neighbours along the inner index, so a load of
// 16 lines at one position is one 64-byte segment, and keep them in LDS as [position][line].  OUTER tiles (z, n_inner = 1) take
// 16 consecutive lines, one contiguous piece of memory, and keep them as [line][position].  Either way the lanes of a
// wavefront read consecutive LDS words while they scan their windows.  Every node of a grid belongs to exactly one tile.
//   seed:     the line holds, per edge a -> a + 1, t = D_a / (D_a - D_b) where the edge is a crossing, +inf where it is not;
//             g(p) = distance along the line from node p to the nearest crossing on edges p - R - 1 .. p + R, +inf if none
//   envelope: out(p) = min over |m| <= R, 0 <= p + m < L of f(p + m) + m^2, scanned outward until m^2 >= the running best
//   finish:   phi from (e / h)^2 and D by the rules of the contract
// Every index is formed after its range test.
#pragma once
#include "grid_stack.h"  // gq_finite, the stack view; common.h unless tests/esdf_body_host.cpp compiles this for the host

#define GQ_EDT_LINES 16
#define GQ_EDT_THREADS 256
#define GQ_EDT_MAX_LINE 1024    // nodes along one axis: 16 lines of 1024 floats are the 64 KB of LDS a block may ask for
#define GQ_EDT_MAX_WINDOW 4096  // R: m^2 stays exact in an int and in a float

struct gqEdtPass {
  int n_outer, L, n_inner;  // the grid as the pass sees it
  int R;                    // window, >= 1
};

// tiles of one grid (what the launches ask for, per grid)
template <bool INNER>
GQ_HOST_DEVICE int gq_edt_tiles(const gqEdtPass& q) {
  const int per_outer = (q.n_inner + GQ_EDT_LINES - 1) / GQ_EDT_LINES;
  return INNER ? q.n_outer * per_outer : (q.n_outer + GQ_EDT_LINES - 1) / GQ_EDT_LINES;
}

// Where element e (0 <= e < GQ_EDT_LINES L) of tile `tile` lives: its position p on the line, its LDS word, its node within the
// grid.  -> false if the element's line lies beyond the grid (nothing may be loaded or stored for it).
template <bool INNER>
__device__ __forceinline__ bool gq_edt_locate(const gqEdtPass& q, int tile, int e, int& p, int& word, size_t& node) {
  if (INNER) {
    const int per_outer = (q.n_inner + GQ_EDT_LINES - 1) / GQ_EDT_LINES;
    const int o = tile / per_outer, col = (tile % per_outer) * GQ_EDT_LINES + e % GQ_EDT_LINES;
    p = e / GQ_EDT_LINES;
    word = e;  // p GQ_EDT_LINES + line
    if (col >= q.n_inner) return false;
    node = ((size_t)o * (size_t)q.L + (size_t)p) * (size_t)q.n_inner + (size_t)col;
    return true;
  }
  const int l = e / q.L, o = tile * GQ_EDT_LINES + l;
  p = e % q.L;
  word = e;  // line L + p
  if (o >= q.n_outer) return false;
  node = (size_t)o * (size_t)q.L + (size_t)p;
  return true;
}
// LDS word of position 0 of the element's line, and the stride of a step along the line
template <bool INNER>
__device__ __forceinline__ int gq_edt_line0(int word, int p) {
  return INNER ? word - p * GQ_EDT_LINES : word - p;
}
template <bool INNER>
__device__ __forceinline__ int gq_edt_stride() {
  return INNER ? GQ_EDT_LINES : 1;
}

// t of the edge from a node with value Da to the next with value Db: in [0,1] where the edge is a crossing (both ends finite,
// exactly one of them free, free = D >= 0), +inf where it is not.  The signs differ, so the denominator is not 0.
__device__ __forceinline__ float gq_edt_edge(float Da, float Db) {
  const bool cross = gq_finite(Da) && gq_finite(Db) && ((Da >= 0.0f) != (Db >= 0.0f));
  return cross ? Da / (Da - Db) : GQ_INF_F;
}

// g^2 of node p: line[a stride] = gq_edt_edge of edge a -> a + 1 for 0 <= a <= L - 2.  The nearest crossing below p is on the
// first crossing edge met going down from p - 1, the nearest above on the first met going up from p.
__device__ __forceinline__ float gq_edt_seed(const float* line, int stride, int L, int p, int R) {
  float g = GQ_INF_F;
  const int lo = p - R - 1 > 0 ? p - R - 1 : 0, hi = p + R < L - 2 ? p + R : L - 2;
  int a = p - 1;
  for (; a - 3 >= lo; a -= 4) {  // four edges per step, loaded together: the scan does not wait for one load per edge
    const float t0 = line[a * stride], t1 = line[(a - 1) * stride], t2 = line[(a - 2) * stride], t3 = line[(a - 3) * stride];
    const int j = t0 < GQ_INF_F ? 0 : t1 < GQ_INF_F ? 1 : t2 < GQ_INF_F ? 2 : t3 < GQ_INF_F ? 3 : -1;
    if (j >= 0) {
      g = (float)(p - a + j) - (j == 0 ? t0 : j == 1 ? t1 : j == 2 ? t2 : t3);  // the integer part first: exact
      a = lo - 1;
      break;
    }
  }
  for (; a >= lo; --a) {
    const float t = line[a * stride];
    if (t < GQ_INF_F) {
      g = (float)(p - a) - t;
      break;
    }
  }
  a = p;
  for (; a + 3 <= hi; a += 4) {
    const float t0 = line[a * stride], t1 = line[(a + 1) * stride], t2 = line[(a + 2) * stride], t3 = line[(a + 3) * stride];
    const int j = t0 < GQ_INF_F ? 0 : t1 < GQ_INF_F ? 1 : t2 < GQ_INF_F ? 2 : t3 < GQ_INF_F ? 3 : -1;
    if (j >= 0) {
      const float d = (float)(a - p + j) + (j == 0 ? t0 : j == 1 ? t1 : j == 2 ? t2 : t3);
      g = d < g ? d : g;
      a = hi + 1;
      break;
    }
  }
  for (; a <= hi; ++a) {
    const float t = line[a * stride];
    if (t < GQ_INF_F) {
      const float d = (float)(a - p) + t;
      g = d < g ? d : g;
      break;
    }
  }
  return g * g;
}

// min over the window of f(p + m) + m^2: line[i stride] = f(i) >= 0 or +inf, never NaN.  A candidate at offset m is >= m^2, so
// the scan stops once m^2 >= best; the result is that of the whole window.
__device__ __forceinline__ float gq_edt_env(const float* line, int stride, int L, int p, int R) {
  float best = line[p * stride];
  int m = 1;
  // four offsets per step while both sides stay inside the line and the window, the eight loads issued together; candidates
  // beyond the stopping offset are >= best, so taking them changes nothing
  for (; m + 3 <= R && p - m - 3 >= 0 && p + m + 3 < L; m += 4) {
    if ((float)(m * m) >= best) return best;
    const float* c = line + p * stride;
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[2 * j] = c[-(m + j) * stride], v[2 * j + 1] = c[(m + j) * stride];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mm = (float)((m + j) * (m + j));
      const float lo = v[2 * j] + mm, hi = v[2 * j + 1] + mm;
      best = lo < best ? lo : best;
      best = hi < best ? hi : best;
    }
  }
  for (; m <= R; ++m) {
    const float mm = (float)(m * m);
    if (mm >= best) break;
    if (p - m >= 0) {
      const float v = line[(p - m) * stride] + mm;
      best = v < best ? v : best;
    }
    if (p + m < L) {
      const float v = line[(p + m) * stride] + mm;
      best = v < best ? v : best;
    }
  }
  return best;
}

// phi of a node from its D and (e / h)^2 (+inf: the grid has no crossing within reach)
__device__ __forceinline__ float gq_edt_finish(float D, float e2, float voxel, float trunc, float max_distance) {
  if (!gq_finite(D)) return D;       // void: bit for bit
  if (fabsf(D) < trunc) return D;        // in band: the fused value, bit for bit
  float e = sqrtf(e2) * voxel;
  e = e > trunc ? e : trunc;
  e = e < max_distance ? e : max_distance;
  return D >= 0.0f ? e : -e;
}
