// Euclidean distance field of a TSDF stack (include/graspqp_hip.h, "Euclidean distance field from a fused TSDF"; the bodies are
// edt_dev.h).  The squared distance to the crossing points of a grid separates exactly into 1-D passes:
//   (e / h)^2 = min( env_x( min( env_y(g_z^2), env_z(g_y^2) ) ), env_y( env_z(g_x^2) ) )
// g_c = the seed of axis c (distance along the node's own c-line to the nearest crossing on it), env_a = the min-plus with m^2
// along axis a over |m| <= R.  Eight launches on three buffers of the workspace, each of the stack's size; dst is written by the
// last one only, src by none:
//   1. seed z: src -> A          2. env y: A -> B            3. seed y: src -> A      4. env z: A, min with B -> C
//   5. env x: C -> B             6. seed x: src -> A         7. env z: A -> C         8. env y: C, min with B, finish -> dst
// A block is a tile of 16 whole lines of one grid in LDS (edt_dev.h), a thread owns the nodes tid, tid + 256, ... of the tile and
// scans its window in LDS.  No atomics, no block waits for another, nothing allocated, synchronised or uploaded: the call can
// sit in a captured graph behind gq_tsdf_integrate.  Windowed minima in a fixed order: bitwise reproducible.
#include "edt_dev.h"

struct GqEdtArgs {
  gqEdtPass q;
  const float* in;     // seed: src (D); envelope: f
  const float* other;  // envelope: a field the result is min-ed with, or null
  const float* src;    // finish: D
  float* out;
  size_t nodes;  // per grid
  int tiles;     // per grid
  float voxel, trunc, max_distance;
};

// block -> (grid, tile of the grid): block-uniform; the pointers move to the block's grid
__device__ __forceinline__ int gq_edt_block(GqEdtArgs& c) {
  const unsigned b = blockIdx.x;
  const size_t g = b / (unsigned)c.tiles;  // < n_grids
  c.in = gq_stack_plane(c.in, c.nodes, g), c.out = gq_stack_plane(c.out, c.nodes, g);
  if (c.other) c.other = gq_stack_plane(c.other, c.nodes, g);
  if (c.src) c.src = gq_stack_plane(c.src, c.nodes, g);
  return (int)(b % (unsigned)c.tiles);
}

template <bool INNER>
__global__ __launch_bounds__(GQ_EDT_THREADS) void gq_edt_seed_kernel(GqEdtArgs c) {
  extern __shared__ float line[];  // GQ_EDT_LINES L words
  const int tile = gq_edt_block(c);
  const int n = GQ_EDT_LINES * c.q.L;
  const size_t step = INNER ? (size_t)c.q.n_inner : 1;  // to the next node of the line
  for (int e = threadIdx.x; e < n; e += GQ_EDT_THREADS) {
    int p, word;
    size_t node;
    if (!gq_edt_locate<INNER>(c.q, tile, e, p, word, node)) continue;
    line[word] = p + 1 < c.q.L ? gq_edt_edge(c.in[node], c.in[node + step]) : GQ_INF_F;  // node + step: position p + 1 < L
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += GQ_EDT_THREADS) {
    int p, word;
    size_t node;
    if (!gq_edt_locate<INNER>(c.q, tile, e, p, word, node)) continue;
    c.out[node] = gq_edt_seed(line + gq_edt_line0<INNER>(word, p), gq_edt_stride<INNER>(), c.q.L, p, c.q.R);
  }
}

template <bool INNER, bool FINISH>
__global__ __launch_bounds__(GQ_EDT_THREADS) void gq_edt_env_kernel(GqEdtArgs c) {
  extern __shared__ float line[];
  const int tile = gq_edt_block(c);
  const int n = GQ_EDT_LINES * c.q.L;
  for (int e = threadIdx.x; e < n; e += GQ_EDT_THREADS) {
    int p, word;
    size_t node;
    if (!gq_edt_locate<INNER>(c.q, tile, e, p, word, node)) continue;
    line[word] = c.in[node];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += GQ_EDT_THREADS) {
    int p, word;
    size_t node;
    if (!gq_edt_locate<INNER>(c.q, tile, e, p, word, node)) continue;
    float v = gq_edt_env(line + gq_edt_line0<INNER>(word, p), gq_edt_stride<INNER>(), c.q.L, p, c.q.R);
    if (c.other) {
      const float o = c.other[node];
      v = o < v ? o : v;
    }
    c.out[node] = FINISH ? gq_edt_finish(c.src[node], v, c.voxel, c.trunc, c.max_distance) : v;
  }
}

int gq_esdf_check(const gqClutterGrids* src, const gqClutterGrids* dst, float trunc, float max_distance, const void* workspace) {
  int rc = gq_stack_check(src, "esdf", "src", true);
  if (rc != GQ_OK) return rc;
  rc = gq_stack_check(dst, "esdf", "dst", true);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(workspace, "esdf: workspace is NULL");
  GQ_REQUIRE(dst->n_grids == src->n_grids, "esdf: dst n_grids must be src's %d, got %d", src->n_grids, dst->n_grids);
  GQ_REQUIRE(dst->nx == src->nx && dst->ny == src->ny && dst->nz == src->nz, "esdf: dst shape must be src's %d x %d x %d, got %d x %d x %d",
             src->nx, src->ny, src->nz, dst->nx, dst->ny, dst->nz);
  for (int a = 0; a < 3; ++a)
    GQ_REQUIRE(dst->origin[a] == src->origin[a], "esdf: dst origin[%d] must be src's %g, got %g", a, (double)src->origin[a],
               (double)dst->origin[a]);
  GQ_REQUIRE(dst->voxel == src->voxel, "esdf: dst voxel must be src's %g, got %g", (double)src->voxel, (double)dst->voxel);
  const size_t bytes = (size_t)src->n_grids * src->nx * src->ny * src->nz * sizeof(float);
  const uintptr_t s = (uintptr_t)src->values, d = (uintptr_t)dst->values;
  GQ_REQUIRE(s + bytes <= d || d + bytes <= s, "esdf: dst values must not alias src values");
  const int n[3] = {src->nx, src->ny, src->nz};
  for (int a = 0; a < 3; ++a)
    GQ_REQUIRE(n[a] <= GQ_EDT_MAX_LINE, "esdf: src n%c = %d, at most %d nodes along an axis (a whole line lives in LDS)", "xyz"[a], n[a],
               GQ_EDT_MAX_LINE);
  // tiles of one grid in the x, y and z passes (every axis <= GQ_EDT_MAX_LINE: the products fit an int)
  const int t[3] = {gq_edt_tiles<true>({1, n[0], n[1] * n[2], 0}), gq_edt_tiles<true>({n[0], n[1], n[2], 0}),
                    gq_edt_tiles<false>({n[0] * n[1], n[2], 1, 0})};
  const long long tiles = (long long)src->n_grids * (t[0] > t[1] ? (t[0] > t[2] ? t[0] : t[2]) : (t[1] > t[2] ? t[1] : t[2]));
  GQ_REQUIRE(tiles <= (1ll << 23), "esdf: src has %lld tiles of %d lines, at most 2^23 per launch", tiles, GQ_EDT_LINES);
  GQ_REQUIRE(gq_finite(trunc) && trunc > 0.0f, "esdf: trunc must be finite and > 0, got %g", (double)trunc);
  GQ_REQUIRE(gq_finite(max_distance) && max_distance >= trunc, "esdf: max_distance must be finite and >= trunc = %g, got %g",
             (double)trunc, (double)max_distance);
  const double window = ceil((double)max_distance / (double)src->voxel);
  GQ_REQUIRE(window <= (double)GQ_EDT_MAX_WINDOW, "esdf: max_distance / voxel gives a window of %.0f nodes, at most %d", window,
             GQ_EDT_MAX_WINDOW);
  return GQ_OK;
}

int gq_esdf_workspace_bytes(const gqClutterGrids* src, size_t* bytes) {
  GQ_REQUIRE(bytes, "esdf: bytes is NULL");
  const int rc = gq_stack_check(src, "esdf", "src", true);
  if (rc != GQ_OK) return rc;
  *bytes = 3 * (size_t)src->n_grids * src->nx * src->ny * src->nz * sizeof(float);  // the buffers A, B, C
  return GQ_OK;
}

template <bool INNER, bool SEED, bool FINISH>
static int gq_esdf_launch(GqEdtArgs c, int n_grids, hipStream_t stream) {
  c.tiles = gq_edt_tiles<INNER>(c.q);
  const dim3 grid((unsigned)((long long)n_grids * c.tiles)), block(GQ_EDT_THREADS);
  const size_t lds = (size_t)GQ_EDT_LINES * c.q.L * sizeof(float);  // <= 64 KB: L <= GQ_EDT_MAX_LINE
  if (SEED)
    hipLaunchKernelGGL(gq_edt_seed_kernel<INNER>, grid, block, lds, stream, c);
  else
    hipLaunchKernelGGL((gq_edt_env_kernel<INNER, FINISH>), grid, block, lds, stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_esdf(const gqClutterGrids* src, const gqClutterGrids* dst, float* dst_values, float trunc, float max_distance, void* workspace,
            void* stream) {
  int rc = gq_esdf_check(src, dst, trunc, max_distance, workspace);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(dst_values && dst_values == dst->values, "esdf: dst_values must be dst->values");
  const int nx = src->nx, ny = src->ny, nz = src->nz, G = src->n_grids;
  GqEdtArgs c{};
  c.nodes = (size_t)nx * ny * nz;
  c.voxel = src->voxel, c.trunc = trunc, c.max_distance = max_distance;
  const int R = (int)ceil((double)max_distance / (double)src->voxel);  // 1 .. GQ_EDT_MAX_WINDOW
  const gqEdtPass X{1, nx, ny * nz, R}, Y{nx, ny, nz, R}, Z{nx * ny, nz, 1, R};
  float* A = (float*)workspace;
  float* B = A + (size_t)G * c.nodes;
  float* C = B + (size_t)G * c.nodes;
  hipStream_t st = (hipStream_t)stream;
  auto pass = [&](const gqEdtPass& q, const float* in, const float* other, float* out) {
    GqEdtArgs a = c;
    a.q = q, a.in = in, a.other = other, a.out = out;
    return a;
  };
  if ((rc = gq_esdf_launch<false, true, false>(pass(Z, src->values, nullptr, A), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<true, false, false>(pass(Y, A, nullptr, B), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<true, true, false>(pass(Y, src->values, nullptr, A), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<false, false, false>(pass(Z, A, B, C), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<true, false, false>(pass(X, C, nullptr, B), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<true, true, false>(pass(X, src->values, nullptr, A), G, st)) != GQ_OK) return rc;
  if ((rc = gq_esdf_launch<false, false, false>(pass(Z, A, nullptr, C), G, st)) != GQ_OK) return rc;
  GqEdtArgs last = pass(Y, C, B, dst_values);
  last.src = src->values;
  return gq_esdf_launch<true, false, true>(last, G, st);
}
