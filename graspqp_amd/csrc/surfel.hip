// Target objects from depth images: the zero level set of every grid of a fused TSDF stack as an oriented point cloud
// (include/graspqp_hip.h, "target objects from depth images"; the body is surfel_dev.h).  Three launches, no atomics, no block
// waits for another, nothing allocated, synchronised or uploaded: the call can sit in a captured graph behind gq_tsdf_integrate.
//   1. gq_surfel_count_kernel: a block is a tile of GQ_CL_TX x GQ_CL_TY x GQ_CL_TZ nodes of one grid (grid_stack.h's block ->
//      (grid, tile) decode); D of the tile and of the next node plane on every axis goes to LDS, NaN where the node is not
//      observed; the block's number of crossing edges (ballot + popcount per wavefront, folded in LDS) goes to workspace[tile].
//   2. gq_surfel_scan_kernel: one block per grid turns that grid's tile counts into their exclusive prefix (a second array of
//      the workspace) and writes count[g] = (total, written).
//   3. gq_surfel_emit_kernel: a tile without crossings leaves at once.  The others load D with the -1 .. +2 halo of the normal
//      stencil, repeat the crossing test, rank their crossings in the order (thread, axis) by ballot prefixes per wavefront and
//      wavefront offsets in LDS, and write position and normal at prefix[tile] + rank while that is below the capacity.
// The output order is (tile, thread in tile, axis): fixed, so two runs and a graph replay agree bit for bit.
#include "surfel_dev.h"

#define GQ_SF_WAVES (GQ_SF_THREADS / GQ_WAVE)
#define GQ_SF_MAX_CAPACITY (1 << 24)
#define GQ_SF_SCAN_THREADS 256

struct GqSurfelArgs {
  gqSurfelGrid s;  // grid 0 of the stack: values / weight advance by nodes per grid
  GqTiling tiling;
  int32_t* tile_count;   // (G tiles)
  int32_t* tile_prefix;  // (G tiles)
  float* points;         // (G,capacity,3) or null
  float* normals;
  int capacity;
  int32_t* count;  // (G,2)
};

// true if no node of the tile lies in the region (block-uniform)
__device__ __forceinline__ bool gq_surfel_outside(const gqSurfelGrid& s, int i0, int j0, int k0) {
  const int* r = s.region;
  return i0 >= r[1] || i0 + GQ_CL_TX <= r[0] || j0 >= r[3] || j0 + GQ_CL_TY <= r[2] || k0 >= r[5] || k0 + GQ_CL_TZ <= r[4];
}

__global__ __launch_bounds__(GQ_SF_THREADS) void gq_surfel_count_kernel(const GqSurfelArgs c) {
  __shared__ float tile[GQ_SF_TILE];
  __shared__ int wave_n[GQ_SF_WAVES];
  const GqTile t = gq_tile_of(blockIdx.x, c.tiling);  // block-uniform
  const gqSurfelGrid s = gq_surfel_of(c.s, t.g);
  const int i0 = t.i0, j0 = t.j0, k0 = t.k0;
  const int tid = threadIdx.x;
  if (gq_surfel_outside(s, i0, j0, k0)) {
    if (tid == 0) c.tile_count[blockIdx.x] = 0;
    return;
  }
  for (int e = tid; e < gq_surfel_entries(0, 1); e += GQ_SF_THREADS) gq_surfel_fill(s, i0, j0, k0, 0, 1, e, tile);
  __syncthreads();
  const unsigned flags = gq_surfel_flags(s, tile, i0, j0, k0, tid);
  const int n = __popcll(__ballot(flags & 1u)) + __popcll(__ballot(flags & 2u)) + __popcll(__ballot(flags & 4u));
  if (gq_lane() == 0) wave_n[tid / GQ_WAVE] = n;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < GQ_SF_WAVES; ++w) total += wave_n[w];
    c.tile_count[blockIdx.x] = total;  // <= 3 * 256
  }
}

// One block per grid: tile_prefix = exclusive prefix of tile_count over the grid's tiles, count[g] = (total, written).
// A grid holds at most 2^28 nodes, so its total is below 3 * 2^28 < 2^31.
__global__ __launch_bounds__(GQ_SF_SCAN_THREADS) void gq_surfel_scan_kernel(const GqSurfelArgs c, int tiles_per_grid) {
  __shared__ int wave_n[GQ_SF_SCAN_THREADS / GQ_WAVE];
  const int tid = threadIdx.x, lane = gq_lane(), wave = tid / GQ_WAVE;
  const size_t base = (size_t)blockIdx.x * (size_t)tiles_per_grid;
  int running = 0;
  for (int first = 0; first < tiles_per_grid; first += GQ_SF_SCAN_THREADS) {  // block-uniform trip count
    const int t = first + tid;
    const int n = t < tiles_per_grid ? c.tile_count[base + t] : 0;
    int incl = n;  // inclusive prefix within the wavefront
#pragma unroll
    for (int o = 1; o < GQ_WAVE; o <<= 1) {
      const int up = __shfl_up(incl, o, GQ_WAVE);
      if (lane >= o) incl += up;
    }
    if (lane == GQ_WAVE - 1) wave_n[wave] = incl;
    __syncthreads();
    int before = 0, chunk = 0;
    for (int w = 0; w < GQ_SF_SCAN_THREADS / GQ_WAVE; ++w) {
      before += w < wave ? wave_n[w] : 0;
      chunk += wave_n[w];
    }
    if (t < tiles_per_grid) c.tile_prefix[base + t] = running + before + incl - n;
    running += chunk;
    __syncthreads();  // wave_n is rewritten by the next chunk
  }
  if (tid == 0) {
    c.count[2 * blockIdx.x] = running;
    c.count[2 * blockIdx.x + 1] = c.points ? min(running, c.capacity) : 0;
  }
}

__global__ __launch_bounds__(GQ_SF_THREADS) void gq_surfel_emit_kernel(const GqSurfelArgs c) {
  __shared__ float tile[GQ_SF_TILE];
  __shared__ int wave_n[GQ_SF_WAVES];
  if (c.tile_count[blockIdx.x] == 0) return;  // block-uniform: most tiles hold no surface
  const int first = c.tile_prefix[blockIdx.x];
  if (first >= c.capacity) return;
  const GqTile t = gq_tile_of(blockIdx.x, c.tiling);  // block-uniform
  const gqSurfelGrid s = gq_surfel_of(c.s, t.g);
  const int i0 = t.i0, j0 = t.j0, k0 = t.k0;
  const int tid = threadIdx.x, lane = gq_lane(), wave = tid / GQ_WAVE;
  for (int e = tid; e < GQ_SF_TILE; e += GQ_SF_THREADS) gq_surfel_fill(s, i0, j0, k0, GQ_SF_LO, GQ_SF_HI, e, tile);
  __syncthreads();
  const unsigned flags = gq_surfel_flags(s, tile, i0, j0, k0, tid);
  const unsigned long long b0 = __ballot(flags & 1u), b1 = __ballot(flags & 2u), b2 = __ballot(flags & 4u);
  const unsigned long long below = (1ull << lane) - 1ull;
  if (lane == 0) wave_n[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();
  int slot = first + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);  // crossings of the lower lanes' nodes
  for (int w = 0; w < GQ_SF_WAVES; ++w) slot += w < wave ? wave_n[w] : 0;
  float* P = c.points + t.g * (size_t)c.capacity * 3;  // g < n_grids
  float* N = c.normals + t.g * (size_t)c.capacity * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((flags >> a) & 1u)) continue;
    if (slot < c.capacity) {  // slot >= 0: the largest index below is 3 capacity - 1 of this grid's part
      float p[3], n[3];
      gq_surfel_emit(s, tile, i0, j0, k0, tid, a, p, n);
      const size_t at = (size_t)slot * 3;
      P[at] = p[0], P[at + 1] = p[1], P[at + 2] = p[2];
      N[at] = n[0], N[at + 1] = n[1], N[at + 2] = n[2];
    }
    ++slot;
  }
}

int gq_tsdf_surfels_check(const gqClutterGrids* grids, const int32_t* region, float min_weight, float trunc, int has_outputs,
                          int64_t capacity) {
  int rc = gq_stack_check(grids, "surfels", "grids");
  if (rc == GQ_OK) rc = gq_tiling_check(grids, "surfels: grids");
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(gq_finite(trunc) && trunc > 0.0f, "surfels: trunc must be finite and > 0, got %g", (double)trunc);
  GQ_REQUIRE(gq_finite(min_weight), "surfels: min_weight must be finite, got %g", (double)min_weight);
  if (region) {
    const int n[3] = {grids->nx, grids->ny, grids->nz};
    for (int a = 0; a < 3; ++a)
      GQ_REQUIRE(region[2 * a] >= 0 && region[2 * a] < region[2 * a + 1] && region[2 * a + 1] <= n[a],
                 "surfels: region [%d,%d) on axis %d must be non-empty and inside 0..%d", region[2 * a], region[2 * a + 1], a, n[a]);
  }
  if (has_outputs)
    GQ_REQUIRE(capacity >= 1, "surfels: capacity must be >= 1 when points are asked for, got %lld", (long long)capacity);
  GQ_REQUIRE(capacity <= GQ_SF_MAX_CAPACITY, "surfels: capacity must be <= 2^24, got %lld", (long long)capacity);
  return GQ_OK;
}

int gq_tsdf_surfels_workspace_bytes(const gqClutterGrids* grids, size_t* bytes) {
  GQ_REQUIRE(bytes, "surfels: bytes is NULL");
  const int rc = gq_tsdf_surfels_check(grids, nullptr, 0.0f, 1.0f, 0, 0);
  if (rc != GQ_OK) return rc;
  const long long tiles = gq_tiling_blocks(gq_tiling(grids->nx, grids->ny, grids->nz), grids->n_grids);
  *bytes = (size_t)tiles * 2 * sizeof(int32_t);  // the tiles' counts and their prefix
  return GQ_OK;
}

int gq_tsdf_surfels(const gqClutterGrids* grids, const float* values, const float* weight, const int32_t* region, float min_weight,
                    float trunc, float* points, float* normals, int64_t capacity, int32_t* count, void* workspace, void* stream) {
  const int rc = gq_tsdf_surfels_check(grids, region, min_weight, trunc, points != nullptr, capacity);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(values && values == grids->values, "surfels: values must be grids->values");
  GQ_REQUIRE((points == nullptr) == (normals == nullptr), "surfels: points and normals must both be given or both be NULL");
  GQ_REQUIRE(count, "surfels: count is NULL");
  GQ_REQUIRE(workspace, "surfels: workspace is NULL");
  GqSurfelArgs c{};
  c.s.grid = gq_stack_grid(grids);  // values == grids->values
  c.s.weight = weight, c.s.min_weight = min_weight, c.s.trunc = trunc;
  const int n[3] = {grids->nx, grids->ny, grids->nz};
  for (int a = 0; a < 3; ++a) c.s.region[2 * a] = region ? region[2 * a] : 0, c.s.region[2 * a + 1] = region ? region[2 * a + 1] : n[a];
  c.tiling = gq_tiling(grids->nx, grids->ny, grids->nz);
  const int per_grid = (int)gq_tiling_blocks(c.tiling, 1);  // <= 2^23
  const long long tiles = gq_tiling_blocks(c.tiling, grids->n_grids);
  c.tile_count = (int32_t*)workspace, c.tile_prefix = (int32_t*)workspace + tiles;
  c.points = points, c.normals = normals, c.capacity = (int)capacity, c.count = count;
  hipLaunchKernelGGL(gq_surfel_count_kernel, dim3((unsigned)tiles), dim3(GQ_SF_THREADS), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(gq_surfel_scan_kernel, dim3((unsigned)grids->n_grids), dim3(GQ_SF_SCAN_THREADS), 0, (hipStream_t)stream, c, per_grid);
  GQ_LAUNCH_CHECK();
  if (points) {
    hipLaunchKernelGGL(gq_surfel_emit_kernel, dim3((unsigned)tiles), dim3(GQ_SF_THREADS), 0, (hipStream_t)stream, c);
    GQ_LAUNCH_CHECK();
  }
  return GQ_OK;
}
