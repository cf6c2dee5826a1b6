// What a stack of scene grids and a tile of one are, in one place, for every launcher that walks a gqClutterGrids node by node
// (clutter.hip compose, tsdf.hip, surfel.hip; edt.hip has its own line tiling in edt_dev.h and takes the stack view, gq_finite
// and the stack check from here).
//   stack: n_grids volumes of nx ny nz nodes, back to back; grid g of `values`, and of every other per-node plane (the TSDF
//          weight), starts g nx ny nz nodes in.  Shape, origin and voxel are shared, so a gqSceneGrid of grid 0 plus g says it all.
//   tile:  a block is GQ_CL_TX x GQ_CL_TY x GQ_CL_TZ nodes of one grid, thread tid = (li GQ_CL_TY + lj) GQ_CL_TZ + lk with the lane
//          along z (64-byte segments), a wavefront is one x slab.  Blocks run over (grid, tile x, tile y, tile z), z fastest.
// The geometric part needs no HIP runtime: tests/grid_stack_host.cpp and the *_body_host.cpp programs compile it for the host
// (GQ_SCENE_HOST_BUILD) and walk blocks and threads through the decode the kernels run.  A host includer provides what it
// always had to (tests/host_shim.h): __device__, __forceinline__ and GQ_INF_F; the rest the header brings itself.
#pragma once
#ifdef GQ_SCENE_HOST_BUILD
#include <math.h>
#include <stddef.h>

#include "../../include/graspqp_hip.h"
#define GQ_HOST_DEVICE __device__ __forceinline__  // usable on both sides: the host build has one side only
#else
#include "common.h"
#define GQ_HOST_DEVICE __host__ __device__ __forceinline__
#endif

#define GQ_CL_TX 4
#define GQ_CL_TY 4
#define GQ_CL_TZ 16
#define GQ_CL_THREADS (GQ_CL_TX * GQ_CL_TY * GQ_CL_TZ)
#define GQ_TILING_MAX_BLOCKS (1ll << 23)

GQ_HOST_DEVICE bool gq_finite(float v) { return fabsf(v) < GQ_INF_F; }  // false for NaN and +-inf

// ---- the stack view ------------------------------------------------------------------------------------------------------
GQ_HOST_DEVICE size_t gq_stack_nodes(const gqSceneGrid& s) { return (size_t)s.nx * (size_t)s.ny * (size_t)s.nz; }
// grid g's part of a per-node plane of the stack (g < n_grids)
template <class T>
GQ_HOST_DEVICE T* gq_stack_plane(T* plane, size_t nodes, size_t g) {
  return plane + g * nodes;
}
// grid g of the stack whose grid 0 is `first`
GQ_HOST_DEVICE gqSceneGrid gq_stack_grid(const gqSceneGrid& first, size_t g) {
  gqSceneGrid grid = first;
  grid.values = gq_stack_plane(first.values, gq_stack_nodes(first), g);
  return grid;
}
static inline gqSceneGrid gq_stack_grid(const gqClutterGrids* grids, size_t g = 0) {
  gqSceneGrid first{};
  first.values = grids->values, first.nx = grids->nx, first.ny = grids->ny, first.nz = grids->nz, first.voxel = grids->voxel;
  for (int a = 0; a < 3; ++a) first.origin[a] = grids->origin[a];
  return gq_stack_grid(first, g);
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------
struct GqTiling {
  int tx, ty, tz;  // tiles of one grid along x, y, z
};
static inline GqTiling gq_tiling(int nx, int ny, int nz) {
  return GqTiling{(nx + GQ_CL_TX - 1) / GQ_CL_TX, (ny + GQ_CL_TY - 1) / GQ_CL_TY, (nz + GQ_CL_TZ - 1) / GQ_CL_TZ};
}
// blocks of a launch over every tile of every grid: what the checks bound and what the launches ask for
static inline long long gq_tiling_blocks(const GqTiling& t, int n_grids) { return (long long)n_grids * t.tx * t.ty * t.tz; }

struct GqTile {
  size_t g;        // grid
  int i0, j0, k0;  // first node
};
// block b < gq_tiling_blocks -> (grid, tile): block-uniform
__device__ __forceinline__ GqTile gq_tile_of(unsigned b, const GqTiling& t) {
  GqTile tile;
  tile.k0 = (int)(b % (unsigned)t.tz) * GQ_CL_TZ;
  b /= (unsigned)t.tz;
  tile.j0 = (int)(b % (unsigned)t.ty) * GQ_CL_TY;
  b /= (unsigned)t.ty;
  tile.i0 = (int)(b % (unsigned)t.tx) * GQ_CL_TX;
  tile.g = b / (unsigned)t.tx;
  return tile;
}
// thread tid < GQ_CL_THREADS -> its node relative to the tile's first
__device__ __forceinline__ void gq_tile_local(int tid, int& li, int& lj, int& lk) {
  li = tid / (GQ_CL_TY * GQ_CL_TZ), lj = (tid / GQ_CL_TZ) % GQ_CL_TY, lk = tid % GQ_CL_TZ;
}
// ... -> its node (i,j,k) = first node + gq_tile_local, one expression per axis (the order the compiler keeps the prologue's
// instructions in); false if the node lies beyond a grid of nx x ny x nz nodes (a partial tile)
__device__ __forceinline__ bool gq_tile_node(const GqTile& tile, int tid, int nx, int ny, int nz, int& i, int& j, int& k) {
  i = tile.i0 + tid / (GQ_CL_TY * GQ_CL_TZ), j = tile.j0 + (tid / GQ_CL_TZ) % GQ_CL_TY, k = tile.k0 + tid % GQ_CL_TZ;
  return i < nx && j < ny && k < nz;
}

// ---- the checks every launcher on a stack makes (library only: they report through gq_last_error) --------------------------
#ifndef GQ_SCENE_HOST_BUILD
// The refusal a check of another unit has just left in gq_last_error, retold as "<unit>: <what>: <why>"
static inline int gq_retell(const char* unit, const char* what) {
  char why[400];
  snprintf(why, sizeof(why), "%s", gq_last_error());
  GQ_FAIL(GQ_ERR_ARG, "%s: %s: %s", unit, what, why);
}
// Everything gq_clutter_check refuses for the stack itself, retold under the unit's name.  own_values: a NULL `values` is refused
// here, in the unit's own words, before gq_scene_check gets to say it in its own.
static inline int gq_stack_check(const gqClutterGrids* grids, const char* unit, const char* name, bool own_values = false) {
  GQ_REQUIRE(grids, "%s: %s is NULL", unit, name);
  if (own_values) GQ_REQUIRE(grids->values, "%s: %s values is NULL", unit, name);
  if (gq_clutter_check(grids, grids->n_grids, 1, 1, 1) != GQ_OK) return gq_retell(unit, name);
  return GQ_OK;
}
// The block count of a launch over the (checked) stack, refused as "<what> has ..." above 2^23: (unsigned)blocks is then exact.
static inline int gq_tiling_check(const gqClutterGrids* grids, const char* what) {
  const long long blocks = gq_tiling_blocks(gq_tiling(grids->nx, grids->ny, grids->nz), grids->n_grids);
  GQ_REQUIRE(blocks <= GQ_TILING_MAX_BLOCKS, "%s has %lld tiles of %d x %d x %d nodes, at most 2^23 per launch", what, blocks, GQ_CL_TX,
             GQ_CL_TY, GQ_CL_TZ);
  return GQ_OK;
}
#endif
