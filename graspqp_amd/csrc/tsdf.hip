// Scenes from depth images: TSDF fusion of a batch of depth frames into a stack of scene grids, in place (include/
// graspqp_hip.h, "scenes from depth images").  The volume is the memory gq_scene_terms / gq_clutter_terms and their corridor
// siblings read: `values` IS the running truncated signed distance, there is no extraction pass.
//
// gq_tsdf_integrate_kernel walks the stack by grid_stack.h's tiles: one thread per node, a block is a tile of
// GQ_CL_TX x GQ_CL_TY x GQ_CL_TZ nodes of one grid, the lane runs along z, loads and stores of D and W go in 64-byte segments.
// The node keeps D and W in registers and visits the views in ascending order (tsdf_dev.h), so a batch of V frames pays the
// 16 bytes per node of grid traffic once and not V times.  Camera poses, intrinsics and the grid's pose and skipped label are
// block-uniform (scalar loads, SGPRs).  Every range test precedes its load: a node outside a view's frustum costs arithmetic
// only.  No atomics, no allocation, no synchronisation, nothing uploaded: the launch can sit in a captured graph, and a
// replay after in-place writes of images, poses or skip re-integrates.
#include "tsdf_dev.h"

#define GQ_TSDF_MAX_VIEWS 64
#define GQ_TSDF_MAX_SIDE 8192

struct GqTsdfArgs {
  gqSceneGrid out;  // grid 0 of the stack
  float* values;
  float* weight;
  const float* target_T;  // (G,12) or null
  const int32_t* skip;    // (G) or null
  gqDepthViews views;
  float trunc, max_weight;
  GqTiling tiling;
};

__global__ __launch_bounds__(GQ_CL_THREADS) void gq_tsdf_integrate_kernel(const GqTsdfArgs c) {
  const GqTile t = gq_tile_of(blockIdx.x, c.tiling);  // block-uniform
  const size_t g = t.g;
  const float* Tg = c.target_T ? c.target_T + g * 12 : nullptr;
  const int skip = c.skip ? c.skip[g] : -1;
  int i, j, k;
  if (!gq_tile_node(t, threadIdx.x, c.out.nx, c.out.ny, c.out.nz, i, j, k)) return;
  const size_t node = ((g * c.out.nx + i) * c.out.ny + j) * c.out.nz + k;  // < n_grids nx ny nz
  float D = c.values[node], W = c.weight[node];
  gq_tsdf_node(c.out, Tg, i, j, k, c.views, skip, c.trunc, c.max_weight, D, W);
  c.values[node] = D;
  c.weight[node] = W;
}

int gq_tsdf_check(const gqClutterGrids* grids, const gqDepthViews* views, float trunc, float max_weight, float unknown) {
  int rc = gq_stack_check(grids, "tsdf", "grids");
  if (rc == GQ_OK) rc = gq_tiling_check(grids, "tsdf: grids");
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(views, "tsdf: views is NULL");
  GQ_REQUIRE(views->depth, "tsdf: views depth is NULL");
  GQ_REQUIRE(views->cam_T, "tsdf: views cam_T is NULL");
  GQ_REQUIRE(views->n_views >= 1 && views->n_views <= GQ_TSDF_MAX_VIEWS, "tsdf: n_views must be in 1..%d, got %d", GQ_TSDF_MAX_VIEWS,
             views->n_views);
  GQ_REQUIRE(views->width >= 1 && views->width <= GQ_TSDF_MAX_SIDE, "tsdf: width must be in 1..%d, got %d", GQ_TSDF_MAX_SIDE,
             views->width);
  GQ_REQUIRE(views->height >= 1 && views->height <= GQ_TSDF_MAX_SIDE, "tsdf: height must be in 1..%d, got %d", GQ_TSDF_MAX_SIDE,
             views->height);
  GQ_REQUIRE(gq_finite(views->fx) && views->fx > 0.0f, "tsdf: fx must be finite and > 0, got %g", (double)views->fx);
  GQ_REQUIRE(gq_finite(views->fy) && views->fy > 0.0f, "tsdf: fy must be finite and > 0, got %g", (double)views->fy);
  GQ_REQUIRE(gq_finite(views->cx), "tsdf: cx must be finite, got %g", (double)views->cx);
  GQ_REQUIRE(gq_finite(views->cy), "tsdf: cy must be finite, got %g", (double)views->cy);
  GQ_REQUIRE(gq_finite(views->depth_min) && views->depth_min > 0.0f, "tsdf: depth_min must be finite and > 0, got %g",
             (double)views->depth_min);
  GQ_REQUIRE(gq_finite(views->depth_max) && views->depth_max >= views->depth_min,
             "tsdf: depth_max must be finite and >= depth_min = %g, got %g", (double)views->depth_min, (double)views->depth_max);
  GQ_REQUIRE(gq_finite(trunc) && trunc > 0.0f, "tsdf: trunc must be finite and > 0, got %g", (double)trunc);
  GQ_REQUIRE(gq_finite(max_weight) && max_weight >= 1.0f, "tsdf: max_weight must be finite and >= 1, got %g", (double)max_weight);
  GQ_REQUIRE(gq_finite(unknown), "tsdf: unknown must be finite, got %g", (double)unknown);
  return GQ_OK;
}

int gq_tsdf_integrate(const gqClutterGrids* grids, float* values, float* weight, const float* target_T, const gqDepthViews* views,
                      const int32_t* skip, float trunc, float max_weight, void* stream) {
  const int rc = gq_tsdf_check(grids, views, trunc, max_weight, 0.0f);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(values && values == grids->values, "tsdf: values must be grids->values");
  GQ_REQUIRE(weight, "tsdf: weight is NULL");
  GqTsdfArgs c{};
  c.out = gq_stack_grid(grids);
  c.values = values, c.weight = weight, c.target_T = target_T, c.skip = skip;
  c.views = *views;
  c.trunc = trunc, c.max_weight = max_weight;
  c.tiling = gq_tiling(grids->nx, grids->ny, grids->nz);
  const long long blocks = gq_tiling_blocks(c.tiling, grids->n_grids);  // <= 2^23: gq_tiling_check
  hipLaunchKernelGGL(gq_tsdf_integrate_kernel, dim3((unsigned)blocks), dim3(GQ_CL_THREADS), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
