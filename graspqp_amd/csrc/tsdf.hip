// Scenes from depth images: TSDF fusion of a batch of depth frames into a stack of scene grids, in place (include/
// graspqp_hip.h, "scenes from depth images").  The volume is the memory gq_scene_terms / gq_clutter_terms and their corridor
// siblings read: `values` IS the running truncated signed distance, there is no extraction pass.
//
// gq_tsdf_integrate_kernel has the compose kernel's shape (clutter.hip): one thread per node, a block is a tile of
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
  int tiles_x, tiles_y, tiles_z;
};

__global__ __launch_bounds__(GQ_CL_TX* GQ_CL_TY* GQ_CL_TZ) void gq_tsdf_integrate_kernel(const GqTsdfArgs c) {
  // block -> (grid, tile): all of it block-uniform
  unsigned b = blockIdx.x;
  const int tk = (int)(b % (unsigned)c.tiles_z);
  b /= (unsigned)c.tiles_z;
  const int tj = (int)(b % (unsigned)c.tiles_y);
  b /= (unsigned)c.tiles_y;
  const int ti = (int)(b % (unsigned)c.tiles_x);
  const size_t g = b / (unsigned)c.tiles_x;
  const float* Tg = c.target_T ? c.target_T + g * 12 : nullptr;
  const int skip = c.skip ? c.skip[g] : -1;
  const int tid = threadIdx.x;
  const int i = ti * GQ_CL_TX + tid / (GQ_CL_TY * GQ_CL_TZ), j = tj * GQ_CL_TY + (tid / GQ_CL_TZ) % GQ_CL_TY, k = tk * GQ_CL_TZ + tid % GQ_CL_TZ;
  if (i >= c.out.nx || j >= c.out.ny || k >= c.out.nz) return;
  const size_t node = ((g * c.out.nx + i) * c.out.ny + j) * c.out.nz + k;  // < n_grids nx ny nz
  float D = c.values[node], W = c.weight[node];
  gq_tsdf_node(c.out, Tg, i, j, k, c.views, skip, c.trunc, c.max_weight, D, W);
  c.values[node] = D;
  c.weight[node] = W;
}

static long long gq_tsdf_tiles(int n, int t) { return ((long long)n + t - 1) / t; }
static bool gq_tsdf_finite(float v) { return v > -GQ_INF_F && v < GQ_INF_F; }  // false for NaN and +-inf

int gq_tsdf_check(const gqClutterGrids* grids, const gqDepthViews* views, float trunc, float max_weight, float unknown) {
  GQ_REQUIRE(grids, "tsdf: grids is NULL");
  if (gq_clutter_check(grids, grids->n_grids, 1, 1, 1) != GQ_OK) {  // retold under this unit's name
    char why[400];
    snprintf(why, sizeof(why), "%s", gq_last_error());
    GQ_FAIL(GQ_ERR_ARG, "tsdf: grids: %s", why);
  }
  const long long blocks = grids->n_grids * gq_tsdf_tiles(grids->nx, GQ_CL_TX) * gq_tsdf_tiles(grids->ny, GQ_CL_TY) *
                           gq_tsdf_tiles(grids->nz, GQ_CL_TZ);
  GQ_REQUIRE(blocks <= (1ll << 23), "tsdf: grids has %lld tiles of %d x %d x %d nodes, at most 2^23 per launch", blocks, GQ_CL_TX,
             GQ_CL_TY, GQ_CL_TZ);
  GQ_REQUIRE(views, "tsdf: views is NULL");
  GQ_REQUIRE(views->depth, "tsdf: views depth is NULL");
  GQ_REQUIRE(views->cam_T, "tsdf: views cam_T is NULL");
  GQ_REQUIRE(views->n_views >= 1 && views->n_views <= GQ_TSDF_MAX_VIEWS, "tsdf: n_views must be in 1..%d, got %d", GQ_TSDF_MAX_VIEWS,
             views->n_views);
  GQ_REQUIRE(views->width >= 1 && views->width <= GQ_TSDF_MAX_SIDE, "tsdf: width must be in 1..%d, got %d", GQ_TSDF_MAX_SIDE,
             views->width);
  GQ_REQUIRE(views->height >= 1 && views->height <= GQ_TSDF_MAX_SIDE, "tsdf: height must be in 1..%d, got %d", GQ_TSDF_MAX_SIDE,
             views->height);
  GQ_REQUIRE(gq_tsdf_finite(views->fx) && views->fx > 0.0f, "tsdf: fx must be finite and > 0, got %g", (double)views->fx);
  GQ_REQUIRE(gq_tsdf_finite(views->fy) && views->fy > 0.0f, "tsdf: fy must be finite and > 0, got %g", (double)views->fy);
  GQ_REQUIRE(gq_tsdf_finite(views->cx), "tsdf: cx must be finite, got %g", (double)views->cx);
  GQ_REQUIRE(gq_tsdf_finite(views->cy), "tsdf: cy must be finite, got %g", (double)views->cy);
  GQ_REQUIRE(gq_tsdf_finite(views->depth_min) && views->depth_min > 0.0f, "tsdf: depth_min must be finite and > 0, got %g",
             (double)views->depth_min);
  GQ_REQUIRE(gq_tsdf_finite(views->depth_max) && views->depth_max >= views->depth_min,
             "tsdf: depth_max must be finite and >= depth_min = %g, got %g", (double)views->depth_min, (double)views->depth_max);
  GQ_REQUIRE(gq_tsdf_finite(trunc) && trunc > 0.0f, "tsdf: trunc must be finite and > 0, got %g", (double)trunc);
  GQ_REQUIRE(gq_tsdf_finite(max_weight) && max_weight >= 1.0f, "tsdf: max_weight must be finite and >= 1, got %g", (double)max_weight);
  GQ_REQUIRE(gq_tsdf_finite(unknown), "tsdf: unknown must be finite, got %g", (double)unknown);
  return GQ_OK;
}

int gq_tsdf_integrate(const gqClutterGrids* grids, float* values, float* weight, const float* target_T, const gqDepthViews* views,
                      const int32_t* skip, float trunc, float max_weight, void* stream) {
  const int rc = gq_tsdf_check(grids, views, trunc, max_weight, 0.0f);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(values && values == grids->values, "tsdf: values must be grids->values");
  GQ_REQUIRE(weight, "tsdf: weight is NULL");
  GqTsdfArgs c{};
  c.out.values = grids->values, c.out.nx = grids->nx, c.out.ny = grids->ny, c.out.nz = grids->nz, c.out.voxel = grids->voxel;
  for (int a = 0; a < 3; ++a) c.out.origin[a] = grids->origin[a];
  c.values = values, c.weight = weight, c.target_T = target_T, c.skip = skip;
  c.views = *views;
  c.trunc = trunc, c.max_weight = max_weight;
  c.tiles_x = (int)gq_tsdf_tiles(grids->nx, GQ_CL_TX), c.tiles_y = (int)gq_tsdf_tiles(grids->ny, GQ_CL_TY);
  c.tiles_z = (int)gq_tsdf_tiles(grids->nz, GQ_CL_TZ);
  const long long blocks = (long long)grids->n_grids * c.tiles_x * c.tiles_y * c.tiles_z;
  hipLaunchKernelGGL(gq_tsdf_integrate_kernel, dim3((unsigned)blocks), dim3(GQ_CL_TX * GQ_CL_TY * GQ_CL_TZ), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
