// Clutter scenes: one signed-distance grid PER OBJECT for the two obstacle terms of the MALA* stepper, and the kernel that
// fills such a stack on the device from posed part grids (include/graspqp_hip.h, "clutter scenes").
//
// The stepper's rows are object-major, n_obj x batch_each, each object's rows in that object's own frame.  In a bin with N
// objects, grasping object g needs the scene "bin + every object but g" in g's frame: a different grid per object.
//
//  - gq_clutter_kernel / gq_clutter_corridor_kernel are gq_scene_kernel / gq_approach_kernel with one more step in front: the
//    block (= row b) builds its gqSceneGrid from the stack, values + (b / rows_per_grid) nx ny nz, and runs the SAME row body
//    (scene_row_dev.h / approach_row_dev.h).  The alternative, one launch of the single-grid kernel per object on a row slice,
//    costs a launch per object and iteration.
//  - gq_clutter_query_kernel is gq_scene_query_kernel with the grid picked per point.
//  - gq_clutter_compose_kernel writes the stack: node (g,i,j,k) = min(far, base, every part but exclude[g]) resampled at the
//    node's world position (clutter_dev.h).  One thread per node, a block is a tile of one grid (grid_stack.h: the stack, the
//    tile and the decode).  Lane p < n_parts of wavefront 0 first tests part p against the tile (gq_clutter_culled); a part
//    that no node of the tile can reach costs the block no loads.  Poses and exclude are read from device memory at launch: no upload, no
//    allocation, no synchronisation, so the launch can sit in a captured graph and a replay recomposes after an in-place
//    pose update.  Parts in ascending order, no atomics: bitwise reproducible run to run.
#include "approach_row_dev.h"
#include "clutter_dev.h"
#include "scene_row_dev.h"

#define GQ_CL_MAX_GRIDS 65536

struct GqClutterArgs {
  GqSceneArgs a;  // a.grid is grid 0 of the stack
  int rows_per_grid;
};

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_clutter_kernel(const GqClutterArgs c) {
  const gqSceneGrid grid = gq_stack_grid(c.a.grid, blockIdx.x / (unsigned)c.rows_per_grid);
  gq_scene_row(c.a, grid);
}

struct GqCorridorArgs {
  GqApproachArgs a;  // a.grid is grid 0 of the stack
  int rows_per_grid;
};

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_clutter_corridor_kernel(const GqCorridorArgs c) {
  const gqSceneGrid grid = gq_stack_grid(c.a.grid, blockIdx.x / (unsigned)c.rows_per_grid);
  gq_approach_row(c.a, grid);
}

// one query per lane, the grid of point i is i / points_per_grid
__global__ __launch_bounds__(256) void gq_clutter_query_kernel(const gqSceneGrid first, int64_t points_per_grid,
                                                               const float* __restrict__ points, int64_t N, float* __restrict__ phi,
                                                               float* __restrict__ grad, uint8_t* __restrict__ inside) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const gqSceneGrid grid = gq_stack_grid(first, (size_t)(i / points_per_grid));
  const gq3 x = gq_mk(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]);
  float f = GQ_INF_F;  // outside the volume: free space
  gq3 gp = gq_mk(0, 0, 0);
  const int where = gq_scene_sample(grid, x, f, gp);
  if (where == GQ_SCENE_NONFINITE) f = gp.x = gp.y = gp.z = __builtin_nanf("");
  phi[i] = f;
  if (grad) grad[i * 3] = gp.x, grad[i * 3 + 1] = gp.y, grad[i * 3 + 2] = gp.z;
  if (inside) inside[i] = where == GQ_SCENE_INSIDE;
}

struct GqComposeArgs {
  gqSceneGrid out;  // grid 0 of the stack
  float* out_values;
  const float* target_T;     // (G,12)
  const float* part_T;       // (n_parts,12)
  const int32_t* exclude;    // (G) or null
  gqSceneGrid parts[GQ_CL_MAX_PARTS];
  gqSceneGrid base;
  int n_parts, has_base;
  GqTiling tiling;
  float far;
};

__global__ __launch_bounds__(GQ_CL_THREADS) void gq_clutter_compose_kernel(const GqComposeArgs c) {
  const GqTile t = gq_tile_of(blockIdx.x, c.tiling);  // block-uniform
  const size_t g = t.g;
  const float* Tg = c.target_T + g * 12;
  const int i0 = t.i0, j0 = t.j0, k0 = t.k0;
  const int tid = threadIdx.x;
  const int exclude = c.exclude ? c.exclude[g] : -1;
#ifndef GQ_CLUTTER_NO_CULL
  __shared__ unsigned s_live;
  if (tid < GQ_WAVE) {  // lane p of wavefront 0 tests part p
    const bool keep = tid < c.n_parts && tid != exclude && !gq_clutter_culled(c.out, Tg, i0, j0, k0, c.parts[tid], c.part_T + 12 * tid);
    const unsigned long long m = __ballot(keep);
    if (tid == 0) s_live = (unsigned)m;
  }
  __syncthreads();
  const unsigned live = s_live;
#else  // a variant build for measurements and for the equality test: every part is sampled by every tile
  const unsigned live = 0xffffffffu;
#endif
  int i, j, k;
  if (!gq_tile_node(t, tid, c.out.nx, c.out.ny, c.out.nz, i, j, k)) return;
  const float v = gq_clutter_node(c.out, Tg, i, j, k, c.parts, c.n_parts, c.part_T, exclude, live, c.has_base ? &c.base : nullptr, c.far);
  c.out_values[((g * c.out.nx + i) * c.out.ny + j) * c.out.nz + k] = v;
}

static int gq_clutter_check_grids(const gqClutterGrids* grids) {
  GQ_REQUIRE(grids, "clutter: grids is NULL");
  GQ_REQUIRE(grids->n_grids >= 1 && grids->n_grids <= GQ_CL_MAX_GRIDS, "clutter: n_grids must be in 1..%d, got %d", GQ_CL_MAX_GRIDS,
             grids->n_grids);
  const gqSceneGrid first = gq_stack_grid(grids);  // shape, origin and voxel are shared: one check holds for every grid
  if (gq_scene_check(&first, 1, 1, 1) != GQ_OK) return gq_retell("clutter", "grids");
  return GQ_OK;
}

int gq_clutter_check(const gqClutterGrids* grids, int64_t batch, int rows_per_grid, int n_links, int64_t n_samples) {
  const int rc = gq_clutter_check_grids(grids);
  if (rc != GQ_OK) return rc;
  const gqSceneGrid first = gq_stack_grid(grids);
  if (gq_scene_check(&first, batch, n_links, n_samples) != GQ_OK) return gq_retell("clutter", "launch");
  GQ_REQUIRE(rows_per_grid >= 1, "clutter: rows_per_grid must be >= 1, got %d", rows_per_grid);
  GQ_REQUIRE(batch == (int64_t)grids->n_grids * rows_per_grid, "clutter: batch must be n_grids * rows_per_grid = %d * %d, got %lld",
             grids->n_grids, rows_per_grid, (long long)batch);
  return GQ_OK;
}

int gq_clutter_terms(const gqClutterGrids* grids, int rows_per_grid, float margin, const float* samples, const int32_t* sample_link,
                     int64_t n_samples, int n_links, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                     int64_t batch, const float* up_scene, float w_scene, float* e_scene, int accumulate, float* link_wrench,
                     float* gRt, void* stream) {
  const int rc = gq_clutter_check(grids, batch, rows_per_grid, n_links, n_samples);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "clutter: bad arguments");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "clutter: margin must be finite and >= 0, got %g", (double)margin);
  GqClutterArgs c{};
  c.a = gq_scene_args(gq_stack_grid(grids), margin, samples, sample_link, n_samples, n_links, hand_pose, pose_dim, Rg, link_T,
                      up_scene, w_scene, e_scene, accumulate, link_wrench, gRt);
  c.rows_per_grid = rows_per_grid;
  hipLaunchKernelGGL(gq_clutter_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_clutter_corridor_terms(const gqClutterGrids* grids, int rows_per_grid, float margin, float distance, int n_stations,
                              const float* samples, const int32_t* sample_link, int64_t n_samples, int n_links,
                              const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, int64_t batch,
                              const float* grasp_axis, const float* up_approach, float w_approach, float* e_approach, int accumulate,
                              float* link_wrench, float* gRt, void* stream) {
  const int rc = gq_clutter_check(grids, batch, rows_per_grid, n_links, n_samples);
  if (rc != GQ_OK) return rc;
  const gqSceneGrid first = gq_stack_grid(grids);
  if (gq_approach_check(&first, batch, n_links, n_samples, distance, n_stations, grasp_axis) != GQ_OK)
    return gq_retell("clutter", "corridor");
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "clutter: bad arguments");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "clutter: margin must be finite and >= 0, got %g", (double)margin);
  GqCorridorArgs c{};
  c.a = gq_approach_args(first, margin, distance, n_stations, samples, sample_link, n_samples, n_links, hand_pose, pose_dim, Rg,
                         link_T, grasp_axis, up_approach, w_approach, e_approach, accumulate, link_wrench, gRt);
  c.rows_per_grid = rows_per_grid;
  hipLaunchKernelGGL(gq_clutter_corridor_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_clutter_query(const gqClutterGrids* grids, const float* points, int64_t n_points, int64_t points_per_grid, float* phi,
                     float* grad, uint8_t* inside, void* stream) {
  const int rc = gq_clutter_check_grids(grids);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(n_points >= 0 && n_points <= (1ll << 31) * 255, "clutter: n_points must be in 0..255*2^31, got %lld", (long long)n_points);
  GQ_REQUIRE(points_per_grid >= 0 && n_points == (int64_t)grids->n_grids * points_per_grid,
             "clutter: n_points must be n_grids * points_per_grid = %d * %lld, got %lld", grids->n_grids, (long long)points_per_grid,
             (long long)n_points);
  if (n_points == 0) return GQ_OK;
  GQ_REQUIRE(points && phi, "clutter: points / phi is NULL");
  hipLaunchKernelGGL(gq_clutter_query_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     gq_stack_grid(grids), points_per_grid, points, n_points, phi, grad, inside);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_clutter_compose_check(const gqClutterGrids* out, const gqSceneGrid* parts, int n_parts, const gqSceneGrid* base, float far) {
  GQ_REQUIRE(out, "clutter: compose: out is NULL");
  GQ_REQUIRE(out->n_grids >= 1 && out->n_grids <= GQ_CL_MAX_GRIDS, "clutter: compose: out n_grids must be in 1..%d, got %d",
             GQ_CL_MAX_GRIDS, out->n_grids);
  const gqSceneGrid first = gq_stack_grid(out);
  if (gq_scene_check(&first, 1, 1, 1) != GQ_OK) return gq_retell("clutter", "compose: out");
  if (gq_tiling_check(out, "clutter: compose: out") != GQ_OK) return GQ_ERR_ARG;
  GQ_REQUIRE(n_parts >= 0 && n_parts <= GQ_CL_MAX_PARTS, "clutter: compose: n_parts must be in 0..%d, got %d", GQ_CL_MAX_PARTS,
             n_parts);
  GQ_REQUIRE(n_parts == 0 || parts, "clutter: compose: parts is NULL");
  GQ_REQUIRE(n_parts > 0 || base, "clutter: compose: n_parts == 0 needs a base");
  if (base && gq_scene_check(base, 1, 1, 1) != GQ_OK) return gq_retell("clutter", "compose: base");
  for (int p = 0; p < n_parts; ++p)
    if (gq_scene_check(parts + p, 1, 1, 1) != GQ_OK) {
      char what[48];
      snprintf(what, sizeof(what), "compose: parts[%d]", p);
      return gq_retell("clutter", what);
    }
  GQ_REQUIRE(far > -GQ_INF_F && far < GQ_INF_F, "clutter: compose: far must be finite, got %g", (double)far);
  return GQ_OK;
}

int gq_clutter_compose(const gqClutterGrids* out, float* out_values, const float* target_T, const gqSceneGrid* parts, int n_parts,
                       const float* part_T, const int32_t* exclude, const gqSceneGrid* base, float far, void* stream) {
  const int rc = gq_clutter_compose_check(out, parts, n_parts, base, far);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(out_values && out_values == out->values, "clutter: compose: out_values must be out->values");
  GQ_REQUIRE(target_T, "clutter: compose: target_T is NULL");
  GQ_REQUIRE(n_parts == 0 || part_T, "clutter: compose: part_T is NULL");
  GqComposeArgs c{};
  c.out = gq_stack_grid(out);
  c.out_values = out_values;
  c.target_T = target_T, c.part_T = part_T, c.exclude = exclude;
  for (int p = 0; p < n_parts; ++p) c.parts[p] = parts[p];
  c.n_parts = n_parts;
  c.has_base = base != nullptr;
  if (base) c.base = *base;
  c.tiling = gq_tiling(out->nx, out->ny, out->nz);
  c.far = far;
  const long long blocks = gq_tiling_blocks(c.tiling, out->n_grids);  // <= 2^23: gq_tiling_check
  hipLaunchKernelGGL(gq_clutter_compose_kernel, dim3((unsigned)blocks), dim3(GQ_CL_THREADS), 0, (hipStream_t)stream, c);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
