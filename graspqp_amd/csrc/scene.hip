// Scene obstacles for the MALA* stepper: the hand's surface samples must stay outside a signed-distance grid of the
// surroundings (an ESDF / TSDF volume, positive outside the obstacles), as ONE launch of its own:
//
//   E_scene = sum_s max(margin - phi(x_w(s)), 0)          x_h = T_link p (hand frame), x_w = R x_h + t
//
// with phi the trilinear interpolant of the grid (scene_dev.h); a sample outside the volume is in free space.  The launch
// also emits the gradient in the form gq_fk_backward takes (include/graspqp_hip.h): link wrenches (f, m about the hand
// origin, hand frame) and gRt = [gsum(3), K(9)] with grad_t = -R gsum and grad_R = R K.  A sample with phi < margin pulls
// with g_w = -up grad phi(x_w), g_h = R' g_w.  Unlike the table plane (tabletop.hip) every sample has its own force, so
// per link six numbers are reduced, and nine more for K:
//
//   f_l = sum g_h        m_l = sum x_h x g_h        gsum = -sum_l f_l        K = sum g_h (x) x_h
//
// One block of eight wavefronts per row, as gq_tabletop_kernel: the link transforms of the row are staged in LDS while the
// first samples are in flight; wavefront w takes the 64-sample chunks w, w+8, ...: lane = sample.  Per sample the
// transform, the cell, the 8 node loads (issued together), then value and gradient.  For every link met in the chunk the
// six masked values are summed over the wavefront by the DPP network and added to the accumulators that lane l keeps for
// link l; K stays in nine per-lane accumulators over the lane's chunks and is folded once at the end.  The upstream factor
// multiplies the finished sums.  The eight wavefronts' partial sums are folded in wavefront order, link l by lane l of
// wavefront 0.  No atomics: the order of every sum depends only on the order of the samples, so results are bitwise
// reproducible run to run.
#include "scene_row_dev.h"  // the row body, shared with gq_clutter_kernel (clutter.hip)

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_scene_kernel(const GqSceneArgs g) { gq_scene_row(g, g.grid); }

// one query per lane: the differentiable building block for arbitrary world points
__global__ __launch_bounds__(256) void gq_scene_query_kernel(const gqSceneGrid grid, const float* __restrict__ points, int64_t N,
                                                             float* __restrict__ phi, float* __restrict__ grad,
                                                             uint8_t* __restrict__ inside) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const gq3 x = gq_mk(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]);
  float f = GQ_INF_F;  // outside the volume: free space
  gq3 gp = gq_mk(0, 0, 0);
  const int where = gq_scene_sample(grid, x, f, gp);
  if (where == GQ_SCENE_NONFINITE) f = gp.x = gp.y = gp.z = __builtin_nanf("");
  phi[i] = f;
  if (grad) grad[i * 3] = gp.x, grad[i * 3 + 1] = gp.y, grad[i * 3 + 2] = gp.z;
  if (inside) inside[i] = where == GQ_SCENE_INSIDE;
}

// total[row] += w_scene E_scene[row]: the FK backward's row total holds the five terms of its own tail
__global__ __launch_bounds__(256) void gq_scene_total_kernel(float* __restrict__ total, const float* __restrict__ e_scene,
                                                             float w_scene, int64_t B) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row < B) total[row] += w_scene * e_scene[row];
}

static int gq_scene_check_grid(const gqSceneGrid* grid) {
  GQ_REQUIRE(grid, "scene: grid is NULL");
  GQ_REQUIRE(grid->values, "scene: grid values is NULL");
  GQ_REQUIRE(grid->nx >= 2, "scene: grid nx must be >= 2, got %d", grid->nx);
  GQ_REQUIRE(grid->ny >= 2, "scene: grid ny must be >= 2, got %d", grid->ny);
  GQ_REQUIRE(grid->nz >= 2, "scene: grid nz must be >= 2, got %d", grid->nz);
  GQ_REQUIRE((long long)grid->nx * grid->ny <= (1ll << 28) && (long long)grid->nx * grid->ny * grid->nz <= (1ll << 28),
             "scene: grid nx*ny*nz must be <= 2^28 nodes, got %d x %d x %d", grid->nx, grid->ny, grid->nz);
  GQ_REQUIRE(grid->voxel > 0.0f && grid->voxel < GQ_INF_F, "scene: grid voxel must be finite and > 0, got %g", (double)grid->voxel);
  for (int a = 0; a < 3; ++a)
    GQ_REQUIRE(grid->origin[a] > -GQ_INF_F && grid->origin[a] < GQ_INF_F, "scene: grid origin[%d] must be finite, got %g", a,
               (double)grid->origin[a]);
  return GQ_OK;
}

int gq_scene_check(const gqSceneGrid* grid, int64_t batch, int n_links, int64_t n_samples) {
  const int rc = gq_scene_check_grid(grid);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "scene: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(n_links > 0 && n_links <= GQ_ROW_MAX_LINKS, "scene: n_links must be in 1..%d, got %d", GQ_ROW_MAX_LINKS, n_links);
  GQ_REQUIRE(n_samples > 0 && n_samples <= (1ll << 24), "scene: n_samples must be in 1..2^24, got %lld", (long long)n_samples);
  return GQ_OK;
}

int gq_scene_terms(const gqSceneGrid* grid, float margin, const float* samples, const int32_t* sample_link, int64_t n_samples,
                   int n_links, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, int64_t batch,
                   const float* up_scene, float w_scene, float* e_scene, int accumulate, float* link_wrench, float* gRt,
                   void* stream) {
  const int rc = gq_scene_check(grid, batch, n_links, n_samples);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "scene: bad arguments");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "scene: margin must be finite and >= 0, got %g", (double)margin);
  const GqSceneArgs a = gq_scene_args(*grid, margin, samples, sample_link, n_samples, n_links, hand_pose, pose_dim, Rg, link_T,
                                      up_scene, w_scene, e_scene, accumulate, link_wrench, gRt);
  hipLaunchKernelGGL(gq_scene_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_scene_query(const gqSceneGrid* grid, const float* points, int64_t n_points, float* phi, float* grad, uint8_t* inside,
                   void* stream) {
  const int rc = gq_scene_check_grid(grid);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(n_points >= 0 && n_points <= (1ll << 31) * 255, "scene: n_points must be in 0..255*2^31, got %lld", (long long)n_points);
  if (n_points == 0) return GQ_OK;
  GQ_REQUIRE(points && phi, "scene: points / phi is NULL");
  hipLaunchKernelGGL(gq_scene_query_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *grid,
                     points, n_points, phi, grad, inside);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_scene_total(float* total, const float* e_scene, float w_scene, int64_t batch, void* stream) {
  GQ_REQUIRE(total && e_scene && batch > 0 && batch <= 0x7fffffffll, "scene_total: bad arguments");
  hipLaunchKernelGGL(gq_scene_total_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total,
                     e_scene, w_scene, batch);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
