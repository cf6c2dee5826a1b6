// Approach clearance for the MALA* stepper: the corridor the hand travels along its approach axis must be free of the
// surroundings' signed-distance grid, as ONE launch of its own.  Station k = 1..K is the whole hand, joints unchanged, moved
// back by d_k = D k / K against its approach direction a (hand frame, HandSpec.grasp_axis):
//
//   y_k = x_h - d_k a      x_w^k = R y_k + t      E_approach = (1/K) sum_k sum_s max(margin - phi(x_w^k), 0)
//
// with x_h = T_link p and phi the trilinear interpolant of scene_dev.h (the contract of E_scene: outside the volume is free
// space, a non-finite point makes the row NaN and is never an index).  d = 0 is not a station: that is E_scene.  The launch
// emits the gradient in the form gq_fk_backward takes.  An active (s, k) pulls with g_w = -up (1/K) grad phi(x_w^k),
// g_h = R' g_w:
//
//   f_l = sum g_h      m_l = sum x_h x g_h  (x_h unshifted: the joints move x_h, not the offset)
//   gsum = -sum_l f_l  K9 = sum g_h (x) y_k (the shifted point: d x_w^k / d R acts on y_k)
//
// Shaped like gq_scene_kernel: one block of eight wavefronts per row, link transforms staged in LDS, lane = sample, wavefront
// w takes the 64-sample chunks w, w+8, ...  x_h is computed once per sample; the stations are an inner loop of the lane in
// ascending k.  The lane sums g_h over its stations (the moment x_h x sum g_h follows from it) and keeps the nine K9
// accumulators, so the per-link DPP reductions run once per chunk, not once per station.
//
// The gathers are the latency chain: K rounds of 8 loads per lane, each round behind the address arithmetic of its own point.
// Each station's loads are issued together inside gq_scene_sample and consumed there; a station's loads are not in flight
// during the previous station's interpolation (DESIGN 15 says what was tried and what the code object showed).  The latency
// is covered by the other seven wavefronts of the row and by the rows that share the compute unit.
//
// No atomics: stations ascending inside the lane, then the orders of gq_scene_kernel; bitwise reproducible run to run.
#include "approach_row_dev.h"  // the row body, shared with gq_clutter_corridor_kernel (clutter.hip)

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_approach_kernel(const GqApproachArgs g) { gq_approach_row(g, g.grid); }

int gq_approach_check(const gqSceneGrid* grid, int64_t batch, int n_links, int64_t n_samples, float distance, int n_stations,
                      const float* grasp_axis) {
  if (gq_scene_check(grid, batch, n_links, n_samples) != GQ_OK) {
    char why[400];
    snprintf(why, sizeof(why), "%s", gq_last_error());
    GQ_FAIL(GQ_ERR_ARG, "approach: %s", why);
  }
  GQ_REQUIRE(distance > 0.0f && distance < GQ_INF_F, "approach: distance must be finite and > 0, got %g", (double)distance);
  GQ_REQUIRE(n_stations >= 1 && n_stations <= GQ_AP_MAX_STATIONS, "approach: n_stations must be in 1..%d, got %d",
             GQ_AP_MAX_STATIONS, n_stations);
  GQ_REQUIRE(grasp_axis, "approach: grasp_axis is NULL");
  for (int i = 0; i < 3; ++i)
    GQ_REQUIRE(grasp_axis[i] > -GQ_INF_F && grasp_axis[i] < GQ_INF_F, "approach: grasp_axis[%d] must be finite, got %g", i,
               (double)grasp_axis[i]);
  GQ_REQUIRE(grasp_axis[0] != 0.0f || grasp_axis[1] != 0.0f || grasp_axis[2] != 0.0f, "approach: grasp_axis must not be all zero");
  return GQ_OK;
}

int gq_approach_terms(const gqSceneGrid* grid, float margin, float distance, int n_stations, const float* samples,
                      const int32_t* sample_link, int64_t n_samples, int n_links, const float* hand_pose, int pose_dim,
                      const float* Rg, const float* link_T, int64_t batch, const float* grasp_axis, const float* up_approach,
                      float w_approach, float* e_approach, int accumulate, float* link_wrench, float* gRt, void* stream) {
  const int rc = gq_approach_check(grid, batch, n_links, n_samples, distance, n_stations, grasp_axis);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "approach: bad arguments");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "approach: margin must be finite and >= 0, got %g", (double)margin);
  const GqApproachArgs a = gq_approach_args(*grid, margin, distance, n_stations, samples, sample_link, n_samples, n_links, hand_pose,
                                            pose_dim, Rg, link_T, grasp_axis, up_approach, w_approach, e_approach, accumulate,
                                            link_wrench, gRt);
  hipLaunchKernelGGL(gq_approach_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
