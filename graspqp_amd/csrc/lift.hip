// Lift clearance for the MALA* stepper: after the fingers close, hand and object leave together, and the object is usually wider
// than the hand.  The rigid body "hand + held object" on the first centimetres of the way out must be free of the surroundings'
// signed-distance grid (a grid that leaves the target out), as ONE launch of its own.  The carry is one straight translation by
// s_k c, c = H u - D R a, s_k = k / K for k = 1..K: u the lift direction (a unit vector of the object's frame, used as given),
// H = height, D = retreat, a the approach axis of the hand (hand frame, HandSpec.grasp_axis).  D = 0 is a pure lift, H = 0 the
// reverse of the approach, both together the diagonal way out of a shelf.  With d_k = D k / K and h_k = H k / K:
//
//   hand    y_k = x_h - d_k a      x_w^k = R y_k + (t + h_k u)
//   object  x^{j,k} = p_j + h_k u - d_k R a             (p_j in the object's frame, which is the grid's)
//   E_lift = (1/K) sum_k [ sum_s max(m_h - phi(x_w^k), 0) + sum_j max(m_o - phi(x^{j,k}), 0) ]
//
// phi is the trilinear interpolant of scene_dev.h under the contract of E_scene (outside the volume is free space, a non-finite
// point makes the row NaN and is never an index).  Station 0 is not part of the term: the hand there is E_scene, and the object at
// rest touches what it stands on.  The gradient, in the form gq_fk_backward takes, with g_h = R' (-up (1/K) grad phi):
//
//   hand    f_l = sum g_h      m_l = sum x_h x g_h      gsum = -sum g_h      K9 += g_h (x) y_k     (h_k u depends on nothing)
//   object  K9 += g_h (x) (-d_k a), and nothing else: t does not move the object (no gsum), no joint does (no wrench)
//
// Shaped like gq_approach_kernel: one block of eight wavefronts per row, link transforms staged in LDS, lane = sample, wavefront w
// takes the hand chunks w, w+8, ... and then the object chunks w, w+8, ... of 64 points; the stations are an inner loop of the lane
// in ascending k.  The object part has no per-link reductions; it feeds the lane's energy and K9 accumulators and a second energy
// sum, the object's share.  One GQ_ROW_WAVE_PARTIALS, the folds of sample_row_dev.h.  With H = 0 and no object points every
// operation on e, the wrenches and gRt is gq_approach_row's in its order: the bits of gq_clutter_corridor_terms.
//
// No atomics, fixed orders: bitwise reproducible run to run, and a row's bits do not depend on the batch around it.
#include "lift_row_dev.h"

__global__ __launch_bounds__(GQ_ROW_WAVES * GQ_WAVE) void gq_lift_kernel(const GqLiftArgs g) {
  const gqSceneGrid grid = gq_stack_grid(g.grid, blockIdx.x / (unsigned)g.rows_per_grid);
  gq_lift_row(g, grid);
}

static bool gq_lift_finite(float v) { return v > -GQ_INF_F && v < GQ_INF_F; }

int gq_lift_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_links, int64_t n_samples, int64_t n_obj,
                  int64_t batch_each, int64_t n_object_points, float height, float retreat, int n_stations, const float* grasp_axis,
                  const float* direction, float margin, float object_margin) {
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "lift: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(rows_per_grid >= 1 && rows_per_grid <= 0x7fffffffll, "lift: rows_per_grid must be in 1..2^31-1, got %lld",
             (long long)rows_per_grid);
  GQ_REQUIRE(n_links > 0 && n_links <= GQ_ROW_MAX_LINKS, "lift: n_links must be in 1..%d, got %d", GQ_ROW_MAX_LINKS, n_links);
  GQ_REQUIRE(n_samples > 0 && n_samples <= (1ll << 24), "lift: n_samples must be in 1..2^24, got %lld", (long long)n_samples);
  // grids == NULL: the parameters alone, before a scene exists (gq_lift_terms refuses a NULL stack itself)
  if (grids && gq_clutter_check(grids, batch, (int)rows_per_grid, n_links, n_samples) != GQ_OK) return gq_retell("lift", "grids");
  // batch / batch_each, not n_obj * batch_each: the product of two unchecked int64 could overflow
  GQ_REQUIRE(n_obj >= 1 && batch_each >= 1 && batch_each <= batch && batch % batch_each == 0 && batch / batch_each == n_obj,
             "lift: batch must be n_obj * batch_each = %lld * %lld, got %lld", (long long)n_obj, (long long)batch_each,
             (long long)batch);
  GQ_REQUIRE(n_object_points >= 0 && n_object_points <= (1ll << 24), "lift: n_object_points must be in 0..2^24, got %lld",
             (long long)n_object_points);
  GQ_REQUIRE(height >= 0.0f && height < GQ_INF_F, "lift: height must be finite and >= 0, got %g", (double)height);
  GQ_REQUIRE(retreat >= 0.0f && retreat < GQ_INF_F, "lift: retreat must be finite and >= 0, got %g", (double)retreat);
  GQ_REQUIRE(height + retreat > 0.0f, "lift: height + retreat must be > 0: the carry has no length");
  GQ_REQUIRE(n_stations >= 1 && n_stations <= GQ_LIFT_MAX_STATIONS, "lift: n_stations must be in 1..%d, got %d", GQ_LIFT_MAX_STATIONS,
             n_stations);
  GQ_REQUIRE(grasp_axis, "lift: grasp_axis is NULL");
  for (int i = 0; i < 3; ++i)
    GQ_REQUIRE(gq_lift_finite(grasp_axis[i]), "lift: grasp_axis[%d] must be finite, got %g", i, (double)grasp_axis[i]);
  GQ_REQUIRE(grasp_axis[0] != 0.0f || grasp_axis[1] != 0.0f || grasp_axis[2] != 0.0f, "lift: grasp_axis must not be all zero");
  GQ_REQUIRE(direction, "lift: direction is NULL");
  for (int i = 0; i < 3; ++i)
    GQ_REQUIRE(gq_lift_finite(direction[i]), "lift: direction[%d] must be finite, got %g", i, (double)direction[i]);
  GQ_REQUIRE(direction[0] != 0.0f || direction[1] != 0.0f || direction[2] != 0.0f, "lift: direction must not be all zero");
  GQ_REQUIRE(margin >= 0.0f && margin < GQ_INF_F, "lift: margin must be finite and >= 0, got %g", (double)margin);
  GQ_REQUIRE(gq_lift_finite(object_margin), "lift: object_margin must be finite, got %g", (double)object_margin);
  return GQ_OK;
}

int gq_lift_terms(const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float object_margin, float height, float retreat,
                  int n_stations, const float* samples, const int32_t* sample_link, int64_t n_samples, int n_links,
                  const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, int64_t batch,
                  const float* object_points, int64_t n_obj, int64_t batch_each, int64_t n_object_points, const float* grasp_axis,
                  const float* direction, const float* up_lift, float w_lift, float* e_lift, float* e_object, int accumulate,
                  float* link_wrench, float* gRt, void* stream) {
  GQ_REQUIRE(grids, "lift: grids is NULL");
  const int rc = gq_lift_check(grids, batch, rows_per_grid, n_links, n_samples, n_obj, batch_each, n_object_points, height, retreat,
                               n_stations, grasp_axis, direction, margin, object_margin);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && link_T && pose_dim >= 9, "lift: bad arguments");
  GQ_REQUIRE(n_object_points == 0 || object_points, "lift: object_points is NULL with n_object_points = %lld",
             (long long)n_object_points);
  GqLiftArgs a{};
  a.grid = gq_stack_grid(grids);
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.link_T = link_T;
  a.object_points = object_points, a.up_lift = up_lift;
  a.Ns = (int)n_samples, a.L = n_links, a.D = pose_dim, a.K = n_stations, a.M = (int)n_object_points;
  a.rows_per_grid = (int)rows_per_grid, a.batch_each = (int)batch_each;
  a.margin = margin, a.object_margin = object_margin, a.w_lift = w_lift, a.height = height, a.retreat = retreat;
  a.ax = grasp_axis[0], a.ay = grasp_axis[1], a.az = grasp_axis[2];
  a.ux = direction[0], a.uy = direction[1], a.uz = direction[2];
  a.accumulate = accumulate != 0;
  a.e_lift = e_lift, a.e_object = e_object, a.wrench = link_wrench, a.gRt = gRt;
  hipLaunchKernelGGL(gq_lift_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
