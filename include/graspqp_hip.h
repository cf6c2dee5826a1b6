/* graspqp_hip.h -- C ABI of libgraspqp_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the per-MALA*-iteration hot path of leggedrobotics/graspqp.  Every entry point
 * replaces one interface of the (Python) reference; the reference file:line it stands in for is cited.
 *
 * Conventions
 *   - all array arguments are DEVICE pointers unless the name ends in _host; tensors are dense, row-major,
 *     float32 / int32 / int64 exactly as noted; the caller owns every buffer (no ownership transfer);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it and
 *     graph-capturable (no allocation / synchronisation inside) except the *_create functions;
 *   - return value 0 = ok, otherwise an error code; gq_last_error() returns a thread-local message;
 *     nothing throws across the ABI;
 *   - workspaces are caller-provided; their sizes come from the matching *_workspace_bytes function.
 */
#ifndef GRASPQP_HIP_H
#define GRASPQP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------------- */
int gq_version(void);
const char* gq_last_error(void);
int gq_device_check(int device, char* arch_out, int arch_len);
/* gqTimer: event pair that a launch taking a `timer` argument fills with the kernel's own start/stop timestamps */
int gq_timer_create(void** out);
int gq_timer_elapsed_ms(void* timer, float* ms);
int gq_timer_destroy(void* timer);

/* ---- mesh signed distance: torchsdf.compute_sdf / index_vertices_by_faces ------------------------
 * reference call sites: core/object_model.py:147,220  core/hand_model.py:352,953
 * contract: dist_sq (N) squared distance; sign (N) int32 +1 outside / -1 inside; normal (N,3) unit
 * (p - closest)/|p - closest| (may be NULL); closest (N,3).  Only dist_sq is differentiable, w.r.t. points. */
typedef struct gqMeshSet gqMeshSet; /* n_mesh triangle soups resident on the device */
int gq_meshset_create(const float* face_verts_host /* (sumF,3,3) */, const int32_t* face_offset_host /* (n_mesh+1) */,
                      int n_mesh, gqMeshSet** out);
int gq_meshset_destroy(gqMeshSet* ms);
/* Device and host allocations currently held by all set-up objects of the process (gqMeshSet, gqBvh, gqPointGrid, gqHand, gqCloudSet):
 * an exact measure of their lifetime -- every create raises it, the matching destroy takes it back.                        */
int gq_setup_live_allocations(int64_t* n);
/* setup-time 32^3 occupancy grid + per-voxel candidate faces per mesh; required by penetration_only = 1 and the fused steps */
int gq_meshset_build_occupancy(gqMeshSet* ms);
int gq_meshset_num_faces(const gqMeshSet* ms, int mesh /* -1 = all */, int64_t* n);
int gq_sdf_workspace_bytes(int64_t n_faces, size_t* bytes);
int gq_sdf_forward(const float* points /* (N,3) */, int64_t n_points, const float* face_verts /* (F,3,3) */,
                   int64_t n_faces, float* dist_sq, int32_t* sign, float* normal, float* closest, void* workspace,
                   size_t workspace_bytes, void* stream);
/* object_model.py:217-220: query q uses mesh q / queries_per_mesh (one mesh per object) */
int gq_sdf_forward_meshset(const gqMeshSet* ms, const float* points, int64_t n_points, int64_t queries_per_mesh,
                           float* dist_sq, int32_t* sign, float* normal, float* closest, void* stream);
/* The same query for MANY points against ONE mesh (the per-link calls of HandModel.cal_distance, core/hand_model.py:
 * 914-953: batch * 2500 surface points per call): one query per lane through an implicit 4-ary box hierarchy over the
 * Morton-sorted faces, staged in LDS when it fits (csrc/bvh.hip).  Exact (same winner rule as gq_sdf_forward: smallest
 * ranking distance, ties to the smallest face index; the winner is finished exactly).  gq_bvh_create takes HOST triangles
 * (n_faces,3,3), 1 <= n_faces <= 65536.                                                                                 */
typedef struct gqBvh gqBvh;
int gq_bvh_create(const float* face_verts_host, int64_t n_faces, gqBvh** out);
int gq_bvh_destroy(gqBvh* bvh);
int gq_sdf_forward_bvh(const gqBvh* bvh, const float* points, int64_t n_points, float* dist_sq, int32_t* sign,
                       float* normal /* or NULL */, float* closest, void* stream);
int gq_sdf_backward(const float* grad_dist_sq, const float* points, const float* closest, int64_t n_points,
                    float* grad_points, void* stream);

/* ---- objects as oriented point clouds: surfel signed distance for the contact query ------------------------------------
 * For objects that come as points with normals (scans, open shells, unions of parts) instead of watertight meshes; it takes
 * the place of gq_sdf_forward_meshset (core/object_model.py:186-255) and has no counterpart in the reference.
 * A cloud is N points p_i with unit outward normals n_i and one radius rho > 0, read as N oriented discs.  For a query x:
 *   1. nearest sample  j = argmin_i |x - p_i|^2, ties to the smallest index (nearest CENTRE);
 *   2. v = x - p_j, h = v . n_j, lat = v - h n_j, l = |lat|;
 *   3. closest = p_j + lat min(1, rho / l): the nearest point of disc j (x - h n_j over the disc, a rim point beyond it);
 *   4. dist_sq = |x - closest|^2;
 *   5. sign = +1 if h >= 0 else -1 (int32, +1 outside);
 *   6. normal = sign n_j for l <= rho (no division; a query on the disc gets n_j), (x - closest)/|x - closest| beyond the rim.
 * Only dist_sq is differentiable, w.r.t. x, as 2 (x - closest) -- exact for the distance to a disc: gq_sdf_backward applies.
 * dist_sq (N), sign (N), normal (N,3) (may be NULL), closest (N,3): layout and meaning of gq_sdf_forward_meshset.
 * gq_cloudset_create takes HOST arrays: points / normals (sumN,3), offsets (n_obj+1) starting at 0, radius (n_obj); normals are
 * normalised in double; 1 <= N <= 2^20 per cloud.  A zero or non-finite normal, a non-finite point, N = 0 or rho <= 0 is
 * refused before anything touches the device.  The set counts in gq_setup_live_allocations.
 * gq_cloud_forward: query q uses cloud q / queries_per_object; one wavefront per query walks the cloud's uniform grid outward
 * from the query's (clamped) cell and returns the brute-force winner (csrc/cloud.hip); no workspace, no atomics, bitwise
 * reproducible.  A non-finite query, or one so far away that d^2 overflows float32, gives NaN outputs with sign +1.
 * gq_cloud_check is the argument check of both on its own (host only, no GPU): gq_cloudset_create calls it with n_points =
 * n_obj and queries_per_object = 1, gq_cloud_forward with the set's own offsets and radii.                               */
typedef struct gqCloudSet gqCloudSet;
int gq_cloud_check(int64_t n_obj, const int32_t* offsets_host /* (n_obj+1) */, const float* radius_host /* (n_obj) */,
                   int64_t n_points, int64_t queries_per_object);
int gq_cloudset_create(const float* points_host /* (sumN,3) */, const float* normals_host /* (sumN,3) */,
                       const int32_t* offsets_host /* (n_obj+1) */, const float* radius_host /* (n_obj) */, int n_obj,
                       gqCloudSet** out);
int gq_cloudset_destroy(gqCloudSet* cs);
int gq_cloud_forward(const gqCloudSet* cs, const float* points /* (n_points,3) */, int64_t n_points,
                     int64_t queries_per_object, float* dist_sq, int32_t* sign, float* normal /* or NULL */, float* closest,
                     void* stream);

/* ---- box-constrained QP: qpth.qp.QPFunction as used by SQPLsqSolver.solve --------------------------
 * reference: metrics/solver/qp_solver.py:8,60-134 (QPFunction(maxIter=12, eps=5e-2), G = [I;-I], h = [u;-l]).
 * lam / slack are (B, 2 nz): upper-bound block then lower-bound block.  lower/upper may be NULL (scalars used).
 * gq_lsq_*: Q = A'A + ridge I, p = -A'b with A (B,m,nz), m <= 8, b (B,m) or NULL (= 0); nz <= 128 (dense Q: <= 64).         */
int gq_boxqp_workspace_bytes(int64_t batch, int nz, int max_iter, size_t* bytes);
int gq_boxqp_forward(const float* Q /* (B,nz,nz) */, const float* p /* (B,nz) or NULL */, const float* lower,
                     const float* upper, float lower_s, float upper_s, int64_t batch, int nz, float eps, int max_iter,
                     int not_improved_lim, float* x, float* lam, float* slack, int32_t* best_iter /* (B) or NULL */,
                     int32_t* n_iter /* (1) or NULL */, void* workspace, size_t workspace_bytes, void* stream);
int gq_boxqp_backward(const float* Q, const float* lam, const float* slack, const float* grad_x, int64_t batch, int nz,
                      float* dx /* (B,nz) = grad_p; grad_Q = (dx x' + x dx')/2 */,
                      float* dlam /* (B,2nz); grad_h = -dlam */, void* stream);
int gq_lsq_boxqp_forward(const float* A, const float* b, const float* lower, const float* upper, float lower_s,
                         float upper_s, int64_t batch, int m, int nz, float ridge, float eps, int max_iter,
                         int not_improved_lim, float* x, float* lam, float* slack, int32_t* best_iter, int32_t* n_iter,
                         void* workspace, size_t workspace_bytes, void* stream);
int gq_lsq_boxqp_backward(const float* A, const float* lam, const float* slack, const float* grad_x, int64_t batch,
                          int m, int nz, float ridge, float* dx, float* dlam, void* stream);
/* qpth's batch-global stopping rule (qpth/solvers/pdipm/batch.py forward loop) on the (B, max_iter)
 * tables of per-iteration residuals and mu that the forward kernels record: kstar[0] = index of the last iteration
 * whose record counts, kstar[1] = *n_iter = kstar[0] + 1.  Stop at the first iteration where no row improved its
 * running-best residual for `not_improved_lim` iterations in a row, or max_rows(best residual) < eps, or
 * min_rows(mu) > 1e32; NaN residuals never improve a row.  The forward entry points call exactly this.            */
int gq_boxqp_stop_rule(const float* resid /* (B,max_iter) */, const float* mu /* (B,max_iter) */, int64_t batch,
                       int max_iter, float eps, int not_improved_lim, float* runmin_scratch /* (B) */,
                       int32_t* kstar /* (2) */, int32_t* n_iter /* (1) or NULL */, void* stream);

/* ---- force-closure energy: energy_fnc for energy_type "graspqp" ------------------------------------
 * reference: metrics/ops/span.py:263-295,313-415  metrics/ops/registry.py:31-89
 * E_fc = values_gain (1/2 |F x|^2 + 0.01) exp(-svd_gain (prod sigma(F))^(1/6)), 1 <= x <= max_limit + 1.
 * cog is (B,3).  gq_fc_backward must follow gq_fc_forward on the same workspace.                           */
int gq_fc_workspace_bytes(int64_t batch, int n_contact, int n_cone, int max_iter, size_t* bytes);
int gq_fc_forward(const float* contact_pts, const float* contact_normals, const float* cog, int64_t batch,
                  int n_contact, int n_cone, float friction, float torque_weight, float max_limit, float svd_gain,
                  float values_gain, float eps, int max_iter, float* e_fc /* (B) */,
                  float* x_sum /* (B,n_contact) or NULL */, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                  void* stream);
int gq_fc_backward(const float* contact_pts, const float* contact_normals, const float* cog, const float* grad_e,
                   int64_t batch, int n_contact, int n_cone, float friction, float torque_weight, float svd_gain,
                   float values_gain, int accumulate /* 1: grad_contact_pts += */, float* grad_contact_pts,
                   void* workspace, size_t workspace_bytes, void* stream);
int gq_fc_peek(void* workspace, size_t workspace_bytes, int64_t batch, int n_contact, int n_cone, const float** F,
               const float** x, const float** val, const float** svd);
/* Fused form of gq_contact_terms + gq_fc_forward + gq_fc_backward for constant upstream weights (the MALA* loop,
 * scripts/fit.py:434-438: w_dis on E_dis, w_fc on E_fc): two launches per iteration instead of nine, the grasp matrix
 * stays in registers between the cone construction and the QP iterations, and qpth's batch-global stop rule is
 * replayed inside the second kernel (batches <= 256 rows: by three wavefronts beside the one that does the row's work)
 * or applied by the first kernel's last block to per-block aggregates (larger batches) -- no launch of its own either
 * way.  Inputs as gq_contact_terms; g_contact_pts receives w_dis dE_dis/dp + w_fc dE_fc/dp, g_hand_normals
 * w_dis dE_dis/dnH.  Workspace: gq_fc_workspace_bytes (it includes, per row, a slot of n_contact * n_cone * 5 floats in
 * which the first kernel keeps the row's best iterate among all iterations but the last, so that the second kernel can
 * ask for its iterate before the stop iteration is known); gq_fc_peek works afterwards.  ZERO-FILL THE WORKSPACE ONCE
 * after allocating it (hipMemset): the block counter of the large-batch stop rule lives in it and wraps back to zero
 * at the end of every launch.                                                                                       */
int gq_fc_step(const float* dist_sq, const int32_t* sign, const float* obj_dir, const float* closest,
               const float* contact_pts, const float* hand_normals, const float* cog, int64_t batch, int n_contact,
               int n_cone, float friction, float torque_weight, float max_limit, float svd_gain, float values_gain,
               float eps, int max_iter, float w_dis, float w_fc, float* obj_normal, float* g_contact_pts,
               float* g_hand_normals, float* e_fc, float* x_sum, int32_t* n_iter, void* workspace,
               size_t workspace_bytes, void* stream);

/* ---- exact grasp-quality metrics: scipy.optimize.lsq_linear behind ScipyLsqSolver -------------------------------------
 * reference: metrics/solver/scipy_solver.py:61-131 (one lsq_linear per problem), metrics/ops/registry.py:108-131
 * (GRASPQP_SCIPY, GRASPQP_EUCLIDIAN_SCIPY), metrics/ops/span.py:94-231 (Euclidean), 313-415 (overall);
 * scripts/vis/visualize_result.py:835-852 scores grasps with the Euclidean one.
 * gq_lsq_exact_forward: x = argmin 1/2 |A x - b|^2 s.t. lower <= x <= upper, solved TO OPTIMALITY (BVLS, fp64 arithmetic)
 *   for each of `batch` problems; A (B,m,nz), b (B,m), m <= 8, nz <= 128, scalar finite bounds lower <= upper.
 *   fp64 = 0: A, b, x (B,nz), cost (B) are float32; fp64 = 1: float64.  cost = 1/2 |A x - b|^2 (scipy's res.cost).
 *   status (B) int32: free-set solves used (>= 0), -1 if max_iter was reached (the last iterate is returned), -2 if
 *   A or b holds a non-finite value (x and cost NaN).  Bitwise reproducible; no workspace.
 * gq_span_exact_forward: the metric's grasp matrix F (6, n_contact * n_cone) of every row, built as gq_fc_forward does,
 *   and n_basis problems per row on it: n_basis = 1 (overall: b = 0), n_basis = 12 (Euclidean: b = +e_i, then -e_i).
 *   value (B,n_basis) = cost, x_sum (B,n_basis,n_contact) per-contact sums of x (or NULL), svd (B) = det(F F')^(1/12),
 *   status (B,n_basis) as above.  The overall metric uses [1, max_limit + 1], the Euclidean one [0, max_limit].
 * The *_check functions validate the sizes and bounds without a GPU (the forward entry points call them first).      */
int gq_lsq_exact_check(int64_t batch, int m, int nz, double lower, double upper, int max_iter);
int gq_lsq_exact_forward(const void* A, const void* b, int fp64, int64_t batch, int m, int nz, double lower,
                         double upper, int max_iter, void* x, void* cost, int32_t* status, void* stream);
int gq_span_exact_check(int64_t batch, int n_contact, int n_cone, int n_basis, double lower, double upper,
                        int max_iter);
int gq_span_exact_forward(const float* contact_pts, const float* contact_normals, const float* cog, int64_t batch,
                          int n_contact, int n_cone, float friction, float torque_weight, int n_basis, double lower,
                          double upper, int max_iter, float* value /* (B,n_basis) */,
                          float* x_sum /* (B,n_basis,n_contact) or NULL */, float* svd /* (B) */,
                          int32_t* status /* (B,n_basis) */, void* stream);

/* ---- the reference's other force-closure energies (scripts/fit.py:343-347, --energy_type dexgrasp | tdg) -------------
 * Same inputs as the graspqp energy: contact points, OBJECT normals at the contacts (constants), cog (B,3).  One launch
 * gives the energy and its gradient w.r.t. the contact points: g_contact_pts (+)= upstream * dE/dp with upstream =
 * grad_e[row] if grad_e != NULL else w; accumulate = 1 adds to g_contact_pts.  e_fc or g_contact_pts may be NULL.
 * gq_dexgrasp_energy: metrics/ops/dexgrasp.py:4-34,  E = |sum_i [n_i ; torque_weight (n_i x (p_i - cog))]|^2.
 * gq_tdg_energy: metrics/ops/tdg.py:147-239 (TDGEnergy.forward behind TDGSpanMetric): directions (P,3) = the force part of
 *   target_direction_6D (unit vectors; the torque part is zero), friction = miu_coef[0], obb_length = obj_obb_length,
 *   scale = the factor 100 of TDGSpanMetric.forward.                                                                */
int gq_dexgrasp_energy(const float* contact_pts, const float* contact_normals, const float* cog, int64_t batch,
                       int n_contact, float torque_weight, const float* grad_e /* (B) or NULL */, float w, int accumulate,
                       float* e_fc /* (B) or NULL */, float* g_contact_pts /* (B,n,3) or NULL */, void* stream);
int gq_tdg_energy(const float* contact_pts, const float* contact_normals, const float* cog, const float* directions,
                  int n_directions, int64_t batch, int n_contact, float friction, float obb_length, int enable_density,
                  float scale, const float* grad_e, float w, int accumulate, float* e_fc, float* g_contact_pts,
                  void* stream);

/* The same step with the hand-penetration branch of the iteration (gq_hand_pen_forward with penetration_only = 1, then
 * gq_hand_pen_backward in its fused-E_pen form) running in the SAME two launches: the two branches are independent
 * until gq_fk_backward, neither fills the GPU on its own at batch 256, and one grid holding both roles overlaps them
 * without a cross-stream dependency.  Fields = the parameters of gq_fc_step / gq_hand_pen_forward /
 * gq_hand_pen_backward of the same names.                                                                      */
typedef struct gqHand gqHand; /* declared with gq_hand_create below */
typedef struct gqPointGrid gqPointGrid; /* gq_pointgrid_create, below */
typedef struct gqFcStepDesc {
  const float* dist_sq; const int32_t* sign; const float* obj_dir; const float* closest;
  const float* contact_pts; const float* hand_normals; const float* cog;
  int64_t batch; int32_t n_contact; int32_t n_cone;
  float friction, torque_weight, max_limit, svd_gain, values_gain, eps; int32_t max_iter; float w_dis, w_fc;
  float* obj_normal; float* g_contact_pts; float* g_hand_normals; float* e_fc; float* x_sum; int32_t* n_iter;
  void* workspace; size_t workspace_bytes;
} gqFcStepDesc;
typedef struct gqPenStepDesc {
  const gqMeshSet* links; const float* surface_points; int64_t n_obj; int64_t n_surface; int64_t batch_each;
  const float* hand_pose; int32_t pose_dim; const float* Rg; const float* link_T;
  float* dis; int32_t* link; float* gvec;       /* link / gvec zero-initialised by the caller, see gq_hand_pen_forward */
  float* link_wrench; float* gRt; float w_pen; float* e_pen;
  uint64_t* span; uint64_t* span_acc;           /* optional in-kernel timing of the query, see gq_hand_pen_backward */
  /* optional third role of the second launch: world sphere centres + self penetration (gq_self_pen_forward on the
   * centres of link_T), so that gq_fk_forward can be called without spheres; hand == NULL: absent               */
  const gqHand* hand; float w_spen; float* e_spen; float* g_sphere_centers; float* sphere_centers /* or NULL */;
  const gqPointGrid* grid;                      /* optional: the query role runs link-driven (gq_hand_pen_forward_cells) */
  const float* patch_spheres;                   /* optional: gq_surface_patches (see gq_hand_pen_forward) */
} gqPenStepDesc;
int gq_fc_pen_step(const gqFcStepDesc* fc, const gqPenStepDesc* pen, void* stream);
/* gq_fc_pen_step for the reference's other energy types (scripts/fit.py:343-347; metrics/ops/dexgrasp.py:4-34,
 * metrics/ops/tdg.py:147-239): the contact terms of E_dis (gq_contact_terms) and gq_dexgrasp_energy / gq_tdg_energy (with
 * upstream weight w_fc, accumulated onto w_dis dE_dis/dp) as the first role of the first launch, beside the penetration
 * query; penetration backward (+ self penetration) in the second.  energy: 1 = dexgrasp, 2 = tdg; the remaining fields are
 * the parameters of the same names of gq_contact_terms / gq_dexgrasp_energy / gq_tdg_energy.  Same bits as the separate
 * launches.                                                                                                          */
typedef struct gqAltFcDesc {
  const float* dist_sq; const int32_t* sign; const float* obj_dir; const float* closest;
  const float* contact_pts; const float* hand_normals; const float* cog;
  int64_t batch; int32_t n_contact; int32_t energy;
  float torque_weight;                                            /* dexgrasp (0 at the reference's call site) */
  const float* directions; int32_t n_directions; float friction, obb_length; int32_t enable_density; float scale; /* tdg */
  float w_dis, w_fc;
  float* obj_normal; float* g_contact_pts; float* g_hand_normals; float* e_fc;
} gqAltFcDesc;
int gq_alt_pen_step(const gqAltFcDesc* alt, const gqPenStepDesc* pen, void* stream);

/* ---- hand kinematics: HandModel.set_parameters / fk / _set_contact_idxs -----------------------------
 * reference: core/hand_model.py:762-766,787-873,1220-1267  utils/transforms.py:5-13
 * The hand is described by a reduced kinematic tree (fixed joints folded, see graspqp_amd/hands/spec.py).
 * hand_pose (B, 9 + JA) = [t(3), rot6d(6), theta_actuated]; transforms are 3x4 row-major [R|t].  JA = number of
 * actuated joints (= n_dofs unless the hand is coupled, see gqHandDesc.n_actuated).                              */
typedef struct gqHandDesc { /* all pointers HOST */
  int32_t n_dofs, n_links, n_cand, n_spheres;
  const int32_t* node_parent; /* (J) parent node, -1 = base; parents precede children */
  const int32_t* node_type;   /* (J) 1 revolute, 2 prismatic */
  const float* node_pre;      /* (J,12) fixed transform parent node frame -> joint frame */
  const float* node_axis;     /* (J,3) unit axis in the joint frame */
  const int32_t* link_node;   /* (L) node a mesh link rides on, -1 = base */
  const float* link_offset;   /* (L,12) node frame -> link frame */
  const float* cand_pos;      /* (C,3) contact candidates, link frame */
  const float* cand_nrm;      /* (C,3) */
  const int32_t* cand_link;   /* (C) */
  const float* sphere;        /* (S,4) penetration spheres x y z r, link frame */
  const int32_t* sphere_link; /* (S) non-decreasing */
  const float* joints_lower;  /* (JA) limits of the ACTUATED joints (JA = n_actuated, or J when n_actuated = 0) */
  const float* joints_upper;  /* (JA) */
  /* coupled hands (reference hands/{ability_hand,panda,schunk}.py: joint_filter + joint_calc_fnc / jacobian_fnc): the pose
   * carries n_actuated joint values, the J tree joints follow theta_tree = coupling theta_actuated + coupling_offset.
   * n_actuated = 0 (or coupling = NULL): every tree joint is actuated, pose dimension 9 + J.                        */
  int32_t n_actuated;
  const float* coupling;        /* (J, n_actuated) row-major, host, or NULL */
  const float* coupling_offset; /* (J) host, or NULL */
} gqHandDesc;
typedef struct gqHand gqHand;
int gq_hand_create(const gqHandDesc* desc, gqHand** out);
int gq_hand_destroy(gqHand* h);
/* Optional head of gq_fk_forward / tail of gq_fk_backward: MalaStar.try_step and MalaStar.accept_step
 * (core/optimizer.py:199-273, 289-340; parameters as gq_mala_propose / gq_mala_accept) run in the row's block of the
 * kinematics launch (the proposal in the kinematics wavefront, the accept step in the energy wavefront of the FK
 * backward's four), so an iteration needs no launch of its own for them.  u_switch / new_idx / u_accept hold
 * `slots` iterations of random draws, (slots,B,n) / (slots,B,n) / (slots,B); slot_ctr (2 x int32, device, zeroed
 * once) selects the current slot and is advanced on the device, so that the whole iteration can be replayed from a
 * hipGraph: the host refills the buffers every `slots` iterations.                                               */
typedef struct gqProposeDesc {
  const float* hand_pose;      /* (B,D) accepted pose; the proposal goes to gq_fk_forward's hand_pose argument      */
  const float* grad;           /* (B,D) */
  const int64_t* contact_idx;  /* (B,n) accepted indices; the proposal goes to gq_fk_forward's contact_idx argument */
  const float* u_switch; const int64_t* new_idx;
  float* ema; int64_t* step; float* step_size_out /* (B) or NULL */; float* g2_scratch /* (D) */;
  const float* energy /* (B) or NULL */; int64_t batch_each; float* z_out;
  float step_size; int32_t stepsize_period; float decay, mu, switch_possibility; int32_t clip_grad;
  int32_t* slot_ctr; int32_t slots;
} gqProposeDesc;
/* Optional: the object SDF of the row's contact points (gq_sdf_forward_meshset on contact_points, queries_per_mesh =
 * batch_size * n_contact) answered in the same launch by extra wavefronts of the row's block.                   */
typedef struct gqSdfDesc {
  const gqMeshSet* meshes; int64_t queries_per_mesh;
  float* dist_sq; int32_t* sign; float* obj_dir; float* closest;
} gqSdfDesc;
typedef struct gqAcceptDesc {
  const float* u_accept; const float* z; const uint8_t* reset_mask; const int64_t* step;
  float starting_temperature, decay; int32_t annealing_period;
  float* energy; float* pose; int64_t* idx; float* grad; uint8_t* accept; float* temperature;
  int32_t n_terms; const float* terms_new; float* terms;
  int32_t* slot_ctr; int32_t slots;
} gqAcceptDesc;
int gq_fk_workspace_bytes(const gqHand* h, int64_t batch, size_t* bytes);
int gq_fk_forward(const gqHand* h, const float* hand_pose, const int64_t* contact_idx /* (B,n) */, int64_t batch,
                  int n_contact, float* Rg /* (B,9) */, float* link_T /* (B,L,12) */, float* contact_points /* (B,n,3) */,
                  float* contact_normals /* (B,n,3) */, float* sphere_centers /* (B,S,3) or NULL */,
                  float spen_scale, float* e_spen /* (B) or NULL: gq_self_pen_forward fused in */,
                  float* g_sphere_centers /* (B,S,3), with e_spen: spen_scale * dE_spen/dcentre */,
                  const gqProposeDesc* propose /* NULL, or: hand_pose / contact_idx are first WRITTEN by the proposal */,
                  const gqSdfDesc* sdf /* NULL, or the object SDF of the contact points in the same launch */,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Optional tail of gq_fk_backward: E_dis, E_joints (with its gradient) and the weighted total of one row
 * (core/energy.py:25-28,47-54; scripts/fit.py:434-438), so the iteration needs no separate reduction launch.     */
typedef struct gqRowEnergyDesc {
  const float* dist_sq;      /* (B,n) object SDF of the contact points (gq_sdf_forward*)  */
  const int32_t* sign;       /* (B,n)                                                      */
  const float* obj_dir;      /* (B,n,3) unit (p - closest)/|.|                             */
  const float* hand_normals; /* (B,n,3) world contact normals of the hand (gq_fk_forward)  */
  const float* joints_lower; /* (J) */
  const float* joints_upper; /* (J) */
  const float* e_fc;         /* (B) */
  const float* e_pen;        /* (B) */
  const float* e_spen;       /* (B) */
  int32_t n;                 /* contacts per row */
  float w_dis, w_fc, w_pen, w_spen, w_joints;
  float* e_dis;              /* (B) out */
  float* e_joints;           /* (B) out */
  float* total;              /* (B) out: sum_k w_k E_k */
} gqRowEnergyDesc;
/* analytic backward (replaces autograd through pytorch_kinematics); the workspace must be the one written by
 * gq_fk_forward for the same hand_pose.  Any gradient input may be NULL.  g_link_wrench (B,L,6) = (f, m about the
 * hand origin) in the hand frame and g_Rt (B,12) come from gq_hand_pen_backward.  energy: NULL or see above.
 * One block of four wavefronts per row: wrench chain, global-pose chain and energy / accept chain side by side,
 * every sum in a fixed order (the same bits as one wavefront per row would give).                                */
int gq_fk_backward(const gqHand* h, const float* hand_pose, const int64_t* contact_idx, int64_t batch, int n_contact,
                   const float* Rg, const float* link_T, const float* g_contact_points, const float* g_contact_normals,
                   const float* g_sphere_centers, const float* g_link_wrench, const float* g_Rt, const float* g_theta,
                   const float* g_R, float* grad_pose /* (B,9+J) */, const gqRowEnergyDesc* energy,
                   const gqAcceptDesc* accept /* NULL, or the Metropolis test on energy->total + state merge */,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- export-time kinematics: scripts/fit.py:224-300 (export_poses) --------------------------------------------
 * Explicit geometric Jacobians in the hand frame.  `workspace` is the FK workspace written by gq_fk_forward for the
 * same poses (it holds the per-joint frames), link_T the link transforms of that call.
 * gq_link_jacobian: HandModel.jacobian (core/hand_model.py:772-777 -> the pytorch_kinematics fork's tree
 *   Chain.jacobian, or the hand's jacobian_fnc for coupled hands): (B,L,6,JA) = [J_v ; J_w] of every mesh link at its
 *   frame origin, columns = actuated joints.
 * gq_contact_jacobian: the linear contact Jacobian J_v + J_w x r of hand_model.py:1176-1196, (B,n,3,J).
 * gq_joint_velocities: HandModel.get_req_joint_velocities (hand_model.py:1155-1218, coupled form): theta =
 *   pinv(J) d with the damped pseudo-inverse of hand_model.py:46-54 (lambda = 1e-3 there), J (B,m,n_dofs) with m = 3 n,
 *   directions (B,m) in the WORLD frame when Rg is given (they are rotated into the hand frame, :1166) else in the hand
 *   frame; residual (B,m) = (J theta - d)^2, ee_vel (B,m) = J theta rotated back to the world frame.  n_dofs <= 64.
 * gq_root_pose_wxyz: (B,7) = [t, unit quaternion w x y z] of hand_pose[:, :9] (fit.py:260-263).                    */
int gq_link_jacobian(const gqHand* h, int64_t batch, const float* link_T /* (B,L,12) */, float* jac /* (B,L,6,JA) */,
                     const void* workspace, size_t workspace_bytes, void* stream);
int gq_contact_jacobian(const gqHand* h, const int64_t* contact_idx /* (B,n) */, int64_t batch, int n_contact,
                        const float* link_T, float* jac /* (B,n,3,JA) */, const void* workspace, size_t workspace_bytes,
                        void* stream);
/* d (sum_ij G_ij . J_ij) / d theta for the contact Jacobian above: grad_jac (B,n,3,JA) -> grad_theta (B,JA), the kinematic
 * Hessian of the tree in closed form (what autograd through the Jacobian gives the reference for E_manipulativity,
 * core/energy.py:80-87 via hand_model.py:1155-1218).  Same link_T / workspace as gq_contact_jacobian.                     */
int gq_contact_jacobian_backward(const gqHand* h, const int64_t* contact_idx /* (B,n) */, int64_t batch, int n_contact,
                                 const float* link_T, const float* grad_jac /* (B,n,3,JA) */, float* grad_theta /* (B,JA) */,
                                 const void* workspace, size_t workspace_bytes, void* stream);
int gq_joint_velocities(const float* jac, const float* directions, const float* Rg /* (B,9) or NULL */, int64_t batch,
                        int m, int n_dofs, float damping, float* theta /* (B,n_dofs) */, float* residual /* or NULL */,
                        float* ee_vel /* or NULL */, void* stream);
int gq_root_pose_wxyz(const float* hand_pose, int64_t batch, int pose_dim, float* root_pose /* (B,7) */, void* stream);

/* ---- hand penetration: HandModel.cal_distance (E_pen) --------------------------------------------------
 * reference: core/hand_model.py:875-987, core/energy.py:57-62.  links = mesh set of the L link meshes.
 * dis (B,P) = max over links of sqrt(d^2 + 1e-8) * (-sign); link (B,P) argmax; gvec (B,P,3) = d dis / d x_h.
 * penetration_only = 0: the exact query, dis exact everywhere (links culled by their boxes only).
 * penetration_only = 1: what E_pen uses (energy.py:59-61 zeroes dis <= 0): dis is exact where it is > 0 and -1e30
 *   elsewhere; link / gvec are WRITTEN ONLY where dis > 0 (pass zero-initialised buffers).  Per link a point is looked
 *   up in the 32^3 voxel grid of the link mesh and only the voxel's candidate faces are ranked; the mesh set must have
 *   its voxel lists (gq_meshset_build_occupancy), otherwise the call fails.
 * penetration_only = 9: diagnostics -- the scan of the voxel query without candidate evaluation (timing runs; the
 *   outputs are meaningless).  Any other value is refused with an error status.
 * workspace / workspace_bytes are ignored (pass NULL, 0); they remain for ABI stability.                          */
int gq_hand_pen_forward(const gqMeshSet* links, const float* surface_points /* (n_obj,P,3) */, int64_t n_obj,
                        int64_t n_surface, int64_t batch_each, const float* hand_pose, int pose_dim, const float* Rg,
                        const float* link_T, int penetration_only, float* dis, int32_t* link, float* gvec,
                        void* workspace /* ignored: NULL */, size_t workspace_bytes /* ignored: 0 */,
                        void* timer /* gqTimer or NULL */,
                        uint64_t* span /* NULL, or {min start, max end} in 100 MHz device ticks, pre-set to {~0, 0} */,
                        const float* patch_spheres /* NULL, or gq_surface_patches of surface_points: lets every block of
                                                      the penetration_only = 1 query drop the links out of reach first */,
                        void* stream);
/* Bounding sphere (centre xyz, radius) of every 256-point slice of every object's surface points, (n_obj, ceil(P/256), 4);
 * set-up time.  Surface points in Morton order (graspqp_amd.utils.meshes.surface_points) give compact slices.        */
int gq_surface_patches(const float* surface_points, int64_t n_obj, int64_t n_surface, float* patch_spheres, void* stream);
/* The same penetration-only query (penetration_only = 1: dis exact where > 0, -1e30 elsewhere; link / gvec written only
 * where dis > 0) driven by the LINKS: a coarse uniform grid over every object's surface points (gqPointGrid, set-up
 * time; cells_per_axis 0 = default 8) lets a row's block test only the points filed under the cells a link's box can
 * touch, so the work follows the overlaps instead of points x links.  Same dis / link / gvec as gq_hand_pen_forward.  */
typedef struct gqPointGrid gqPointGrid;
int gq_pointgrid_create(const float* surface_points_host /* (n_obj,P,3) */, int64_t n_obj, int64_t n_surface,
                        int cells_per_axis, gqPointGrid** out);
int gq_pointgrid_destroy(gqPointGrid* grid);
int gq_hand_pen_forward_cells(const gqMeshSet* links, const gqPointGrid* grid, const float* surface_points, int64_t n_obj,
                              int64_t n_surface, int64_t batch_each, const float* hand_pose, int pose_dim, const float* Rg,
                              const float* link_T, float* dis, int32_t* link, float* gvec, void* timer /* gqTimer or NULL */,
                              uint64_t* span /* as gq_hand_pen_forward */, void* stream);
/* diagnostics (NULL = off): 12 device words.  Stand-alone gq_hand_pen_forward (penetration_only = 1) adds [4] (point,
 * link) pairs that reach candidate evaluation, [5] executed point-triangle rankings, [6] pairs ranked inline because the
 * block's LDS lists were full, [7] blocks, [8] (wavefront, link) bounding-sphere tests executed, [9] of those with a point
 * inside the sphere, [10] (point, link) pairs inside the link box, [11] scanning wavefronts; gq_sdf_forward_meshset adds
 * [0] 64-face cluster visits, [1] queries, sets [2] = max visits of a query, adds [3] queries with > 16 visits.  Not
 * read by the fused launches.                                                                                      */
int gq_debug_set_pen_counters(uint64_t* counters /* device, 12 words, or NULL */);
/* A/B switch: 1 = plain block -> query mapping in gq_sdf_forward_meshset; 0 (default) = XCD-aware (with >= 8 meshes the
 * queries of mesh m run on the blocks b with b % 8 == m % 8, i.e. on one XCD, so each L2 holds only its own meshes). */
int gq_debug_set_sdf_mapping(int plain);
/* clusters taken up per round by the stand-alone mesh-distance kernel: 0 = default (4), 2 / 4 forced (A/B runs; results
 * do not depend on it).                                                                                             */
int gq_debug_set_sdf_topk(int topk);
/* LDS list capacities of the stand-alone hand-penetration query: 0 = by launch size (default), 1 / 2 / 3 = 512 / 256 /
 * 128 entries per block (A/B runs; results do not depend on it).                                                  */
int gq_debug_set_pen_caps(int mode);
/* surface points per thread of the hand-penetration query: 0 = defaults (2 as a role of gq_fc_pen_step, 1 in
 * gq_hand_pen_forward), 1 / 2 forced for both (A/B runs; results do not depend on it).                              */
int gq_debug_set_pen_ppt(int ppt);
/* grad_dis (B,P) = upstream d E / d dis.  grad_dis == NULL selects the fused E_pen form: the weights are
 * w_pen * [dis > 0] and e_pen (B) = sum_j relu(dis_j) is written as well (core/energy.py:59-61).
 * span / span_acc (optional): the 64 x {min start, max end} shards filled by gq_hand_pen_forward are folded into
 * span_acc = {sum of launch spans, launches} (100 MHz ticks) and re-armed, so a hipGraph replay can time the query. */
int gq_hand_pen_backward(int n_links, const float* surface_points, int64_t n_obj, int64_t n_surface,
                         int64_t batch_each, const float* hand_pose, int pose_dim, const float* Rg,
                         const float* grad_dis /* (B,P) or NULL */, const int32_t* link, const float* gvec,
                         float* link_wrench /* (B,L,6) */, float* gRt /* (B,12) */, const float* dis /* (B,P) */,
                         float w_pen, float* e_pen /* (B) */, uint64_t* span, uint64_t* span_acc, void* stream);

/* ---- self penetration: HandModel.self_penetration (E_spen), core/hand_model.py:989-1040 ------------------
 * On given world centres: one wavefront per row stages the centres and the radii in LDS and runs the SAME pair scan as
 * the fused forms (the e_spen tail of gq_fk_forward, the self-penetration role of gq_fc_pen_step, gq_spheres_self_pen),
 * with grad_scale in the place of their w_spen: same bits on the same centres.  S <= 256, at most 64 scanned groups. */
int gq_self_pen_forward(const gqHand* h, const float* sphere_centers /* (B,S,3) world */, int64_t batch,
                        float grad_scale, float* e_spen /* (B) */,
                        float* g_centers /* (B,S,3) grad_scale * dE/dcentre */, void* stream);

/* The same term straight from the kinematics of gq_fk_forward (world sphere centres from link_T / Rg / the translation in
 * hand_pose, then the pair scan): the self-penetration role of gq_fc_pen_step as a launch of its own, bit-identical to
 * it and to the e_spen tail of gq_fk_forward.  For large batches, where it rides on the penetration branch of the
 * iteration instead of lengthening the FK forward launch.  sphere_centers (B,S,3) may be NULL.                     */
int gq_spheres_self_pen(const gqHand* h, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                        int64_t batch, float w_spen, float* sphere_centers, float* e_spen /* (B) */,
                        float* g_sphere_centers /* (B,S,3) w_spen * dE/dcentre */, void* stream);

/* ---- energy composition: core/energy.py:25-28,47-62 and scripts/fit.py:434-438 ---------------------------- */
int gq_contact_terms(const float* dist_sq, const int32_t* sign, const float* onrm, const float* closest,
                     const float* contact_pts, const float* contact_normals, int64_t batch, int n_contact, float w_dis,
                     float* obj_normal /* (B,n,3) = onrm*sign */, float* g_contact_pts, float* g_contact_normals,
                     void* stream);
/* The same terms one by one, each with its derivative, for the autograd route of the class surface (calculate_energy on
 * HandModel / ObjectModel): the derivative is written by the forward launch and the backward is a broadcast multiply with
 * the upstream row gradient -- one launch per term where the reference's torch expressions issue a dozen.
 *   gq_signed_distance: ObjectModel.cal_distance, core/object_model.py:222-227 -- distance = sqrt(dist_sq + 1e-8) * (-sign),
 *                       normal_out = normal_in * sign, g_dist_sq = d distance / d dist_sq; n = number of queries.
 *   gq_energy_dis:      core/energy.py:25-28 -- "gendexgrasp": e = sum_j exp(1 - (-obj_normal . hand_normal)) |distance|,
 *                       g_distance = d e / d distance, g_hand_normal = d e / d hand_normal; obj_normal == NULL selects the
 *                       "dexgraspnet" form e = sum_j |distance| (hand_normal / g_hand_normal unused).
 *   gq_energy_joints:   core/energy.py:47-52 -- e = sum relu(theta - upper) + relu(lower - theta) over the last n_dofs
 *                       columns of hand_pose; g_hand_pose (B, pose_dim) = d e / d hand_pose (zero in the root columns).
 *   gq_energy_pen:      core/energy.py:58-61 -- e = sum_p where(distances <= 0, 0, distances).                            */
int gq_signed_distance(const float* dist_sq, const int32_t* sign, const float* normal_in, int64_t n, float* distance,
                       float* normal_out, float* g_dist_sq, void* stream);
int gq_energy_dis(const float* distance /* (B,n) */, const float* obj_normal /* (B,n,3) or NULL */,
                  const float* hand_normal /* (B,n,3) */, int64_t batch, int n_contact, float* e_dis /* (B) */,
                  float* g_distance /* (B,n) */, float* g_hand_normal /* (B,n,3) */, void* stream);
int gq_energy_joints(const float* hand_pose, const float* joints_lower, const float* joints_upper, int64_t batch, int pose_dim,
                     int n_dofs, float* e_joints /* (B) */, float* g_hand_pose /* (B,pose_dim) */, void* stream);
int gq_energy_pen(const float* distances /* (B,P) */, int64_t batch, int64_t n_surface, float* e_pen /* (B) */, void* stream);
int gq_fill(float* y, float a, int64_t n, void* stream);

/* ---- tabletop terms of the stepper: core/energy.py:68-78 (scripts/fit.py:77-78,369-373: --w_prior, --w_wall) ------
 * One launch for both terms and their gradient, in the form gq_fk_backward takes.  Per hand surface sample (link-frame
 * point p of link sample_link): x_h = T_link p, x_w = R x_h + t with t = hand_pose[:, :3].
 *   E_wall  = sum_s max(table_z - x_w.z, 0)   (energy.py:76-78 with the plane z = table_z; the reference has table_z = 0)
 *   E_prior = 1 + (R grasp_axis)_z            (energy.py:68-74: 1 - (R grasp_axis) . (0,0,-1))
 * e_wall / e_prior are written UNWEIGHTED.  The gradient carries the upstream factor of the row: up_*[row] if the pointer
 * is given, else w_* (the idiom of gq_dexgrasp_energy).  With g_h = R' (0,0,-up) for the samples below the plane:
 *   link_wrench (B,L,6): f_l = sum g_h, m_l = sum x_h x g_h (about the hand origin, hand frame)
 *   gRt (B,12) = [gsum(3), K(9)]: gsum = -sum g_h, K = sum g_h (x) x_h  (grad_t = -R gsum, grad_R = R K)
 *   g_R (B,9): row 2 = up_prior * grasp_axis, zero elsewhere
 * accumulate = 1 adds to the three gradient buffers (the penetration branch's wrench / gRt), 0 overwrites them; links
 * without samples get a zero wrench when overwriting and are left alone when accumulating.  Fixed-order sums, no atomics:
 * bitwise reproducible run to run (the sums follow the order of the samples).  n_links <= 64; n_samples need not be a multiple of 64.
 * gq_tabletop_check is the argument check of the launch on its own (host only, no GPU).                            */
int gq_tabletop_check(int64_t batch, int n_links, int64_t n_samples);
int gq_tabletop_terms(const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                      int64_t n_samples, int n_links, const float* hand_pose, int pose_dim,
                      const float* Rg /* (B,9) */, const float* link_T /* (B,L,12) */, int64_t batch,
                      const float* grasp_axis /* 3 floats, host */, float table_z,
                      const float* up_wall /* (B) or NULL */, float w_wall,
                      const float* up_prior /* (B) or NULL */, float w_prior,
                      float* e_wall /* (B) or NULL, unweighted */, float* e_prior /* (B) or NULL, unweighted */,
                      int accumulate /* 1: add to the three gradient buffers, 0: overwrite */,
                      float* link_wrench /* (B,L,6) or NULL */, float* gRt /* (B,12) or NULL */,
                      float* g_R /* (B,9) or NULL */, void* stream);
/* total[row] += w_prior * e_prior[row] + w_wall * e_wall[row] (scripts/fit.py:434-438 for the two terms): the row total that
 * gq_fk_backward writes holds the five terms of its own tail.                                                        */
int gq_tabletop_total(float* total /* (B) in/out */, const float* e_prior, float w_prior, const float* e_wall, float w_wall,
                      int64_t batch, void* stream);

/* ---- scene obstacles of the stepper: E_scene on a signed-distance grid of the surroundings (ESDF / TSDF volume) -----
 * The grid is a plain struct.  values is phi at the nodes in metres, POSITIVE OUTSIDE the obstacles, fp32 on the device,
 * (nx,ny,nz) row-major with z fastest; origin is the world position of node (0,0,0); voxel is the one node spacing h of
 * all axes.  The memory belongs to the caller, who may overwrite values in place between launches (moving obstacles; a
 * captured graph reads the new numbers).  Limits: 2 <= nx, ny, nz, nx ny nz <= 2^28, h finite and > 0, origin finite.
 *   phi at a world point x: u = (x - origin) / h per axis.  x is INSIDE the volume iff every u_a is finite and
 *   0 <= u_a <= n_a - 1 (both ends inclusive); the cell is i_a = min(floor(u_a), n_a - 2), the weights f_a = u_a - i_a in
 *   [0,1]; phi(x) is the trilinear interpolant of the 8 nodes of the cell and grad phi(x) its own gradient, e.g.
 *   d phi / dx = (1/h) sum_jk w_j(f_y) w_k(f_z) (v_1jk - v_0jk).  A point outside the volume is free space and contributes
 *   nothing.  A point with a non-finite coordinate gives NaN and never becomes an index: the finiteness test and the clamp
 *   to [0, n_a - 2] come before the float -> int conversion and before any load.  The inside test is made on exact
 *   quantities (x_a >= origin_a, and x_a - origin_a <= h (n_a - 1) in double): one ulp beyond the last node plane is outside.
 * gq_scene_terms: one launch for the energy and its gradient, in the form gq_fk_backward takes.  Per hand surface sample
 * (link-frame point p of link sample_link): x_h = T_link p, x_w = R x_h + t with t = hand_pose[:, :3].
 *   E_scene = sum_s max(margin - phi(x_w), 0)       margin >= 0: a clearance in metres
 * (phi = z - table_z and margin 0 make it E_wall).  e_scene is written UNWEIGHTED.  The gradient carries the upstream
 * factor of the row: up_scene[row] if the pointer is given, else w_scene.  With g_w = -up grad phi(x_w) and g_h = R' g_w
 * for the samples with phi < margin:
 *   link_wrench (B,L,6): f_l = sum g_h, m_l = sum x_h x g_h (about the hand origin, hand frame)
 *   gRt (B,12) = [gsum(3), K(9)]: gsum = -sum g_h, K = sum g_h (x) x_h, row-major K[a][j] = g_h[a] x_h[j]
 *   (grad_t = -R gsum, grad_R = R K); there is no g_R.
 * accumulate = 1 adds to the two gradient buffers (a plain rounded add of the finished value: the bits of buffer + the
 * overwriting launch's value), 0 overwrites them; links without samples get a zero wrench when overwriting and are left
 * alone when accumulating.  Fixed-order sums, no atomics: bitwise reproducible run to run (the sums follow the order of the
 * samples).  n_links <= 64; n_samples need not be a multiple of 64; a link id outside the hand is ignored.  A row with a
 * non-finite sample position gets a NaN energy and gradient; the other rows are unaffected.
 * gq_scene_check is the argument check of the launch on its own (host only, no GPU); its message names the argument.
 * gq_scene_query: phi (N), grad phi (N,3) and inside (N) at arbitrary world points (N,3), one point per lane, by the same
 * device body (csrc/scene_dev.h): bit for bit the fused launch's numbers at the same point.  Outside the volume
 * phi = +inf, grad = 0, inside = 0; a non-finite point gives NaN phi and grad, inside = 0.                            */
typedef struct gqSceneGrid {
  const float* values;  /* (nx,ny,nz) device, fp32, z fastest: phi at the nodes, positive outside the obstacles */
  int nx, ny, nz;
  float origin[3];      /* world position of node (0,0,0) */
  float voxel;          /* node spacing h > 0, all axes */
} gqSceneGrid;
int gq_scene_check(const gqSceneGrid* grid, int64_t batch, int n_links, int64_t n_samples);
int gq_scene_terms(const gqSceneGrid* grid, float margin, const float* samples /* (Ns,3) link frame, device */,
                   const int32_t* sample_link /* (Ns) */, int64_t n_samples, int n_links, const float* hand_pose, int pose_dim,
                   const float* Rg /* (B,9) */, const float* link_T /* (B,L,12) */, int64_t batch,
                   const float* up_scene /* (B) or NULL */, float w_scene, float* e_scene /* (B) or NULL, unweighted */,
                   int accumulate /* 1: add to the two gradient buffers, 0: overwrite */,
                   float* link_wrench /* (B,L,6) or NULL */, float* gRt /* (B,12) or NULL */, void* stream);
int gq_scene_query(const gqSceneGrid* grid, const float* points /* (N,3) world, device */, int64_t n_points,
                   float* phi /* (N) */, float* grad /* (N,3) or NULL */, uint8_t* inside /* (N) or NULL */, void* stream);
/* total[row] += w_scene * e_scene[row]: the row total that gq_fk_backward writes holds the five terms of its own tail. */
int gq_scene_total(float* total /* (B) in/out */, const float* e_scene, float w_scene, int64_t batch, void* stream);

/* ---- approach clearance of the stepper: E_approach, the scene grid along the hand's approach corridor ---------------
 * E_scene asks that the hand is free of the surroundings at the grasp pose; this term asks the same of the way there.
 * With a = grasp_axis (hand frame, used as given), D = distance > 0 in metres, K = n_stations in 1..32 and
 * d_k = D k / K for k = 1..K, station k is the whole hand, joints unchanged, moved back by d_k against its approach
 * direction (-d_k R a in the world).  Per hand surface sample with x_h = T_link p:
 *   y_k = x_h - d_k a (hand frame)      x_w^k = R y_k + t
 *   E_approach = (1/K) sum_k sum_s max(margin - phi(x_w^k), 0)
 * phi is the trilinear interpolant of the gqSceneGrid under exactly the contract of "scene obstacles" above: a station
 * point outside the volume is free space, a non-finite one makes the row's energy and gradient NaN and touches no memory.
 * d = 0 is not a station (that is E_scene).  e_approach is written UNWEIGHTED.  The gradient carries the upstream factor
 * of the row: up_approach[row] if the pointer is given, else w_approach.  With g_w = -up (1/K) grad phi(x_w^k) and
 * g_h = R' g_w for every (s, k) with phi < margin:
 *   link_wrench (B,L,6): f_l = sum g_h, m_l = sum x_h x g_h (x_h unshifted: the joints move x_h, not the offset)
 *   gRt (B,12) = [gsum(3), K9(9)]: gsum = -sum g_h, K9 = sum g_h (x) y_k (the shifted point), row-major; there is no g_R.
 * accumulate, links without samples, n_samples not a multiple of 64 and link ids outside the hand are as in
 * gq_scene_terms.  1/K is one 1.0f / K, multiplied into the finished row energy, and into `up` before `up` scales the
 * finished sums.  Fixed-order sums (stations ascending inside a sample, then the orders of gq_scene_terms), no atomics:
 * bitwise reproducible run to run.  The row total takes gq_scene_total(total, e_approach, w_approach, B).
 * gq_approach_check is the argument check of the launch on its own (host only, no GPU): everything gq_scene_check refuses,
 * a distance that is not finite or <= 0, n_stations outside 1..32, a NULL, non-finite or all-zero grasp_axis; its message
 * contains "approach" and names the argument.                                                                         */
int gq_approach_check(const gqSceneGrid* grid, int64_t batch, int n_links, int64_t n_samples, float distance, int n_stations,
                      const float* grasp_axis /* 3 floats, host */);
int gq_approach_terms(const gqSceneGrid* grid, float margin, float distance, int n_stations,
                      const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                      int64_t n_samples, int n_links, const float* hand_pose, int pose_dim, const float* Rg /* (B,9) */,
                      const float* link_T /* (B,L,12) */, int64_t batch, const float* grasp_axis /* 3 floats, host */,
                      const float* up_approach /* (B) or NULL */, float w_approach,
                      float* e_approach /* (B) or NULL, unweighted */,
                      int accumulate /* 1: add to the two gradient buffers, 0: overwrite */,
                      float* link_wrench /* (B,L,6) or NULL */, float* gRt /* (B,12) or NULL */, void* stream);

/* ---- clutter scenes: one scene grid per object, composed on the device from posed part grids ------------------------
 * The stepper's rows are object-major (n_obj x batch_each), every object's rows in that object's own frame; in a bin with N
 * objects, grasping object g needs "bin + every object but g" in g's frame.  gqClutterGrids is a stack of n_grids grids
 * that share shape, origin and voxel: grid g is exactly the gqSceneGrid {values + g nx ny nz, nx, ny, nz, origin, voxel},
 * under the contract of "scene obstacles" above (phi, the inside rule, free space outside, the NaN rule, the order of the
 * operations: the same device body, csrc/scene_dev.h).  The memory belongs to the caller.  Limits: those of gqSceneGrid per
 * grid, 1 <= n_grids <= 65536.
 * Row-to-grid mapping: row b reads grid b / rows_per_grid; batch == n_grids * rows_per_grid is required exactly.
 * gq_clutter_terms / gq_clutter_corridor_terms take the arguments of gq_scene_terms / gq_approach_terms behind (grids,
 * rows_per_grid), one launch each.  Outputs, accumulate, the upstream factor, links without samples, link ids outside the
 * hand and NaN rows are word for word those of the single-grid entry points, and row b's numbers are BIT FOR BIT those of
 * the single-grid entry point called on row b with grid b / rows_per_grid (the kernels run the same row body, csrc/
 * scene_row_dev.h and approach_row_dev.h).  The row totals take gq_scene_total.
 * gq_clutter_query: point i reads grid i / points_per_grid, n_points == n_grids * points_per_grid; the bits of gq_scene_query
 * on the same point and grid.
 * gq_clutter_check is the argument check of the two launches on its own (host only, no GPU): everything gq_scene_check
 * refuses, n_grids outside 1..65536, rows_per_grid < 1, batch != n_grids * rows_per_grid; its message contains "clutter"
 * and names the argument (gq_clutter_corridor_terms adds what gq_approach_check refuses).
 *
 * gq_clutter_compose fills the stack `out`.  Inputs are what a perception stack holds: one grid per part in the part's own
 * frame (a HOST array of descriptors, values on the device; copied into the kernel's arguments, nothing is uploaded), a
 * rigid pose per part and per target as 12 floats row-major [R|t] (world_from_part, world_from_frame_g) ON THE DEVICE, and
 * optionally a static grid `base` in the world frame.  Node (g,i,j,k) of the output:
 *   x_f = origin + h (i,j,k)  (one fmaf per axis)      x_w = R_g x_f + t_g      q_p = R_p' (x_w - t_p)
 *   phi = min over { far; base(x_w) if x_w is inside base's volume; phi_p(q_p) for every part p != exclude[g] whose volume
 *         contains q_p }
 * Every phi is the trilinear interpolant of "scene obstacles".  The rotations are used as given, not re-orthonormalised.
 * A non-finite x_w or q_p, or a NaN among the sampled values, makes the node NaN (the min never drops a NaN).  exclude[g]
 * outside 0..n_parts-1, or exclude == NULL, leaves no part out.  Parts are visited in ascending order, no atomics: bitwise
 * reproducible run to run.  A block is a tile of 4 x 4 x 16 nodes of one grid and leaves out the parts whose volume none of
 * its nodes can reach, by a conservative test that never changes a result.  No allocation and no synchronisation; poses
 * and exclude are read at launch, so the call can be captured in a graph and a replay after an in-place pose update
 * recomposes.  out_values is out->values, writable.  n_grids x tiles <= 2^23 per launch.
 * gq_clutter_compose_check (host only): everything gq_scene_check refuses for out, for base and for every part (the message
 * names the part's index), n_parts outside 0..32, n_parts == 0 without a base, a non-finite far; the message contains
 * "clutter".                                                                                                          */
typedef struct gqClutterGrids {
  const float* values;   /* (n_grids,nx,ny,nz) device fp32, z fastest; phi at the nodes, positive outside */
  int n_grids, nx, ny, nz;
  float origin[3];       /* of node (0,0,0), the same in every grid's own frame */
  float voxel;
} gqClutterGrids;
int gq_clutter_check(const gqClutterGrids* grids, int64_t batch, int rows_per_grid, int n_links, int64_t n_samples);
int gq_clutter_terms(const gqClutterGrids* grids, int rows_per_grid, float margin,
                     const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                     int64_t n_samples, int n_links, const float* hand_pose, int pose_dim, const float* Rg /* (B,9) */,
                     const float* link_T /* (B,L,12) */, int64_t batch, const float* up_scene /* (B) or NULL */, float w_scene,
                     float* e_scene /* (B) or NULL, unweighted */,
                     int accumulate /* 1: add to the two gradient buffers, 0: overwrite */,
                     float* link_wrench /* (B,L,6) or NULL */, float* gRt /* (B,12) or NULL */, void* stream);
int gq_clutter_corridor_terms(const gqClutterGrids* grids, int rows_per_grid, float margin, float distance, int n_stations,
                              const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                              int64_t n_samples, int n_links, const float* hand_pose, int pose_dim,
                              const float* Rg /* (B,9) */, const float* link_T /* (B,L,12) */, int64_t batch,
                              const float* grasp_axis /* 3 floats, host */, const float* up_approach /* (B) or NULL */,
                              float w_approach, float* e_approach /* (B) or NULL, unweighted */,
                              int accumulate /* 1: add to the two gradient buffers, 0: overwrite */,
                              float* link_wrench /* (B,L,6) or NULL */, float* gRt /* (B,12) or NULL */, void* stream);
int gq_clutter_query(const gqClutterGrids* grids, const float* points /* (N,3) device */, int64_t n_points,
                     int64_t points_per_grid, float* phi /* (N) */, float* grad /* (N,3) or NULL */,
                     uint8_t* inside /* (N) or NULL */, void* stream);
int gq_clutter_compose_check(const gqClutterGrids* out, const gqSceneGrid* parts /* HOST array */, int n_parts,
                             const gqSceneGrid* base /* or NULL */, float far);
int gq_clutter_compose(const gqClutterGrids* out, float* out_values /* = out->values, writable */,
                       const float* target_T /* (G,12) device: world_from_frame_g, row-major [R|t] */,
                       const gqSceneGrid* parts /* HOST array, n_parts in 0..32, each in its own part frame */, int n_parts,
                       const float* part_T /* (n_parts,12) device: world_from_part */,
                       const int32_t* exclude /* (G) device or NULL: the part left out of grid g */,
                       const gqSceneGrid* base /* static grid in the world frame, or NULL */,
                       float far /* finite: the value where nothing is known */, void* stream);

/* ---- pre-grasp clearance of the stepper: E_pregrasp, the OPENED hand along the approach corridor ---------------------
 * E_approach moves the hand back with its joints unchanged; a hand travels the corridor open and closes at the end.  This term
 * asks that the opened hand is free of the grid at every station, the grasp pose (d = 0) included, so the grid may contain the
 * target itself.  With theta the actuated joints of hand_pose (B, 9 + JA), q_o = open_joints (JA) and alpha = opening in [0,1]:
 *   theta_o = (1 - alpha) theta + alpha q_o   (coupled hands: the tree angles follow by coupling theta_o + coupling_offset)
 *   x_h = T_l(theta_o) p      y_k = x_h - d_k a      x_w^k = R y_k + t      d_k = D k / K for k = 0..K (K = 0: d = 0 only)
 *   E_pregrasp = 1/(K+1) sum_k sum_s max(margin - phi(x_w^k), 0)
 * Root pose and R are the closed hand's; a = grasp_axis (hand frame, used as given); phi is the trilinear interpolant of
 * "scene obstacles" by the same device body: outside the volume is free space, a non-finite point makes the row's energy and
 * gradient NaN and loads nothing.  ONE launch per call does the opened kinematics of the row, the stations and the joint
 * gradient: no link_T goes in and no link wrench comes out.  e_pregrasp is written UNWEIGHTED and always overwritten.  The
 * gradient carries the upstream factor of the row: up_pregrasp[row] if given, else w_pregrasp.  With g_w = -up/(K+1) grad phi
 * and g_h = R' g_w for every active (s, k):
 *   gRt (B,12) = [gsum(3), K9(9)]: gsum = -sum g_h, K9 = sum g_h (x) y_k, the layout and signs of gq_approach_terms
 *   g_theta (B,JA) = (1 - alpha) C' tau: per link f_l = sum g_h, m_l = sum x_h x g_h (x_h unshifted), folded onto the nodes the
 *     links ride on and children into parents, deepest level first; tau_j = a_j . (m_j - o_j x f_j) (revolute) or a_j . f_j
 *     (prismatic) with axis a_j and origin o_j of node j in the hand frame at theta_o; C' for a coupled hand.  It is the direct
 *     joint gradient gq_fk_backward takes as g_theta, next to gRt.
 * accumulate is two bits: bit 0 (1) adds to gRt, bit 1 (2) adds to g_theta (a plain rounded add of the finished value: the
 * bits of buffer + the overwriting launch's value); a cleared bit overwrites that buffer.  The stepper passes 1: gRt is shared
 * with the other terms, g_theta is this term's own.  1/(K+1) is one 1.0f / (K+1), multiplied into the finished row energy and into `up`.
 * Fixed-order sums, no atomics: bitwise reproducible run to run.  The grids are a gqClutterGrids stack, row b reads grid
 * b / rows_per_grid; a single grid is the stack of one with rows_per_grid = batch.  The hand has at most 64 joints and 64
 * links (gq_hand_create).  The row total takes gq_scene_total(total, e_pregrasp, w_pregrasp, B).
 * gq_pregrasp_check is the argument check of the launch on its own (host only, no GPU): everything gq_clutter_check and
 * gq_approach_check refuse (but n_stations = 0 is allowed), an opening outside [0,1] or not finite, n_stations outside 0..32;
 * its message contains "pregrasp" and names the argument.                                                              */
int gq_pregrasp_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_links, int64_t n_samples,
                      float distance, int n_stations, const float* grasp_axis /* 3 floats, host */, float opening);
int gq_pregrasp_terms(const gqHand* h, const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float distance,
                      int n_stations /* 0..32 */, float opening /* 0..1 */, const float* open_joints /* (JA) device */,
                      const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                      int64_t n_samples, const float* hand_pose, int pose_dim, const float* Rg /* (B,9) */, int64_t batch,
                      const float* grasp_axis /* 3 floats, host */, const float* up_pregrasp /* (B) or NULL */,
                      float w_pregrasp, float* e_pregrasp /* (B) or NULL, unweighted */,
                      int accumulate /* bit 0: add to gRt, bit 1: add to g_theta; a cleared bit overwrites */,
                      float* g_theta /* (B,JA) or NULL */, float* gRt /* (B,12) or NULL */, void* stream);

/* ---- contact closing feasibility of the stepper: E_squeeze ------------------------------------------------------------
 * reference: core/energy.py:80-87 (E_manipulativity) -> core/hand_model.py:1155-1218 (get_req_joint_velocities, coupled form)
 * with the damped pseudo-inverse of hand_model.py:46-54; the same least-squares problem writes the squeeze command of every
 * exported grasp (scripts/fit.py:224-300).  At min_travel = 5e-3 and damping = 1e-3 the term IS the reference's E_manipulativity
 * in value and gradient.  Per row, with the n contacts contact_idx, J (3n x JA) the linear contact Jacobian in the hand frame
 * (gq_contact_jacobian's, the fold with the coupling matrix C included), n_i = obj_normal, tau = min_travel, lambda = damping:
 *   s_i = max(sqrt(dist_sq_i + 1e-8), tau)    d_i = n_i s_i    d_h = R' d
 *   M = J'J + lambda I    theta = M^-1 J' d_h    r = J theta - d_h    E = 1/(3n) sum r^2
 * M, its Cholesky factor and the solves are fp64 (as gq_joint_velocities); J, r and the rest fp32.  Gradient with the row's
 * upstream c = w (up[row] if given, else 1) / (3n), g = 2 c r, u = M^-1 J' g = -2 c lambda M^-1 theta, v = g - J u:
 *   g_theta (B,JA)        = sum_ij (theta_j v_i - u_j r_i) . dJ_ij/dtheta_k, the closed-form kinematic Hessian of
 *                           gq_contact_jacobian_backward (C / C' for coupled hands): the direct joint gradient gq_fk_backward takes
 *   g_R (B,9)             = dE/dR[a][c] = sum_i d_i[a] (-v_i)[c], plus g_R_base (B,9) if given (a constant of another term: the
 *                           launch reads it and never writes it); always overwritten; gq_fk_backward takes it as g_R
 *   g_contact_pts (B,n,3) = (n_i . R(-v_i)) [s_i > tau] (p_i - closest_i) / sqrt(dist_sq_i + 1e-8); the normals are constants
 * accumulate is two bits: bit 0 (1) adds to g_contact_pts, bit 1 (2) adds to g_theta; a cleared bit overwrites.  e (B) is written
 * UNWEIGHTED and always overwritten; theta (B,JA) are the squeeze joint velocities.  Any output may be NULL; without a gradient
 * output the second solve and the Hessian walk are skipped.  link_T / workspace are gq_fk_forward's of the same poses.
 * One wavefront per row, fixed-order sums, no atomics: bitwise reproducible run to run.  J, JA, n_contact <= 64, else an error
 * status.  The row total takes gq_scene_total(total, e, w, B).                                                             */
int gq_squeeze_terms(const gqHand* h, const int64_t* contact_idx /* (B,n) */, int64_t batch, int n_contact,
                     const float* dist_sq /* (B,n) */, const float* obj_normal /* (B,n,3) outward */,
                     const float* closest /* (B,n,3) or NULL without g_contact_pts */,
                     const float* contact_pts /* (B,n,3) or NULL without g_contact_pts */, const float* Rg /* (B,9) */,
                     const float* link_T /* (B,L,12) */, const void* workspace, size_t workspace_bytes, float min_travel,
                     float damping, const float* up /* (B) or NULL */, float w, float* e /* (B) or NULL */,
                     float* theta /* (B,JA) or NULL */, int accumulate, float* g_theta /* (B,JA) or NULL */,
                     float* g_R /* (B,9) or NULL */, const float* g_R_base /* (B,9) or NULL */,
                     float* g_contact_pts /* (B,n,3) or NULL */, void* stream);

/* ---- payload holding: E_hold, the load wrenches a grasp can carry -----------------------------------------------------------
 * Can these contacts, at this friction and with at most max_force newtons per cone edge, carry the object's load?  Row b has n
 * contacts p_c with OUTWARD object normals n_c, k = n_cone cone edges per contact, nz = n k <= 128 columns, mu = friction,
 * tw = torque_weight, cog (B,3): the inputs of the E_fc step.  Column i = (c, e) of F (6 x nz) is that step's cone column on the
 * INWARD normal -n_c (a finger pushes): force rows f_i, torque rows tw (p_c - cog) x f_i.  A load l < L <= 8 is an external
 * wrench on the object about its centre of mass in the object frame, (force in N, torque in N m); w_l is that wrench with its
 * torque rows multiplied by tw.  loads is (n_load_sets, L, 6) on the device, row b takes set b / loads_each; loads_host holds the
 * same values on the host for the checks (NULL: the caller has checked them; a load with |w_l| = 0 then gives NaN in its row's
 * outputs, never a fault).
 *   x_l = argmin over 0 <= x <= max_force of V_l(x) = |F x + w_l|^2 + ridge |x|^2       E_hold = (1/L) sum_l V_l(x_l) / |w_l|^2
 * the unheld share of the load: dimensionless, 1 when the contacts can do nothing, down to a floor set by the ridge.  max_force
 * bounds every EDGE coefficient; the normal force of contact c is sqrt(1 - mu^2) / k * sum_e x_(c,e) (the cone edges carry the
 * 1/k of the E_fc step; nothing is rescaled).  x_l is the iterate with the problem's own smallest residual among exactly
 * n_iterations PDIPM iterations (the shared loop with the low-rank solver, in fp64; p = F' w_l, bounds [0, max_force]; first strict
 * minimum, a NaN never becomes best); the batch-global stop rule is NOT used, so a row's numbers depend on the row alone.
 * Gradient (envelope theorem: E_hold is the optimal value, the box does not depend on the pose, no KKT backward):
 *   dE/dF = (2 / (L |w_l|^2)) r_l x_l',  r_l = F x_l + w_l;  the normals are held fixed as in the E_fc step, so only the torque
 *   rows carry it: g_contact_pts (B,n,3) = c sum_l sum_e tw f_i x g_tau,i with the row's upstream c = w (up[row] if given, else 1).
 * It is exact at the optimum and an approximation at an iterate (DESIGN section 30 has the measured error per iteration count).
 * Outputs, all UNWEIGHTED, any may be NULL:
 *   e (B)             E_hold
 *   resid (B,L)       |r_l| / |w_l|, the pure residual without the ridge part: what one gates on
 *   x (B,L,nz)        edge coefficients
 *   force (B,L,n,3)   force of finger c on the object, sum_e x f_i, world frame, newtons
 *   torque (B,L,JA)   actuated joint torques tau = J_act' R' force with the linear contact Jacobian of gq_contact_jacobian (the
 *                     squeeze term's column, J_act = J_tree C for a coupled hand); VALUES ONLY, no gradient flows through them
 *   effort (B)        max over l, j of |tau_lj| / torque_limits[j] (JA, device, > 0); needs torque_limits; values only
 * accumulate bit 0 adds to g_contact_pts, cleared it overwrites.  h, contact_idx, Rg, link_T / workspace (gq_fk_forward's of the
 * same poses) are read for torque / effort only and may be NULL without them.  One block per row, one wavefront per load, no
 * atomics, fixed-order sums: bitwise reproducible run to run and row by row, graph-capturable.  An error status, never a device
 * fault, for: n, J, JA outside 1..64, n_cone < 3, nz > 128, L outside 1..8, n_iterations outside 1..64, a load that is not
 * finite or has |w_l| = 0, max_force or ridge not finite and > 0, friction outside (0, 1], load sets that do not cover the batch. */
int gq_hold_terms(const gqHand* h, const int64_t* contact_idx /* (B,n) */, int64_t batch, int n_contact, int n_cone,
                  const float* obj_normal /* (B,n,3) outward */, const float* contact_pts /* (B,n,3) */,
                  const float* cog /* (B,3) */, const float* Rg /* (B,9) */, const float* link_T /* (B,L,12) */,
                  const void* workspace, size_t workspace_bytes, const float* loads /* (n_load_sets,L,6) device */,
                  const float* loads_host /* the same on the host, or NULL */, int64_t n_load_sets, int n_loads, int64_t loads_each,
                  float friction, float torque_weight, float max_force, float ridge, int n_iterations,
                  const float* torque_limits /* (JA) or NULL */, const float* up /* (B) or NULL */, float w,
                  float* e /* (B) */, float* resid /* (B,L) */, float* x /* (B,L,nz) */, float* force /* (B,L,n,3) */,
                  float* torque /* (B,L,JA) */, float* effort /* (B) */, int accumulate,
                  float* g_contact_pts /* (B,n,3) or NULL */, void* stream);

/* ---- finger closing: where the hand really touches when the squeeze command is executed ---------------------------------------
 * Kinematic only (no forces, no object motion): the actuated joints are stepped along a closing direction until the links touch the
 * object grid, a joint limit, or the steps run out.  Per row b: theta_0 = the joints of hand_pose (B, 9 + JA), R = Rg (B,9), t the
 * translation of hand_pose, v = direction (B,JA), the hand's surface samples (p_i in the frame of link sample_link[i]) and grid
 * b / rows_per_grid of a gqClutterGrids stack that CONTAINS THE TARGET (a single grid is the stack of one with rows_per_grid =
 * batch).  Parameters: S = n_steps in 1..64, step (JA) finite and > 0 (the largest increment of each actuated joint per step),
 * tau = touch >= 0 (metres), joint_links (JA) 64-bit masks over the links.
 *   direction  u_a = v_a / step_a, m = max_a |u_a|, Delta_a = step_a (u_a / m): the fastest joint moves exactly its step.  A row
 *              with m = 0, or with any u_a not finite, has Delta = 0 and does not move.
 *   steps      s = 0..S (S + 1 evaluations, S updates):
 *     1. tree angles C theta_s + c0 for a coupled hand, link transforms T_l in the hand frame, as gq_fk_forward
 *     2. every sample x_i = R (T_l p_i) + t, phi_i by the device body of "scene obstacles" on the row's grid; a sample outside the
 *        volume, at a non-finite point or with a NaN phi takes no part (it never touches and loads nothing out of range)
 *     3. per link l: m_l = min phi_i over its samples that take part, ties to the LOWEST sample index (+inf, no sample: none)
 *     4. touched_l becomes true, and stays true, when m_l <= tau; touch_step_l = the first such s
 *     5. joint a is stopped from step s on when a touched link lies in joint_links[a]; joint_stop_a = the first such s
 *     6. if s < S: theta_(s+1),a = min(max(theta_s,a + Delta_a, lower_a), upper_a) for the joints that are not stopped and have
 *        Delta_a != 0; every other joint keeps its value bit for bit
 *   When step 6 changes no joint, every later evaluation repeats this one and the launch stops there (block-uniform).
 * joint_links[a] has bit l set when link l rides on a tree node in the subtree of a tree node that joint a drives (coupling[j][a]
 * != 0; an uncoupled hand drives node a alone); it is built on the host once per hand.  A touching link so stops its own joint
 * and every joint between it and the palm, the joints beyond it keep closing; a link fixed to the base stops nothing.  A touched
 * link never moves again, so the state of its first touch is its final state.  No sub-step refinement: the overshoot is at most
 * step x lever arm and max(-phi, 0) reports it.
 * Outputs, all of the final state theta_S, any may be NULL:
 *   theta (B,JA)          closed joints
 *   touch_step (B,L) i32  -1: never touched
 *   joint_stop (B,JA) i32 -1: not stopped by a touch (it may stand on a joint limit)
 *   phi (B,L)             m_l; +inf without a sample that takes part
 *   sample (B,L) i32      the argmin sample, -1 if none
 *   point (B,L,3)         world position of that sample (zeros if none)
 *   normal (B,L,3)        grad phi / |grad phi| there, the object's outward normal; zeros if none or |grad phi| = 0
 * One block of eight wavefronts per row; minima with a lowest-index tie-break, no sums, no atomics: bitwise reproducible run to run
 * and row by row, graph-capturable, the host never waits.  An error status, never a device fault, for every bad argument.
 * gq_close_check is the host-only part (no GPU): everything gq_clutter_check refuses (a stack that does not cover the batch), n_steps
 * outside 1..64, a step that is not finite or <= 0 (step_host: the (JA) values on the host, NULL = the caller has checked them),
 * touch < 0 or not finite, more than 64 tree joints, actuated joints or links; its message contains "close".              */
int gq_close_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_joints, int n_actuated, int n_links,
                   int64_t n_samples, int n_steps, const float* step_host /* (JA) host or NULL */, float touch);
int gq_close_fingers(const gqHand* h, const gqClutterGrids* grids, int64_t rows_per_grid, const float* samples /* (Ns,3) device */,
                     const int32_t* sample_link /* (Ns) */, int64_t n_samples, const float* hand_pose, int pose_dim,
                     const float* Rg /* (B,9) */, int64_t batch, const float* direction /* (B,JA) */, int n_steps,
                     const float* step /* (JA) device */, const float* step_host /* (JA) host or NULL */, float touch,
                     const int64_t* joint_links /* (JA) device, bit l = link l */, float* theta /* (B,JA) */,
                     int32_t* touch_step /* (B,L) */, int32_t* joint_stop /* (B,JA) */, float* phi /* (B,L) */,
                     int32_t* sample /* (B,L) */, float* point /* (B,L,3) */, float* normal /* (B,L,3) */, void* stream);

/* ---- arm reachability of the stepper: E_reach, batched damped-least-squares wrist IK ----------------------------------------
 * Every other term treats the hand as a free-flying body; this one knows that it sits on an arm.  The arm is a serial chain of
 * N <= 8 revolute (1) or prismatic (2) joints with limits: FK(q) = base_T joint_T[0] m_0(q_0) ... joint_T[N-1] m_{N-1}(q_{N-1}) tool_T
 * is the hand-root pose (p(q), R(q)) in the frame the row lives in (its object's): base_T[b / batch_each] is the arm base in that
 * frame, joint_T[j] the fixed transform parent -> joint frame, m_j the rotation about / shift along the unit joint_axis[j], tool_T
 * flange -> hand root.  Transforms are 3x4 row-major [R|t].  gq_arm_create takes HOST arrays, checks them (types, unit axes, finite
 * limits with lower < upper, seeds (S,N) inside the limits, 1 <= N <= 8, 1 <= S <= 8) and owns the device copy
 * (counted in gq_setup_live_allocations).
 * Row b with root translation t and root rotation R (Rg of gq_fk_forward), station k = 0..K (K = n_stations, station 0 = the grasp
 * pose): R*_k = R, p*_k = t - (D k / K) R a, a = grasp_axis as given (the direction convention of gq_approach_terms).  Per station and
 * seed q0: q <- q0, then M = n_iterations times
 *   e = [p* - p(q) ; rho log(R* R(q)')]    J = [J_v ; rho J_w] (6 x N, geometric, same frame)    dq = J' (J J' + lambda I)^-1 e
 *   if max|dq| > 0.5: dq <- dq 0.5 / max|dq|    q <- clamp(q + dq, lower, upper)
 * and one more FK for e and E_{k,seed} = |e|^2.  The log map takes its angle from atan2(|vee|, (trace - 1) / 2) and the series
 * 1 + |vee|^2 / 6 of angle / |vee| for |vee| < 1e-6 (a target exactly half a turn away therefore reads as no rotation error).
 * E_k = min over the seeds, the lowest seed index on a tie; E_reach = 1/(K+1) sum_k E_k in m^2, all fp32 (csrc/reach_dev.h says why
 * the 6 x 6 is too).  Gradient: the partial derivative with respect to the target with the winner's final q held fixed,
 * dE_k/dp*_k = 2 e_p and, for R* <- exp(d^) R*, the torque 2 rho^2 log(R* R(q)') = 2 rho e_w.  Where the iteration has reached a
 * fixed point with no joint on a limit -- target reachable or not -- this IS the gradient of the converged E (envelope theorem:
 * dq = 0 means J'e = 0, E is stationary in q); elsewhere it is an approximation: before convergence, with a joint ON its limit (the
 * clamped fixed point is not the constrained minimiser), and past the outer boundary of a revolute arm, where at the default damping
 * the iteration ends in a two-cycle about the stretched configuration.  With c = w (up[row] if given, else 1) / (K+1) and d_k = D k / K it goes to
 *   gRt (B,12) = [gsum(3), K9(9)]: gsum = -R' sum_k 2 c e_p,k;  K9 = sum_k (R' 2 c e_p,k) (x) (-d_k a) + hat(R' sum_k 2 c rho e_w,k) / 2
 * in the layout and signs of gq_approach_terms (grad_t = -R gsum, grad_R = R K9); accumulate = 1 adds to gRt, 0 overwrites it.
 * g_R and g_theta of gq_fk_backward are not touched.  e_reach (B) is written UNWEIGHTED and always overwritten; reach_q (B,K+1,N) is
 * the winner's joint vector per station and reach_seed (B,K+1) its seed.  Any output may be NULL.  One block per row, eight lanes
 * per IK problem, fixed-order sums, no atomics: bitwise reproducible run to run; no joint state is carried between launches, so the
 * term is a pure function of the pose.  The row total takes gq_scene_total(total, e_reach, w, B).
 * gq_reach_check is the parameter check on its own (host only, no GPU); its message contains "reach" and names the argument.   */
typedef struct gqArmDesc { /* all pointers HOST */
  int32_t n_joints, n_seeds;
  const int32_t* joint_type; /* (N) 1 revolute, 2 prismatic */
  const float* joint_T;      /* (N,12) */
  const float* joint_axis;   /* (N,3) unit */
  const float* lower;        /* (N) */
  const float* upper;        /* (N) */
  const float* tool_T;       /* (12) */
  const float* seeds;        /* (S,N) */
} gqArmDesc;
typedef struct gqArm gqArm;
int gq_arm_create(const gqArmDesc* desc, gqArm** out);
int gq_arm_destroy(gqArm* arm);
int gq_reach_check(int n_joints, int n_seeds, float distance, int n_stations, int n_iterations, float damping, float rot_scale,
                   const float* grasp_axis /* (3) host */);
int gq_reach_terms(const gqArm* arm, const float* hand_pose /* (B,pose_dim) */, int pose_dim, const float* Rg /* (B,9) */,
                   int64_t batch, const float* base_T /* (n_obj,12) */, int64_t n_obj, int64_t batch_each,
                   const float* grasp_axis /* (3) host */, float distance, int n_stations, int n_iterations, float damping,
                   float rot_scale, const float* up /* (B) or NULL */, float w, float* e_reach /* (B) or NULL */,
                   float* reach_q /* (B,K+1,N) or NULL */, int32_t* reach_seed /* (B,K+1) or NULL */, int accumulate,
                   float* gRt /* (B,12) or NULL */, void* stream);

/* ---- arm clearance of the stepper: E_arm, the arm's collision spheres on the scene grid -----------------------------------------
 * E_reach says whether the wrist can get to a pose and leaves the arm configuration of every station in reach_q; this term looks at
 * where that configuration puts the arm.  The arm carries Ns <= 64 collision spheres (link l_s in 0..N-1, centre c_s in the link
 * frame, radius r_s > 0), all three arrays on the device.  Link j is the frame after joint j has moved,
 * W_j(q) = base_T joint_T[0] m_0(q_0) ... joint_T[j] m_j(q_j), the chain of gq_reach_terms in the row's object frame (products taken
 * left to right).  The hand is not part of the term (the hand-surface terms cover it), nor is a fixed base link.  Per row b and
 * station k = 0..K (K = n_stations, distance and grasp_axis are the reach term's), with q_k = reach_q[b,k] -- an INPUT, the winner's
 * joints of the reach launch of the same evaluation; nothing is recomputed:
 *   x_s = W_{l_s}(q_k) c_s      h_s = max((margin + r_s) - phi(x_s), 0)      E_k = sum_s h_s (spheres ascending)
 *   E_arm = 1/(K+1) sum_k E_k   in metres, written UNWEIGHTED and always overwritten
 * phi is the trilinear interpolant of "scene obstacles" by the same device body (the bits of gq_clutter_query at the same point):
 * h_s = 0 outside the volume and at a non-finite point.  The grids are a gqClutterGrids stack, row b reads grid b / rows_per_grid,
 * batch == n_grids * rows_per_grid; n_grids = 1 is the single scene.  The grid may contain the target object.
 * Gradient.  E_arm depends on the pose only through q.  The term DEFINES dq = J' (J J' + lambda_a I)^-1 de, the minimum-norm joint
 * motion that follows a small motion de = [dp* ; rho d omega] of the target; J = [J_v ; rho J_w] (6 x N) is the reach term's matrix at
 * the hand root, lambda_a = damping is this term's OWN parameter (default 1e-6, not the reach iteration's 1e-4: beside
 * sigma_min^2(J) of 1e-4..1e-2 at rho = 0.1 the latter is not small).  With f_s = -grad phi(x_s) where h_s > 0:
 *   g_q[j] = sum_{s : l_s >= j} f_s . col_j(x_s)     col_j(x) = z_j x (x - o_j) (revolute) or z_j (prismatic)
 *   a joint is free when lower_j < q_j < upper_j on the float32 numbers the device holds; a joint ON a limit gets g_q[j] = 0 and a
 *   zero column in J
 *   y = (J J' + lambda_a I)^-1 J g_q      dE_k/dp*_k = y_p      the torque for R* <- exp(d^) R* is rho y_w
 * and with c = w (up[row] if given, else 1) / (K+1), d_k = D k / K, in the layout and signs of gq_reach_terms (2 e_p -> y_p,
 * 2 rho e_w -> rho y_w):
 *   gRt (B,12) = [gsum(3), K9(9)]: gsum = -R' sum_k c y_p,k;  K9 = sum_k (R' c y_p,k) (x) (-d_k a) + hat(R' sum_k c rho y_w,k) / 2
 * accumulate = 1 adds to gRt, 0 overwrites it; g_R and g_theta of gq_fk_backward are not touched; gRt = NULL skips the gradient.
 * What this is: for a target the arm reaches with no joint on a limit it is the derivative of E_arm along the arm's minimum-norm
 * tracking of the target, with an error of at most lambda_a / sigma_min^2(J).  Elsewhere it is an approximation: for an unreachable
 * target the Jacobian of the log map is dropped; a joint on a limit is frozen; for a redundant arm the from-seed iteration of the
 * reach term need not follow the minimum-norm branch.  |y| <= |g_q| / (2 sqrt(lambda_a)) bounds it at a singular configuration.
 * Precision: J g_q, J J' and the 6 x 6 Cholesky solve are fp64 (one solve per station whose result IS the gradient, usable to a
 * condition number of 8e6); the kinematics, the sphere points, the field samples and the columns are fp32.
 * One block per row, one wavefront per station, lane = sphere; fixed-order sums, no atomics: bitwise reproducible run to run, and a
 * pure function of (reach_q, Rg).  hand_pose is the row's pose as every term takes it (the term reads its rotation from Rg).
 * The row total takes gq_scene_total(total, e_arm, w, B).
 * gq_arm_check is the argument check on its own (host only, no GPU): the stack and the batch (gq_clutter_check; grids = NULL checks
 * the parameters alone, before a scene exists -- gq_arm_terms itself refuses a NULL stack), n_joints in 1..8,
 * n_spheres in 1..64, a finite margin >= 0, finite damping > 0 and rot_scale > 0, n_stations in 0..3, a finite distance > 0 when
 * there are stations, a finite non-zero grasp_axis; its message contains "arm" and names the argument.                          */
int gq_arm_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_joints, int n_spheres, float margin,
                 float damping, float rot_scale, float distance, int n_stations, const float* grasp_axis /* (3) host */);
int gq_arm_terms(const gqArm* arm, const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float damping, float rot_scale,
                 const int32_t* sphere_link /* (Ns) device */, const float* sphere_centre /* (Ns,3) device */,
                 const float* sphere_radius /* (Ns) device */, int n_spheres, const float* hand_pose /* (B,pose_dim) */,
                 int pose_dim, const float* Rg /* (B,9) */, int64_t batch, const float* base_T /* (n_obj,12) */, int64_t n_obj,
                 int64_t batch_each, const float* grasp_axis /* (3) host */, float distance, int n_stations,
                 const float* reach_q /* (B,K+1,N) input */, const float* up /* (B) or NULL */, float w,
                 float* e_arm /* (B) or NULL */, int accumulate, float* gRt /* (B,12) or NULL */, void* stream);

/* ---- approach tracking of the stepper: E_track, one continuous arm path along the retreat line -------------------------------
 * E_reach solves every station of the retreat from scratch, the best of its seeds: nothing puts two neighbouring stations on the
 * same IK branch, so reach_q is not a path.  This term follows the straight approach line from ONE start configuration, each
 * waypoint warm-started from the one before.  The arm, base_T, batch_each, grasp_axis a, D = distance > 0, lambda = damping and
 * rho = rot_scale are those of gq_reach_terms.  Row b with root translation t and rotation R (Rg), T = n_waypoints waypoints beyond
 * the first, i = 0..T in the order the robot moves:
 *   d_i = D (T - i) / T      p*_i = t - d_i R a      R*_i = R      (waypoint 0: the retreated pose, the target of the reach term's
 *                                                                   station K; waypoint T: the grasp pose)
 * q_{-1} = q_start[b] (q_start_stride floats from row to row, so reach_q[:, K] is passed as a view: pointer reach_q + K N, stride
 * (K+1) N; it is used as given, not clamped).  For i = 0..T: q <- q_{i-1}, then U = n_updates times exactly the update of
 * gq_reach_terms, by the same device bodies:
 *   e = [p*_i - p(q) ; rho log(R* R(q)')]    J = [J_v ; rho J_w]    dq = J' (J J' + lambda I)^-1 e
 *   if max|dq| > 0.5: dq <- dq 0.5 / max|dq|    q <- clamp(q + dq, lower, upper)
 * and one more FK for e_i and E_i = |e_i|^2; q_i = q.  Outputs, all fp32, any may be NULL:
 *   e_track (B)              1/(T+1) sum_i E_i in m^2, i ascending, then x 1/(T+1); UNWEIGHTED, always overwritten
 *   track_q (B,T+1,N)        the q_i
 *   track_worst (B)          max_i E_i
 *   track_step (B)           max over i = 0..T and j < N of |q_i,j - q_{i-1},j| (rad or m), the first move from q_start included
 *   track_station_q (B,K+1,N) given only with K = n_stations >= 1 that divides T: station k holds q_i at i = T (K - k) / K, in the
 *                            layout and station order of reach_q and bitwise equal to those track_q entries -- what gq_arm_terms
 *                            takes in place of reach_q to look at the configurations the arm passes through
 * Gradient: the partial derivative with respect to the targets with every q_i held fixed, in the form of gq_reach_terms: with
 * c = w (up[row] if given, else 1) / (T+1), waypoints ascending,
 *   gRt (B,12) = [gsum(3), K9(9)]: gsum = -R' sum_i 2 c e_p,i;  K9 = sum_i (R' 2 c e_p,i) (x) (-d_i a) + hat(R' sum_i 2 c rho e_w,i) / 2
 * accumulate = 1 adds to gRt, 0 overwrites it; g_R and g_theta of gq_fk_backward are not touched.  What this is: the gradient of the
 * converged path energy where every waypoint has reached a fixed point with no joint on a limit (J'e_i = 0: E_i is stationary in
 * q_i, and the warm start drops out).  It is an approximation elsewhere: at finite U, with a clamped joint, and in the two-cycle
 * past the outer boundary of a revolute arm.
 * Limits: T in 1..64, U in 1..16, D, lambda and rho finite and > 0, K in 0..3 (K >= 1 and K | T when track_station_q is given),
 * batch, base_T, n_obj and batch_each as in gq_reach_terms, q_start_stride >= N.  Eight lanes per row, eight rows per wavefront,
 * one wavefront per block; no LDS, no atomics, fixed-order sums: bitwise reproducible run to run, a row's bits do not depend on the
 * batch it sits in, and the term is a pure function of (pose, q_start).  The row total takes gq_scene_total(total, e_track, w, B).
 * gq_track_check is the parameter check on its own (host only, no GPU; with_station_q != 0 checks K against T as the launch with
 * a track_station_q does); its message contains "track" and names the argument.                                               */
int gq_track_check(int n_joints, float distance, int n_waypoints, int n_updates, float damping, float rot_scale, int n_stations,
                   int with_station_q, const float* grasp_axis /* (3) host */);
int gq_track_terms(const gqArm* arm, const float* hand_pose /* (B,pose_dim) */, int pose_dim, const float* Rg /* (B,9) */,
                   int64_t batch, const float* base_T /* (n_obj,12) */, int64_t n_obj, int64_t batch_each,
                   const float* grasp_axis /* (3) host */, float distance, int n_waypoints, int n_updates, float damping,
                   float rot_scale, const float* q_start /* row b at q_start + b q_start_stride, (N) */, int64_t q_start_stride,
                   int n_stations, const float* up /* (B) or NULL */, float w, float* e_track /* (B) or NULL */,
                   float* track_q /* (B,T+1,N) or NULL */, float* track_worst /* (B) or NULL */, float* track_step /* (B) or NULL */,
                   float* track_station_q /* (B,K+1,N) or NULL */, int accumulate, float* gRt /* (B,12) or NULL */, void* stream);

/* ---- lift clearance of the stepper: E_lift, the hand and the held object on the way out --------------------------------------
 * Every obstacle term above follows the hand on its way in.  This one asks what happens after the fingers close: hand and object
 * leave as one rigid body, and the object is usually wider than the hand.  Row b of object o = b / batch_each with rotation R (Rg)
 * and translation t; a = grasp_axis (hand frame, used as given), u = direction (a unit vector of the object's frame, which is the
 * grid's; used as given, the caller normalises), H = height >= 0 and D = retreat >= 0 in metres with H + D > 0, K = n_stations in
 * 1..32, d_k = D k / K and h_k = H k / K for k = 1..K.  The carry is the straight translation by (k / K) (H u - D R a): D = 0 is a
 * pure lift, H = 0 the reverse of the approach.
 *   hand sample, x_h = T_link p:   y_k = x_h - d_k a      x_w^k = R y_k + (t + h_k u)
 *   object point p_j of object o:  x^{j,k} = p_j + h_k u - d_k R a           (object_points (n_obj,M,3), object frame, device)
 *   E_lift = (1/K) sum_k [ sum_s max(margin - phi(x_w^k), 0) + sum_j max(object_margin - phi(x^{j,k}), 0) ]
 * phi is the trilinear interpolant under exactly the contract of "scene obstacles": a point outside the volume is free space, a
 * non-finite one makes the row's energy and gradient NaN and touches no memory.  margin >= 0 is finite; object_margin is finite
 * and may be negative (an object dragged along its support sits at phi ~ 0).  Station 0 is not part of the term: the hand there is
 * E_scene, the object at rest touches what it stands on.  M = n_object_points = 0 is the hand alone.  The grid of row b is grid
 * b / rows_per_grid of the stack (n_grids = 1: the single scene, as in gq_arm_terms) and must not contain the target.
 * e_lift is written UNWEIGHTED; e_object (B, optional) is the object's share of it, (1/K) sum_k sum_j.  The gradient carries
 * up = (up_lift[row] if given, else w_lift) (1/K), in the conventions of gq_approach_terms, with g_h = R' (-up grad phi):
 *   active hand (s,k):    f_l = sum g_h, m_l = sum x_h x g_h (x_h unshifted), gsum = -sum g_h, K9 += g_h (x) y_k; the world shift
 *                         h_k u depends on nothing and adds nothing
 *   active object (j,k):  K9 += g_h (x) (-d_k a) and nothing else: t does not move the object (no gsum), no joint does (no wrench).
 *                         With D = 0 the object part has a value and no gradient, the same value for every row of an object.
 * g_R and g_theta of gq_fk_backward are not touched.  accumulate, links without samples, n_samples or M not a multiple of 64 and
 * link ids outside the hand are as in gq_approach_terms.  One block of eight wavefronts per row; a wavefront takes its hand chunks,
 * then its chunks of 64 object points, stations ascending inside a lane; fixed-order sums, no atomics: bitwise reproducible run to
 * run, a row's bits do not depend on the batch around it.  With H = 0 and M = 0 the launch gives BIT FOR BIT e, link_wrench and
 * gRt of gq_clutter_corridor_terms at the same inputs.  The row total takes gq_scene_total(total, e_lift, w, B).
 * gq_lift_check is the argument check on its own (host only, no GPU; grids = NULL checks the parameters alone, before a scene
 * exists -- gq_lift_terms itself refuses a NULL stack): everything gq_clutter_check refuses, batch != n_obj * batch_each,
 * n_object_points outside 0..2^24, a height or retreat that is negative or not finite, height + retreat == 0, n_stations outside
 * 1..32, a NULL, non-finite or all-zero grasp_axis or direction, a margin that is negative or not finite, an object_margin that is
 * not finite; its message contains "lift" and names the argument.                                                            */
int gq_lift_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_links, int64_t n_samples, int64_t n_obj,
                  int64_t batch_each, int64_t n_object_points, float height, float retreat, int n_stations,
                  const float* grasp_axis /* (3) host */, const float* direction /* (3) host */, float margin, float object_margin);
int gq_lift_terms(const gqClutterGrids* grids, int64_t rows_per_grid, float margin, float object_margin, float height, float retreat,
                  int n_stations, const float* samples /* (Ns,3) link frame, device */, const int32_t* sample_link /* (Ns) */,
                  int64_t n_samples, int n_links, const float* hand_pose, int pose_dim, const float* Rg /* (B,9) */,
                  const float* link_T /* (B,L,12) */, int64_t batch, const float* object_points /* (n_obj,M,3) or NULL with M = 0 */,
                  int64_t n_obj, int64_t batch_each, int64_t n_object_points, const float* grasp_axis /* (3) host */,
                  const float* direction /* (3) host */, const float* up_lift /* (B) or NULL */, float w_lift,
                  float* e_lift /* (B) or NULL, unweighted */, float* e_object /* (B) or NULL */,
                  int accumulate /* 1: add to the two gradient buffers, 0: overwrite */, float* link_wrench /* (B,L,6) or NULL */,
                  float* gRt /* (B,12) or NULL */, void* stream);

/* ---- scenes from depth images: TSDF fusion on the device into scene grids ---------------------------------------------
 * What a robot has is depth images, not a signed-distance volume.  gq_tsdf_integrate fuses a batch of depth frames into a
 * gqClutterGrids stack IN PLACE, one launch per batch (n_grids = 1 is the single world grid).  State: `values` of the stack IS
 * the running truncated signed distance D in metres, positive in seen free space -- the memory gq_scene_terms /
 * gq_clutter_terms and their corridor siblings read, there is no extraction pass -- and beside it `weight` (n_grids,nx,ny,nz)
 * fp32, the number of views that updated the node, capped.  A fresh volume is values = unknown, weight = 0; -trunc (unobserved
 * space is occupied) is the conservative unknown for a hand that must stay in seen free space, +trunc makes it free.
 * Views: V depth images of one camera model (pinhole, pixel centres at integer (col,row)), metres along the optical axis,
 * an optional segmentation id per pixel, and a pose per view, world_from_camera as 12 floats row-major [R|t], used as given.
 * Node (g,i,j,k) carries D and W in registers and visits the views in ascending order.  Per view:
 *   x_f = origin + h (i,j,k), x_w = R_g x_f + t_g   exactly as gq_clutter_compose (x_w = x_f when target_T is NULL)
 *   x_c = R_c' (x_w - t_c)                          exactly as its part-frame point
 *   z = x_c.z; the view is skipped unless z >= depth_min (tested before any division)
 *   u = fmaf(fx, x_c.x / z, cx), v = fmaf(fy, x_c.y / z, cy), true divisions; the node is in the image iff
 *   u >= -0.5 && u < width - 0.5 && v >= -0.5 && v < height - 0.5, tested on the floats before the float -> int conversion;
 *   col = (int)floorf(u + 0.5f), row = (int)floorf(v + 0.5f) (held to width - 1 / height - 1 when the sum rounds up to the
 *   bound), d = depth[view][row][col], valid iff depth_min <= d <= depth_max (0, negative, NaN, inf: the view is skipped)
 *   if labels and skip are given, skip[g] >= 0 and labels[pix] == skip[g]:  s = trunc (the target is no obstacle of its own
 *   grid: this view takes the whole ray through the pixel as free); otherwise sdf = d - z, the view is skipped if
 *   sdf < -trunc (occluded), else s = min(sdf, trunc)
 *   D = fmaf(W, D, s) / (W + 1.0f), then W = min(W + 1.0f, max_weight)
 * After the loop both are stored.  A non-finite x_w makes the node NaN and leaves its weight alone; a non-finite x_c does the
 * same in that view (the NaN is sticky: every later mean keeps it).  A node no view updates keeps D and W bit for bit.  No
 * atomics, views ascending: bitwise reproducible, and one launch with V views gives the bits of V launches with one view each.
 * No allocation, no synchronisation, no upload: poses, skip, images and labels are read at launch, so the call can sit in a
 * captured graph and a replay after in-place writes re-integrates.  A block is a tile of 4 x 4 x 16 nodes of one grid;
 * n_grids x tiles <= 2^23 per launch.  values is grids->values, writable.
 * gq_tsdf_check (host only, no GPU): everything gq_clutter_check refuses for the stack (called with batch = n_grids,
 * rows_per_grid = 1), a NULL views, depth or cam_T, n_views outside 1..64, width or height outside 1..8192, fx or fy
 * non-finite or <= 0, non-finite cx or cy, depth_min not finite or not > 0, depth_max not finite or < depth_min, trunc not
 * finite or not > 0, max_weight not finite or < 1, a non-finite unknown; its message contains "tsdf" and names the
 * argument.                                                                                                            */
typedef struct gqDepthViews {
  const float*   depth;    /* (V,H,W) device, metres along the optical axis (z of the camera frame), row-major, W fastest */
  const int32_t* labels;   /* (V,H,W) device or NULL: a segmentation id per pixel */
  const float*   cam_T;    /* (V,12) device: world_from_camera, row-major [R|t], read at launch, used as given */
  int n_views, width, height;
  float fx, fy, cx, cy;    /* pinhole; pixel centres at integer (col,row) */
  float depth_min, depth_max;
} gqDepthViews;
int gq_tsdf_check(const gqClutterGrids* grids, const gqDepthViews* views, float trunc, float max_weight, float unknown);
int gq_tsdf_integrate(const gqClutterGrids* grids, float* values /* = grids->values, writable */,
                      float* weight /* (n_grids,nx,ny,nz) device */,
                      const float* target_T /* (G,12) device world_from_frame_g, or NULL = identity */,
                      const gqDepthViews* views, const int32_t* skip /* (G) device or NULL */,
                      float trunc, float max_weight, void* stream);

/* ---- target objects from depth images: the zero level set of a fused stack as oriented point clouds -------------------
 * gq_tsdf_surfels turns every grid of a gqClutterGrids stack that gq_tsdf_integrate has fused (values = D, positive in free
 * space; weight = W or NULL = every node observed) into surfels: positions and unit outward normals in the grid's frame, the
 * input of gq_cloudset_create.  Per grid, inside the half-open node region [i0,i1) x [j0,j1) x [k0,k1) (region = 6 ints on the
 * HOST in that order, NULL = the whole grid):
 *   node n is OBSERVED iff it lies in the grid, D(n) is finite and W(n) >= min_weight
 *   node a owns the edges to b = a + e_c, c = x, y, z; an edge is a CROSSING iff a and b are in the region, both are observed,
 *   (D_a >= 0) != (D_b >= 0), |D_a| < trunc and |D_b| < trunc -- exact tests on the fp32 inputs
 *   t = D_a / (D_a - D_b) in [0,1];  p = x_a + t voxel e_c,  x_a = fmaf(voxel, (i,j,k), origin) as gq_clutter_compose's x_f
 *   d_c(m) = (D(m + e_c) - D(m - e_c)) / 2 if both neighbours are observed, the one-sided difference if one is, 0 if none
 *   g_c(n) = sum w d_c(m) / sum w over the OBSERVED nodes m of the 3 x 3 neighbourhood of n transverse to c,
 *            w = (1,2,1) x (1,2,1) (n itself is observed: the sum of the weights is >= 4); the stencils read the whole grid
 *   v = (1 - t) g(a) + t g(b);  normal = v / |v| if |v|^2 > 1e-20, else e_c sign(D_b - D_a): the number of surfels never
 *   depends on a floating-point decision.
 * Outputs: points, normals (G,capacity,3) fp32; count (G,2) int32 = (crossings found, min(found, capacity) written; 0 written
 * when points is NULL).  Slots at and beyond the written count are not touched.  points == normals == NULL runs the count only.
 * Order: (tile of 4 x 4 x 16 nodes as gq_tsdf_integrate's blocks, x slowest; node within the tile, z fastest; axis), fixed: two
 * runs agree bit for bit.  Three launches (count per tile, one block per grid scans the tile counts, emit) and nothing else: no
 * atomics, no block waits for another, no allocation, synchronisation or upload -- the call can sit in a captured graph
 * behind gq_tsdf_integrate.  workspace: gq_tsdf_surfels_workspace_bytes(grids) bytes on the device, contents irrelevant.
 * gq_tsdf_surfels_check (host only, no GPU): a NULL grids, everything gq_clutter_check refuses for the stack, more than 2^23
 * tiles, trunc not finite or not > 0, a non-finite min_weight, a region that is empty on an axis or leaves the grid,
 * capacity < 1 when has_outputs, capacity > 2^24; the message starts with "surfels:" and names the argument.            */
int gq_tsdf_surfels_check(const gqClutterGrids* grids, const int32_t* region /* 6 ints, HOST, or NULL */, float min_weight,
                          float trunc, int has_outputs, int64_t capacity);
int gq_tsdf_surfels_workspace_bytes(const gqClutterGrids* grids, size_t* bytes);
int gq_tsdf_surfels(const gqClutterGrids* grids, const float* values /* = grids->values */,
                    const float* weight /* (n_grids,nx,ny,nz) device or NULL */, const int32_t* region /* 6 ints, HOST, or NULL */,
                    float min_weight, float trunc, float* points /* (G,capacity,3) device or NULL */,
                    float* normals /* (G,capacity,3) device or NULL */, int64_t capacity, int32_t* count /* (G,2) device */,
                    void* workspace, void* stream);

/* ---- Euclidean distance field from a fused TSDF (ESDF) ------------------------------------------------------------------
 * A fused volume holds a truncated, projective distance: deeper than trunc inside an obstacle or inside unobserved space every
 * node holds -trunc, the interpolant is flat there and E_scene / E_approach have no gradient; margins must stay below trunc.
 * gq_esdf turns a gqClutterGrids stack `src` (values = D, positive in free space; n_grids = 1 is the single grid) into a second
 * stack `dst` of the same n_grids, shape, origin and voxel that holds phi, a Euclidean signed distance up to max_distance.  src
 * is not written; dst is memory the scene launches read unchanged.  Every test on D is an exact test on the fp32 inputs, trunc
 * is compared as an fp32 value.  Per grid, h = voxel:
 *   a node is VOID iff D is not finite: phi = D bit for bit (a NaN stays a NaN), and no edge with a void end is a crossing
 *   a finite node is FREE iff D >= 0 (0.0 and -0.0 are free, as in gq_tsdf_surfels), else OCCUPIED
 *   node a owns the edges to b = a + e_c, c = x, y, z; an edge is a CROSSING iff both ends are finite and exactly one is free --
 *   unlike the surfel rule there is no |D| < trunc condition and no weight: the boundary between seen free space and unknown
 *   (+.. | -trunc) is a crossing, and an edge between +trunc and -trunc crosses at t = 1/2
 *   crossing point p = a + t e_c in node units, t = D_a / (D_a - D_b) in [0,1]
 *   e(n) = h min over all crossing points p of the grid of |n - p|, +inf if the grid has no crossing
 *   a node is IN BAND iff it is finite and |D| < trunc: phi = D bit for bit (the sub-voxel accuracy of the fused value is kept)
 *   any other finite node: phi = s min(max(e, trunc), max_distance), s = +1 if free, -1 if occupied
 * A grid knows only its own crossings: next to the grid's border, where the nearest surface point lies outside the grid, e is
 * the distance to the nearest crossing inside it, which is larger.
 * The computation separates exactly.  With g_c(n) = the distance along axis c from n to the nearest crossing on n's own c-line
 * and env_a(f)(n) = min over m of f(n + m e_a) + m^2:
 *   (e / h)^2 = min( env_x( min( env_y(g_z^2), env_z(g_y^2) ) ), env_y( env_z(g_x^2) ) )
 * Because the output is clamped at max_distance, every 1-D pass looks at offsets |m| <= R = ceil(max_distance / h) only (seeds:
 * crossings on edges within R + 1 nodes).  Eight launches (three seed passes, five envelope passes, the last of which finishes),
 * windowed minima in a fixed order: no atomics, no block waits for another, no allocation, synchronisation or upload, bitwise
 * reproducible, and a grid of a stack gets the bits of the single-grid call.  The call can sit in a captured graph behind
 * gq_tsdf_integrate.  A block holds 16 whole lines of the pass axis in LDS, so an axis may have at most 1024 nodes; R <= 4096;
 * n_grids x tiles of 16 lines <= 2^23 per launch.  workspace: gq_esdf_workspace_bytes(src) bytes on the device (three times the
 * stack), contents irrelevant.  dst_values is dst->values, writable.
 * gq_esdf_check (host only, no GPU) refuses: a NULL src, dst, values pointer or workspace; everything gq_clutter_check refuses
 * for either stack; dst differing from src in n_grids, shape, origin or voxel; dst values aliasing src values; an axis longer
 * than 1024 nodes; more than 2^23 tiles; trunc not finite or <= 0; max_distance not finite or < trunc; a window R > 4096.  The
 * message starts with "esdf:" and names the argument.                                                                   */
int gq_esdf_check(const gqClutterGrids* src, const gqClutterGrids* dst, float trunc, float max_distance,
                  const void* workspace /* only tested against NULL */);
int gq_esdf_workspace_bytes(const gqClutterGrids* src, size_t* bytes);
int gq_esdf(const gqClutterGrids* src, const gqClutterGrids* dst, float* dst_values /* = dst->values, writable */, float trunc,
            float max_distance, void* workspace, void* stream);

/* ---- (re-)initialisation: initialize_convex_hull, core/initializations.py:15-193 (scripts/fit.py:315,408-422) --------
 * Per object: samples_per_object points on its convex hull (area-weighted), pushed out by `inflate` (0.01 in the
 * reference) along the face normal; farthest-point sampling of batch_each of them (start = sample 0); per row the look-at
 * rotation towards the hull composed with a random roll / pitch / tilt, a random stand-off distance, and joint angles
 * from a truncated normal around default_state (sigma = jitter_strength * joint range).  hand_pose (B, 9 + n_dofs),
 * B = n_obj * batch_each, is written for ALL rows; applying it to the rows of an env_mask is the caller's business
 * (HandModel.set_parameters(env_mask=...), GraspStepper.step_reset).  The hull (triangles oriented outward, set-up time)
 * and every random number are inputs: u_face (n_obj, samples) and u_len (n_obj, samples, 2) pick the samples, u_pose
 * (B,4) = distance / rotate / pitch / tilt and u_joint (B, n_dofs), all uniform in [0,1).  Contact indices are a plain
 * randint (initializations.py:190-192) and stay with the caller.                                                    */
typedef struct gqInitDesc {
  const float* hull_face_verts;   /* (sumF,3,3) device */
  const float* hull_cdf;          /* (sumF) device: cumulative face area / total area, per object */
  const int32_t* hull_offsets;    /* (n_obj+1) device */
  int64_t n_obj, batch_each, samples_per_object;
  int32_t n_dofs;
  float inflate;
  float forward_axis[3], up_axis[3];                 /* HandModel.forward_axis / up_axis */
  const float* default_state; const float* joints_lower; const float* joints_upper;  /* (n_dofs) device */
  float jitter_strength, distance_lower, distance_upper, rotate_lower, rotate_upper, pitch_lower, pitch_upper,
      tilt_lower, tilt_upper;                         /* scripts/fit.py:59-71 */
  const float* u_face; const float* u_len; const float* u_pose; const float* u_joint;
  float* hand_pose;               /* (B, 9 + n_dofs) out */
  float* shell_points;            /* (B,3) out or NULL: the inflated hull point each row looks at */
  float* shell_dirs;              /* (B,3) out or NULL: unit direction from that point towards the hull */
  void* workspace; size_t workspace_bytes;           /* gq_init_workspace_bytes */
} gqInitDesc;
int gq_init_workspace_bytes(int64_t n_obj, int64_t samples_per_object, int64_t batch_each, size_t* bytes);
int gq_init_convex_hull(const gqInitDesc* desc, void* stream);

/* ---- scene-aware initialisation: screened hull candidates -------------------------------------------------------------
 * An opt-in route for hands that start next to obstacles: every hull sample becomes a complete candidate pose, the caller
 * scores every candidate with the obstacle terms the stepper evaluates (gq_fk_forward, gq_scene_terms, gq_approach_terms on
 * the candidate rows, unweighted, link_wrench = gRt = NULL), and batch_each candidates per object are picked by farthest-point
 * sampling among the collision-free ones only.
 *
 * gq_init_candidates is gq_init_convex_hull with every sample a row: it requires batch_each == samples_per_object = M, runs
 * no farthest-point pass (the selection is the identity), reads u_pose (n_obj M, 4) and u_joint (n_obj M, n_dofs) and writes
 * hand_pose (n_obj M, 9 + n_dofs); shell_points and shell_dirs (n_obj M, 3) are required: they are the candidate points and
 * directions.  n_obj M < 2^28.  Workspace: gq_init_workspace_bytes(n_obj, M, M).  Contract: candidate m's pose is, bit for
 * bit, what gq_init_convex_hull gives a row that picked sample m with the draws u_pose[m], u_joint[m] (one row body).
 *
 * gq_init_penalty: penalty[i] = fmaf(w_approach, e_approach[i], w_scene * e_scene[i]) for i < n; a NULL term is off and
 * contributes exactly 0.
 *
 * gq_init_select: points (n_obj,M,3) and penalty (n_obj,M) -> sel (n_obj,K) int32 candidate indices and n_feasible (n_obj)
 * int32.  Per object, with A = {m : penalty[m] <= tol} (a NaN penalty is never in A, -0.0 is at tol = 0) and
 * n_feasible = |A|, not capped by K:
 *   phase 1, slots t = 0 .. min(K, |A|) - 1: d[m] = +inf, c = min A; repeat: sel[t] = c, remove c from A, for m in A
 *     d[m] = min(d[m], |P[m] - P[c]|^2), c = argmax over A of d, the smallest index among equals.  The squared distance is the
 *     expression of gq_init_convex_hull's farthest-point pass: with every candidate feasible and distinct points sel is that
 *     pass's, bit for bit.  The picks are distinct also among duplicate points.
 *   phase 2, the remaining slots: the candidates outside the original A in ascending order of (penalty, index); NaN sorts
 *     after +inf.
 * One block of 1024 threads per object; no atomics, no block waits for another, every loop is bounded by K; no allocation,
 * synchronisation or upload: graph-capturable and bitwise reproducible.  workspace: gq_init_select_workspace_bytes(n_obj, M)
 * bytes on the device, contents irrelevant.
 * gq_init_select_check (host only, no GPU) refuses: a NULL points, penalty, sel, n_feasible or workspace; n_obj <= 0; K <= 0;
 * M < K; M >= 2^30; a tol that is NaN or negative.  The message contains "init_select" and names the argument.           */
int gq_init_candidates(const gqInitDesc* desc, void* stream);
int gq_init_penalty(const float* e_scene /* (n) or NULL */, float w_scene, const float* e_approach /* (n) or NULL */,
                    float w_approach, int64_t n, float* penalty, void* stream);
int gq_init_select_check(const float* points, const float* penalty, int64_t n_obj, int64_t M, int64_t K, float tol,
                         const int32_t* sel, const int32_t* n_feasible, const void* workspace /* only tested against NULL */);
int gq_init_select_workspace_bytes(int64_t n_obj, int64_t M, size_t* bytes);
int gq_init_select(const float* points, const float* penalty, int64_t n_obj, int64_t M, int64_t K, float tol, int32_t* sel,
                   int32_t* n_feasible, void* workspace, size_t workspace_bytes, void* stream);
/* ---- grasp-set selection: feasible, ranked, distinct grasps ---------------------------------------------------------------
 * The last stage after the optimiser: of the batch_each rows of every object, the K best that are feasible and pairwise
 * different grasps.  The reference has no counterpart; this replaces the consumer's rule of
 * graspqp_isaaclab/utils/data.py:97-102,105-150 (get_saved_poses: sort by `values`, take the first num_grasps), which returns
 * one basin K times and does not look at the obstacle terms.
 *
 * Distance of two rows i, j of one object: d(i,j)^2 = (1/Ns) sum_s |x_w,i(s) - x_w,j(s)|^2 over the Ns hand-surface samples
 * (x_w = Rg (A_l p_s + b_l) + t, link_T = [A_l | b_l] row-major 3x4, t = hand_pose[0:3]), in metres, evaluated in closed form:
 * with W_l = [Rg A_l | Rg b_l + t], dA, db the difference of two rows' W_l, and per link n_l, the centroid c_l and the centred
 * second moment C_l = sum (p - c_l)(p - c_l)',
 *   sum_{s in l} |dA p_s + db|^2 = n_l |dA c_l + db|^2 + tr(dA C_l dA').
 * link_moments (n_links,10) = n_l, c_l (3), Cxx Cxy Cxz Cyy Cyz Czz, built once at set-up (fp64 sums, stored as float).  Both
 * summands are >= 0 (the quadratic form is clamped at 0 against rounding), the links are summed serially in ascending order,
 * a link with n_l = 0 is skipped: d(i,i) = 0 exactly, d(i,j) = d(j,i) exactly.
 *
 * gq_grasp_select.  hand_pose (batch,pose_dim), Rg (batch,9), link_T (batch,n_links,12), rows object-major with batch_each per
 * object; score (batch), lower is better; terms (n_terms,batch); tol: n_terms HOST floats (copied at the call).
 *   Row b is feasible iff score[b] is finite and terms[t,b] <= tol[t] for every t with tol[t] < +inf (a NaN term under a gate
 *   makes the row infeasible; a term with tol = +inf is not read).
 *   Per object, at most K times: pick the feasible row, neither picked nor suppressed, with the smallest key
 *   (order-preserving bits of score, row) -- ties go to the smallest row; write its global row index to the next slot;
 *   suppress every remaining row r with d^2(r, pick) < radius^2 (strict: radius = 0 suppresses nothing); stop when no row is left.
 * Out: sel (n_obj,K) int32 in pick order, unused slots -1; n_selected (n_obj); n_feasible (n_obj), not capped by K; feasible
 * (batch) 0/1.  There is no fill with infeasible rows.
 * Two launches: one thread per (row, link) writes W, feasible and the keys into the workspace; one block of 256 threads per
 * object selects.  No atomics, no block waits for another, every loop is bounded by K or batch_each; no allocation,
 * synchronisation, upload or host read: graph-capturable on one stream and bitwise reproducible.
 * Limits: n_links <= 64, 1 <= K <= batch_each < 2^30, batch < 2^31, n_terms <= 16.  Workspace:
 * gq_grasp_select_workspace_bytes(batch, n_links) bytes on the device, contents irrelevant.
 *
 * gq_grasp_distances: dist (n_obj,batch_each,batch_each) = d (not d^2) of every pair of rows of an object, through the same
 * device function; batch_each <= 4096.  Same workspace.
 *
 * gq_grasp_select_check / gq_grasp_distances_check (host only, no GPU) refuse: a NULL pointer (terms and tol may be NULL at
 * n_terms = 0); pose_dim < 3; n_links outside 1..64; n_samples <= 0; batch_each out of range; a batch that is not a positive
 * multiple of batch_each; n_terms outside 0..16; a NaN tol; K outside 1..batch_each; a radius that is NaN, negative or
 * infinite; a workspace that is too small.  The message contains "grasp_select" and names the argument.                  */
int gq_grasp_select_workspace_bytes(int64_t batch, int n_links, size_t* bytes);
int gq_grasp_select_check(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                          int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, const float* score,
                          const float* terms, const float* tol /* host */, int n_terms, int64_t K, float radius,
                          const int32_t* sel, const int32_t* n_selected, const int32_t* n_feasible, const int32_t* feasible,
                          const void* workspace /* only tested against NULL */, size_t workspace_bytes);
int gq_grasp_select(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                    int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, const float* score, const float* terms,
                    const float* tol /* host */, int n_terms, int64_t K, float radius, int32_t* sel, int32_t* n_selected,
                    int32_t* n_feasible, int32_t* feasible, void* workspace, size_t workspace_bytes, void* stream);
int gq_grasp_distances_check(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                             const float* link_moments, int n_links, int64_t n_samples, int64_t batch, int64_t batch_each,
                             const float* dist, const void* workspace /* only tested against NULL */, size_t workspace_bytes);
int gq_grasp_distances(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                       int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, float* dist, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Surface samples of object meshes on the device (reference core/object_model.py:163-178: pytorch3d
 * sample_points_from_meshes with 100 x num_samples points, then sample_farthest_points(K = num_samples) starting at sample
 * 0): face_verts (sumF,3,3) of n_obj meshes, area_cdf (sumF) normalised cumulative face area per mesh, face_offsets
 * (n_obj+1); u_face (n_obj,M), u_len (n_obj,M,2) uniform draws; points_out (n_obj,n_keep,3).  Workspace:
 * gq_init_workspace_bytes(n_obj, samples_per_object, n_keep).                                                          */
int gq_surface_fps(const float* face_verts, const float* area_cdf, const int32_t* face_offsets, int64_t n_obj,
                   int64_t samples_per_object, int64_t n_keep, const float* u_face, const float* u_len, float* points_out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- MALA* optimiser: MalaStar.try_step / accept_step, core/optimizer.py:199-273,289-340; fit.py:403-406,454-458
 * random draws are inputs: u_switch (B,n) U[0,1), new_idx (B,n) in [0,C), u_accept (B) U[0,1).  pose_dim <= 128;
 * gq_mala_accept merges n_terms <= 64 rows of terms_new (n_terms,B) into terms, one term per lane.           */
int gq_mala_propose(const float* hand_pose, const float* grad, const int64_t* contact_idx, const float* u_switch,
                    const int64_t* new_idx, int64_t batch, int pose_dim, int n_contact, float step_size,
                    int stepsize_period, float decay, float mu, float switch_possibility, int clip_grad,
                    float* ema /* (B,D) in/out */, int64_t* step /* (B) in/out */, float* pose_out, int64_t* idx_out,
                    float* step_size_out /* (B) or NULL */, float* g2_scratch /* (D) */,
                    const float* energy /* (B) or NULL: also emit the per-object z-score of the accepted energies */,
                    int64_t batch_each, float* z_out /* (B) */, void* stream);
int gq_mala_accept(const float* new_energy, const float* u_accept, const float* z, const uint8_t* reset_mask,
                   const int64_t* step, const float* pose_new, const int64_t* idx_new, const float* grad_new,
                   int64_t batch, int pose_dim, int n_contact, float starting_temperature, float decay,
                   int annealing_period, float* energy, float* pose, int64_t* idx, float* grad, uint8_t* accept,
                   float* temperature, int n_terms, const float* terms_new, float* terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRASPQP_HIP_H */
