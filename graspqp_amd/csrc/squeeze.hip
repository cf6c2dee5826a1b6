// E_squeeze: can the fingers close onto the object from this pose?  (reference core/energy.py:80-87, E_manipulativity, through
// hand_model.py:1155-1218 get_req_joint_velocities and the damped pseudo-inverse of hand_model.py:46-54.)
//
// Every contact moves along the outward object normal by s = max(|distance|, tau); theta = (J'J + lambda I)^-1 J' d_h are the joint
// velocities that produce this motion best, r = J theta - d_h is the part they cannot produce, E = mean r^2.  ONE launch computes
// the value and all three gradient parts of every row (include/graspqp_hip.h, "contact closing feasibility", has the formulas):
//
//   0. lane = contact: the contact in the hand frame, its motion d and d_h = R' d (the dependent loads of all contacts side by side)
//   1. per contact: the Jacobian column of every joint (lane = tree joint, folded with C for a coupled hand), the motion d and
//      d_h = R' d, the contact's share of J'J (lower triangle, lane = column) and of J'd_h -- fp64 in LDS
//   2. left-looking Cholesky of J'J + lambda I, lane = row; the two solves (theta, then M^-1 theta: J'r = -lambda theta, so the
//      backward's second solve reuses the factor) with lane i owning entry i of the right-hand side and the solved entry handed
//      round by v_readlane: no step is left to one lane
//   3. per contact again: r and v = g - J u from six wave sums of fixed shape, the energy, g_R, the contact-point gradient and the
//      walk over the closed-form kinematic Hessian with the rank-two dE/dJ = v theta' - r u' formed on the fly
//
// One wavefront per row, no atomics, every sum in a fixed order: bitwise reproducible and graph-capturable.  J is recomputed in
// step 3 (three cross products per lane and contact) rather than kept: the normal matrix alone takes up to 33 KB of LDS.
#include "kin_dev.h"
#include "squeeze_dev.h"

struct GqSqueezeArgs {
  gqHand h;
  const float* node_W;   // (B,J,12) from gq_fk_forward's workspace
  const float* link_T;   // (B,L,12)
  const int64_t* idx;    // (B,n)
  const float *dist_sq, *obj_normal, *closest, *contact_pts, *Rg, *up, *g_R_base;
  int n, accumulate;
  float tau, lambda, w;
  float *e, *theta, *g_theta, *g_R, *g_contact_pts;
};

__device__ __forceinline__ double gq_sq_readlane_d(double v, int l) {
  const GqD2 s = gq_split_d(v);
  return gq_join_d(__builtin_amdgcn_readlane(s.lo, l), __builtin_amdgcn_readlane(s.hi, l));
}

// tree-joint column -> actuated column (J_act = J_tree C) through LDS; identity for an uncoupled hand
__device__ __forceinline__ gq3 gq_sq_fold(const gqHand& h, int lane, gq3 col, float* s_col) {
  if (!h.coup) return col;
  gq_wave_sync();
  s_col[lane * 3] = col.x; s_col[lane * 3 + 1] = col.y; s_col[lane * 3 + 2] = col.z;
  gq_wave_sync();
  gq3 v = gq_mk(0.0f, 0.0f, 0.0f);
  if (lane < h.JA)
    for (int j = 0; j < h.J; ++j) {
      const float cj = h.coup[j * h.JA + lane];
      v = gq_mk(fmaf(cj, s_col[j * 3], v.x), fmaf(cj, s_col[j * 3 + 1], v.y), fmaf(cj, s_col[j * 3 + 2], v.z));
    }
  return v;
}

// L L' x = b for the factor in A; lane i < JA owns b_i and dinv = 1 / L[i][i] (one division per lane for both solves), the other
// lanes carry dead values
__device__ __forceinline__ double gq_sq_solve(const double* A, int LD, int JA, int lane, double b, double dinv) {
  for (int k = 0; k < JA; ++k) {
    const double yk = gq_sq_readlane_d(b * dinv, k);
    if (lane == k) b = yk;
    else if (lane > k && lane < JA) b = gq_squeeze_sub(b, A[(size_t)lane * LD + k], yk);
  }
  for (int k = JA - 1; k >= 0; --k) {
    const double xk = gq_sq_readlane_d(b * dinv, k);
    if (lane == k) b = xk;
    else if (lane < k) b = gq_squeeze_sub(b, A[(size_t)k * LD + lane], xk);
  }
  return b;
}

__global__ __launch_bounds__(GQ_WAVE) void gq_squeeze_kernel(const GqSqueezeArgs g) {
  extern __shared__ double gq_sq_A[];  // JA x LD, lower triangle: J'J + lambda I, then its Cholesky factor
  __shared__ int s_parent[GQ_SQ_MAX], s_type[GQ_SQ_MAX];
  __shared__ float s_a[GQ_SQ_MAX * 3], s_p[GQ_SQ_MAX * 3], s_col[GQ_SQ_MAX * 3], s_cola[GQ_SQ_MAX * 3];
  __shared__ float s_x[GQ_SQ_MAX * 3], s_dh[GQ_SQ_MAX * 3], s_th[GQ_SQ_MAX], s_u[GQ_SQ_MAX], s_tt[GQ_SQ_MAX], s_ut[GQ_SQ_MAX];
  __shared__ float s_d[GQ_SQ_MAX * 3], s_v[GQ_SQ_MAX * 3];
  __shared__ int s_start[GQ_SQ_MAX], s_free[GQ_SQ_MAX];
  __shared__ unsigned long long s_mask[GQ_SQ_MAX];
  const gqHand& h = g.h;
  const int J = h.J, JA = h.JA, n = g.n, LD = gq_squeeze_ld(JA);
  const int lane = gq_lane();
  const size_t row = blockIdx.x;
  double* A = gq_sq_A;
  gq3 ak = gq_mk(0, 0, 0), pk = gq_mk(0, 0, 0);
  int tk = 0;
  if (lane < J) {
    const GqT W = gq_t_load(g.node_W + (row * J + lane) * 12);
    ak = gq_t_rot(W, gq_mk(h.node_axis[lane * 3], h.node_axis[lane * 3 + 1], h.node_axis[lane * 3 + 2]));
    pk = gq_t_pos(W);
    tk = h.node_type[lane];
    s_parent[lane] = h.node_parent[lane];
    s_type[lane] = tk;
    s_a[lane * 3] = ak.x; s_a[lane * 3 + 1] = ak.y; s_a[lane * 3 + 2] = ak.z;
    s_p[lane * 3] = pk.x; s_p[lane * 3 + 1] = pk.y; s_p[lane * 3 + 2] = pk.z;
  }
  for (int i = lane; i < JA * LD; i += GQ_WAVE) A[i] = 0.0;
  float R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = g.Rg[row * 9 + i];
  // lane c = contact c: its point in the hand frame, the node its link rides on, its motion.  The chain of dependent loads
  // (index -> link -> transform) runs once, for all contacts side by side, not once per turn of the loops below.
  if (lane < n) {
    const size_t q = row * n + lane;
    const int ci = (int)g.idx[q];
    const int l = h.cand_link[ci];
    const gq3 x = gq_t_apply(gq_t_load(g.link_T + (row * h.L + l) * 12),
                             gq_mk(h.cand_pos[ci * 3], h.cand_pos[ci * 3 + 1], h.cand_pos[ci * 3 + 2]));
    float s;
    bool free_travel;
    const gq3 d = gq_squeeze_dir(g.dist_sq[q], gq_mk(g.obj_normal[q * 3], g.obj_normal[q * 3 + 1], g.obj_normal[q * 3 + 2]), g.tau,
                                 s, free_travel);
    const gq3 dh = gq_squeeze_to_hand(R, d);
    s_start[lane] = h.link_node[l];
    s_free[lane] = free_travel ? 1 : 0;
    s_x[lane * 3] = x.x; s_x[lane * 3 + 1] = x.y; s_x[lane * 3 + 2] = x.z;
    s_d[lane * 3] = d.x; s_d[lane * 3 + 1] = d.y; s_d[lane * 3 + 2] = d.z;
    s_dh[lane * 3] = dh.x; s_dh[lane * 3 + 1] = dh.y; s_dh[lane * 3 + 2] = dh.z;
  }
  gq_wave_sync();

  // ---- 1. columns, motions, normal equations ---------------------------------------------------------------------------------
  double b = 0.0;
  for (int c = 0; c < n; ++c) {  // wave-uniform loop
    const gq3 x = gq_mk(s_x[c * 3], s_x[c * 3 + 1], s_x[c * 3 + 2]);
    const gq3 dh = gq_mk(s_dh[c * 3], s_dh[c * 3 + 1], s_dh[c * 3 + 2]);
    bool on_path = false;
    for (int nd = s_start[c]; nd >= 0; nd = s_parent[nd]) on_path |= (nd == lane);
    on_path = on_path && lane < J;
    const unsigned long long mask = __ballot(on_path);
    const gq3 col = gq_sq_fold(h, lane, gq_squeeze_col(tk, on_path, ak, pk, x), s_col);
    gq_wave_sync();  // the previous contact's columns have been read
    if (lane == 0) s_mask[c] = mask;
    if (lane < JA) {
      s_cola[lane * 3] = col.x; s_cola[lane * 3 + 1] = col.y; s_cola[lane * 3 + 2] = col.z;
      b += gq_squeeze_gram(col, dh);
    }
    gq_wave_sync();
    if (lane < JA)
      for (int i = lane; i < JA; ++i)
        A[(size_t)i * LD + lane] += gq_squeeze_gram(gq_mk(s_cola[i * 3], s_cola[i * 3 + 1], s_cola[i * 3 + 2]), col);
  }
  if (lane < JA) A[(size_t)lane * LD + lane] += (double)g.lambda;
  gq_wave_sync();

  // ---- 2. Cholesky (left-looking, lane = row) and the solves -----------------------------------------------------------------
  for (int k = 0; k < JA; ++k) {
    double s = 1.0;
    if (lane >= k && lane < JA) s = gq_squeeze_chol_dot(A, LD, lane, k);
    const double dkk = sqrt(gq_sq_readlane_d(s, k));
    if (lane == k) A[(size_t)k * LD + k] = dkk;
    else if (lane > k && lane < JA) A[(size_t)lane * LD + k] = s / dkk;
    gq_wave_sync();
  }
  const double dinv = lane < JA ? 1.0 / A[(size_t)lane * LD + lane] : 0.0;
  const double th = gq_sq_solve(A, LD, JA, lane, b, dinv);
  const float thf = lane < JA ? (float)th : 0.0f;
  if (g.theta && lane < JA) g.theta[row * JA + lane] = thf;
  const bool grad = g.g_theta || g.g_R || g.g_contact_pts;
  const float c_up = (g.up ? g.up[row] * g.w : g.w) / (float)(3 * n);
  float uf = 0.0f;
  if (grad) {  // u = M^-1 J' g with g = 2 c r, and J' r = -lambda theta
    const double m = gq_sq_solve(A, LD, JA, lane, th, dinv);
    uf = lane < JA ? (float)(-2.0 * (double)c_up * (double)g.lambda * m) : 0.0f;
  }
  // theta and u per TREE joint (C theta, C u) for the Hessian walk
  s_th[lane] = thf;
  s_u[lane] = uf;
  gq_wave_sync();
  if (lane < J) {
    float tt = thf, ut = uf;
    if (h.coup) {
      tt = ut = 0.0f;
      for (int a = 0; a < JA; ++a) {
        const float cj = h.coup[lane * JA + a];
        tt = fmaf(cj, s_th[a], tt);
        ut = fmaf(cj, s_u[a], ut);
      }
    }
    s_tt[lane] = tt;
    s_ut[lane] = ut;
  }
  gq_wave_sync();

  // ---- 3. residuals, energy, gradients ---------------------------------------------------------------------------------------
  float e = 0.0f, acc = 0.0f;
  float gR[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int c = 0; c < n; ++c) {
    const gq3 x = gq_mk(s_x[c * 3], s_x[c * 3 + 1], s_x[c * 3 + 2]);
    const gq3 dh = gq_mk(s_dh[c * 3], s_dh[c * 3 + 1], s_dh[c * 3 + 2]);
    const bool on_path = (s_mask[c] >> lane) & 1ull;
    const gq3 col = gq_sq_fold(h, lane, gq_squeeze_col(tk, on_path, ak, pk, x), s_col);  // lanes >= JA: thf = uf = 0
    float sums[6] = {col.x * thf, col.y * thf, col.z * thf, col.x * uf, col.y * uf, col.z * uf};
    gq_wave_sums_f<6>(sums);
    const gq3 r = gq_squeeze_resid(gq_mk(sums[0], sums[1], sums[2]), dh);
    e = fmaf(r.x, r.x, fmaf(r.y, r.y, fmaf(r.z, r.z, e)));
    if (!grad) continue;
    const float c2 = 2.0f * c_up;
    const gq3 v = gq_mk(fmaf(c2, r.x, -sums[3]), fmaf(c2, r.y, -sums[4]), fmaf(c2, r.z, -sums[5]));
    const gq3 d = gq_mk(s_d[c * 3], s_d[c * 3 + 1], s_d[c * 3 + 2]);
    // dE/dR[a][cc] = sum_i d_i[a] (-v_i)[cc]
    gR[0] = fmaf(d.x, -v.x, gR[0]); gR[1] = fmaf(d.x, -v.y, gR[1]); gR[2] = fmaf(d.x, -v.z, gR[2]);
    gR[3] = fmaf(d.y, -v.x, gR[3]); gR[4] = fmaf(d.y, -v.y, gR[4]); gR[5] = fmaf(d.y, -v.z, gR[5]);
    gR[6] = fmaf(d.z, -v.x, gR[6]); gR[7] = fmaf(d.z, -v.y, gR[7]); gR[8] = fmaf(d.z, -v.z, gR[8]);
    if (lane == 0) {
      s_v[c * 3] = v.x; s_v[c * 3 + 1] = v.y; s_v[c * 3 + 2] = v.z;
    }
    if (g.g_theta && on_path) acc += gq_squeeze_hess(lane, s_start[c], s_parent, s_type, s_a, s_p, x, v, r, s_tt, s_ut);
  }
  if (g.g_contact_pts) {  // lane c = contact c again: its loads side by side
    gq_wave_sync();
    if (lane < n) {
      const size_t q = row * n + lane;
      const gq3 gp = gq_squeeze_gp(R, gq_mk(g.obj_normal[q * 3], g.obj_normal[q * 3 + 1], g.obj_normal[q * 3 + 2]),
                                   gq_mk(s_v[lane * 3], s_v[lane * 3 + 1], s_v[lane * 3 + 2]), s_free[lane] != 0, g.dist_sq[q],
                                   gq_mk(g.contact_pts[q * 3], g.contact_pts[q * 3 + 1], g.contact_pts[q * 3 + 2]),
                                   gq_mk(g.closest[q * 3], g.closest[q * 3 + 1], g.closest[q * 3 + 2]));
      float* o = g.g_contact_pts + q * 3;
      const bool add = g.accumulate & 1;
      o[0] = add ? o[0] + gp.x : gp.x;
      o[1] = add ? o[1] + gp.y : gp.y;
      o[2] = add ? o[2] + gp.z : gp.z;
    }
  }
  if (lane == 0 && g.e) g.e[row] = e / (float)(3 * n);
  if (g.g_R && lane < 9) {
    float val = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) val = lane == i ? gR[i] : val;
    if (g.g_R_base) val += g.g_R_base[row * 9 + lane];
    g.g_R[row * 9 + lane] = val;
  }
  if (g.g_theta) {
    if (h.coup) {  // the tree gradient folded back with C'
      gq_wave_sync();
      s_col[lane] = lane < J ? acc : 0.0f;
      gq_wave_sync();
      acc = 0.0f;
      if (lane < JA)
        for (int j = 0; j < J; ++j) acc = fmaf(h.coup[j * JA + lane], s_col[j], acc);
    }
    if (lane < JA) {
      float* o = g.g_theta + row * JA + lane;
      *o = (g.accumulate & 2) ? *o + acc : acc;
    }
  }
}

extern "C" int gq_squeeze_terms(const gqHand* h, const int64_t* contact_idx, int64_t batch, int n_contact, const float* dist_sq,
                                const float* obj_normal, const float* closest, const float* contact_pts, const float* Rg,
                                const float* link_T, const void* workspace, size_t workspace_bytes, float min_travel, float damping,
                                const float* up, float w, float* e, float* theta, int accumulate, float* g_theta, float* g_R,
                                const float* g_R_base, float* g_contact_pts, void* stream) {
  GQ_REQUIRE(h, "squeeze: hand is NULL");
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "squeeze: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(h->J >= 1 && h->J <= GQ_SQ_MAX && h->JA >= 1 && h->JA <= GQ_SQ_MAX && n_contact >= 1 && n_contact <= GQ_SQ_MAX,
             "squeeze: at most %d joints and %d contacts are supported, got J=%d JA=%d n=%d", GQ_SQ_MAX, GQ_SQ_MAX, h->J, h->JA,
             n_contact);
  GQ_REQUIRE(contact_idx && dist_sq && obj_normal && Rg && link_T && workspace, "squeeze: null pointer");
  GQ_REQUIRE(!g_contact_pts || (closest && contact_pts), "squeeze: g_contact_pts needs closest and contact_pts");
  GQ_REQUIRE(workspace_bytes >= (size_t)batch * h->J * 12 * sizeof(float), "squeeze: not an FK workspace of this batch");
  GQ_REQUIRE(min_travel > 0.0f && min_travel < GQ_INF_F, "squeeze: min_travel must be finite and > 0, got %g", (double)min_travel);
  GQ_REQUIRE(damping > 0.0f && damping < GQ_INF_F, "squeeze: damping must be finite and > 0, got %g", (double)damping);
  GqSqueezeArgs a{};
  a.h = *h;
  a.node_W = (const float*)workspace;
  a.link_T = link_T, a.idx = contact_idx;
  a.dist_sq = dist_sq, a.obj_normal = obj_normal, a.closest = closest, a.contact_pts = contact_pts, a.Rg = Rg, a.up = up;
  a.g_R_base = g_R_base;
  a.n = n_contact, a.accumulate = accumulate & 3;
  a.tau = min_travel, a.lambda = damping, a.w = w;
  a.e = e, a.theta = theta, a.g_theta = g_theta, a.g_R = g_R, a.g_contact_pts = g_contact_pts;
  const size_t lds = (size_t)h->JA * gq_squeeze_ld(h->JA) * sizeof(double);
  hipLaunchKernelGGL(gq_squeeze_kernel, dim3((unsigned)batch), dim3(GQ_WAVE), lds, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
