// E_hold: can these contacts, at this friction and with at most F newtons per cone edge, carry the object's load wrenches?
// (include/graspqp_hip.h, "payload holding", has the formulas.)
//
// Per row and load l: F (6 x nz) is the E_fc step's cone matrix on the INWARD normals, w_l the load with its torque rows in F's
// units, x_l = argmin_{0 <= x <= u} |F x + w_l|^2 + ridge |x|^2 by `iterations` PDIPM iterations of the low-rank (Woodbury)
// solver in fp64 (hold_dev.h), E = mean_l V_l(x_l) / |w_l|^2.  ONE launch, one block per row, one wavefront per load:
//
//   0. the row's contacts (points, inward normals; with a torque output their hand-frame position and joint path) once, in LDS
//   1. wavefront l, lane = column(s): the cone column, p = F'w_l, the row-local loop (hold_dev.h), its best iterate evaluated
//      (seven wave sums), then per column the force share x f and the share of dE/dp, folded per contact in edge order
//   2. wavefront l, lane = tree joint: tau = J' R' force walked over the row's contacts, folded with C' for a coupled hand
//   3. wavefront 0: the mean over the loads, the sum of dE/dp over the loads and the largest effort, in load order through LDS
//
// No atomics, every sum in a fixed order, nothing read from another row: bitwise reproducible run to run and row by row, and
// graph-capturable.
#include "kin_dev.h"
#include "hold_dev.h"

struct GqHoldArgs {
  gqHand h;
  const float* node_W;  // (B,J,12) from gq_fk_forward's workspace
  const float* link_T;  // (B,L,12)
  const int64_t* idx;   // (B,n)
  const float *obj_normal, *contact_pts, *cog, *Rg, *loads, *limits, *up;
  long long loads_each;
  int n, k, nz, L, iters, accumulate, kin;
  float mu, tw, upper, ridge, w;
  float *e, *resid, *x, *force, *torque, *effort, *g_contact_pts;
};

template <int NC>
__global__ __launch_bounds__(GQ_HOLD_MAX_L* GQ_WAVE) void gq_hold_kernel(const GqHoldArgs g) {
  __shared__ float s_cp[GQ_SQ_MAX * 3], s_nin[GQ_SQ_MAX * 3], s_xh[GQ_SQ_MAX * 3];
  __shared__ unsigned long long s_mask[GQ_SQ_MAX];
  __shared__ float s_col[GQ_HOLD_MAX_L][GQ_HOLD_MAX_NZ * 6];
  __shared__ float s_fh[GQ_HOLD_MAX_L][GQ_SQ_MAX * 3], s_gp[GQ_HOLD_MAX_L][GQ_SQ_MAX * 3], s_tt[GQ_HOLD_MAX_L][GQ_SQ_MAX];
  __shared__ float s_e[GQ_HOLD_MAX_L], s_eff[GQ_HOLD_MAX_L];
  const gqHand& h = g.h;
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid >> 6;  // wavefront wv = load wv
  const size_t row = blockIdx.x;
  const int n = g.n, nz = g.nz, L = g.L;
  float R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = g.Rg ? g.Rg[row * 9 + i] : 0.0f;

  // ---- 0. the row's contacts, once --------------------------------------------------------------------------------------------
  if (tid < n) {
    const size_t q = row * n + tid;
    const gq3 nin = gq_hold_inward(gq_mk(g.obj_normal[q * 3], g.obj_normal[q * 3 + 1], g.obj_normal[q * 3 + 2]));
    s_cp[tid * 3] = g.contact_pts[q * 3]; s_cp[tid * 3 + 1] = g.contact_pts[q * 3 + 1]; s_cp[tid * 3 + 2] = g.contact_pts[q * 3 + 2];
    s_nin[tid * 3] = nin.x; s_nin[tid * 3 + 1] = nin.y; s_nin[tid * 3 + 2] = nin.z;
    if (g.kin) {
      const int ci = (int)g.idx[q];
      const int l = h.cand_link[ci];
      const gq3 x = gq_t_apply(gq_t_load(g.link_T + (row * h.L + l) * 12),
                               gq_mk(h.cand_pos[ci * 3], h.cand_pos[ci * 3 + 1], h.cand_pos[ci * 3 + 2]));
      s_xh[tid * 3] = x.x; s_xh[tid * 3 + 1] = x.y; s_xh[tid * 3 + 2] = x.z;
      unsigned long long m = 0;
      for (int nd = h.link_node[l]; nd >= 0; nd = h.node_parent[nd]) m |= 1ull << nd;
      s_mask[tid] = m;
    }
  }
  __syncthreads();

  // ---- 1. columns, the loop, the iterate evaluated ----------------------------------------------------------------------------
  GqHoldLr<NC> S;
  S.ridge = (double)g.ridge;
  float w[6];
  gq_hold_load(g.loads + ((size_t)((long long)row / g.loads_each) * L + wv) * 6, g.tw, w);
  const float* cog = g.cog + row * 3;
  bool live[NC];
  double p[NC], hu[NC], hl[NC], xd[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int i = lane + GQ_WAVE * c;
    live[c] = i < nz;
    hu[c] = live[c] ? (double)g.upper : 1.0;
    hl[c] = live[c] ? 0.0 : 1.0;
    xd[c] = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) S.a[c][r] = 0.0f;
    if (live[c]) gq_hold_column(s_cp, s_nin, cog, i, g.k, g.mu, g.tw, S.a[c]);
    p[c] = gq_hold_p(S.a[c], w);
  }
  gq_hold_iterate<NC>(nz, g.iters, S, live, p, hu, hl, xd);

  // the iterate's seven sums in fp64 (F x cancels against w where the load is carried), rounded once; the rest is fp32
  float xb[NC];
  double dsum[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    xb[c] = (float)xd[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) dsum[r] = fma((double)S.a[c][r], xd[c], dsum[r]);
    dsum[6] = fma(xd[c], xd[c], dsum[6]);
  }
  gq_wave_sums_d<7>(dsum);
  float sums[7];
#pragma unroll
  for (int r = 0; r < 7; ++r) sums[r] = (float)dsum[r];
  const GqHoldEval ev = gq_hold_eval(sums, w, g.ridge, L);
  const float c_up = g.up ? g.up[row] * g.w : g.w;
  if (lane == 0) {
    s_e[wv] = ev.e;
    if (g.resid) g.resid[row * L + wv] = ev.resid;
  }
  float* col = s_col[wv];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (live[c]) {
      const int i = lane + GQ_WAVE * c;
      if (g.x) g.x[(row * L + wv) * nz + i] = xb[c];
      const gq3 f = gq_hold_force(S.a[c], xb[c]);
      const gq3 gp = gq_hold_gp(S.a[c], xb[c], ev.r, ev.c2 * c_up, g.tw);
      col[i * 6] = f.x; col[i * 6 + 1] = f.y; col[i * 6 + 2] = f.z;
      col[i * 6 + 3] = gp.x; col[i * 6 + 4] = gp.y; col[i * 6 + 5] = gp.z;
    }
  }
  gq_wave_sync();
  if (lane < n) {  // lane c = contact c: its k columns in edge order
    float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = 0; e < g.k; ++e)
#pragma unroll
      for (int r = 0; r < 6; ++r) a[r] += col[(lane * g.k + e) * 6 + r];
    if (g.force) {
      float* o = g.force + ((row * L + wv) * n + lane) * 3;
      o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
    }
    const gq3 fh = gq_squeeze_to_hand(R, gq_mk(a[0], a[1], a[2]));
    s_fh[wv][lane * 3] = fh.x; s_fh[wv][lane * 3 + 1] = fh.y; s_fh[wv][lane * 3 + 2] = fh.z;
    s_gp[wv][lane * 3] = a[3]; s_gp[wv][lane * 3 + 1] = a[4]; s_gp[wv][lane * 3 + 2] = a[5];
  }
  gq_wave_sync();

  // ---- 2. joint torques of this load: lane = tree joint, the row's contacts in order -------------------------------------------
  if (g.kin) {
    const int J = h.J, JA = h.JA;
    gq3 ak = gq_mk(0, 0, 0), pk = gq_mk(0, 0, 0);
    int tk = 0;
    if (lane < J) {
      const GqT W = gq_t_load(g.node_W + (row * J + lane) * 12);
      ak = gq_t_rot(W, gq_mk(h.node_axis[lane * 3], h.node_axis[lane * 3 + 1], h.node_axis[lane * 3 + 2]));
      pk = gq_t_pos(W);
      tk = h.node_type[lane];
    }
    float tau = 0.0f;
    for (int c = 0; c < n; ++c) {
      const bool on_path = lane < J && ((s_mask[c] >> lane) & 1ull);
      tau += gq_hold_torque(tk, on_path, ak, pk, gq_mk(s_xh[c * 3], s_xh[c * 3 + 1], s_xh[c * 3 + 2]),
                            gq_mk(s_fh[wv][c * 3], s_fh[wv][c * 3 + 1], s_fh[wv][c * 3 + 2]));
    }
    if (h.coup) {
      s_tt[wv][lane] = tau;  // 0 for lanes >= J
      gq_wave_sync();
      tau = lane < JA ? gq_hold_fold(h.coup, J, JA, lane, s_tt[wv]) : 0.0f;
    }
    if (g.torque && lane < JA) g.torque[(row * L + wv) * JA + lane] = tau;
    if (g.effort) {
      const float m = -gq_dpp_min(lane < JA ? -fabsf(tau) / g.limits[lane] : 0.0f);
      if (lane == 0) s_eff[wv] = m;
    }
  }
  __syncthreads();

  // ---- 3. the loads folded in load order ---------------------------------------------------------------------------------------
  if (wv != 0) return;
  if (lane == 0) {
    float e = 0.0f, m = 0.0f;
    for (int l = 0; l < L; ++l) e += s_e[l];
    if (g.e) g.e[row] = e / (float)L;
    if (g.effort) {
      for (int l = 0; l < L; ++l) m = fmaxf(m, s_eff[l]);
      g.effort[row] = m;
    }
  }
  if (g.g_contact_pts && lane < n) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int l = 0; l < L; ++l) {
      sx += s_gp[l][lane * 3];
      sy += s_gp[l][lane * 3 + 1];
      sz += s_gp[l][lane * 3 + 2];
    }
    float* o = g.g_contact_pts + (row * n + lane) * 3;
    const bool add = g.accumulate & 1;
    o[0] = add ? o[0] + sx : sx;
    o[1] = add ? o[1] + sy : sy;
    o[2] = add ? o[2] + sz : sz;
  }
}

extern "C" int gq_hold_terms(const gqHand* h, const int64_t* contact_idx, int64_t batch, int n_contact, int n_cone,
                             const float* obj_normal, const float* contact_pts, const float* cog, const float* Rg,
                             const float* link_T, const void* workspace, size_t workspace_bytes, const float* loads,
                             const float* loads_host, int64_t n_load_sets, int n_loads, int64_t loads_each, float friction,
                             float torque_weight, float max_force, float ridge, int n_iterations, const float* torque_limits,
                             const float* up, float w, float* e, float* resid, float* x, float* force, float* torque,
                             float* effort, int accumulate, float* g_contact_pts, void* stream) {
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll, "hold: batch must be in 1..2^31-1, got %lld", (long long)batch);
  GQ_REQUIRE(n_contact >= 1 && n_contact <= GQ_SQ_MAX, "hold: 1..%d contacts are supported, got n=%d", GQ_SQ_MAX, n_contact);
  GQ_REQUIRE(n_cone >= 3 && (long long)n_contact * n_cone <= GQ_HOLD_MAX_NZ,
             "hold: n_cone >= 3 and n_contact * n_cone <= %d columns are supported, got %d x %d", GQ_HOLD_MAX_NZ, n_contact, n_cone);
  GQ_REQUIRE(n_loads >= 1 && n_loads <= GQ_HOLD_MAX_L, "hold: 1..%d loads are supported, got %d", GQ_HOLD_MAX_L, n_loads);
  GQ_REQUIRE(n_iterations >= 1 && n_iterations <= 64, "hold: iterations must be in 1..64, got %d", n_iterations);
  GQ_REQUIRE(friction > 0.0f && friction <= 1.0f, "hold: friction must be in (0, 1], got %g", (double)friction);
  GQ_REQUIRE(torque_weight >= 0.0f && torque_weight < GQ_INF_F, "hold: torque_weight must be finite and >= 0, got %g",
             (double)torque_weight);
  GQ_REQUIRE(max_force > 0.0f && max_force < GQ_INF_F, "hold: max_force must be finite and > 0, got %g", (double)max_force);
  GQ_REQUIRE(ridge > 0.0f && ridge < GQ_INF_F, "hold: ridge must be finite and > 0, got %g", (double)ridge);
  GQ_REQUIRE(obj_normal && contact_pts && cog && loads, "hold: null pointer");
  GQ_REQUIRE(n_load_sets >= 1 && loads_each >= 1 && (batch - 1) / loads_each < n_load_sets,
             "hold: %lld load sets of %lld rows each do not cover %lld rows", (long long)n_load_sets, (long long)loads_each,
             (long long)batch);
  for (int64_t i = 0; loads_host && i < n_load_sets * n_loads; ++i) {
    float ww = 0.0f;
    for (int r = 0; r < 6; ++r) {
      const float wl = r < 3 ? loads_host[i * 6 + r] : torque_weight * loads_host[i * 6 + r];
      ww += wl * wl;
    }
    GQ_REQUIRE(ww > 0.0f && ww < GQ_INF_F, "hold: load %lld must be finite with |w| > 0 (torque rows times torque_weight), got |w|^2 = %g",
               (long long)i, (double)ww);
  }
  const bool kin = torque || effort;
  GQ_REQUIRE(!effort || torque_limits, "hold: effort needs torque_limits");
  if (kin) {
    GQ_REQUIRE(h && contact_idx && Rg && link_T && workspace, "hold: torque / effort need the hand and its kinematic state");
    GQ_REQUIRE(h->J >= 1 && h->J <= GQ_SQ_MAX && h->JA >= 1 && h->JA <= GQ_SQ_MAX,
               "hold: at most %d joints are supported, got J=%d JA=%d", GQ_SQ_MAX, h->J, h->JA);
    GQ_REQUIRE(workspace_bytes >= (size_t)batch * h->J * 12 * sizeof(float), "hold: not an FK workspace of this batch");
  }
  GqHoldArgs a{};
  if (kin) a.h = *h;
  a.node_W = (const float*)workspace;
  a.link_T = link_T, a.idx = contact_idx;
  a.obj_normal = obj_normal, a.contact_pts = contact_pts, a.cog = cog, a.Rg = Rg, a.loads = loads, a.limits = torque_limits, a.up = up;
  a.loads_each = loads_each;
  a.n = n_contact, a.k = n_cone, a.nz = n_contact * n_cone, a.L = n_loads, a.iters = n_iterations, a.accumulate = accumulate & 1;
  a.kin = kin ? 1 : 0;
  a.mu = friction, a.tw = torque_weight, a.upper = max_force, a.ridge = ridge, a.w = w;
  a.e = e, a.resid = resid, a.x = x, a.force = force, a.torque = torque, a.effort = effort, a.g_contact_pts = g_contact_pts;
  const dim3 grid((unsigned)batch), block((unsigned)(n_loads * GQ_WAVE));
  if (a.nz <= GQ_WAVE) hipLaunchKernelGGL(gq_hold_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(gq_hold_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
