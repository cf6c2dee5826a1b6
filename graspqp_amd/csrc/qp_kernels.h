// The PDIPM loop and the KKT backward row of the batched box QP (see qp.hip for the overview): the loop is shared by the
// low-rank kernels (qp_lr.h), the dense LDS kernels (qp_dense.hip) and the fused force-closure head (fcstep_dev.h), the
// backward row by every backward kernel.  Below them the register-Cholesky kernels for dense Q with nz <= 64,
// instantiated per NZ in qp_nz*.hip so that the heavily unrolled bodies compile in parallel.
#pragma once
#include "qp_core.h"
#include "wave.h"

struct GqQpArgs {
  const float* A;      // low-rank form Q = A'A + ridge I: (B, m, nz); null for a dense Q
  const float* b;      // low-rank form: (B, m) or null (= 0)
  const float* Q;      // dense form: (B, nz, nz)
  const float* p;      // dense form: (B, nz) or null
  const float* lower;  // (B, nz) or null -> lower_s
  const float* upper;  // (B, nz) or null -> upper_s
  float lower_s, upper_s, ridge;
  int B, m, nz, max_iter;
  float* resid;  // (B, max_iter)
  float* mu;     // (B, max_iter)
  float* snap;   // (B, max_iter, 5, nz): x, lam_u, lam_l, slack_u, slack_l
  float* slot;   // (B, nz, 5), gq_qp_lr_iterate<true> only: the row's best iterate among iterations 0 .. max_iter - 2, five words per column
                 // (the last iteration's snapshot has a fixed address in `snap` anyway)
};

// ---- backward: (dx, _, dlam) = solve_kkt(d, grad_x, 0, 0), d = clamp(lam,1e-8)/clamp(slack,1e-8) ---------------
struct GqQpBwdArgs {
  const float* A;  // low-rank form; null for a dense Q
  const float* Q;  // dense form
  const float* lam;
  const float* slack;
  const float* grad_x;
  float ridge;
  int B, m, nz;
  float* dx;    // (B, nz)  = grad wrt p
  float* dlam;  // (B, 2nz) ; grad wrt h = -dlam
  // optional per-row scale of grad_x (fc energy: grad_x = Ftr, scale = g_e * values_gain * exp(-svd_gain * svd))
  const float* scale_ge;
  const float* scale_svd;
  float svd_gain, values_gain;
};

// The linear solver behind the loop and the backward row.  Lane l owns the NC columns l, l + 64, ...; live[c]: column
// c exists (< nz), lam[c] = ridge + d_u + d_l of that column.
//   factor(lam, live)  factor Q + diag(lam - ridge)
//   solve(rhs, dx)     dx = (Q + diag(lam - ridge))^-1 rhs with the last factor
//   matvec(x, out)     out = Q x
// GqLr (qp_lr.h): Q = A'A + ridge I by the Woodbury identity.  GqDenseLds (qp_dense.hip): dense Q of 65..128 variables
// in LDS.  GqRegChol (qp_core.h, backward row only): dense Q of <= 64 variables in registers.  A dense Q holds its own
// ridge, so its callers set g.ridge = 0.

// qpth get_step ratio -v/dv (blocking only for dv < 0) with the hardware reciprocal; zeros and infinities behave like the
// IEEE division (dv = +-0 -> -+inf, 0/0 -> NaN)
__device__ __forceinline__ float gq_step_ratio_rcp(float v, float dv) {
  const float a = -v * __builtin_amdgcn_rcpf(dv);
  return (dv > 0.0f) ? GQ_INF : a;
}

// qpth solve_kkt on the reduced system (oracle _solve_kkt_box) for the lane's columns; S holds the factor of
// Q + diag(du + dl), idu / idl = 1 / du, 1 / dl
template <int NC, class SOLVER>
__device__ __forceinline__ void gq_lr_kkt(const SOLVER& S, const float (&du)[NC], const float (&dl)[NC],
                                          const float (&idu)[NC], const float (&idl)[NC], const float (&rx)[NC],
                                          const float (&rsu)[NC], const float (&rsl)[NC], const float (&rzu)[NC],
                                          const float (&rzl)[NC], float (&dx)[NC], float (&dsu)[NC], float (&dsl)[NC],
                                          float (&dzu)[NC], float (&dzl)[NC]) {
  float rhs[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float tu = du[c] * rzu[c] - rsu[c], tl = dl[c] * rzl[c] - rsl[c];
    rhs[c] = -rx[c] - (tu - tl);
  }
  S.solve(rhs, dx);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dzu[c] = du[c] * (dx[c] + rzu[c]) - rsu[c];
    dzl[c] = dl[c] * (-dx[c] + rzl[c]) - rsl[c];
    dsu[c] = (-rsu[c] - dzu[c]) * idu[c];  // idu = 1 / du
    dsl[c] = (-rsl[c] - dzl[c]) * idl[c];
  }
}

// All PDIPM iterations of one problem (qpth 0.0.18 semantics, oracle/ref_cpu/qp.py::pdipm_forward_box), recording
// resid / mu of every iteration and a snapshot of every iterate that improves the row's best residual.  S: the solver,
// its matrix loaded by the caller.
// SLOT: the recorded iterates of iterations 0 .. max_iter - 2 also go into g.slot (the fused force-closure head only; the
// generic solvers are compiled without the branch and keep their registers).
template <bool SLOT = false, int NC, class SOLVER>
__device__ __forceinline__ void gq_qp_lr_iterate(const GqQpArgs& g, int row, int lane, SOLVER& S,
                                                 const bool (&live)[NC], const float (&p)[NC], const float (&hu)[NC],
                                                 const float (&hl)[NC], float* hist_resid = nullptr,
                                                 float* hist_mu = nullptr) {
  // hist_*: lane it keeps the residual / mu of iteration it (max_iter <= 64) for the caller's stop-rule epilogue
  float h_r = 0.0f, h_m = 0.0f;
  const int nz = g.nz;
  const float m2 = 2.0f * (float)nz;
  float x[NC], su[NC], sl[NC], zu[NC], zl[NC];
  float lam[NC], ones[NC], zero[NC], nhu[NC], nhl[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    lam[c] = g.ridge + 2.0f;
    ones[c] = 1.0f;
    zero[c] = 0.0f;
    nhu[c] = -hu[c];
    nhl[c] = -hl[c];
  }
  // ---- initial point: solve_kkt(d = 1, rx = p, rs = 0, rz = -h) ----------------------------------------------
  S.factor(lam, live);
  gq_lr_kkt(S, ones, ones, ones, ones, p, zero, zero, nhu, nhl, x, su, sl, zu, zl);
  {
    float ms = GQ_INF, mz = GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (live[c]) {
        ms = gq_nanmin(ms, gq_nanmin(su[c], sl[c]));
        mz = gq_nanmin(mz, gq_nanmin(zu[c], zl[c]));
      }
    }
    ms = gq_dpp_nanmin(ms);
    mz = gq_dpp_nanmin(mz);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (ms < 0.0f) {
        su[c] = su[c] - ms + 1.0f;
        sl[c] = sl[c] - ms + 1.0f;
      }
      if (mz < 0.0f) {
        zu[c] = zu[c] - mz + 1.0f;
        zl[c] = zl[c] - mz + 1.0f;
      }
      if (!live[c]) {
        x[c] = 0.0f;
        su[c] = sl[c] = zu[c] = zl[c] = 1.0f;
      }
    }
  }

  float best = 0.0f;
  for (int it = 0; it < g.max_iter; ++it) {
    float Qx[NC], rx[NC], rzu[NC], rzl[NC];
    S.matvec(x, Qx);
    float a_sz = 0.0f, a_rz = 0.0f, a_rx = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      rx[c] = (zu[c] - zl[c]) + Qx[c] + p[c];
      rzu[c] = x[c] + su[c] - hu[c];
      rzl[c] = -x[c] + sl[c] - hl[c];
      if (live[c]) {
        a_sz += su[c] * zu[c] + sl[c] * zl[c];
        a_rz += rzu[c] * rzu[c] + rzl[c] * rzl[c];
        a_rx += rx[c] * rx[c];
      }
    }
    float red[3] = {a_sz, a_rz, a_rx};
    gq_wave_sums_f<3>(red);
    const float sz = red[0];
    const float mu = fabsf(sz / m2);
    const float resid = sqrtf(red[1]) + sqrtf(red[2]) + m2 * mu;
    const bool record = (it == 0) || (resid < best);  // false for NaN: a NaN iterate never becomes best
    if (record) {
      best = resid;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (live[c]) {
          float* s = g.snap + (((size_t)row * g.max_iter + it) * 5) * nz + lane + GQ_WAVE * c;
          s[0] = x[c];
          s[nz] = zu[c];
          s[2 * nz] = zl[c];
          s[3 * nz] = su[c];
          s[4 * nz] = sl[c];
          if (SLOT && it < g.max_iter - 1) {  // fixed address per row: a reader can ask for it before it knows k*
            // Five adjacent words per column, so that one address serves the five stores, and that address is formed
            // here, every time: left to itself the compiler keeps loop-invariant 64-bit addresses in registers across
            // all iterations (ten VGPRs with a (5, nz) layout, which the fused head does not have).
            unsigned r = (unsigned)row;
            asm volatile("" : "+v"(r));
            float* b = g.slot + (r * (unsigned)nz + (unsigned)(lane + GQ_WAVE * c)) * 5u;  // B * 5 * nz < 2^32
            b[0] = x[c];
            b[1] = zu[c];
            b[2] = zl[c];
            b[3] = su[c];
            b[4] = sl[c];
          }
        }
      }
    }
    if (lane == 0) {
      g.resid[(size_t)row * g.max_iter + it] = resid;
      g.mu[(size_t)row * g.max_iter + it] = mu;
    }
    if (lane == it) {
      h_r = resid;
      h_m = mu;
    }
    if (it == g.max_iter - 1) break;  // qpth returns `best` after the loop; the last update is never used

    // reciprocals of s and z once per iteration (v_rcp_f32, 1 ulp): d = z/s, 1/d = s/z, and the corrector's 1/s
    float du[NC], dl[NC], idu[NC], idl[NC], isu[NC], isl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      isu[c] = __builtin_amdgcn_rcpf(su[c]);
      isl[c] = __builtin_amdgcn_rcpf(sl[c]);
      du[c] = zu[c] * isu[c];
      dl[c] = zl[c] * isl[c];
      idu[c] = su[c] * __builtin_amdgcn_rcpf(zu[c]);
      idl[c] = sl[c] * __builtin_amdgcn_rcpf(zl[c]);
      lam[c] = g.ridge + du[c] + dl[c];
    }
    S.factor(lam, live);
    // affine scaling direction
    float dxa[NC], dsua[NC], dsla[NC], dzua[NC], dzla[NC];
    gq_lr_kkt(S, du, dl, idu, idl, rx, zu, zl, rzu, rzl, dxa, dsua, dsla, dzua, dzla);
    float st = GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (live[c])
        st = gq_nanmin(st, gq_nanmin(gq_nanmin(gq_step_ratio_rcp(zu[c], dzua[c]), gq_step_ratio_rcp(zl[c], dzla[c])),
                                     gq_nanmin(gq_step_ratio_rcp(su[c], dsua[c]), gq_step_ratio_rcp(sl[c], dsla[c]))));
    float alpha = gq_nanmin(gq_dpp_nanmin(st), 1.0f);
    float a_t3 = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (live[c])
        a_t3 += (su[c] + alpha * dsua[c]) * (zu[c] + alpha * dzua[c]) + (sl[c] + alpha * dsla[c]) * (zl[c] + alpha * dzla[c]);
    float sig = gq_dpp_sum(a_t3) / sz;
    sig = sig * sig * sig;
    // centering-corrector direction: rx = 0, rs = (-mu*sig + ds_aff*dz_aff)/s, rz = 0
    float rs2u[NC], rs2l[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      rs2u[c] = (-mu * sig + dsua[c] * dzua[c]) * isu[c];
      rs2l[c] = (-mu * sig + dsla[c] * dzla[c]) * isl[c];
    }
    float dxc[NC], dsuc[NC], dslc[NC], dzuc[NC], dzlc[NC];
    gq_lr_kkt(S, du, dl, idu, idl, zero, rs2u, rs2l, zero, zero, dxc, dsuc, dslc, dzuc, dzlc);
    st = GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      dxa[c] += dxc[c];
      dsua[c] += dsuc[c];
      dsla[c] += dslc[c];
      dzua[c] += dzuc[c];
      dzla[c] += dzlc[c];
      if (live[c])
        st = gq_nanmin(st, gq_nanmin(gq_nanmin(gq_step_ratio_rcp(zu[c], dzua[c]), gq_step_ratio_rcp(zl[c], dzla[c])),
                                     gq_nanmin(gq_step_ratio_rcp(su[c], dsua[c]), gq_step_ratio_rcp(sl[c], dsla[c]))));
    }
    alpha = gq_nanmin(0.999f * gq_dpp_nanmin(st), 1.0f);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (live[c]) {
        x[c] += alpha * dxa[c];
        su[c] += alpha * dsua[c];
        sl[c] += alpha * dsla[c];
        zu[c] += alpha * dzua[c];
        zl[c] += alpha * dzla[c];
      }
    }
  }
  if (hist_resid) *hist_resid = h_r;
  if (hist_mu) *hist_mu = h_m;
}

// Backward of one row (qpth QPFunction.backward): dx = -(Q + diag(d_u + d_l))^-1 (scale * grad_x), dlam = d * (G dx).
// S: the solver, its matrix loaded by the caller.
template <int NC, class SOLVER>
__device__ __forceinline__ void gq_qp_bwd_row(const GqQpBwdArgs& g, SOLVER& S, int row, int lane) {
  const int nz = g.nz;
  const float gscale = g.scale_ge ? g.scale_ge[row] * g.values_gain * expf(-g.svd_gain * g.scale_svd[row]) : 1.0f;
  bool live[NC];
  float du[NC], dl[NC], lam[NC], rhs[NC], dx[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int k = lane + GQ_WAVE * c;
    live[c] = k < nz;
    du[c] = dl[c] = 1.0f;
    rhs[c] = 0.0f;
    if (live[c]) {
      const float* lm = g.lam + (size_t)row * 2 * nz;
      const float* sk = g.slack + (size_t)row * 2 * nz;
      du[c] = fmaxf(lm[k], 1e-8f) / fmaxf(sk[k], 1e-8f);
      dl[c] = fmaxf(lm[nz + k], 1e-8f) / fmaxf(sk[nz + k], 1e-8f);
      rhs[c] = -gscale * g.grad_x[(size_t)row * nz + k];
    }
    lam[c] = g.ridge + du[c] + dl[c];
  }
  S.factor(lam, live);
  S.solve(rhs, dx);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (live[c]) {
      const int k = lane + GQ_WAVE * c;
      g.dx[(size_t)row * nz + k] = dx[c];
      g.dlam[(size_t)row * 2 * nz + k] = du[c] * dx[c];
      g.dlam[(size_t)row * 2 * nz + nz + k] = -dl[c] * dx[c];
    }
  }
}

// ---- dense Q, nz <= 64: the matrix row of each lane in registers (GqRegChol) ---------------------------------------
// The forward keeps its own loop in IEEE-division arithmetic.  On the shared loop's arithmetic (v_rcp_f32) one row of
// tests/test_gpu_qp_variants.py::test_dense_fixed_iterations[17-64] gets an affine slack step of exactly 0 in fp32 at
// iteration 4: qpth's get_step turns it into a -inf step and the iterate into NaN, which the fp64 oracle never sees.
template <int NZ>
__global__ __launch_bounds__(GQ_WAVE) void gq_qp_iter_kernel(GqQpArgs g) {
  const int row = blockIdx.x;
  const int lane = gq_lane();
  const int nz = g.nz;
  const bool live = lane < nz;
  float q[NZ];
#pragma unroll
  for (int k = 0; k < NZ; ++k) {
    const bool ok = live && (k < nz);
    q[k] = ok ? g.Q[((size_t)row * nz + lane) * nz + k] : ((lane == k) ? 1.0f : 0.0f);
  }
  float p = 0.0f;
  if (g.p != nullptr && live) p = g.p[(size_t)row * nz + lane];
  const float up = live ? (g.upper ? g.upper[(size_t)row * nz + lane] : g.upper_s) : 1.0f;
  const float lo = live ? (g.lower ? g.lower[(size_t)row * nz + lane] : g.lower_s) : -1.0f;
  const float hu = up, hl = -lo;
  const float m2 = 2.0f * (float)nz;

  float a[NZ];
  float dinv = 1.0f;
  // ---- initial point: solve_kkt(d = 1, rx = p, rs = 0, rz = -h) --------------------------------------
  GqChol<NZ>::form(a, q, 2.0f, lane);
  GqChol<NZ>::factor(a, dinv, lane);
  float x, su, sl, zu, zl;
  gq_kkt_solve<NZ>(a, dinv, lane, 1.0f, 1.0f, p, 0.0f, 0.0f, -hu, -hl, x, su, sl, zu, zl);
  {
    float ms = gq_dpp_nanmin(live ? gq_nanmin(su, sl) : GQ_INF);
    if (ms < 0.0f) {
      su = su - ms + 1.0f;
      sl = sl - ms + 1.0f;
    }
    float mz = gq_dpp_nanmin(live ? gq_nanmin(zu, zl) : GQ_INF);
    if (mz < 0.0f) {
      zu = zu - mz + 1.0f;
      zl = zl - mz + 1.0f;
    }
  }
  if (!live) {
    x = 0.0f;
    su = sl = zu = zl = 1.0f;
  }

  float best = 0.0f;
  for (int it = 0; it < g.max_iter; ++it) {
    const float Qx = GqChol<NZ>::matvec(q, x);
    const float rx = (zu - zl) + Qx + p;
    const float rzu = x + su - hu;
    const float rzl = -x + sl - hl;
    const float sz = gq_dpp_sum(live ? (su * zu + sl * zl) : 0.0f);
    const float mu = fabsf(sz / m2);
    const float nrz = sqrtf(gq_dpp_sum(live ? (rzu * rzu + rzl * rzl) : 0.0f));
    const float nrx = sqrtf(gq_dpp_sum(live ? rx * rx : 0.0f));
    const float resid = nrz + nrx + m2 * mu;
    const bool record = (it == 0) || (resid < best);  // false for NaN: a NaN iterate never becomes best
    if (record) {
      best = resid;
      if (live) {
        float* s = g.snap + (((size_t)row * g.max_iter + it) * 5) * nz + lane;
        s[0] = x;
        s[nz] = zu;
        s[2 * nz] = zl;
        s[3 * nz] = su;
        s[4 * nz] = sl;
      }
    }
    if (lane == 0) {
      g.resid[(size_t)row * g.max_iter + it] = resid;
      g.mu[(size_t)row * g.max_iter + it] = mu;
    }
    if (it == g.max_iter - 1) break;  // qpth returns `best` after the loop; the last update is never used

    const float du = zu / su, dl = zl / sl;
    GqChol<NZ>::form(a, q, live ? (du + dl) : 2.0f, lane);
    GqChol<NZ>::factor(a, dinv, lane);
    // affine scaling direction
    float dxa, dsua, dsla, dzua, dzla;
    gq_kkt_solve<NZ>(a, dinv, lane, du, dl, rx, zu, zl, rzu, rzl, dxa, dsua, dsla, dzua, dzla);
    float st = gq_nanmin(gq_nanmin(gq_step_ratio(zu, dzua), gq_step_ratio(zl, dzla)),
                         gq_nanmin(gq_step_ratio(su, dsua), gq_step_ratio(sl, dsla)));
    float alpha = gq_nanmin(gq_dpp_nanmin(live ? st : GQ_INF), 1.0f);
    const float t3 = gq_dpp_sum(
        live ? ((su + alpha * dsua) * (zu + alpha * dzua) + (sl + alpha * dsla) * (zl + alpha * dzla)) : 0.0f);
    float sig = t3 / sz;
    sig = sig * sig * sig;
    // centering-corrector direction: rx = 0, rs = (-mu*sig + ds_aff*dz_aff)/s, rz = 0
    const float rs2u = (-mu * sig + dsua * dzua) / su;
    const float rs2l = (-mu * sig + dsla * dzla) / sl;
    float dxc, dsuc, dslc, dzuc, dzlc;
    gq_kkt_solve<NZ>(a, dinv, lane, du, dl, 0.0f, rs2u, rs2l, 0.0f, 0.0f, dxc, dsuc, dslc, dzuc, dzlc);
    const float dx = dxa + dxc, dsu = dsua + dsuc, dsl = dsla + dslc, dzu = dzua + dzuc, dzl = dzla + dzlc;
    st = gq_nanmin(gq_nanmin(gq_step_ratio(zu, dzu), gq_step_ratio(zl, dzl)),
                   gq_nanmin(gq_step_ratio(su, dsu), gq_step_ratio(sl, dsl)));
    alpha = gq_nanmin(0.999f * gq_dpp_nanmin(live ? st : GQ_INF), 1.0f);
    if (live) {
      x += alpha * dx;
      su += alpha * dsu;
      sl += alpha * dsl;
      zu += alpha * dzu;
      zl += alpha * dzl;
    }
  }
}

template <int NZ>
__global__ __launch_bounds__(GQ_WAVE) void gq_qp_bwd_kernel(GqQpBwdArgs g) {
  const int row = blockIdx.x, lane = gq_lane();
  GqRegChol<NZ> S;
  S.load(g.Q, row, g.nz, lane);
  g.ridge = 0.0f;
  gq_qp_bwd_row<1>(g, S, row, lane);
}

// launchers of the register kernels, explicitly instantiated in qp_nz16/32/48/64.hip
template <int NZ>
struct GqQpRegLaunch {
  static int iter(const GqQpArgs& a, hipStream_t st);
  static int bwd(const GqQpBwdArgs& a, hipStream_t st);
};
template <int NZ>
int GqQpRegLaunch<NZ>::iter(const GqQpArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(gq_qp_iter_kernel<NZ>, dim3(a.B), dim3(GQ_WAVE), 0, st, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
template <int NZ>
int GqQpRegLaunch<NZ>::bwd(const GqQpBwdArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(gq_qp_bwd_kernel<NZ>, dim3(a.B), dim3(GQ_WAVE), 0, st, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
extern template struct GqQpRegLaunch<16>;
extern template struct GqQpRegLaunch<32>;
extern template struct GqQpRegLaunch<48>;
extern template struct GqQpRegLaunch<64>;

int gq_qp_lr_launch_iter(const GqQpArgs& a, hipStream_t st);  // qp_lr.hip
int gq_qp_lr_launch_bwd(const GqQpBwdArgs& a, hipStream_t st);
