// Device bodies of the payload-holding term (include/graspqp_hip.h, "payload holding"): what gq_hold_kernel (hold.hip) does per
// column, per load and per (contact, joint), as plain functions of their operands.  tests/hold_body_host.cpp compiles the first
// part for the host and walks one row through it serially.  The second part (device only) is the inward cone column -- fc_dev.h's
// gq_cone_column itself, called with the negated normal -- and the row-local PDIPM loop: gq_qp_lr_iterate of qp_kernels.h
// statement for statement in fp64, with the record of an improving iterate kept in registers (x alone is needed afterwards)
// where the shared body writes its snapshot, residual and mu tables.  The shared body keeps its own text, so every kernel built
// from it keeps its code object.
#pragma once
#include "squeeze_dev.h"

#define GQ_HOLD_MAX_NZ 128  // columns of a row (contacts x cone edges)
#define GQ_HOLD_MAX_L 8     // loads of a launch

// A finger pushes: the cone of contact c opens along the INWARD object normal
__device__ __forceinline__ gq3 gq_hold_inward(gq3 n) { return gq_mk(-n.x, -n.y, -n.z); }

// w_l: the load (force in N, torque in N m) with its torque rows in the units of F's torque rows
__device__ __forceinline__ void gq_hold_load(const float* load, float tw, float (&w)[6]) {
  w[0] = load[0]; w[1] = load[1]; w[2] = load[2];
  w[3] = tw * load[3]; w[4] = tw * load[4]; w[5] = tw * load[5];
}

// p_i = (F' w)_i of column a = F[:, i], in fp64 on the fp32 operands (the loop runs in fp64)
__device__ __forceinline__ double gq_hold_p(const float (&a)[6], const float (&w)[6]) {
  double s = 0.0;
  for (int r = 0; r < 6; ++r) s = fma((double)a[r], (double)w[r], s);
  return s;
}

// An iterate evaluated from its seven wave sums (rows of F x, then sum x^2): r = F x + w, V = |r|^2 + ridge |x|^2,
// resid = |r| / |w| (without the ridge part), e = V / |w|^2, and c2 = 2 / (L |w|^2), the factor of dE/dF = c2 r x'
struct GqHoldEval {
  float r[6];
  float V, resid, e, c2;
};
__device__ __forceinline__ GqHoldEval gq_hold_eval(const float (&sums)[7], const float (&w)[6], float ridge, int L) {
  GqHoldEval o;
  float rr = 0.0f, ww = 0.0f;
  for (int i = 0; i < 6; ++i) {
    o.r[i] = sums[i] + w[i];
    rr = fmaf(o.r[i], o.r[i], rr);
    ww = fmaf(w[i], w[i], ww);
  }
  o.V = fmaf(ridge, sums[6], rr);
  o.resid = sqrtf(rr / ww);
  o.e = o.V / ww;
  o.c2 = 2.0f / ((float)L * ww);
  return o;
}

// column i's share of its contact's force on the object: x_i f_i (world frame, newtons)
__device__ __forceinline__ gq3 gq_hold_force(const float (&a)[6], float x) { return gq_mk(x * a[0], x * a[1], x * a[2]); }

// column i's share of dE/dp_c: the torque rows tw (p_c - cog) x f_i carry g_tau = c2 r[3..5] x_i, and d/dp = tw f_i x g_tau
__device__ __forceinline__ gq3 gq_hold_gp(const float (&a)[6], float x, const float (&r)[6], float c2, float tw) {
  const float k = c2 * x;
  const gq3 gt = gq_mk(k * r[3], k * r[4], k * r[5]);
  const gq3 v = gq_sq_cross(gq_mk(a[0], a[1], a[2]), gt);
  return gq_mk(tw * v.x, tw * v.y, tw * v.z);
}

// Contact c's share of the torque of TREE joint j: (column of the linear contact Jacobian, squeeze_dev.h) . f_h, f_h = R' force
__device__ __forceinline__ float gq_hold_torque(int type, bool on_path, gq3 a, gq3 p, gq3 x, gq3 fh) {
  return gq_sq_dot(gq_squeeze_col(type, on_path, a, p, x), fh);
}

// tau_act[a] = sum_j C[j][a] tau_tree[j] (J_act = J_tree C), ascending j
__device__ __forceinline__ float gq_hold_fold(const float* coup, int J, int JA, int a, const float* tau_tree) {
  float s = 0.0f;
  for (int j = 0; j < J; ++j) s = fmaf(coup[j * JA + a], tau_tree[j], s);
  return s;
}

#ifndef GQ_SCENE_HOST_BUILD
#include "fc_dev.h"
#include "qp_lr.h"

// Column i = (contact i / k, edge i % k) of F: gq_cone_column on the inward normals nin (see gq_hold_inward)
__device__ __forceinline__ void gq_hold_column(const float* cp, const float* nin, const float* cog, int i, int k, float mu,
                                               float tw, float (&a)[6]) {
  const GqCone cone = gq_cone_column(cp, nin, cog, i / k, i % k, k, mu, tw);
  a[0] = cone.f.x; a[1] = cone.f.y; a[2] = cone.f.z;
  a[3] = cone.tau.x; a[4] = cone.tau.y; a[5] = cone.tau.z;
}

// The solver and the loop below restate GqLr<6,NC> (qp_lr.h) and gq_qp_lr_iterate (qp_kernels.h) statement for statement with the
// iterates, the residuals and the step rules in fp64 (the columns of F stay the fp32 columns of the E_fc step).  Where a load is
// carried, x is fixed along the internal-force directions by the ridge alone (1e-4 against residuals that fp32 resolves to ~1e-6):
// fp32 iterates leave the contact forces 1e-3 off and the loop's pick among its last iterates to the last bits.  In fp64 the loop
// follows the fp64 reference, and its 16 iterations are worth what DESIGN 30 says of them.
__device__ __forceinline__ double gq_hold_nanmin(double a, double b) {
  const double m = fmin(a, b);
  return __builtin_isunordered(a, b) ? __builtin_nan("") : m;
}
__device__ __forceinline__ double gq_hold_wave_nanmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = gq_hold_nanmin(v, __shfl_xor(v, o, GQ_WAVE));
  return v;
}
// qpth get_step ratio -v/dv, blocking only for dv < 0
__device__ __forceinline__ double gq_hold_step_ratio(double v, double dv) { return (dv > 0.0) ? (double)GQ_INF : -v / dv; }

template <int NC>
struct GqHoldLr {
  float a[NC][6];  // my columns of F
  double il[NC];   // 1 / Lam of my columns (0 for dead columns)
  double L[21];    // Cholesky factor of I + F Lam^-1 F'
  double ridge;

  __device__ __forceinline__ void factor(const double (&lam)[NC], const bool (&live)[NC]) {
    double part[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) part[i] = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      il[c] = live[c] ? 1.0 / lam[c] : 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double ai = (double)a[c][i] * il[c];
#pragma unroll
        for (int j = 0; j <= i; ++j) part[i * (i + 1) / 2 + j] += ai * (double)a[c][j];
      }
    }
    gq_wave_sums_d<21>(part);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[i * (i + 1) / 2 + j] = part[i * (i + 1) / 2 + j] + (i == j ? 1.0 : 0.0);
    GqSmall<6>::factor(L);
  }
  // dx = (Lam + F'F)^-1 rhs
  __device__ __forceinline__ void solve(const double (&rhs)[NC], double (&dx)[NC]) const {
    double v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) s += (double)a[c][i] * (rhs[c] * il[c]);
      v[i] = s;
    }
    gq_wave_sums_d<6>(v);
    GqSmall<6>::solve(L, v);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double num = rhs[c];
#pragma unroll
      for (int i = 0; i < 6; ++i) num -= (double)a[c][i] * v[i];
      dx[c] = num * il[c];
    }
  }
  // Q x = F'(F x) + ridge x
  __device__ __forceinline__ void matvec(const double (&x)[NC], double (&out)[NC]) const {
    double ax[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) s = fma((double)a[c][i], x[c], s);
      ax[i] = s;
    }
    gq_wave_sums_d<6>(ax);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double s = ridge * x[c];
#pragma unroll
      for (int i = 0; i < 6; ++i) s = fma((double)a[c][i], ax[i], s);
      out[c] = s;
    }
  }
};

// qpth solve_kkt on the reduced system (gq_lr_kkt of qp_kernels.h in fp64)
template <int NC>
__device__ __forceinline__ void gq_hold_kkt(const GqHoldLr<NC>& S, const double (&du)[NC], const double (&dl)[NC],
                                            const double (&rx)[NC], const double (&rsu)[NC], const double (&rsl)[NC],
                                            const double (&rzu)[NC], const double (&rzl)[NC], double (&dx)[NC], double (&dsu)[NC],
                                            double (&dsl)[NC], double (&dzu)[NC], double (&dzl)[NC]) {
  double rhs[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double tu = du[c] * rzu[c] - rsu[c], tl = dl[c] * rzl[c] - rsl[c];
    rhs[c] = -rx[c] - (tu - tl);
  }
  S.solve(rhs, dx);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dzu[c] = du[c] * (dx[c] + rzu[c]) - rsu[c];
    dzl[c] = dl[c] * (-dx[c] + rzl[c]) - rsl[c];
    dsu[c] = (-rsu[c] - dzu[c]) / du[c];
    dsl[c] = (-rsl[c] - dzl[c]) / dl[c];
  }
}

// All PDIPM iterations of one problem, exactly `max_iter` of them, row-local: xb is the iterate with the problem's own smallest
// residual (the first strict minimum; a NaN never becomes best).  No stop rule, nothing read or written outside the wavefront.
template <int NC>
__device__ __forceinline__ void gq_hold_iterate(int nz, int max_iter, GqHoldLr<NC>& S, const bool (&live)[NC], const double (&p)[NC],
                                                const double (&hu)[NC], const double (&hl)[NC], double (&xb)[NC]) {
  const double m2 = 2.0 * (double)nz;
  double x[NC], su[NC], sl[NC], zu[NC], zl[NC];
  {
    double lam[NC], ones[NC], zero[NC], nhu[NC], nhl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      lam[c] = S.ridge + 2.0;
      ones[c] = 1.0;
      zero[c] = 0.0;
      nhu[c] = -hu[c];
      nhl[c] = -hl[c];
    }
    // ---- initial point: solve_kkt(d = 1, rx = p, rs = 0, rz = -h) ----------------------------------------------
    S.factor(lam, live);
    gq_hold_kkt(S, ones, ones, p, zero, zero, nhu, nhl, x, su, sl, zu, zl);
  }
  {
    double ms = (double)GQ_INF, mz = (double)GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (live[c]) {
        ms = gq_hold_nanmin(ms, gq_hold_nanmin(su[c], sl[c]));
        mz = gq_hold_nanmin(mz, gq_hold_nanmin(zu[c], zl[c]));
      }
    }
    ms = gq_hold_wave_nanmin(ms);
    mz = gq_hold_wave_nanmin(mz);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (ms < 0.0) {
        su[c] = su[c] - ms + 1.0;
        sl[c] = sl[c] - ms + 1.0;
      }
      if (mz < 0.0) {
        zu[c] = zu[c] - mz + 1.0;
        zl[c] = zl[c] - mz + 1.0;
      }
      if (!live[c]) {
        x[c] = 0.0;
        su[c] = sl[c] = zu[c] = zl[c] = 1.0;
      }
    }
  }

  double best = 0.0;
  for (int it = 0; it < max_iter; ++it) {
    double rx[NC], rzu[NC], rzl[NC];
    S.matvec(x, rx);
    double red[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      rx[c] = (zu[c] - zl[c]) + rx[c] + p[c];
      rzu[c] = x[c] + su[c] - hu[c];
      rzl[c] = -x[c] + sl[c] - hl[c];
      if (live[c]) {
        red[0] += su[c] * zu[c] + sl[c] * zl[c];
        red[1] += rzu[c] * rzu[c] + rzl[c] * rzl[c];
        red[2] += rx[c] * rx[c];
      }
    }
    gq_wave_sums_d<3>(red);
    const double sz = red[0];
    const double mu = fabs(sz / m2);
    const double resid = sqrt(red[1]) + sqrt(red[2]) + m2 * mu;
    const bool record = (it == 0) || (resid < best);  // false for NaN: a NaN iterate never becomes best
    if (record) {
      best = resid;
#pragma unroll
      for (int c = 0; c < NC; ++c) xb[c] = live[c] ? x[c] : 0.0;
    }
    if (it == max_iter - 1) break;  // the last update is never used

    double du[NC], dl[NC], lam[NC], zero[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      du[c] = zu[c] / su[c];
      dl[c] = zl[c] / sl[c];
      lam[c] = S.ridge + du[c] + dl[c];
      zero[c] = 0.0;
    }
    S.factor(lam, live);
    // affine scaling direction
    double dxa[NC], dsua[NC], dsla[NC], dzua[NC], dzla[NC];
    gq_hold_kkt(S, du, dl, rx, zu, zl, rzu, rzl, dxa, dsua, dsla, dzua, dzla);
    double st = (double)GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (live[c])
        st = gq_hold_nanmin(st, gq_hold_nanmin(gq_hold_nanmin(gq_hold_step_ratio(zu[c], dzua[c]), gq_hold_step_ratio(zl[c], dzla[c])),
                                               gq_hold_nanmin(gq_hold_step_ratio(su[c], dsua[c]), gq_hold_step_ratio(sl[c], dsla[c]))));
    double alpha = gq_hold_nanmin(gq_hold_wave_nanmin(st), 1.0);
    double a_t3 = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (live[c])
        a_t3 += (su[c] + alpha * dsua[c]) * (zu[c] + alpha * dzua[c]) + (sl[c] + alpha * dsla[c]) * (zl[c] + alpha * dzla[c]);
    double sig = gq_dpp_sum_d(a_t3) / sz;
    sig = sig * sig * sig;
    // centering-corrector direction: rx = 0, rs = (-mu*sig + ds_aff*dz_aff)/s, rz = 0
    double rs2u[NC], rs2l[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      rs2u[c] = (-mu * sig + dsua[c] * dzua[c]) / su[c];
      rs2l[c] = (-mu * sig + dsla[c] * dzla[c]) / sl[c];
    }
    double dxc[NC], dsuc[NC], dslc[NC], dzuc[NC], dzlc[NC];
    gq_hold_kkt(S, du, dl, zero, rs2u, rs2l, zero, zero, dxc, dsuc, dslc, dzuc, dzlc);
    st = (double)GQ_INF;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      dxa[c] += dxc[c];
      dsua[c] += dsuc[c];
      dsla[c] += dslc[c];
      dzua[c] += dzuc[c];
      dzla[c] += dzlc[c];
      if (live[c])
        st = gq_hold_nanmin(st, gq_hold_nanmin(gq_hold_nanmin(gq_hold_step_ratio(zu[c], dzua[c]), gq_hold_step_ratio(zl[c], dzla[c])),
                                               gq_hold_nanmin(gq_hold_step_ratio(su[c], dsua[c]), gq_hold_step_ratio(sl[c], dsla[c]))));
    }
    alpha = gq_hold_nanmin(0.999 * gq_hold_wave_nanmin(st), 1.0);
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
}
#endif  // !GQ_SCENE_HOST_BUILD
