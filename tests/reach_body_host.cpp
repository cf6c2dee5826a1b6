// The device bodies of the reach term (graspqp_amd/csrc/reach_dev.h) compiled for the HOST, and one row of gq_reach_kernel
// (csrc/reach.hip) walked through them serially in the kernel's order: every lane group (station x seed) of the row, eight lanes
// each; the inclusive scan of the joint transforms in the kernel's three shift steps, the 21 sums of J J' in the shape of the
// kernel's butterfly (xor 1, xor 2, mirror of the eight lanes), the unrolled 6 x 6 solve, the capped and clamped step; then the
// row's tail (winner per station, mean, gradient in the gRt layout).  tests/test_reach_body_host.py builds this program with the
// host compiler and sanitizers and compares its results with the fp64 oracle.  Every buffer is exactly sized.  No GPU involved.
// usage: reach_body_host in.bin out.bin
//   in.bin : int32 N S K M, float32 D lambda rho c (= w up), axis[3] t[3] R[9] base[12] tool[12], int32 type[8], float32 pre[8][12]
//            jaxis[8][3] lower[8] upper[8] seeds[S][8]      (the padded arrays gq_arm_create uploads)
//   out.bin: float32 E, gRt[12], seed[K+1], Eks[(K+1) S], q[(K+1) N]
#include "host_shim.h"
#include "../graspqp_amd/csrc/reach_dev.h"

static const int G = GQ_REACH_MAX_JOINTS;

static float group_sum(const float* v) {  // quad_perm xor 1, xor 2, row_half_mirror: all eight lanes end with the same bits
  float a[G], b[G];
  for (int j = 0; j < G; ++j) a[j] = v[j] + v[j ^ 1];
  for (int j = 0; j < G; ++j) b[j] = a[j] + a[j ^ 2];
  return b[0] + b[7];
}

struct Arm {
  std::vector<int> type;
  std::vector<float> pre, axis, lower, upper, seeds;
};

// base -> hand root for the group's joints; W[j] = base -> joint j
static GqRT group_fk(const Arm& A, const GqRT& base, const GqRT& tool, const float* q, GqRT* W) {
  GqRT X[G], Y[G];
  for (int j = 0; j < G; ++j) {
    GqRT pre;
    memcpy(pre.m, A.pre.data() + (size_t)j * 12, sizeof(pre.m));
    X[j] = gq_reach_joint(pre, A.type[j], gq_mk(A.axis[j * 3], A.axis[j * 3 + 1], A.axis[j * 3 + 2]), q[j]);
  }
  for (int d = 1; d < G; d *= 2) {
    for (int j = 0; j < G; ++j) Y[j] = j >= d ? gq_reach_mul(X[j - d], X[j]) : X[j];
    for (int j = 0; j < G; ++j) X[j] = Y[j];
  }
  for (int j = 0; j < G; ++j) W[j] = gq_reach_mul(base, X[j]);
  return gq_reach_mul(W[G - 1], tool);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[4];
  float par[4], axis3[3], t3[3], R[9];
  GqRT base, tool;
  if (fread(hd, 4, 4, f) != 4 || fread(par, 4, 4, f) != 4 || fread(axis3, 4, 3, f) != 3 || fread(t3, 4, 3, f) != 3 ||
      fread(R, 4, 9, f) != 9 || fread(base.m, 4, 12, f) != 12 || fread(tool.m, 4, 12, f) != 12)
    return 4;
  const int N = hd[0], S = hd[1], K = hd[2], M = hd[3];
  if (N < 1 || N > G || S < 1 || S > GQ_REACH_MAX_SEEDS || K < 0 || K > GQ_REACH_MAX_STATIONS || M < 0) return 4;
  const float D = par[0], lambda = par[1], rho = par[2], cw = par[3];
  Arm A;
  A.type.resize(G), A.pre.resize((size_t)G * 12), A.axis.resize((size_t)G * 3), A.lower.resize(G), A.upper.resize(G);
  A.seeds.resize((size_t)S * G);
  if (fread(A.type.data(), 4, G, f) != (size_t)G || fread(A.pre.data(), 4, (size_t)G * 12, f) != (size_t)G * 12 ||
      fread(A.axis.data(), 4, (size_t)G * 3, f) != (size_t)G * 3 || fread(A.lower.data(), 4, G, f) != (size_t)G ||
      fread(A.upper.data(), 4, G, f) != (size_t)G || fread(A.seeds.data(), 4, (size_t)S * G, f) != (size_t)S * G)
    return 5;
  fclose(f);
  const gq3 axis = gq_mk(axis3[0], axis3[1], axis3[2]), t = gq_mk(t3[0], t3[1], t3[2]);
  const int P = (K + 1) * S;
  std::vector<float> sE(P), se((size_t)P * 6), sq((size_t)P * G);

  for (int p = 0; p < P; ++p) {  // a lane group
    const int k = p / S, sd = p - k * S;
    const gq3 ps = gq_reach_target(R, t, axis, gq_reach_station(D, k, K));
    std::vector<float> q(A.seeds.begin() + (size_t)sd * G, A.seeds.begin() + (size_t)(sd + 1) * G);
    float e[6];
    for (int it = 0;; ++it) {
      GqRT W[G];
      const GqRT T = group_fk(A, base, tool, q.data(), W);
      gq_reach_err(R, ps, T, rho, e);
      if (it >= M) break;
      float c[G][6], g[G][21], Asum[21], y[6], lanes[G], dq[G], mx = 0.0f;
      for (int j = 0; j < G; ++j) {
        gq_reach_col(A.type[j], W[j], gq_mk(A.axis[j * 3], A.axis[j * 3 + 1], A.axis[j * 3 + 2]), gq_mk(T.m[3], T.m[7], T.m[11]), rho,
                     c[j]);
        gq_reach_gram(c[j], g[j]);
      }
      for (int i = 0; i < 21; ++i) {
        for (int j = 0; j < G; ++j) lanes[j] = g[j][i];
        Asum[i] = group_sum(lanes);
      }
      gq_reach_solve6(Asum, lambda, e, y);
      for (int j = 0; j < G; ++j) {
        dq[j] = gq_reach_dq(c[j], y);
        mx = fmaxf(mx, fabsf(dq[j]));
      }
      for (int j = 0; j < G; ++j) q[j] = gq_reach_step(q[j], dq[j], mx, A.lower[j], A.upper[j]);
    }
    for (int j = 0; j < G; ++j) sq[(size_t)p * G + j] = q[j];
    for (int i = 0; i < 6; ++i) se[(size_t)p * 6 + i] = e[i];
    sE[p] = gq_reach_energy(e);
  }

  // the row's tail
  float esum = 0.0f, gRt[12] = {0}, tau_h[3] = {0};
  const float inv = 1.0f / (float)(K + 1), cu = cw * inv;
  std::vector<float> seed(K + 1), qout((size_t)(K + 1) * N);
  for (int k = 0; k <= K; ++k) {
    const int best = gq_reach_pick(sE.data() + (size_t)k * S, S);
    seed[k] = (float)best;
    esum += sE[(size_t)k * S + best];
    gq_reach_grad_add(R, se.data() + ((size_t)k * S + best) * 6, cu, rho, gq_reach_station(D, k, K), axis, gRt, tau_h);
    for (int j = 0; j < N; ++j) qout[(size_t)k * N + j] = sq[((size_t)k * S + best) * G + j];
  }
  gq_reach_grad_close(tau_h, gRt);
  const float E = esum * inv;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&E, 4, 1, o);
  fwrite(gRt, 4, 12, o);
  fwrite(seed.data(), 4, seed.size(), o);
  fwrite(sE.data(), 4, sE.size(), o);
  fwrite(qout.data(), 4, qout.size(), o);
  fclose(o);
  return 0;
}
