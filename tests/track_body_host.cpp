// The device bodies of the approach tracking term (graspqp_amd/csrc/track_dev.h on top of reach_dev.h) compiled for the HOST, and
// the lane groups of gq_track_kernel (csrc/track.hip) walked through them serially in the kernel's order: every row is a group of
// eight lanes; per waypoint, U times the reach term's update (the inclusive scan of the joint transforms in the kernel's three shift
// steps, the 21 sums of J J' in the shape of the kernel's butterfly, the unrolled 6 x 6 solve, the capped and clamped step), one
// more FK for e_i, then the row's running sums (mean, worst waypoint, largest joint move, gradient in the gRt layout) and the
// station copies.  tests/test_track_body_host.py builds this program with the host compiler and sanitizers and compares its
// results with the fp64 oracle.  Every buffer is exactly sized.  No GPU involved.
// usage: track_body_host in.bin out.bin
//   in.bin : int32 B N T U K, float32 D lambda rho, axis[3], int32 type[8], float32 pre[8][12] jaxis[8][3] lower[8] upper[8] tool[12],
//            then per row float32 cw t[3] R[9] base[12] q_start[N]
//   out.bin: per row float32 E, worst, step, gRt[12], q[(T+1) N], station_q[(K+1) N] (K >= 1 only)
#include "host_shim.h"
#include "../graspqp_amd/csrc/track_dev.h"

static const int G = GQ_REACH_MAX_JOINTS;

static float group_sum(const float* v) {  // quad_perm xor 1, xor 2, row_half_mirror: all eight lanes end with the same bits
  float a[G], b[G];
  for (int j = 0; j < G; ++j) a[j] = v[j] + v[j ^ 1];
  for (int j = 0; j < G; ++j) b[j] = a[j] + a[j ^ 2];
  return b[0] + b[7];
}

struct Arm {
  std::vector<int> type;
  std::vector<float> pre, axis, lower, upper;
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
  int hd[5];
  float par[3], axis3[3];
  if (fread(hd, 4, 5, f) != 5 || fread(par, 4, 3, f) != 3 || fread(axis3, 4, 3, f) != 3) return 4;
  const int B = hd[0], N = hd[1], T = hd[2], U = hd[3], K = hd[4];
  if (B < 1 || N < 1 || N > G || T < 1 || T > GQ_TRACK_MAX_WAYPOINTS || U < 1 || U > GQ_TRACK_MAX_UPDATES || K < 0 ||
      K > GQ_REACH_MAX_STATIONS || (K >= 1 && T % K))
    return 4;
  const float D = par[0], lambda = par[1], rho = par[2];
  Arm A;
  GqRT tool;
  A.type.resize(G), A.pre.resize((size_t)G * 12), A.axis.resize((size_t)G * 3), A.lower.resize(G), A.upper.resize(G);
  if (fread(A.type.data(), 4, G, f) != (size_t)G || fread(A.pre.data(), 4, (size_t)G * 12, f) != (size_t)G * 12 ||
      fread(A.axis.data(), 4, (size_t)G * 3, f) != (size_t)G * 3 || fread(A.lower.data(), 4, G, f) != (size_t)G ||
      fread(A.upper.data(), 4, G, f) != (size_t)G || fread(tool.m, 4, 12, f) != 12)
    return 5;
  const gq3 axis = gq_mk(axis3[0], axis3[1], axis3[2]);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;

  for (int b = 0; b < B; ++b) {  // a lane group
    float cw, t3[3], R[9];
    GqRT base;
    std::vector<float> qs(N);
    if (fread(&cw, 4, 1, f) != 1 || fread(t3, 4, 3, f) != 3 || fread(R, 4, 9, f) != 9 || fread(base.m, 4, 12, f) != 12 ||
        fread(qs.data(), 4, N, f) != (size_t)N)
      return 7;
    const gq3 t = gq_mk(t3[0], t3[1], t3[2]);
    const float inv = 1.0f / (float)(T + 1), cu = cw * inv;
    std::vector<float> q(G, 0.0f), qout((size_t)(T + 1) * N), sq(K >= 1 ? (size_t)(K + 1) * N : 0);
    for (int j = 0; j < N; ++j) q[j] = qs[j];
    GqTrackAcc acc;
    gq_track_acc_init(acc);
    for (int i = 0; i <= T; ++i) {
      const float d = gq_track_dist(D, i, T);
      const gq3 ps = gq_reach_target(R, t, axis, d);
      const std::vector<float> q_prev = q;
      float e[6];
      for (int it = 0;; ++it) {
        GqRT W[G];
        const GqRT Tee = group_fk(A, base, tool, q.data(), W);
        gq_reach_err(R, ps, Tee, rho, e);
        if (it >= U) break;
        float c[G][6], g[G][21], Asum[21], y[6], lanes[G], dq[G], mx = 0.0f;
        for (int j = 0; j < G; ++j) {
          gq_reach_col(A.type[j], W[j], gq_mk(A.axis[j * 3], A.axis[j * 3 + 1], A.axis[j * 3 + 2]),
                       gq_mk(Tee.m[3], Tee.m[7], Tee.m[11]), rho, c[j]);
          gq_reach_gram(c[j], g[j]);
        }
        for (int s = 0; s < 21; ++s) {
          for (int j = 0; j < G; ++j) lanes[j] = g[j][s];
          Asum[s] = group_sum(lanes);
        }
        gq_reach_solve6(Asum, lambda, e, y);
        for (int j = 0; j < G; ++j) {
          dq[j] = gq_reach_dq(c[j], y);
          mx = fmaxf(mx, fabsf(dq[j]));
        }
        for (int j = 0; j < G; ++j) q[j] = gq_reach_step(q[j], dq[j], mx, A.lower[j], A.upper[j]);
      }
      float move = 0.0f;
      for (int j = 0; j < G; ++j) move = fmaxf(move, fabsf(q[j] - q_prev[j]));
      gq_track_acc_add(acc, R, e, move, cu, rho, d, axis, true);
      for (int j = 0; j < N; ++j) qout[(size_t)i * N + j] = q[j];
      const int k = gq_track_station(i, T, K);
      if (k >= 0)
        for (int j = 0; j < N; ++j) sq[(size_t)k * N + j] = q[j];
    }
    gq_reach_grad_close(acc.tau_h, acc.gRt);
    const float head[3] = {acc.esum * inv, acc.worst, acc.step};
    fwrite(head, 4, 3, o);
    fwrite(acc.gRt, 4, 12, o);
    fwrite(qout.data(), 4, qout.size(), o);
    fwrite(sq.data(), 4, sq.size(), o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
