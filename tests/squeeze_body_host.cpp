// The device bodies of the squeeze term (graspqp_amd/csrc/squeeze_dev.h) compiled for the HOST, and one row of gq_squeeze_kernel
// (csrc/squeeze.hip) walked through them serially in the kernel's order: the columns and the normal equations contact by contact,
// the left-looking Cholesky column by column, the two substitutions step by step, then residuals, energy, g_R, the contact-point
// gradient and the Hessian walk contact by contact, the six wave sums in the shape of wave.h's gq_wave_sums_f.
// tests/test_squeeze_body_host.py builds this program with the host compiler and sanitizers and compares its results with the fp64
// oracle.  Every buffer is exactly sized, so an index outside one ends the program.  Uncoupled hands (JA = J).  No GPU involved.
// usage: squeeze_body_host in.bin out.bin
//   in.bin : int32 n J, float32 R[9] tau lambda c (= w up), int32 parent[J] type[J], float32 a[J][3] p[J][3] (joint axes and
//            origins, hand frame), int32 start[n] (the node each contact's link rides on), float32 T[n][12] (that link's transform)
//            cpos[n][3] (candidate, link frame) dist_sq[n] normal[n][3] closest[n][3] pw[n][3] (contact point, world)
//   out.bin: float32 E, theta[J], g_theta[J], g_R[9], g_p[n][3]
#include "host_shim.h"
#include "../graspqp_amd/csrc/squeeze_dev.h"

static const int LANES = 64;

// gq_wave_sums_f of wave.h for one value: halves folded (l + l+32), row pairs folded (+16), then xor 1, xor 2, half mirror, mirror
// inside the row; every stage adds a pair symmetrically, so all lanes end with the same bits.
static float wave_sum(const float* x) {
  float s[32], t[16], u[16];
  for (int i = 0; i < 32; ++i) s[i] = x[i] + x[i + 32];
  for (int i = 0; i < 16; ++i) t[i] = s[i] + s[i + 16];
  for (int i = 0; i < 16; ++i) u[i] = t[i] + t[i ^ 1];
  for (int i = 0; i < 16; ++i) t[i] = u[i] + u[i ^ 2];
  for (int i = 0; i < 16; ++i) u[i] = t[i] + t[(i & 8) | (7 - (i & 7))];
  return u[0] + u[15];
}

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[2];
  float c12[12];
  if (fread(hd, 4, 2, f) != 2 || fread(c12, 4, 12, f) != 12) return 4;
  const int n = hd[0], J = hd[1], JA = J;
  if (n < 1 || n > GQ_SQ_MAX || J < 1 || J > GQ_SQ_MAX) return 4;
  const float* R = c12;
  const float tau = c12[9], lambda = c12[10], cw = c12[11];
  std::vector<int> parent(J), type(J), start(n);
  std::vector<float> a3((size_t)J * 3), p3((size_t)J * 3), T((size_t)n * 12), cpos((size_t)n * 3), d2(n), nrm((size_t)n * 3),
      closest((size_t)n * 3), pw((size_t)n * 3);
  if (!rd(f, parent) || !rd(f, type) || !rd(f, a3) || !rd(f, p3) || !rd(f, start) || !rd(f, T) || !rd(f, cpos) || !rd(f, d2) ||
      !rd(f, nrm) || !rd(f, closest) || !rd(f, pw))
    return 5;
  fclose(f);
  const int LD = gq_squeeze_ld(JA);
  std::vector<double> A((size_t)JA * LD, 0.0), b(JA, 0.0);
  std::vector<float> sx((size_t)n * 3), sdh((size_t)n * 3);
  std::vector<unsigned long long> mask(n);
  auto v3 = [](const std::vector<float>& v, int i) { return gq_mk(v[(size_t)i * 3], v[(size_t)i * 3 + 1], v[(size_t)i * 3 + 2]); };

  // 1. columns, motions, normal equations
  for (int c = 0; c < n; ++c) {
    const float* t = T.data() + (size_t)c * 12;
    const gq3 cp = v3(cpos, c);
    const gq3 x = gq_mk(t[0] * cp.x + t[1] * cp.y + t[2] * cp.z + t[3], t[4] * cp.x + t[5] * cp.y + t[6] * cp.z + t[7],
                        t[8] * cp.x + t[9] * cp.y + t[10] * cp.z + t[11]);
    unsigned long long m = 0;
    for (int nd = start[c]; nd >= 0; nd = parent[nd]) m |= 1ull << nd;
    mask[c] = m;
    float s;
    bool free_travel;
    const gq3 d = gq_squeeze_dir(d2[c], v3(nrm, c), tau, s, free_travel);
    const gq3 dh = gq_squeeze_to_hand(R, d);
    sx[(size_t)c * 3] = x.x, sx[(size_t)c * 3 + 1] = x.y, sx[(size_t)c * 3 + 2] = x.z;
    sdh[(size_t)c * 3] = dh.x, sdh[(size_t)c * 3 + 1] = dh.y, sdh[(size_t)c * 3 + 2] = dh.z;
    std::vector<gq3> col(JA);
    for (int lane = 0; lane < JA; ++lane)
      col[lane] = gq_squeeze_col(type[lane], (m >> lane) & 1ull, v3(a3, lane), v3(p3, lane), x);
    for (int lane = 0; lane < JA; ++lane) b[lane] += gq_squeeze_gram(col[lane], dh);
    for (int lane = 0; lane < JA; ++lane)
      for (int i = lane; i < JA; ++i) A[(size_t)i * LD + lane] += gq_squeeze_gram(col[i], col[lane]);
  }
  for (int lane = 0; lane < JA; ++lane) A[(size_t)lane * LD + lane] += (double)lambda;

  // 2. Cholesky and the solves
  for (int k = 0; k < JA; ++k) {
    std::vector<double> s(JA, 1.0);
    for (int lane = k; lane < JA; ++lane) s[lane] = gq_squeeze_chol_dot(A.data(), LD, lane, k);
    const double dkk = sqrt(s[k]);
    A[(size_t)k * LD + k] = dkk;
    for (int lane = k + 1; lane < JA; ++lane) A[(size_t)lane * LD + k] = s[lane] / dkk;
  }
  std::vector<double> dinv(JA);
  for (int lane = 0; lane < JA; ++lane) dinv[lane] = 1.0 / A[(size_t)lane * LD + lane];
  auto solve = [&](std::vector<double> v) {
    for (int k = 0; k < JA; ++k) {
      const double yk = v[k] * dinv[k];
      v[k] = yk;
      for (int lane = k + 1; lane < JA; ++lane) v[lane] = gq_squeeze_sub(v[lane], A[(size_t)lane * LD + k], yk);
    }
    for (int k = JA - 1; k >= 0; --k) {
      const double xk = v[k] * dinv[k];
      v[k] = xk;
      for (int lane = 0; lane < k; ++lane) v[lane] = gq_squeeze_sub(v[lane], A[(size_t)k * LD + lane], xk);
    }
    return v;
  };
  const std::vector<double> th = solve(b), mm = solve(th);
  const float c_up = cw / (float)(3 * n);
  std::vector<float> thf(JA), uf(JA);
  for (int lane = 0; lane < JA; ++lane) {
    thf[lane] = (float)th[lane];
    uf[lane] = (float)(-2.0 * (double)c_up * (double)lambda * mm[lane]);
  }

  // 3. residuals, energy, gradients
  float e = 0.0f, gR[9] = {0};
  std::vector<float> acc(J, 0.0f), gp((size_t)n * 3);
  for (int c = 0; c < n; ++c) {
    const gq3 x = v3(sx, c), dh = v3(sdh, c);
    float lanes[6][LANES] = {{0}};
    for (int lane = 0; lane < JA; ++lane) {
      const gq3 col = gq_squeeze_col(type[lane], (mask[c] >> lane) & 1ull, v3(a3, lane), v3(p3, lane), x);
      lanes[0][lane] = col.x * thf[lane], lanes[1][lane] = col.y * thf[lane], lanes[2][lane] = col.z * thf[lane];
      lanes[3][lane] = col.x * uf[lane], lanes[4][lane] = col.y * uf[lane], lanes[5][lane] = col.z * uf[lane];
    }
    float sums[6];
    for (int q = 0; q < 6; ++q) sums[q] = wave_sum(lanes[q]);
    const gq3 r = gq_squeeze_resid(gq_mk(sums[0], sums[1], sums[2]), dh);
    e = fmaf(r.x, r.x, fmaf(r.y, r.y, fmaf(r.z, r.z, e)));
    const float c2 = 2.0f * c_up;
    const gq3 v = gq_mk(fmaf(c2, r.x, -sums[3]), fmaf(c2, r.y, -sums[4]), fmaf(c2, r.z, -sums[5]));
    float s;
    bool free_travel;
    const gq3 d = gq_squeeze_dir(d2[c], v3(nrm, c), tau, s, free_travel);
    gR[0] = fmaf(d.x, -v.x, gR[0]), gR[1] = fmaf(d.x, -v.y, gR[1]), gR[2] = fmaf(d.x, -v.z, gR[2]);
    gR[3] = fmaf(d.y, -v.x, gR[3]), gR[4] = fmaf(d.y, -v.y, gR[4]), gR[5] = fmaf(d.y, -v.z, gR[5]);
    gR[6] = fmaf(d.z, -v.x, gR[6]), gR[7] = fmaf(d.z, -v.y, gR[7]), gR[8] = fmaf(d.z, -v.z, gR[8]);
    const gq3 g = gq_squeeze_gp(R, v3(nrm, c), v, free_travel, d2[c], v3(pw, c), v3(closest, c));
    gp[(size_t)c * 3] = g.x, gp[(size_t)c * 3 + 1] = g.y, gp[(size_t)c * 3 + 2] = g.z;
    for (int lane = 0; lane < J; ++lane)
      if ((mask[c] >> lane) & 1ull)
        acc[lane] += gq_squeeze_hess(lane, start[c], parent.data(), type.data(), a3.data(), p3.data(), x, v, r, thf.data(), uf.data());
  }
  const float E = e / (float)(3 * n);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&E, 4, 1, o);
  fwrite(thf.data(), 4, JA, o);
  fwrite(acc.data(), 4, J, o);
  fwrite(gR, 4, 9, o);
  fwrite(gp.data(), 4, gp.size(), o);
  fclose(o);
  return 0;
}
