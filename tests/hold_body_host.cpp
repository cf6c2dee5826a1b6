// The per-lane device bodies of the payload-holding term (graspqp_amd/csrc/hold_dev.h) compiled for the HOST, and one row of
// gq_hold_kernel (csrc/hold.hip) walked through them serially in the kernel's order, load by load: the inward normals, w_l and
// p = F' w_l, the evaluation of an iterate from its seven wave sums (the shape of wave.h's gq_wave_sums_f), per column the force
// share and the share of dE/dp folded per contact in edge order, then the torque of every tree joint over the row's contacts and
// its fold with the coupling matrix; last the loads folded in load order.  The cone columns and the iterates x come with the
// input (the column is fc_dev.h's, device only; the wave-level loop is the GPU tests' subject).
// tests/test_hold_body_host.py builds this program with the host compiler and sanitizers and compares its results with fp64.
// Every buffer is exactly sized, so an index outside one ends the program.  No GPU involved.
// usage: hold_body_host in.bin out.bin
//   in.bin : int32 n k L J JA coupled, float32 R[9] tw ridge c_up, float32 normal[n][3] (outward) cols[nz][6] loads[L][6] x[L][nz],
//            int32 parent[J] type[J], float32 a[J][3] p[J][3] (joint axes and origins, hand frame), int32 start[n] (the node each
//            contact's link rides on), float32 xh[n][3] (contact, hand frame), float32 coup[J][JA] if coupled
//   out.bin: float32 nin[n][3], p[L][nz], E, resid[L], V[L], force[L][n][3], torque[L][JA], g[n][3]
#include "host_shim.h"
#include "../graspqp_amd/csrc/hold_dev.h"

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
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[6];
  float c12[12];
  if (fread(hd, 4, 6, f) != 6 || fread(c12, 4, 12, f) != 12) return 4;
  const int n = hd[0], k = hd[1], L = hd[2], J = hd[3], JA = hd[4], coupled = hd[5], nz = n * k;
  if (n < 1 || n > GQ_SQ_MAX || k < 3 || nz > GQ_HOLD_MAX_NZ || L < 1 || L > GQ_HOLD_MAX_L || J < 1 || J > GQ_SQ_MAX || JA < 1 || JA > J)
    return 4;
  const float* R = c12;
  const float tw = c12[9], ridge = c12[10], c_up = c12[11];
  std::vector<float> nrm((size_t)n * 3), cols((size_t)nz * 6), loads((size_t)L * 6), x((size_t)L * nz), a3((size_t)J * 3),
      p3((size_t)J * 3), xh((size_t)n * 3), coup(coupled ? (size_t)J * JA : 0);
  std::vector<int> parent(J), type(J), start(n);
  if (!rd(f, nrm) || !rd(f, cols) || !rd(f, loads) || !rd(f, x) || !rd(f, parent) || !rd(f, type) || !rd(f, a3) || !rd(f, p3) ||
      !rd(f, start) || !rd(f, xh) || !rd(f, coup))
    return 5;
  fclose(f);
  auto v3 = [](const std::vector<float>& v, int i) { return gq_mk(v[(size_t)i * 3], v[(size_t)i * 3 + 1], v[(size_t)i * 3 + 2]); };

  // 0. the row's contacts
  std::vector<float> nin((size_t)n * 3);
  std::vector<unsigned long long> mask(n);
  for (int c = 0; c < n; ++c) {
    const gq3 v = gq_hold_inward(v3(nrm, c));
    nin[(size_t)c * 3] = v.x, nin[(size_t)c * 3 + 1] = v.y, nin[(size_t)c * 3 + 2] = v.z;
    unsigned long long m = 0;
    for (int nd = start[c]; nd >= 0; nd = parent[nd]) m |= 1ull << nd;
    mask[c] = m;
  }
  std::vector<float> pout((size_t)L * nz), resid(L), V(L), e(L), force((size_t)L * n * 3), torque((size_t)L * JA), gp((size_t)L * n * 3),
      g((size_t)n * 3, 0.0f);
  const int NC = nz <= LANES ? 1 : 2;
  for (int l = 0; l < L; ++l) {
    // 1. w_l, p, the iterate evaluated
    float w[6];
    gq_hold_load(loads.data() + (size_t)l * 6, tw, w);
    float lanes[7][LANES] = {{0}};
    for (int lane = 0; lane < LANES; ++lane)
      for (int c = 0; c < NC; ++c) {
        const int i = lane + LANES * c;
        if (i >= nz) continue;
        float a[6];
        for (int r = 0; r < 6; ++r) a[r] = cols[(size_t)i * 6 + r];
        pout[(size_t)l * nz + i] = gq_hold_p(a, w);
        const float xi = x[(size_t)l * nz + i];
        for (int r = 0; r < 6; ++r) lanes[r][lane] = fmaf(a[r], xi, lanes[r][lane]);
        lanes[6][lane] = fmaf(xi, xi, lanes[6][lane]);
      }
    float sums[7];
    for (int q = 0; q < 7; ++q) sums[q] = wave_sum(lanes[q]);
    const GqHoldEval ev = gq_hold_eval(sums, w, ridge, L);
    resid[l] = ev.resid, V[l] = ev.V, e[l] = ev.e;
    // per column, then per contact in edge order
    std::vector<float> col((size_t)nz * 6);
    for (int i = 0; i < nz; ++i) {
      float a[6];
      for (int r = 0; r < 6; ++r) a[r] = cols[(size_t)i * 6 + r];
      const float xi = x[(size_t)l * nz + i];
      const gq3 fo = gq_hold_force(a, xi), gg = gq_hold_gp(a, xi, ev.r, ev.c2 * c_up, tw);
      float* o = col.data() + (size_t)i * 6;
      o[0] = fo.x, o[1] = fo.y, o[2] = fo.z, o[3] = gg.x, o[4] = gg.y, o[5] = gg.z;
    }
    std::vector<float> fh((size_t)n * 3);
    for (int c = 0; c < n; ++c) {
      float a[6] = {0, 0, 0, 0, 0, 0};
      for (int ed = 0; ed < k; ++ed)
        for (int r = 0; r < 6; ++r) a[r] += col[(size_t)(c * k + ed) * 6 + r];
      for (int r = 0; r < 3; ++r) force[((size_t)l * n + c) * 3 + r] = a[r], gp[((size_t)l * n + c) * 3 + r] = a[3 + r];
      const gq3 h = gq_squeeze_to_hand(R, gq_mk(a[0], a[1], a[2]));
      fh[(size_t)c * 3] = h.x, fh[(size_t)c * 3 + 1] = h.y, fh[(size_t)c * 3 + 2] = h.z;
    }
    // 2. joint torques
    std::vector<float> tt(J, 0.0f);
    for (int lane = 0; lane < J; ++lane)
      for (int c = 0; c < n; ++c)
        tt[lane] += gq_hold_torque(type[lane], (mask[c] >> lane) & 1ull, v3(a3, lane), v3(p3, lane), v3(xh, c), v3(fh, c));
    for (int a = 0; a < JA; ++a) torque[(size_t)l * JA + a] = coupled ? gq_hold_fold(coup.data(), J, JA, a, tt.data()) : tt[a];
  }
  // 3. the loads folded in load order
  float E = 0.0f;
  for (int l = 0; l < L; ++l) E += e[l];
  E /= (float)L;
  for (int c = 0; c < n * 3; ++c)
    for (int l = 0; l < L; ++l) g[c] += gp[(size_t)l * n * 3 + c];
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  wr(o, nin), wr(o, pout);
  fwrite(&E, 4, 1, o);
  wr(o, resid), wr(o, V), wr(o, force), wr(o, torque), wr(o, g);
  fclose(o);
  return 0;
}
