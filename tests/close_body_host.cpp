// The decision bodies of finger closing (graspqp_amd/csrc/close_dev.h) compiled for the HOST and walked serially over dumped records
// in the kernel's order: the direction (fold of m, then Delta), the per-link (phi, index) key fold over the samples in ascending
// order, the stop mask and the clamped update.  tests/test_close_body_host.py writes the records and holds the results against the
// fp64 oracle.  Every buffer is exactly sized (std::vector + at()), so an index outside one ends the program under the sanitizers.
//   in : int32 JA, L, Ns, R | step[JA] lo[JA] hi[JA] f32 | masks[JA] u64 | link[Ns] i32 | R x { v[JA] theta[JA] f32, touched u64, phi[Ns] f32 }
//   out: R x { delta[JA] f32, m f32, m_l[L] f32, idx[L] i32, stopped[JA] i32, theta_new[JA] f32 }
#include "host_shim.h"

#include "../graspqp_amd/csrc/close_dev.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) exit(3);
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  const auto hdr = take<int32_t>(in, 4);
  const int JA = hdr.at(0), L = hdr.at(1), Ns = hdr.at(2), R = hdr.at(3);
  const auto step = take<float>(in, JA), lo = take<float>(in, JA), hi = take<float>(in, JA);
  const auto masks = take<uint64_t>(in, JA);
  const auto link = take<int32_t>(in, Ns);
  for (int r = 0; r < R; ++r) {
    const auto v = take<float>(in, JA), theta = take<float>(in, JA);
    const uint64_t touched = take<uint64_t>(in, 1).at(0);
    const auto phi = take<float>(in, Ns);
    // the direction: u, the fold of m over the joints (any order: here descending, the kernel's is a butterfly), Delta
    std::vector<float> u(JA), delta(JA), tnew(JA), ml(L, GQ_INF_F);
    std::vector<int32_t> idx(L, GQ_CLOSE_NONE), stopped(JA);
    float m = 0.0f;
    for (int a = JA - 1; a >= 0; --a) {
      u.at(a) = gq_close_units(v.at(a), step.at(a));
      m = gq_close_umax(m, u.at(a));
    }
    for (int a = 0; a < JA; ++a) delta.at(a) = gq_close_delta(u.at(a), step.at(a), m);
    // the key fold: samples in ascending order, a sample with phi = +inf stands for one that takes no part (the kernel skips it)
    for (int s = 0; s < Ns; ++s) {
      const int l = link.at(s);
      if (phi.at(s) == GQ_INF_F) continue;
      if (gq_close_key_less(phi.at(s), s, ml.at(l), idx.at(l))) ml.at(l) = phi.at(s), idx.at(l) = s;
    }
    // ... and the same fold in DESCENDING order must give the same keys: the tie-break does not depend on the order
    std::vector<float> ml2(L, GQ_INF_F);
    std::vector<int32_t> idx2(L, GQ_CLOSE_NONE);
    for (int s = Ns - 1; s >= 0; --s) {
      const int l = link.at(s);
      if (phi.at(s) == GQ_INF_F) continue;
      if (gq_close_key_less(phi.at(s), s, ml2.at(l), idx2.at(l))) ml2.at(l) = phi.at(s), idx2.at(l) = s;
    }
    for (int l = 0; l < L; ++l)
      if (idx.at(l) != idx2.at(l) || !(ml.at(l) == ml2.at(l))) {
        fprintf(stderr, "key fold depends on the order: record %d link %d\n", r, l);
        return 4;
      }
    for (int l = 0; l < L; ++l)
      if (idx.at(l) == GQ_CLOSE_NONE) idx.at(l) = -1;
    for (int a = 0; a < JA; ++a) {
      stopped.at(a) = gq_close_stopped(touched, masks.at(a)) ? 1 : 0;
      tnew.at(a) = gq_close_update(theta.at(a), delta.at(a), lo.at(a), hi.at(a), stopped.at(a) != 0);
    }
    put(out, delta), put(out, std::vector<float>{m}), put(out, ml), put(out, idx), put(out, stopped), put(out, tnew);
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 5;
}
