// gq_init_select_kernel's per-candidate bodies (graspqp_amd/csrc/init_select_dev.h) on the HOST: a block of T threads is emulated
// serially -- every thread's body runs to the point where the kernel has a barrier, then the block-wide reduction of the kernel
// (a sum, a minimum, a maximum / minimum of 64-bit keys) is taken over the threads' results in thread order.
//
//   init_select_host <case file> <T>
// case file: int32 n_obj, M, K; float32 tol; float32 points[n_obj][M][3]; float32 penalty[n_obj][M]
// stdout: per object one line "n_feasible sel[0] ... sel[K-1]"
//
// dist and sel are allocations of exactly M floats and K ints per object, so an index outside them ends the program under ASan.
#include "host_shim.h"
#include <stdlib.h>
static inline unsigned __float_as_uint(float f) {
  unsigned u;
  memcpy(&u, &f, sizeof(u));
  return u;
}
#include "../graspqp_amd/csrc/init_select_dev.h"

static void select_object(const float* P, const float* pen, int M, int K, float tol, int T, int* sel, int* n_feasible) {
  std::vector<float> dist((size_t)M);
  int nA = 0, cur = M;
  for (int tid = 0; tid < T; ++tid) {
    int c, f;
    gq_sel_init_thread(pen, dist.data(), M, tol, tid, T, &c, &f);
    nA += c;
    cur = f < cur ? f : cur;
  }
  *n_feasible = nA;
  const int n1 = nA < K ? nA : K;
  for (int it = 0; it < n1; ++it) {
    sel[it] = cur;
    const float cx = P[(size_t)cur * 3], cy = P[(size_t)cur * 3 + 1], cz = P[(size_t)cur * 3 + 2];
    unsigned long long best = GQ_SEL_NO_FPS_KEY;
    for (int tid = 0; tid < T; ++tid) {
      const unsigned long long k = gq_sel_fps_thread(P, dist.data(), M, tid, T, cur, cx, cy, cz);
      best = k > best ? k : best;
    }
    cur = gq_fps_key_index(best);
  }
  unsigned long long last = 0ull;
  for (int it = n1; it < K; ++it) {
    unsigned long long best = GQ_SEL_NO_FILL_KEY;
    for (int tid = 0; tid < T; ++tid) {
      const unsigned long long k = gq_sel_fill_thread(pen, M, tol, tid, T, it > n1, last);
      best = k < best ? k : best;
    }
    sel[it] = gq_sel_fill_key_index(best);
    last = best;
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int T = atoi(argv[2]);
  int32_t hdr[3];
  float tol;
  if (fread(hdr, sizeof(int32_t), 3, f) != 3 || fread(&tol, sizeof(float), 1, f) != 1) return 2;
  const int n_obj = hdr[0], M = hdr[1], K = hdr[2];
  if (n_obj <= 0 || M <= 0 || K <= 0 || M < K || T <= 0) return 2;
  std::vector<float> P((size_t)n_obj * M * 3), pen((size_t)n_obj * M);
  if (fread(P.data(), sizeof(float), P.size(), f) != P.size() || fread(pen.data(), sizeof(float), pen.size(), f) != pen.size()) return 2;
  fclose(f);
  for (int o = 0; o < n_obj; ++o) {
    std::vector<int> sel((size_t)K);
    int nf = 0;
    select_object(P.data() + (size_t)o * M * 3, pen.data() + (size_t)o * M, M, K, tol, T, sel.data(), &nf);
    printf("%d", nf);
    for (int k = 0; k < K; ++k) printf(" %d", sel[k]);
    printf("\n");
  }
  return 0;
}
