// The device bodies of the arm clearance term (graspqp_amd/csrc/armscene_dev.h, with the reach term's joint bodies of reach_dev.h and
// gq_scene_sample of scene_dev.h) compiled for the HOST, and one row of gq_arm_kernel (csrc/armscene.hip) walked through them
// serially in the kernel's order: per station the joint transforms, the chain of link frames multiplied left to right, every sphere
// (lane) with its point, hinge and eight scalars, the eight wave sums in the shape of gq_wave_sums_f (the halves of the wave, the
// row pairs, then the four in-row stages), the columns with a joint on a limit frozen, J g_q and J J' in fp64, the unrolled fp64
// Cholesky; then the row's tail (stations ascending, gq_reach_grad_add / gq_reach_grad_close).  tests/test_arm_body_host.py builds
// this program with the host compiler and sanitizers and compares its results with the fp64 oracle.  Every buffer is exactly sized.
// usage: armscene_body_host in.bin out.bin
//   in.bin : int32 N K Ns nx ny nz, float32 D lambda rho c (= w up) margin voxel, origin[3] axis[3] R[9] base[12] tool[12],
//            int32 type[8], float32 pre[8][12] jaxis[8][3] lower[8] upper[8], q[(K+1)][N], int32 link[Ns], float32 centre[Ns][3]
//            radius[Ns], values[nx ny nz]
//   out.bin: float32 E, gRt[12], Ek[K+1]
#include "host_shim.h"
#include "../graspqp_amd/csrc/armscene_dev.h"

static const int G = GQ_REACH_MAX_JOINTS, WAVE = 64;

// the sum of the 64 lanes of one value as gq_wave_sums_f forms it: lanes l and l + 32, rows r and r + 1, then inside a row of 16
// quad_perm xor 1, xor 2, row_half_mirror, row_mirror.  Every stage adds pairs symmetrically: all lanes end with the same bits.
static float wave_sum(const float* v) {
  float a[32], b[16];
  for (int l = 0; l < 32; ++l) a[l] = v[l] + v[l + 32];
  for (int l = 0; l < 16; ++l) b[l] = a[l] + a[l + 16];
  float c[16], d[16], e[16];
  for (int l = 0; l < 16; ++l) c[l] = b[l] + b[l ^ 1];
  for (int l = 0; l < 16; ++l) d[l] = c[l] + c[l ^ 2];
  for (int l = 0; l < 16; ++l) e[l] = d[l] + d[(l & 8) | (7 - (l & 7))];
  return e[0] + e[15];
}

template <class T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[6];
  float par[6], origin[3], axis3[3], R[9];
  GqRT base, tool;
  if (fread(hd, 4, 6, f) != 6 || fread(par, 4, 6, f) != 6 || fread(origin, 4, 3, f) != 3 || fread(axis3, 4, 3, f) != 3 ||
      fread(R, 4, 9, f) != 9 || fread(base.m, 4, 12, f) != 12 || fread(tool.m, 4, 12, f) != 12)
    return 4;
  const int N = hd[0], K = hd[1], Ns = hd[2], nx = hd[3], ny = hd[4], nz = hd[5];
  if (N < 1 || N > G || K < 0 || K > GQ_REACH_MAX_STATIONS || Ns < 1 || Ns > GQ_ARM_MAX_SPHERES || nx < 2 || ny < 2 || nz < 2) return 4;
  const float D = par[0], lambda = par[1], rho = par[2], cw = par[3], margin = par[4], voxel = par[5];
  std::vector<int32_t> type, link;
  std::vector<float> pre, jaxis, lower, upper, q, centre, radius, values;
  if (!rd(f, type, G) || !rd(f, pre, (size_t)G * 12) || !rd(f, jaxis, (size_t)G * 3) || !rd(f, lower, G) || !rd(f, upper, G) ||
      !rd(f, q, (size_t)(K + 1) * N) || !rd(f, link, Ns) || !rd(f, centre, (size_t)Ns * 3) || !rd(f, radius, Ns) ||
      !rd(f, values, (size_t)nx * ny * nz))
    return 5;
  fclose(f);
  gqSceneGrid grid{};
  grid.values = values.data(), grid.nx = nx, grid.ny = ny, grid.nz = nz, grid.voxel = voxel;
  for (int i = 0; i < 3; ++i) grid.origin[i] = origin[i];
  const gq3 axis = gq_mk(axis3[0], axis3[1], axis3[2]);

  std::vector<float> sY((size_t)(K + 1) * 8), Ek(K + 1);
  for (int k = 0; k <= K; ++k) {  // a wavefront
    std::vector<float> sX((size_t)G * 12), sW((size_t)G * 12), sC((size_t)G * 6), sH(Ns), qk(G, 0.0f);
    std::vector<GqRT> W(G);
    for (int j = 0; j < G; ++j) {  // lanes 0..7: the joint transforms
      GqRT p;
      memcpy(p.m, pre.data() + (size_t)j * 12, sizeof(p.m));
      if (j < N) qk[j] = q[(size_t)k * N + j];
      const GqRT X = gq_reach_joint(p, type[j], gq_mk(jaxis[j * 3], jaxis[j * 3 + 1], jaxis[j * 3 + 2]), qk[j]);
      memcpy(sX.data() + (size_t)j * 12, X.m, sizeof(X.m));
    }
    for (int j = 0; j < G; ++j) {  // ... and the chain
      W[j] = gq_arm_chain(base, sX.data(), j);
      memcpy(sW.data() + (size_t)j * 12, W[j].m, sizeof(W[j].m));
    }
    float lanes[G][WAVE];
    for (int j = 0; j < G; ++j)
      for (int l = 0; l < WAVE; ++l) lanes[j][l] = 0.0f;
    for (int s = 0; s < Ns; ++s) {  // lane = sphere
      float g[G] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, h = 0.0f;
      const int l = link[s];
      if ((unsigned)l < (unsigned)N) {
        const gq3 x = gq_arm_point(sW.data() + (size_t)l * 12, gq_mk(centre[s * 3], centre[s * 3 + 1], centre[s * 3 + 2]));
        gq3 fs;
        h = gq_arm_hinge(grid, x, margin, radius[s], fs);
        gq_arm_joint_terms(l, x, fs, sW.data(), type.data(), jaxis.data(), g);
      }
      sH[s] = h;
      for (int j = 0; j < G; ++j) lanes[j][s] = g[j];
    }
    float gq[G];
    for (int j = 0; j < G; ++j) gq[j] = wave_sum(lanes[j]);
    GqRT W7;
    memcpy(W7.m, sW.data() + (size_t)(G - 1) * 12, sizeof(W7.m));
    const GqRT T = gq_reach_mul(W7, tool);
    for (int j = 0; j < G; ++j) {
      float c[6];
      gq_arm_col(type[j], W[j], gq_mk(jaxis[j * 3], jaxis[j * 3 + 1], jaxis[j * 3 + 2]), gq_mk(T.m[3], T.m[7], T.m[11]), rho, qk[j], lower[j],
                 upper[j], c);
      memcpy(sC.data() + (size_t)j * 6, c, sizeof(c));
    }
    double A[21], b[6], y[6];
    gq_arm_normal(sC.data(), gq, A, b);
    gq_arm_solve6(A, (double)lambda, b, y);
    for (int i = 0; i < 6; ++i) sY[(size_t)k * 8 + i] = 0.5f * (float)y[i];
    sY[(size_t)k * 8 + 6] = Ek[k] = gq_arm_station_sum(sH.data(), Ns);
    sY[(size_t)k * 8 + 7] = 0.0f;
  }
  // the row's tail
  const float inv = 1.0f / (float)(K + 1), cu = cw * inv;
  float esum = 0.0f, gRt[12] = {0}, tau_h[3] = {0};
  for (int k = 0; k <= K; ++k) esum += sY[(size_t)k * 8 + 6];
  for (int k = 0; k <= K; ++k) gq_reach_grad_add(R, sY.data() + (size_t)k * 8, cu, rho, gq_reach_station(D, k, K), axis, gRt, tau_h);
  gq_reach_grad_close(tau_h, gRt);
  const float E = esum * inv;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&E, 4, 1, o);
  fwrite(gRt, 4, 12, o);
  fwrite(Ek.data(), 4, Ek.size(), o);
  fclose(o);
  return 0;
}
