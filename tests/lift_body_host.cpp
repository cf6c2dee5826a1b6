// The device bodies of the lift term (graspqp_amd/csrc/lift_dev.h, on top of scene_dev.h) compiled for the HOST:
// tests/test_lift_body_host.py builds this program with the host compiler and sanitizers and compares its float32 results with the
// fp64 oracle.  No GPU involved.
// usage: lift_body_host in.bin out.bin
//   in.bin : int32 nx ny nz, float32 origin[3] voxel, float32 R[9] t[3] a[3] u[3] height retreat margin object_margin,
//            int32 K N M, float32 values[nx ny nz], float32 x_h[N][3], float32 p[M][3]
//   out.bin: per hand sample float32 e, G[3], K9[9], then per object point float32 e, 0[3], K9[9]
//            (sums over the point's stations, upstream 1, without 1/K)
#include "host_shim.h"
#include "../graspqp_amd/csrc/lift_dev.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int d[3], knm[3];
  float oh[4], c[22];
  if (fread(d, 4, 3, f) != 3 || fread(oh, 4, 4, f) != 4 || fread(c, 4, 22, f) != 22 || fread(knm, 4, 3, f) != 3) return 4;
  const int K = knm[0], N = knm[1], M = knm[2];
  std::vector<float> v((size_t)d[0] * d[1] * d[2]), p((size_t)N * 3), q((size_t)M * 3);
  if (fread(v.data(), 4, v.size(), f) != v.size() || fread(p.data(), 4, p.size(), f) != p.size() ||
      fread(q.data(), 4, q.size(), f) != q.size())
    return 5;
  fclose(f);
  gqSceneGrid g{v.data(), d[0], d[1], d[2], {oh[0], oh[1], oh[2]}, oh[3]};
  const gq3 r1 = gq_mk(c[0], c[1], c[2]), r2 = gq_mk(c[3], c[4], c[5]), r3 = gq_mk(c[6], c[7], c[8]);
  const gq3 t = gq_mk(c[9], c[10], c[11]), a = gq_mk(c[12], c[13], c[14]), u = gq_mk(c[15], c[16], c[17]);
  const float height = c[18], retreat = c[19], margin = c[20], object_margin = c[21];
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  for (int i = 0; i < N; ++i) {
    float out[13] = {0};
    gq3 G = gq_mk(0, 0, 0);
    gq_lift_hand_stations(g, gq_mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]), a, r1, r2, r3, t, u, height, retreat, K, margin, out[0], G,
                          out + 4);
    out[1] = G.x, out[2] = G.y, out[3] = G.z;
    fwrite(out, 4, 13, o);
  }
  const gq3 Ra = gq_lift_world_axis(a, r1, r2, r3);
  for (int j = 0; j < M; ++j) {
    float out[13] = {0};
    gq_lift_object_stations(g, gq_mk(q[3 * j], q[3 * j + 1], q[3 * j + 2]), a, Ra, r1, r2, r3, u, height, retreat, K, object_margin,
                            out[0], out + 4);
    fwrite(out, 4, 13, o);
  }
  fclose(o);
  return 0;
}
