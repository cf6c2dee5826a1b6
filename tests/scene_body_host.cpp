// The device body of the scene term (graspqp_amd/csrc/scene_dev.h) compiled for the HOST: tests/test_scene_body_host.py builds
// this program with the host compiler and sanitizers and compares its float32 results with the fp64 oracle.  No GPU involved.
// usage: scene_body_host in.bin out.bin
//   in.bin : int32 nx ny nz, float32 origin[3] voxel, int32 N, float32 values[nx ny nz], float32 points[N][3]
//   out.bin: per point float32 phi, grad[3], state (0 outside, 1 inside, 2 non-finite)
#include "host_shim.h"
#include "../graspqp_amd/csrc/scene_dev.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int d[3], N = 0;
  float oh[4];
  if (fread(d, 4, 3, f) != 3 || fread(oh, 4, 4, f) != 4 || fread(&N, 4, 1, f) != 1) return 4;
  std::vector<float> v((size_t)d[0] * d[1] * d[2]), p((size_t)N * 3);
  if (fread(v.data(), 4, v.size(), f) != v.size() || fread(p.data(), 4, p.size(), f) != p.size()) return 5;
  fclose(f);
  gqSceneGrid g{v.data(), d[0], d[1], d[2], {oh[0], oh[1], oh[2]}, oh[3]};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  for (int i = 0; i < N; ++i) {
    float phi = GQ_INF_F;
    gq3 gr = gq_mk(0, 0, 0);
    const int where = gq_scene_sample(g, gq_mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]), phi, gr);
    if (where == GQ_SCENE_NONFINITE) phi = gr.x = gr.y = gr.z = __builtin_nanf("");
    const float out[5] = {phi, gr.x, gr.y, gr.z, (float)where};
    fwrite(out, 4, 5, o);
  }
  fclose(o);
  return 0;
}
