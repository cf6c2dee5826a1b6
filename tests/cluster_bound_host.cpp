// The bound of the pruned cluster search (graspqp_amd/csrc/cluster_bound.h) compiled for the HOST: the Morton order and the
// oriented 64-face boxes exactly as gq_meshset_create builds them, and the fp32 lower bound exactly as the query wavefronts
// evaluate it (gq_cluster_lb from memory, gq_cluster_lb4 from registers, times the 0.9999 of gq_sdf_wave_query).
// tests/test_cluster_bound_host.py builds this program with the host compiler and sanitizers and holds the bound against exact
// fp64 distances; tests/_sdf_set_oracle.py uses it to find the clusters of a mesh.  Every array lives in an allocation of exactly
// its size.  No GPU involved.
// usage: cluster_bound_host bound in.bin out.bin
//          in.bin : int32 F, float32 face_verts[F][3][3]
//          out.bin: int32 n_clusters, int32 perm[F] (position -> face; cluster k = positions 64 k ..), float32 box[n_clusters][16]
//        cluster_bound_host lb in.bin out.bin
//          in.bin : int32 n_clusters, int32 P, float32 box[n_clusters][16], float32 points[n_clusters][P][3]
//          out.bin: float32 lb[n_clusters][P] = 0.9999f * gq_cluster_lb(box, point)
#include "host_shim.h"
struct alignas(16) float4 {
  float x, y, z, w;
};
#include "../graspqp_amd/csrc/cluster_bound.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  std::vector<T>(n).swap(v);  // capacity == size: one element past the end is outside the allocation
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  if (!strcmp(argv[1], "bound")) {
    int32_t F;
    std::vector<float> fv;
    if (fread(&F, 4, 1, f) != 1 || F <= 0 || !read_n(f, fv, (size_t)F * 9)) return 4;
    fclose(f);
    // gq_meshset_create, one mesh
    std::vector<int32_t> perm(F);
    float mesh_bb[8];
    for (int32_t i = 0; i < F; ++i) perm[i] = i;
    gq_box_of(fv.data(), perm.data(), 0, F, mesh_bb);
    gq_morton_order(fv.data(), perm.data(), 0, F, mesh_bb);
    const int32_t nC = (F + 63) / 64;
    std::vector<float> cl((size_t)nC * 16);
    for (int64_t i = 0; i < F; i += 64)
      gq_cluster_bound(fv.data(), perm.data(), i, std::min<int64_t>(i + 64, F), &cl[(size_t)(i / 64) * 16]);
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 6;
    fwrite(&nC, 4, 1, o);
    fwrite(perm.data(), 4, perm.size(), o);
    fwrite(cl.data(), 4, cl.size(), o);
    fclose(o);
    return 0;
  }
  if (!strcmp(argv[1], "lb")) {
    int32_t hd[2];
    if (fread(hd, 4, 2, f) != 2 || hd[0] <= 0 || hd[1] <= 0) return 4;
    const int nC = hd[0], P = hd[1];
    std::vector<float4> cl;  // 16-byte aligned like the device allocation: gq_cluster_lb reads float4
    std::vector<float> pts, lb((size_t)nC * P);
    if (!read_n(f, cl, (size_t)nC * 4) || !read_n(f, pts, (size_t)nC * P * 3)) return 5;
    fclose(f);
    for (int c = 0; c < nC; ++c) {
      const float* r = reinterpret_cast<const float*>(&cl[(size_t)c * 4]);
      const float4 reg[4] = {cl[(size_t)c * 4], cl[(size_t)c * 4 + 1], cl[(size_t)c * 4 + 2], cl[(size_t)c * 4 + 3]};
      for (int i = 0; i < P; ++i) {
        const float* x = &pts[((size_t)c * P + i) * 3];
        const gq3 p = gq_mk(x[0], x[1], x[2]);
        const float a = gq_cluster_lb(r, p) * 0.9999f, b = gq_cluster_lb4(reg, p) * 0.9999f;
        if (memcmp(&a, &b, 4) != 0) return 8;  // the two forms of the bound are one arithmetic
        lb[(size_t)c * P + i] = a;
      }
    }
    FILE* o = fopen(argv[3], "wb");
    if (!o) return 6;
    fwrite(lb.data(), 4, lb.size(), o);
    fclose(o);
    return 0;
  }
  return 2;
}
