// The device body of the TSDF integration (graspqp_amd/csrc/tsdf_dev.h: one node through every view) compiled for the HOST:
// tests/test_tsdf_body_host.py builds this program with the host compiler and sanitizers and compares its float32 results with
// the fp64 oracle.  The program walks the launch of tsdf.hip one block and one thread at a time, by the kernel's own decode
// (grid_stack.h).  Every image, label and grid buffer lives in an allocation of exactly its size, so a pixel or node read
// outside it, or a float -> int conversion of an out-of-range value, ends the program.  No GPU involved.
// usage: tsdf_body_host in.bin out.bin
//   in.bin : int32 G nx ny nz, float32 origin[3] voxel, int32 has_target has_skip has_labels, int32 V H W,
//            float32 fx fy cx cy depth_min depth_max trunc max_weight, float32 target_T[G][12] if has_target, int32 skip[G] if
//            has_skip, float32 cam_T[V][12], float32 depth[V][H][W], int32 labels[V][H][W] if has_labels,
//            float32 D[G][nx][ny][nz], float32 W[G][nx][ny][nz]
//   out.bin: float32 D[G][nx][ny][nz], float32 W[G][nx][ny][nz]
#include "host_shim.h"
#include "../graspqp_amd/csrc/tsdf_dev.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  std::vector<T>(n).swap(v);  // capacity == size: one element past the end is outside the allocation
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[4], has[3], im[3];
  float oh[4], cam[8];
  if (fread(hd, 4, 4, f) != 4 || fread(oh, 4, 4, f) != 4 || fread(has, 4, 3, f) != 3 || fread(im, 4, 3, f) != 3 || fread(cam, 4, 8, f) != 8)
    return 4;
  const int G = hd[0], V = im[0], H = im[1], Wd = im[2];
  const size_t nodes = (size_t)G * hd[1] * hd[2] * hd[3], pixels = (size_t)V * H * Wd;
  std::vector<float> tT, cT, depth, D, W;
  std::vector<int32_t> skip, labels;
  if (has[0] && !read_n(f, tT, (size_t)G * 12)) return 4;
  if (has[1] && !read_n(f, skip, (size_t)G)) return 4;
  if (!read_n(f, cT, (size_t)V * 12) || !read_n(f, depth, pixels)) return 4;
  if (has[2] && !read_n(f, labels, pixels)) return 4;
  if (!read_n(f, D, nodes) || !read_n(f, W, nodes)) return 5;
  fclose(f);
  const gqSceneGrid out{nullptr, hd[1], hd[2], hd[3], {oh[0], oh[1], oh[2]}, oh[3]};
  gqDepthViews views{};
  views.depth = depth.data(), views.labels = has[2] ? labels.data() : nullptr, views.cam_T = cT.data();
  views.n_views = V, views.width = Wd, views.height = H;
  views.fx = cam[0], views.fy = cam[1], views.cx = cam[2], views.cy = cam[3], views.depth_min = cam[4], views.depth_max = cam[5];
  const float trunc = cam[6], max_weight = cam[7];
  const GqTiling tiling = gq_tiling(out.nx, out.ny, out.nz);
  for (long long block = 0; block < gq_tiling_blocks(tiling, G); ++block) {
    const GqTile t = gq_tile_of((unsigned)block, tiling);
    const size_t g = t.g;
    for (int tid = 0; tid < GQ_CL_THREADS; ++tid) {
      int i, j, k;
      if (!gq_tile_node(t, tid, out.nx, out.ny, out.nz, i, j, k)) continue;
      const size_t node = ((g * out.nx + i) * out.ny + j) * out.nz + k;
      gq_tsdf_node(out, has[0] ? tT.data() + 12 * g : nullptr, i, j, k, views, has[1] ? skip[g] : -1, trunc, max_weight, D[node], W[node]);
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(D.data(), 4, D.size(), o);
  fwrite(W.data(), 4, W.size(), o);
  fclose(o);
  return 0;
}
