// The device body of the compose kernel (graspqp_amd/csrc/clutter_dev.h: one output node, and the tile's conservative cull)
// compiled for the HOST: tests/test_clutter_body_host.py builds this program with the host compiler and sanitizers and compares
// its float32 results with the fp64 oracle.  The program walks the launch of clutter.hip one block and one thread at a time, by
// the kernel's own decode (grid_stack.h).  Every grid lives in a vector of exactly its size, so a node read outside it ends
// the program.  Every node is computed twice -- with every part sampled, and with the parts the tile's cull leaves -- and the
// program fails (exit 7) if the two differ in a single bit.  No GPU involved.
// usage: clutter_body_host in.bin out.bin
//   in.bin : int32 G nx ny nz, float32 origin[3] voxel far, float32 target_T[G][12], int32 exclude[G], int32 n_parts has_base,
//            float32 part_T[n_parts][12], then per grid (the parts, then the base if has_base):
//            int32 nx ny nz, float32 origin[3] voxel, float32 values[nx ny nz]
//   out.bin: float32 phi[G][nx][ny][nz], then int32 culled (tile, part) pairs, int32 all (tile, part) pairs
#include "host_shim.h"
#include "../graspqp_amd/csrc/clutter_dev.h"

struct Grid {
  std::vector<float> v;
  gqSceneGrid g;
};

static bool read_grid(FILE* f, Grid& G) {
  int d[3];
  float oh[4];
  if (fread(d, 4, 3, f) != 3 || fread(oh, 4, 4, f) != 4) return false;
  G.v.resize((size_t)d[0] * d[1] * d[2]);
  if (fread(G.v.data(), 4, G.v.size(), f) != G.v.size()) return false;
  G.g = gqSceneGrid{G.v.data(), d[0], d[1], d[2], {oh[0], oh[1], oh[2]}, oh[3]};
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[4], np[2];
  float oh[5];
  if (fread(hd, 4, 4, f) != 4 || fread(oh, 4, 5, f) != 5) return 4;
  const int G = hd[0];
  std::vector<float> tT((size_t)G * 12);
  std::vector<int32_t> excl(G);
  if (fread(tT.data(), 4, tT.size(), f) != tT.size() || fread(excl.data(), 4, G, f) != (size_t)G || fread(np, 4, 2, f) != 2) return 4;
  const int n_parts = np[0], has_base = np[1];
  if (n_parts < 0 || n_parts > GQ_CL_MAX_PARTS) return 4;
  std::vector<float> pT((size_t)n_parts * 12);
  if (fread(pT.data(), 4, pT.size(), f) != pT.size()) return 4;
  std::vector<Grid> grids(n_parts + (has_base ? 1 : 0));
  for (auto& g : grids)
    if (!read_grid(f, g)) return 5;
  fclose(f);
  std::vector<gqSceneGrid> parts(n_parts);
  for (int p = 0; p < n_parts; ++p) parts[p] = grids[p].g;
  const gqSceneGrid* base = has_base ? &grids[n_parts].g : nullptr;
  const gqSceneGrid out{nullptr, hd[1], hd[2], hd[3], {oh[0], oh[1], oh[2]}, oh[3]};
  const float far = oh[4];
  std::vector<float> phi((size_t)G * out.nx * out.ny * out.nz, -7777.0f);  // a node no thread reaches keeps the sentinel
  int culled = 0, pairs = 0;
  const GqTiling tiling = gq_tiling(out.nx, out.ny, out.nz);
  for (long long block = 0; block < gq_tiling_blocks(tiling, G); ++block) {
    const GqTile t = gq_tile_of((unsigned)block, tiling);
    const size_t g = t.g;
    const float* Tg = tT.data() + 12 * g;
    unsigned live = 0;
    for (int p = 0; p < n_parts; ++p) {
      const bool c = gq_clutter_culled(out, Tg, t.i0, t.j0, t.k0, parts[p], pT.data() + 12 * p);
      if (!c) live |= 1u << p;
      culled += c, ++pairs;
    }
    for (int tid = 0; tid < GQ_CL_THREADS; ++tid) {
      int i, j, k;
      if (!gq_tile_node(t, tid, out.nx, out.ny, out.nz, i, j, k)) continue;
      const float a = gq_clutter_node(out, Tg, i, j, k, parts.data(), n_parts, pT.data(), excl[g], 0xffffffffu, base, far);
      const float b = gq_clutter_node(out, Tg, i, j, k, parts.data(), n_parts, pT.data(), excl[g], live, base, far);
      if (memcmp(&a, &b, 4) != 0 && !(a != a && b != b)) {
        fprintf(stderr, "the cull changed node (%d,%d,%d,%d): %a -> %a\n", (int)g, i, j, k, (double)a, (double)b);
        return 7;
      }
      phi[((g * out.nx + i) * out.ny + j) * out.nz + k] = a;
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(phi.data(), 4, phi.size(), o);
  fwrite(&culled, 4, 1, o);
  fwrite(&pairs, 4, 1, o);
  fclose(o);
  return 0;
}
