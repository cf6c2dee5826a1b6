// The device body of the TSDF surfel extraction (graspqp_amd/csrc/surfel_dev.h: tile fill, crossing test, stencil normal) compiled
// for the HOST: tests/test_surfel_body_host.py builds this program with the host compiler and sanitizers and compares its float32
// results with the fp64 oracle.  The program walks the launches of surfel.hip one block and one thread at a time, by the kernels' own
// decode (grid_stack.h): per tile the fill of the count
// pass and the crossing flags, the exclusive prefix over a grid's tiles, then per tile the fill with the stencil's halo, the rank in
// the order (thread, axis) and the write below the capacity.  The volume, the weight, the tile and the outputs each live in an
// allocation of exactly their size, so a node or a slot touched outside one ends the program.  No GPU involved.
// usage: surfel_body_host in.bin out.bin
//   in.bin : int32 G nx ny nz, float32 origin[3] voxel, int32 has_weight has_region capacity, float32 min_weight trunc,
//            int32 region[6] if has_region, float32 D[G][nx][ny][nz], float32 W[G][nx][ny][nz] if has_weight
//   out.bin: int32 count[G][2], float32 points[G][capacity][3], float32 normals[G][capacity][3]; capacity 0 = the count only;
//            both arrays start as -7777
#include "host_shim.h"
#include "../graspqp_amd/csrc/surfel_dev.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  std::vector<T>(n).swap(v);  // capacity == size: one element past the end is outside the allocation
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[4], has[3], region[6];
  float oh[4], mt[2];
  if (fread(hd, 4, 4, f) != 4 || fread(oh, 4, 4, f) != 4 || fread(has, 4, 3, f) != 3 || fread(mt, 4, 2, f) != 2) return 4;
  const int G = hd[0], nx = hd[1], ny = hd[2], nz = hd[3], capacity = has[2];
  if (has[1] && fread(region, 4, 6, f) != 6) return 4;
  if (!has[1]) region[0] = 0, region[1] = nx, region[2] = 0, region[3] = ny, region[4] = 0, region[5] = nz;
  const size_t nodes = (size_t)nx * ny * nz;
  std::vector<std::vector<float>> D(G), W(G);  // one allocation per grid: the next grid's memory is no neighbour
  for (int g = 0; g < G; ++g)
    if (!read_n(f, D[g], nodes)) return 5;
  for (int g = 0; g < G && has[0]; ++g)
    if (!read_n(f, W[g], nodes)) return 5;
  fclose(f);
  const GqTiling tiling = gq_tiling(nx, ny, nz);
  const long long per_grid = gq_tiling_blocks(tiling, 1), tiles = gq_tiling_blocks(tiling, G);
  std::vector<int32_t> count((size_t)G * 2), tile_count((size_t)tiles), tile_prefix((size_t)tiles);
  std::vector<float> points((size_t)G * capacity * 3, -7777.0f), normals((size_t)G * capacity * 3, -7777.0f);
  auto grid = [&](size_t g) {  // the launch's view of grid g; a g the stack does not have ends the program (at)
    gqSurfelGrid s{};
    s.grid = gqSceneGrid{D.at(g).data(), nx, ny, nz, {oh[0], oh[1], oh[2]}, oh[3]};
    s.weight = has[0] ? W.at(g).data() : nullptr;
    s.min_weight = mt[0], s.trunc = mt[1];
    memcpy(s.region, region, sizeof(region));
    return s;
  };
  // launch 1: the count pass fills local 0 .. T only; the rest of the tile holds a value that would cross with anything
  for (long long b = 0; b < tiles; ++b) {
    const GqTile t = gq_tile_of((unsigned)b, tiling);
    const gqSurfelGrid s = grid(t.g);
    std::vector<float> tile(GQ_SF_TILE, b % 2 ? 1e-9f : -1e-9f);
    for (int e = 0; e < gq_surfel_entries(0, 1); ++e) gq_surfel_fill(s, t.i0, t.j0, t.k0, 0, 1, e, tile.data());
    int n = 0;
    for (int tid = 0; tid < GQ_SF_THREADS; ++tid) n += __builtin_popcount(gq_surfel_flags(s, tile.data(), t.i0, t.j0, t.k0, tid));
    tile_count[b] = n;
  }
  // launch 2: one block per grid
  for (int g = 0; g < G; ++g) {
    int running = 0;
    for (long long b = g * per_grid; b < (g + 1) * per_grid; ++b) tile_prefix[b] = running, running += tile_count[b];
    count[2 * g] = running, count[2 * g + 1] = capacity ? min(running, capacity) : 0;
  }
  // launch 3
  for (long long b = 0; b < tiles && capacity; ++b) {
    if (tile_count[b] == 0 || tile_prefix[b] >= capacity) continue;
    const GqTile t = gq_tile_of((unsigned)b, tiling);
    const gqSurfelGrid s = grid(t.g);
    std::vector<float> tile(GQ_SF_TILE);
    for (int e = 0; e < GQ_SF_TILE; ++e) gq_surfel_fill(s, t.i0, t.j0, t.k0, GQ_SF_LO, GQ_SF_HI, e, tile.data());
    int slot = tile_prefix[b];
    for (int tid = 0; tid < GQ_SF_THREADS; ++tid) {
      const unsigned flags = gq_surfel_flags(s, tile.data(), t.i0, t.j0, t.k0, tid);
      for (int c = 0; c < 3; ++c) {
        if (!((flags >> c) & 1u)) continue;
        if (slot < capacity) {
          const size_t at = (t.g * capacity + slot) * 3;
          gq_surfel_emit(s, tile.data(), t.i0, t.j0, t.k0, tid, c, points.data() + at, normals.data() + at);
        }
        ++slot;
      }
    }
    if (slot - tile_prefix[b] != tile_count[b]) return 7;  // the two passes must see the same crossings
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(count.data(), 4, count.size(), o);
  if (!points.empty()) {  // capacity 0: the vectors hold no memory
    fwrite(points.data(), 4, points.size(), o);
    fwrite(normals.data(), 4, normals.size(), o);
  }
  fclose(o);
  return 0;
}
