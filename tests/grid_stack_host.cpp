// The tiling and the decode of graspqp_amd/csrc/grid_stack.h compiled for the HOST: tests/test_grid_stack_host.py builds this
// program with the host compiler and sanitizers.  It walks every block of a launch over a stack of G grids of nx x ny x nz nodes
// and the 256 threads of each, exactly as the kernels do (gq_tile_of, gq_tile_node), and marks the node a thread is given in a
// vector of exactly the grid's size, one allocation per grid, so a node outside the grid is a sanitizer report.  No GPU involved.
// usage: grid_stack_host G nx ny nz   -> prints the launch's block count; exit 0 only if
//   every block's grid is < G (else 3), every node a thread passes the bounds test with lies in the grid (4), every thread the
//   test turns away lies outside it (5), and every node of every grid is hit exactly once (6)
#include <stdlib.h>

#include "host_shim.h"
#include "../graspqp_amd/csrc/grid_stack.h"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int G = atoi(argv[1]), nx = atoi(argv[2]), ny = atoi(argv[3]), nz = atoi(argv[4]);
  std::vector<std::vector<uint8_t>> hits(G);
  for (auto& h : hits) std::vector<uint8_t>((size_t)nx * ny * nz, 0).swap(h);  // capacity == size
  const GqTiling tiling = gq_tiling(nx, ny, nz);
  const long long blocks = gq_tiling_blocks(tiling, G);
  for (long long block = 0; block < blocks; ++block) {
    const GqTile t = gq_tile_of((unsigned)block, tiling);
    if (t.g >= (size_t)G) return 3;
    for (int tid = 0; tid < GQ_CL_THREADS; ++tid) {
      int i, j, k;
      const bool inside = gq_tile_node(t, tid, nx, ny, nz, i, j, k);
      const bool in_grid = i >= 0 && i < nx && j >= 0 && j < ny && k >= 0 && k < nz;
      if (inside && !in_grid) return 4;
      if (!inside && in_grid) return 5;
      if (inside) ++hits[t.g][((size_t)i * ny + j) * nz + k];
    }
  }
  for (const auto& h : hits)
    for (const uint8_t n : h)
      if (n != 1) return 6;
  printf("%lld\n", blocks);
  return 0;
}
