// The device bodies of the ESDF (graspqp_amd/csrc/edt_dev.h: tile geometry, seed, envelope, finish) compiled for the HOST:
// tests/test_esdf_body_host.py builds this program with the host compiler and sanitizers and compares its float32 result with the
// fp64 oracle.  The program walks the eight launches of edt.hip one block and one thread at a time: per tile the fill, then per
// element the body.  The volume, the three intermediate buffers, the output and every tile live in allocations of exactly their
// size (per grid), so a node or an LDS word touched outside one ends the program.  No GPU involved.
// usage: esdf_body_host in.bin out.bin
//   in.bin : int32 G nx ny nz, float32 voxel trunc max_distance, float32 D[G][nx][ny][nz]
//   out.bin: float32 phi[G][nx][ny][nz]
#include "host_shim.h"
#include "../graspqp_amd/csrc/edt_dev.h"

typedef std::vector<float> Buf;

template <bool INNER>
static void seed_pass(const gqEdtPass& q, const Buf& in, Buf& out) {
  const int n = GQ_EDT_LINES * q.L;
  const size_t step = INNER ? (size_t)q.n_inner : 1;
  for (int tile = 0; tile < gq_edt_tiles<INNER>(q); ++tile) {
    Buf line((size_t)n, -1.0f);  // a word of a line beyond the grid holds a crossing: it must never be read
    for (int e = 0; e < n; ++e) {
      int p, word;
      size_t node;
      if (!gq_edt_locate<INNER>(q, tile, e, p, word, node)) continue;
      line.at(word) = p + 1 < q.L ? gq_edt_edge(in.at(node), in.at(node + step)) : GQ_INF_F;
    }
    for (int e = 0; e < n; ++e) {
      int p, word;
      size_t node;
      if (!gq_edt_locate<INNER>(q, tile, e, p, word, node)) continue;
      out.at(node) = gq_edt_seed(line.data() + gq_edt_line0<INNER>(word, p), gq_edt_stride<INNER>(), q.L, p, q.R);
    }
  }
}

template <bool INNER>
static void env_pass(const gqEdtPass& q, const Buf& in, const Buf* other, const Buf* src, Buf& out, float voxel, float trunc, float maxd) {
  const int n = GQ_EDT_LINES * q.L;
  for (int tile = 0; tile < gq_edt_tiles<INNER>(q); ++tile) {
    Buf line((size_t)n, -1.0f);
    for (int e = 0; e < n; ++e) {
      int p, word;
      size_t node;
      if (!gq_edt_locate<INNER>(q, tile, e, p, word, node)) continue;
      line.at(word) = in.at(node);
    }
    for (int e = 0; e < n; ++e) {
      int p, word;
      size_t node;
      if (!gq_edt_locate<INNER>(q, tile, e, p, word, node)) continue;
      float v = gq_edt_env(line.data() + gq_edt_line0<INNER>(word, p), gq_edt_stride<INNER>(), q.L, p, q.R);
      if (other) v = other->at(node) < v ? other->at(node) : v;
      out.at(node) = src ? gq_edt_finish(src->at(node), v, voxel, trunc, maxd) : v;
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[4];
  float par[3];
  if (fread(hd, 4, 4, f) != 4 || fread(par, 4, 3, f) != 3) return 4;
  const int G = hd[0], nx = hd[1], ny = hd[2], nz = hd[3];
  const float voxel = par[0], trunc = par[1], maxd = par[2];
  const size_t nodes = (size_t)nx * ny * nz;
  const int R = (int)ceil((double)maxd / (double)voxel);
  if (nx > GQ_EDT_MAX_LINE || ny > GQ_EDT_MAX_LINE || nz > GQ_EDT_MAX_LINE || R > GQ_EDT_MAX_WINDOW) return 8;
  const gqEdtPass X{1, nx, ny * nz, R}, Y{nx, ny, nz, R}, Z{nx * ny, nz, 1, R};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  for (int g = 0; g < G; ++g) {  // one allocation per grid and buffer: the next grid's memory is no neighbour
    Buf D(nodes), A(nodes, -7777.0f), B(nodes, -7777.0f), C(nodes, -7777.0f), phi(nodes, -7777.0f);
    if (fread(D.data(), 4, nodes, f) != nodes) return 5;
    const Buf keep = D;
    seed_pass<false>(Z, D, A);
    env_pass<true>(Y, A, nullptr, nullptr, B, voxel, trunc, maxd);
    seed_pass<true>(Y, D, A);
    env_pass<false>(Z, A, &B, nullptr, C, voxel, trunc, maxd);
    env_pass<true>(X, C, nullptr, nullptr, B, voxel, trunc, maxd);
    seed_pass<true>(X, D, A);
    env_pass<false>(Z, A, nullptr, nullptr, C, voxel, trunc, maxd);
    env_pass<true>(Y, C, &B, &D, phi, voxel, trunc, maxd);
    if (memcmp(keep.data(), D.data(), nodes * 4) != 0) return 7;  // src is never written
    fwrite(phi.data(), 4, nodes, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
