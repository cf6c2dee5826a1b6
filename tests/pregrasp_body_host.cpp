// The device bodies of the pre-grasp term (graspqp_amd/csrc/pregrasp_dev.h, on top of scene_dev.h) compiled for the HOST, and one
// block of gq_pregrasp_kernel (csrc/pregrasp.hip) walked through them serially: eight wavefronts of 64 lanes, the chunks in the
// kernel's order, every reduction in the kernel's order (the DPP network of common.h's gq_dpp_sum, the wavefront folds, the tree
// sweep).  tests/test_pregrasp_body_host.py builds this program with the host compiler and sanitizers and compares its float32
// results with the fp64 oracle.  Every buffer is exactly sized, so an index outside one ends the program.  No GPU involved.
// usage: pregrasp_body_host in.bin out.bin
//   in.bin : int32 nx ny nz K Ns L J max_depth, float32 origin[3] voxel, float32 R[9] t[3] a[3] distance margin alpha up,
//            int32 link_node[L] node_type[J] node_depth[J] child_off[J+1] child_idx[child_off[J]],
//            float32 T[L][12] (link transforms at the opened joints) W[J][12] (node frames there) aw[J][3] (joint axes, hand frame),
//            float32 theta[J] q_open[J], float32 samples[Ns][3], int32 sample_link[Ns], float32 values[nx ny nz]
//   out.bin: float32 theta_o[J], E, gRt[12], g_theta[J]   (uncoupled hand: JA = J)
#include "host_shim.h"
#include "../graspqp_amd/csrc/pregrasp_dev.h"

static const int WAVES = 8, LANES = 64;

// gq_dpp_sum of common.h on 64 lane values: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_shr:4, row_shr:8, row_bcast:15 (rows
// 1,3), row_bcast:31 (rows 2,3); a lane that shifts in nothing, or whose row is masked, adds 0.  The result is lane 63's.
static float dpp_sum(const float* in) {
  float v[LANES], s[LANES];
  for (int i = 0; i < LANES; ++i) v[i] = in[i];
  for (int i = 0; i < LANES; ++i) s[i] = v[i] + v[i ^ 1];
  for (int i = 0; i < LANES; ++i) v[i] = s[i] + s[i ^ 2];
  for (int i = 0; i < LANES; ++i) s[i] = v[i] + (i % 16 >= 4 ? v[i - 4] : 0.0f);
  for (int i = 0; i < LANES; ++i) v[i] = s[i] + (i % 16 >= 8 ? s[i - 8] : 0.0f);
  for (int i = 0; i < LANES; ++i) s[i] = v[i] + ((i / 16) % 2 == 1 ? v[(i / 16) * 16 - 1] : 0.0f);
  for (int i = 0; i < LANES; ++i) v[i] = s[i] + (i / 16 >= 2 ? s[31] : 0.0f);
  return v[63];
}

template <class T>
static bool rd(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int hd[8];
  float oh[4], c[19];
  if (fread(hd, 4, 8, f) != 8 || fread(oh, 4, 4, f) != 4 || fread(c, 4, 19, f) != 19) return 4;
  const int K = hd[3], Ns = hd[4], L = hd[5], J = hd[6], max_depth = hd[7];
  if (L < 1 || L > 64 || J < 1 || J > 64 || K < 0 || K > 32) return 4;
  std::vector<int> link_node(L), node_type(J), node_depth(J), child_off(J + 1);
  if (!rd(f, link_node) || !rd(f, node_type) || !rd(f, node_depth) || !rd(f, child_off)) return 5;
  std::vector<int> child_idx(child_off[J]);
  std::vector<float> T((size_t)L * 12), W((size_t)J * 12), aw((size_t)J * 3), theta(J), q_open(J), smp((size_t)Ns * 3);
  std::vector<int> slink(Ns);
  std::vector<float> values((size_t)hd[0] * hd[1] * hd[2]);
  if (!rd(f, child_idx) || !rd(f, T) || !rd(f, W) || !rd(f, aw) || !rd(f, theta) || !rd(f, q_open) || !rd(f, smp) || !rd(f, slink) ||
      !rd(f, values))
    return 5;
  fclose(f);
  gqSceneGrid grid{values.data(), hd[0], hd[1], hd[2], {oh[0], oh[1], oh[2]}, oh[3]};
  const gq3 r1 = gq_mk(c[0], c[1], c[2]), r2 = gq_mk(c[3], c[4], c[5]), r3 = gq_mk(c[6], c[7], c[8]);
  const gq3 t = gq_mk(c[9], c[10], c[11]), a = gq_mk(c[12], c[13], c[14]);
  const float distance = c[15], margin = c[16], alpha = c[17], up_row = c[18];

  // head: the opened joint values (the tree walk itself is kin_dev.h's; its frames come in with the inputs)
  std::vector<float> theta_o(J);
  for (int j = 0; j < J; ++j) theta_o[j] = gq_pregrasp_open(theta[j], q_open[j], alpha);

  // stations: wavefront w takes the chunks w, w + 8, ...; lane = sample
  std::vector<float> s_part((size_t)WAVES * L * 6, 0.0f), s_K((size_t)WAVES * 9, 0.0f), s_e(WAVES, 0.0f);
  const int chunks = (Ns + LANES - 1) / LANES;
  for (int w = 0; w < WAVES; ++w) {
    float e[LANES] = {0}, Kl[LANES][9] = {{0}};
    std::vector<float> acc((size_t)L * 6, 0.0f);  // lane l of the wavefront owns link l
    for (int ch = w; ch < chunks; ch += WAVES) {
      float v[LANES][6] = {{0}};
      int lk[LANES];
      for (int lane = 0; lane < LANES; ++lane) {
        const int s = ch * LANES + lane;
        lk[lane] = -1;
        if (s >= Ns) continue;
        const int l = slink[s];
        if ((unsigned)l >= (unsigned)L) continue;
        lk[lane] = l;
        const gq3 xh = gq_pregrasp_point(T.data() + (size_t)l * 12, gq_mk(smp[3 * s], smp[3 * s + 1], smp[3 * s + 2]));
        gq3 G = gq_mk(0, 0, 0);
        gq_pregrasp_stations(grid, xh, a, r1, r2, r3, t, distance, K, margin, e[lane], G, Kl[lane]);
        const gq3 m = gq_pregrasp_moment(xh, G);
        v[lane][0] = G.x, v[lane][1] = G.y, v[lane][2] = G.z, v[lane][3] = m.x, v[lane][4] = m.y, v[lane][5] = m.z;
      }
      for (int k = 0; k < L; ++k) {
        bool any = false;
        for (int lane = 0; lane < LANES; ++lane) any = any || lk[lane] == k;
        if (!any) continue;
        for (int q = 0; q < 6; ++q) {
          float sel[LANES];
          for (int lane = 0; lane < LANES; ++lane) sel[lane] = lk[lane] == k ? v[lane][q] : 0.0f;
          acc[(size_t)k * 6 + q] += dpp_sum(sel);
        }
      }
    }
    s_e[w] = dpp_sum(e);
    for (int q = 0; q < 9; ++q) {
      float col[LANES];
      for (int lane = 0; lane < LANES; ++lane) col[lane] = Kl[lane][q];
      s_K[(size_t)w * 9 + q] = dpp_sum(col);
    }
    for (int i = 0; i < L * 6; ++i) s_part[(size_t)w * L * 6 + i] = acc[i];
  }

  // tail: links over the wavefronts, the row sums, links -> nodes -> parents, torques
  const float invK = 1.0f / (float)(K + 1);
  const float up = up_row * invK;
  std::vector<float> wr((size_t)L * 6, 0.0f), nf((size_t)J * 6, 0.0f);
  for (int l = 0; l < L; ++l)
    for (int w = 0; w < WAVES; ++w)
      for (int q = 0; q < 6; ++q) wr[(size_t)l * 6 + q] += s_part[((size_t)w * L + l) * 6 + q];
  float out_gRt[12];
  for (int q = 0; q < 3; ++q) {
    float col[LANES] = {0};
    for (int l = 0; l < L; ++l) col[l] = wr[(size_t)l * 6 + q];
    out_gRt[q] = up * -dpp_sum(col);
  }
  for (int q = 0; q < 9; ++q) {
    float val = 0.0f;
    for (int w = 0; w < WAVES; ++w) val += s_K[(size_t)w * 9 + q];
    out_gRt[3 + q] = up * val;
  }
  const float E = (((s_e[0] + s_e[1]) + (s_e[2] + s_e[3])) + ((s_e[4] + s_e[5]) + (s_e[6] + s_e[7]))) * invK;
  for (int j = 0; j < J; ++j)
    for (int k = 0; k < 6; ++k) nf[(size_t)j * 6 + k] = gq_pregrasp_fold_links(j, k, link_node.data(), L, wr.data());
  for (int d = max_depth - 1; d >= 0; --d) {
    std::vector<float> next = nf;  // the lanes of a level read the deeper levels' finished sums, then store
    for (int j = 0; j < J; ++j)
      if (node_depth[j] == d)
        for (int k = 0; k < 6; ++k)
          next[(size_t)j * 6 + k] =
              gq_pregrasp_fold_children(nf[(size_t)j * 6 + k], k, child_idx.data(), child_off[j], child_off[j + 1], nf.data());
    nf = next;
  }
  std::vector<float> g_theta(J);
  for (int j = 0; j < J; ++j) {
    const float tau = gq_pregrasp_torque(node_type[j], gq_mk(aw[3 * j], aw[3 * j + 1], aw[3 * j + 2]),
                                         gq_mk(W[(size_t)j * 12 + 3], W[(size_t)j * 12 + 7], W[(size_t)j * 12 + 11]),
                                         gq_mk(nf[(size_t)j * 6], nf[(size_t)j * 6 + 1], nf[(size_t)j * 6 + 2]),
                                         gq_mk(nf[(size_t)j * 6 + 3], nf[(size_t)j * 6 + 4], nf[(size_t)j * 6 + 5]));
    g_theta[j] = (1.0f - alpha) * (up * tau);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(theta_o.data(), 4, J, o);
  fwrite(&E, 4, 1, o);
  fwrite(out_gRt, 4, 12, o);
  fwrite(g_theta.data(), 4, J, o);
  fclose(o);
  return 0;
}
