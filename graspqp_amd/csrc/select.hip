// Grasp-set selection (include/graspqp_hip.h, "grasp-set selection"): per object the K best feasible rows that are pairwise at
// least `radius` apart, the distance being the RMS displacement of the hand surface between two rows in closed form.
//
// Two launches on one stream.  gq_grasp_prepare_kernel, one thread per (row, link): the world transform of the link into the
// workspace; the thread of link 0 also writes the row's feasibility and its 64-bit key.  gq_grasp_select_kernel, one block of
// 256 threads per object: a block-wide minimum of the keys per pick (the pattern of gq_init_select_kernel), the pick's
// transforms and the link moments staged in LDS, every thread then tests the rows it owns against the pick through gq_gs_dist2 (select_dev.h).
// No atomics, no block waits for another, the loops are bounded by K and batch_each, nothing is allocated, uploaded or read
// back: graph-capturable and bitwise reproducible.  gq_grasp_distance_kernel gives the whole matrix through the same function.
#include "common.h"
#include "sample_row_dev.h"  // GQ_ROW_MAX_LINKS: the link limit of the surface samples
#include "select_dev.h"

#define GQ_GS_THREADS 256
#define GQ_GS_WAVES (GQ_GS_THREADS / GQ_WAVE)

struct GqSelectArgs {
  const float* hand_pose;  // (B,D)
  const float* Rg;         // (B,9)
  const float* link_T;     // (B,L,12)
  const float* mom;        // (L,10)
  const float* score;      // (B) or null (distances: no keys)
  const float* terms;      // (nT,B)
  float tol[GQ_GS_MAX_TERMS];
  int n_terms, L, D, be, K;
  int64_t B;
  float inv_ns, r2;
  float* W;                 // (B,L,12) workspace
  unsigned long long* key;  // (B) workspace
  int32_t *sel, *n_selected, *n_feasible, *feasible;
  float* dist;  // (n_obj,be,be)
};

__global__ __launch_bounds__(256) void gq_grasp_prepare_kernel(GqSelectArgs g) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.B * g.L) return;
  const size_t b = (size_t)(i / g.L);
  const int l = (int)(i % g.L);
  gq_gs_world(g.Rg + b * 9, g.hand_pose + b * g.D, g.link_T + (b * g.L + l) * 12, g.W + (b * g.L + l) * 12);
  if (l != 0 || !g.score) return;
  const bool ok = gq_gs_feasible(g.score, g.terms, g.n_terms, (size_t)g.B, b, g.tol);
  g.feasible[b] = ok ? 1 : 0;
  g.key[b] = ok ? gq_sel_fill_key(g.score[b], (int)(b % (size_t)g.be)) : GQ_GS_NO_KEY;
}

// block-wide minimum of the threads' keys -> *s_best (valid behind the closing barrier)
__device__ __forceinline__ void gq_gs_block_min(unsigned long long best, unsigned long long* s_key, unsigned long long* s_best) {
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, GQ_WAVE);
    best = other < best ? other : best;
  }
  if (lane == 0) s_key[wv] = best;
  __syncthreads();
  if (tid == 0) {
    unsigned long long b = s_key[0];
    for (int w = 1; w < GQ_GS_WAVES; ++w) b = s_key[w] < b ? s_key[w] : b;
    *s_best = b;
  }
  __syncthreads();
}

__global__ __launch_bounds__(GQ_GS_THREADS) void gq_grasp_select_kernel(GqSelectArgs g) {
  __shared__ float s_W[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_mom[GQ_ROW_MAX_LINKS * GQ_GS_MOM];
  __shared__ unsigned long long s_key[GQ_GS_WAVES];
  __shared__ unsigned long long s_best;
  __shared__ int s_cnt[GQ_GS_WAVES];
  const int obj = blockIdx.x, tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const int L = g.L, be = g.be, K = g.K;
  unsigned long long* key = g.key + (size_t)obj * be;
  const float* W = g.W + (size_t)obj * be * L * 12;
  int32_t* out = g.sel + (size_t)obj * K;
  for (int i = tid; i < L * GQ_GS_MOM; i += GQ_GS_THREADS) s_mom[i] = g.mom[i];  // read behind the barriers of the first minimum
  int cnt;
  unsigned long long best = gq_gs_first_thread(key, be, tid, GQ_GS_THREADS, &cnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, GQ_WAVE);
  if (lane == 0) s_cnt[wv] = cnt;
  gq_gs_block_min(best, s_key, &s_best);
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < GQ_GS_WAVES; ++w) c += s_cnt[w];
    g.n_feasible[obj] = c;
  }
  int n = 0;
  for (; n < K; ++n) {
    const unsigned long long b = s_best;  // rewritten only behind the barrier below
    if (b == GQ_GS_NO_KEY) break;         // block-uniform: no row is left
    const int pick = gq_sel_fill_key_index(b);
    if (tid == 0) out[n] = obj * be + pick;
    for (int i = tid; i < L * 12; i += GQ_GS_THREADS) s_W[i] = W[(size_t)pick * L * 12 + i];
    __syncthreads();
    best = gq_gs_suppress_thread(key, W, be, tid, GQ_GS_THREADS, pick, s_W, s_mom, L, g.inv_ns, g.r2);
    gq_gs_block_min(best, s_key, &s_best);
  }
  for (int i = n + tid; i < K; i += GQ_GS_THREADS) out[i] = -1;
  if (tid == 0) g.n_selected[obj] = n;
}

// blockIdx.x: the global row i, staged in LDS; blockIdx.y, thread: the row j of the same object
__global__ __launch_bounds__(GQ_GS_THREADS) void gq_grasp_distance_kernel(GqSelectArgs g) {
  __shared__ float s_W[GQ_ROW_MAX_LINKS * 12];
  __shared__ float s_mom[GQ_ROW_MAX_LINKS * GQ_GS_MOM];
  const int tid = threadIdx.x, L = g.L, be = g.be;
  const size_t i = blockIdx.x;
  for (int k = tid; k < L * 12; k += GQ_GS_THREADS) s_W[k] = g.W[i * L * 12 + k];
  for (int k = tid; k < L * GQ_GS_MOM; k += GQ_GS_THREADS) s_mom[k] = g.mom[k];
  __syncthreads();
  const int j = blockIdx.y * GQ_GS_THREADS + tid;
  if (j >= be) return;
  const size_t first = (i / be) * be;  // the object's first row
  g.dist[i * be + j] = sqrtf(gq_gs_dist2(g.W + (first + j) * L * 12, s_W, s_mom, L, g.inv_ns));
}

// what both entries ask of the shared arguments; `who` = "grasp_select" or "grasp_select: grasp_distances"
static int gq_grasp_common_check(const char* who, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                                 const float* link_moments, int n_links, int64_t n_samples, int64_t batch, int64_t batch_each,
                                 int64_t max_each, const void* workspace, size_t workspace_bytes) {
  GQ_REQUIRE(hand_pose, "%s: hand_pose is NULL", who);
  GQ_REQUIRE(Rg, "%s: Rg is NULL", who);
  GQ_REQUIRE(link_T, "%s: link_T is NULL", who);
  GQ_REQUIRE(link_moments, "%s: link_moments is NULL", who);
  GQ_REQUIRE(workspace, "%s: workspace is NULL", who);
  GQ_REQUIRE(pose_dim >= 3, "%s: pose_dim must be >= 3, got %d", who, pose_dim);
  GQ_REQUIRE(n_links > 0 && n_links <= GQ_ROW_MAX_LINKS, "%s: n_links must be in 1..%d, got %d", who, GQ_ROW_MAX_LINKS, n_links);
  GQ_REQUIRE(n_samples > 0, "%s: n_samples must be > 0, got %lld", who, (long long)n_samples);
  GQ_REQUIRE(batch_each > 0 && batch_each <= max_each, "%s: batch_each must be in 1..%lld, got %lld", who, (long long)max_each,
             (long long)batch_each);
  GQ_REQUIRE(batch > 0 && batch <= 0x7fffffffll && batch % batch_each == 0,
             "%s: batch must be a positive multiple of batch_each below 2^31, got batch = %lld, batch_each = %lld", who,
             (long long)batch, (long long)batch_each);
  size_t need = 0;
  gq_grasp_select_workspace_bytes(batch, n_links, &need);
  GQ_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
  return GQ_OK;
}

static void gq_grasp_fill(GqSelectArgs& a, const float* hand_pose, int pose_dim, const float* Rg, const float* link_T,
                          const float* link_moments, int n_links, int64_t n_samples, int64_t batch, int64_t batch_each,
                          void* workspace) {
  a.hand_pose = hand_pose;
  a.Rg = Rg;
  a.link_T = link_T;
  a.mom = link_moments;
  a.L = n_links;
  a.D = pose_dim;
  a.be = (int)batch_each;
  a.B = batch;
  a.inv_ns = 1.0f / (float)n_samples;
  a.W = (float*)workspace;  // the keys behind the transforms: 48 B L bytes keep them 8-byte aligned
  a.key = (unsigned long long*)((char*)workspace + (size_t)batch * n_links * 12 * sizeof(float));
}

extern "C" {

int gq_grasp_select_workspace_bytes(int64_t batch, int n_links, size_t* bytes) {
  GQ_REQUIRE(bytes && batch > 0 && n_links > 0, "grasp_select_workspace_bytes: bad arguments");
  *bytes = (size_t)batch * (size_t)n_links * 12 * sizeof(float) + (size_t)batch * sizeof(unsigned long long);
  return GQ_OK;
}

int gq_grasp_select_check(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                          int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, const float* score,
                          const float* terms, const float* tol, int n_terms, int64_t K, float radius, const int32_t* sel,
                          const int32_t* n_selected, const int32_t* n_feasible, const int32_t* feasible, const void* workspace,
                          size_t workspace_bytes) {
  const int rc = gq_grasp_common_check("grasp_select", hand_pose, pose_dim, Rg, link_T, link_moments, n_links, n_samples, batch,
                                       batch_each, (1ll << 30) - 1, workspace, workspace_bytes);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(score, "grasp_select: score is NULL");
  GQ_REQUIRE(sel, "grasp_select: sel is NULL");
  GQ_REQUIRE(n_selected, "grasp_select: n_selected is NULL");
  GQ_REQUIRE(n_feasible, "grasp_select: n_feasible is NULL");
  GQ_REQUIRE(feasible, "grasp_select: feasible is NULL");
  GQ_REQUIRE(n_terms >= 0 && n_terms <= GQ_GS_MAX_TERMS, "grasp_select: n_terms must be in 0..%d, got %d", GQ_GS_MAX_TERMS, n_terms);
  GQ_REQUIRE(n_terms == 0 || terms, "grasp_select: terms is NULL with n_terms = %d", n_terms);
  GQ_REQUIRE(n_terms == 0 || tol, "grasp_select: tol is NULL with n_terms = %d", n_terms);
  for (int t = 0; t < n_terms; ++t) GQ_REQUIRE(tol[t] == tol[t], "grasp_select: tol[%d] is NaN", t);
  GQ_REQUIRE(K >= 1 && K <= batch_each, "grasp_select: K must be in 1..batch_each = %lld, got %lld", (long long)batch_each,
             (long long)K);
  GQ_REQUIRE(radius >= 0.0f && radius < GQ_INF_F, "grasp_select: radius must be finite, >= 0 and not NaN, got %g", (double)radius);
  return GQ_OK;
}

int gq_grasp_select(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                    int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, const float* score, const float* terms,
                    const float* tol, int n_terms, int64_t K, float radius, int32_t* sel, int32_t* n_selected, int32_t* n_feasible,
                    int32_t* feasible, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gq_grasp_select_check(hand_pose, pose_dim, Rg, link_T, link_moments, n_links, n_samples, batch, batch_each, score,
                                       terms, tol, n_terms, K, radius, sel, n_selected, n_feasible, feasible, workspace,
                                       workspace_bytes);
  if (rc != GQ_OK) return rc;
  GqSelectArgs a{};
  gq_grasp_fill(a, hand_pose, pose_dim, Rg, link_T, link_moments, n_links, n_samples, batch, batch_each, workspace);
  a.score = score;
  a.terms = terms;
  a.n_terms = n_terms;
  for (int t = 0; t < n_terms; ++t) a.tol[t] = tol[t];
  a.K = (int)K;
  a.r2 = radius * radius;
  a.sel = sel;
  a.n_selected = n_selected;
  a.n_feasible = n_feasible;
  a.feasible = feasible;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = batch * n_links;
  hipLaunchKernelGGL(gq_grasp_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  GQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(gq_grasp_select_kernel, dim3((unsigned)(batch / batch_each)), dim3(GQ_GS_THREADS), 0, st, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_grasp_distances_check(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                             int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, const float* dist,
                             const void* workspace, size_t workspace_bytes) {
  const int rc = gq_grasp_common_check("grasp_select: grasp_distances", hand_pose, pose_dim, Rg, link_T, link_moments, n_links,
                                       n_samples, batch, batch_each, 4096, workspace, workspace_bytes);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(dist, "grasp_select: grasp_distances: dist is NULL");
  return GQ_OK;
}

int gq_grasp_distances(const float* hand_pose, int pose_dim, const float* Rg, const float* link_T, const float* link_moments,
                       int n_links, int64_t n_samples, int64_t batch, int64_t batch_each, float* dist, void* workspace,
                       size_t workspace_bytes, void* stream) {
  const int rc = gq_grasp_distances_check(hand_pose, pose_dim, Rg, link_T, link_moments, n_links, n_samples, batch, batch_each, dist,
                                          workspace, workspace_bytes);
  if (rc != GQ_OK) return rc;
  GqSelectArgs a{};
  gq_grasp_fill(a, hand_pose, pose_dim, Rg, link_T, link_moments, n_links, n_samples, batch, batch_each, workspace);
  a.dist = dist;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = batch * n_links;
  hipLaunchKernelGGL(gq_grasp_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  GQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(gq_grasp_distance_kernel, dim3((unsigned)batch, (unsigned)((batch_each + GQ_GS_THREADS - 1) / GQ_GS_THREADS)),
                     dim3(GQ_GS_THREADS), 0, st, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
