// Finger closing (include/graspqp_hip.h, "finger closing"): the actuated joints are stepped along a closing direction until the
// links touch the object grid -- S + 1 dependent rounds of kinematics, grid query, per-link minimum, masks and update, as ONE
// launch that a captured graph can hold.
//
// One block of eight wavefronts per row, shaped like gq_pregrasp_row (pregrasp.hip):
//   head      wavefront 0 loads the hand tables of its lanes (lane = joint node, = link, = actuated joint), the row's joints, its
//             command and the stop masks, ONCE; every lane loads the sample of its first chunk, ONCE; the block copies the
//             coupling matrix of a coupled hand to LDS.  One barrier.
//   round e   wavefront 0: decisions of round e - 1 (below), then the tree walk of gq_pregrasp_row at theta_e into LDS, level by
//             level.  Barrier.  Eight wavefronts: lane = sample, x_w and phi by gq_scene_sample; for every link present in the chunk
//             the wavefront's minimum (DPP) and its lowest lane (ballot), kept by lane l for link l as a (phi, index) key; the keys
//             of the wavefronts to LDS.  Barrier.
//   decide    wavefront 0: lane l folds link l over the wavefronts by gq_close_key_less; touch; the touched links as one ballot;
//             lane a: stop mask and clamped update (close_dev.h).  No joint changed, or e = S: the outputs, and the block leaves.
// Two barriers per round.  Minima and a lowest-index tie-break only: no sums, no atomics, bitwise reproducible.
#include "kin_dev.h"
#include "sample_row_dev.h"  // GQ_ROW_WAVES, gq_row_point
#include "scene_dev.h"
#include "close_dev.h"

struct GqCloseArgs {
  gqHand h;
  gqSceneGrid grid;  // grid 0 of the stack
  int rows_per_grid;
  const float* samples;        // (Ns,3) link frame
  const int32_t* sample_link;  // (Ns)
  const float* hand_pose;      // (B,D), D = 9 + JA
  const float* Rg;             // (B,9)
  const float* direction;      // (B,JA)
  const float* step;           // (JA)
  const int64_t* joint_links;  // (JA)
  int Ns, D, S;
  float touch;
  float* theta;         // (B,JA) or null
  int32_t* touch_step;  // (B,L) or null
  int32_t* joint_stop;  // (B,JA) or null
  float* phi;           // (B,L) or null
  int32_t* sample;      // (B,L) or null
  float* point;         // (B,L,3) or null
  float* normal;        // (B,L,3) or null
};

__global__ __launch_bounds__(GQ_ROW_WAVES* GQ_WAVE) void gq_close_kernel(const GqCloseArgs g) {
  __shared__ float sW[64 * 12];  // node frames at theta_e
  __shared__ float sT[64 * 12];  // link transforms at theta_e
  __shared__ float sTh[64];      // coupled hands: the actuated joints
  __shared__ float sC[64 * 64];  // coupled hands: the coupling matrix (J,JA)
  __shared__ float s_phi[GQ_ROW_WAVES][64];  // per wavefront and link: the key of the smallest phi
  __shared__ int s_idx[GQ_ROW_WAVES][64];
  __shared__ int s_go;
  const int tid = threadIdx.x, lane = gq_lane(), wv = tid / GQ_WAVE;
  const size_t row = blockIdx.x;
  const gqHand& h = g.h;
  const int L = h.L, J = h.J, JA = h.JA, S = g.S;
  const gqSceneGrid grid = gq_stack_grid(g.grid, blockIdx.x / (unsigned)g.rows_per_grid);
  // ---- head: everything that does not change from round to round ----------------------------------------------------------
  int parent = -1, depth = -1, ntype = 0, lnode = -1;
  GqT pre = gq_t_identity(), loff = gq_t_identity();
  gq3 axj = gq_mk(0, 0, 0);
  float th = 0.0f, c0 = 0.0f, u = 0.0f, stp = 1.0f, lo = 0.0f, hi = 0.0f;
  uint64_t links = 0;
  const float* hp = g.hand_pose + row * g.D;
  if (wv == 0) {
    if (lane < J) {
      parent = h.node_parent[lane];
      depth = h.node_depth[lane];
      ntype = h.node_type[lane];
      pre = gq_t_load(h.node_pre + lane * 12);
      axj = gq_mk(h.node_axis[lane * 3], h.node_axis[lane * 3 + 1], h.node_axis[lane * 3 + 2]);
      if (h.coup) c0 = h.coup0[lane];
    }
    if (lane < L) {
      lnode = h.link_node[lane];
      loff = gq_t_load(h.link_offset + lane * 12);
    }
    if (lane < JA) {
      th = hp[9 + lane];
      stp = g.step[lane];
      u = gq_close_units(g.direction[row * JA + lane], stp);
      lo = h.jlo[lane], hi = h.jhi[lane];
      links = (uint64_t)g.joint_links[lane];
    }
  }
  const float* R = g.Rg + row * 9;
  const gq3 r1 = gq_mk(R[0], R[1], R[2]), r2 = gq_mk(R[3], R[4], R[5]), r3 = gq_mk(R[6], R[7], R[8]);
  const gq3 t = gq_mk(hp[0], hp[1], hp[2]);
  const int chunks = (g.Ns + GQ_WAVE - 1) / GQ_WAVE;
  int l0 = -1;  // the lane's sample of its first chunk: loaded once
  gq3 p0 = gq_mk(0, 0, 0);
  if (wv < chunks && wv * GQ_WAVE + lane < g.Ns) {
    const int s0 = wv * GQ_WAVE + lane;
    l0 = g.sample_link[s0];
    p0 = gq_mk(g.samples[(size_t)s0 * 3], g.samples[(size_t)s0 * 3 + 1], g.samples[(size_t)s0 * 3 + 2]);
  }
  if (h.coup)
    for (int i = tid; i < J * JA; i += GQ_ROW_WAVES * GQ_WAVE) sC[i] = h.coup[i];
  __syncthreads();
  // the command of the row: m = max |u_a| over the wavefront, Delta_a = step_a u_a / m (lanes >= JA hold u = 0)
  float delta = 0.0f;
  if (wv == 0) {
    float m = gq_close_umax(0.0f, u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float other = __shfl_xor(m, o, GQ_WAVE);  // |.| of a fold result is itself
      m = gq_close_umax(m, other);
    }
    delta = gq_close_delta(u, stp, m);
  }
  bool touched = false, done = false;
  int tstep = -1, jstop = -1;
  // ---- rounds ---------------------------------------------------------------------------------------------------------------
  for (int e = 0;; ++e) {
    if (wv == 0) {
      if (e > 0) {  // decisions of round e - 1
        const int ev = e - 1;
        float ml = GQ_INF_F;
        int il = GQ_CLOSE_NONE;
        if (lane < L) {
          for (int w = 0; w < GQ_ROW_WAVES; ++w) {
            const float pw = s_phi[w][lane];
            const int iw = s_idx[w][lane];
            if (gq_close_key_less(pw, iw, ml, il)) ml = pw, il = iw;
          }
          if (!touched && gq_close_touches(ml, g.touch)) touched = true, tstep = ev;
        }
        const uint64_t tm = __ballot(touched);
        bool stopped = false, moved = false;
        if (lane < JA) {
          stopped = gq_close_stopped(tm, links);
          if (stopped && jstop < 0) jstop = ev;
          if (ev < S) {
            const float nt = gq_close_update(th, delta, lo, hi, stopped);
            moved = nt != th;
            th = nt;
          }
        }
        done = ev == S || __ballot(moved) == 0ull;
        if (done) {  // the outputs, all of the final state: sT still holds its transforms
          if (lane < JA) {
            if (g.theta) g.theta[row * JA + lane] = th;
            if (g.joint_stop) g.joint_stop[row * JA + lane] = jstop;
          }
          if (lane < L) {
            const size_t o = row * L + lane;
            if (g.touch_step) g.touch_step[o] = tstep;
            if (g.phi) g.phi[o] = ml;
            if (g.sample) g.sample[o] = (unsigned)il < (unsigned)g.Ns ? il : -1;
            if (g.point || g.normal) {
              gq3 x = gq_mk(0, 0, 0), n = gq_mk(0, 0, 0);
              if ((unsigned)il < (unsigned)g.Ns) {  // GQ_CLOSE_NONE is beyond every sample
                const gq3 p = gq_mk(g.samples[(size_t)il * 3], g.samples[(size_t)il * 3 + 1], g.samples[(size_t)il * 3 + 2]);
                x = gq_close_world(r1, r2, r3, t, gq_row_point(sT + lane * 12, p));
                float ph = 0.0f;
                gq3 gr = gq_mk(0, 0, 0);
                if (gq_scene_sample(grid, x, ph, gr) == GQ_SCENE_INSIDE) {
                  const float len = sqrtf(gq_dot(gr, gr));
                  if (len > 0.0f && len < GQ_INF_F) n = gq_mk(gr.x / len, gr.y / len, gr.z / len);
                }
              }
              if (g.point) g.point[o * 3] = x.x, g.point[o * 3 + 1] = x.y, g.point[o * 3 + 2] = x.z;
              if (g.normal) g.normal[o * 3] = n.x, g.normal[o * 3 + 1] = n.y, g.normal[o * 3 + 2] = n.z;
            }
          }
        }
      }
      if (!done) {  // the tree walk at theta_e: gq_pregrasp_row's head
        float q = th;
        if (h.coup) {  // theta_tree = C theta + c0, as gq_fk_forward
          sTh[lane] = th;
          gq_wave_sync();
          q = c0;
          if (lane < J)
            for (int k = 0; k < JA; ++k) q = fmaf(sC[lane * JA + k], sTh[k], q);
        }
        GqT A = gq_t_identity();
        if (lane < J) {
          A = gq_t_mul(pre, gq_joint_motion(ntype, axj, q));
          if (parent < 0) gq_t_store(sW + lane * 12, A);
        }
        gq_wave_sync();
        for (int d = 1; d <= h.max_depth; ++d) {
          if (depth == d) {
            A = gq_t_mul(gq_t_load(sW + parent * 12), A);
            gq_t_store(sW + lane * 12, A);
          }
          gq_wave_sync();
        }
        if (lane < L) {
          GqT T = loff;
          if (lnode >= 0) T = gq_t_mul(gq_t_load(sW + lnode * 12), T);
          gq_t_store(sT + lane * 12, T);
        }
      }
      if (lane == 0) s_go = done ? 0 : 1;
    }
    __syncthreads();
    if (!s_go) break;  // block-uniform
    // evaluation e: lane = sample
    float bphi = GQ_INF_F;  // lane k: the key of link k in this wavefront
    int bidx = GQ_CLOSE_NONE;
    for (int c = wv; c < chunks; c += GQ_ROW_WAVES) {
      int l = l0;
      gq3 p = p0;
      if (c != wv) {  // more than 512 samples: the later chunks are re-read every round
        const int s = c * GQ_WAVE + lane;
        l = -1;
        if (s < g.Ns) {
          l = g.sample_link[s];
          p = gq_mk(g.samples[(size_t)s * 3], g.samples[(size_t)s * 3 + 1], g.samples[(size_t)s * 3 + 2]);
        }
      }
      float ph = GQ_INF_F;
      bool part = false;
      if ((unsigned)l < (unsigned)L) {  // a link id outside the hand (refused by ops.SurfaceSamples): the sample is ignored
        const gq3 x = gq_close_world(r1, r2, r3, t, gq_row_point(sT + l * 12, p));
        gq3 gr = gq_mk(0, 0, 0);
        part = gq_scene_sample(grid, x, ph, gr) == GQ_SCENE_INSIDE && ph == ph;
      }
      const int lk = part ? l : -1;
      unsigned long long todo = __ballot(part);
      while (todo) {  // wave-uniform: one pass per link present in the chunk
        const int src = __ffsll(todo) - 1;
        const int k = __builtin_amdgcn_readlane(lk, src);
        const bool mine = lk == k;
        todo &= ~__ballot(mine);
        const float m = gq_dpp_min(mine ? ph : GQ_INF_F);
        const int first = __ffsll(__ballot(mine && ph == m)) - 1;  // the lowest lane is the lowest sample index of the chunk
        const int idx = c * GQ_WAVE + first;
        if (lane == k && gq_close_key_less(m, idx, bphi, bidx)) bphi = m, bidx = idx;
      }
    }
    if (lane < L) s_phi[wv][lane] = bphi, s_idx[wv][lane] = bidx;
    __syncthreads();
  }
}

int gq_close_check(const gqClutterGrids* grids, int64_t batch, int64_t rows_per_grid, int n_joints, int n_actuated, int n_links,
                   int64_t n_samples, int n_steps, const float* step_host, float touch) {
  GQ_REQUIRE(rows_per_grid >= 1 && rows_per_grid <= 0x7fffffffll, "close: rows_per_grid must be in 1..2^31-1, got %lld",
             (long long)rows_per_grid);
  GQ_REQUIRE(n_joints >= 1 && n_joints <= 64 && n_links >= 1 && n_links <= 64 && n_actuated >= 1 && n_actuated <= 64,
             "close: the hand must have 1..64 tree joints, actuated joints and links, got J=%d JA=%d L=%d", n_joints, n_actuated,
             n_links);
  if (gq_clutter_check(grids, batch, (int)rows_per_grid, n_links, n_samples) != GQ_OK) return gq_retell("close", "grids");
  GQ_REQUIRE(n_steps >= 1 && n_steps <= GQ_CLOSE_MAX_STEPS, "close: n_steps must be in 1..%d, got %d", GQ_CLOSE_MAX_STEPS, n_steps);
  GQ_REQUIRE(touch >= 0.0f && touch < GQ_INF_F, "close: touch must be finite and >= 0, got %g", (double)touch);
  if (step_host)
    for (int a = 0; a < n_actuated; ++a)
      GQ_REQUIRE(step_host[a] > 0.0f && step_host[a] < GQ_INF_F, "close: step[%d] must be finite and > 0, got %g", a,
                 (double)step_host[a]);
  return GQ_OK;
}

int gq_close_fingers(const gqHand* h, const gqClutterGrids* grids, int64_t rows_per_grid, const float* samples,
                     const int32_t* sample_link, int64_t n_samples, const float* hand_pose, int pose_dim, const float* Rg,
                     int64_t batch, const float* direction, int n_steps, const float* step, const float* step_host, float touch,
                     const int64_t* joint_links, float* theta, int32_t* touch_step, int32_t* joint_stop, float* phi, int32_t* sample,
                     float* point, float* normal, void* stream) {
  GQ_REQUIRE(h, "close: hand is NULL");
  const int rc = gq_close_check(grids, batch, rows_per_grid, h->J, h->JA, h->L, n_samples, n_steps, step_host, touch);
  if (rc != GQ_OK) return rc;
  GQ_REQUIRE(samples && sample_link && hand_pose && Rg && direction && step && joint_links, "close: bad arguments");
  GQ_REQUIRE(pose_dim == 9 + h->JA, "close: pose_dim must be 9 + the hand's actuated joints = %d, got %d", 9 + h->JA, pose_dim);
  GqCloseArgs a{};
  a.h = *h;
  a.grid = gq_stack_grid(grids);
  a.rows_per_grid = (int)rows_per_grid;
  a.samples = samples, a.sample_link = sample_link, a.hand_pose = hand_pose, a.Rg = Rg, a.direction = direction, a.step = step;
  a.joint_links = joint_links;
  a.Ns = (int)n_samples, a.D = pose_dim, a.S = n_steps;
  a.touch = touch;
  a.theta = theta, a.touch_step = touch_step, a.joint_stop = joint_stop, a.phi = phi, a.sample = sample, a.point = point;
  a.normal = normal;
  hipLaunchKernelGGL(gq_close_kernel, dim3((unsigned)batch), dim3(GQ_ROW_WAVES * GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}
