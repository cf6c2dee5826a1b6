// Elementwise / small-reduction pieces of one MALA* iteration:
//   gq_contact_terms    per-contact pieces of E_dis and the outward object normals fed to E_fc
//                       (reference core/energy.py:25-28; core/object_model.py:246)
//   gq_mala_propose     RMS-normalised gradient step + contact re-sampling  (core/optimizer.py:199-273)
//   gq_mala_accept      Metropolis accept with z-score-scaled temperature and state merge (optimizer.py:289-340,
//                       fit.py:454-458)
// Random numbers are inputs (drawn by the host-side generator), exactly like the oracle.
#include "fc_dev.h"
#include "loop_dev.h"

struct GqCombineArgs {  // argument block of gq_contact_terms
  const float* dist_sq;   // (B,n) object SDF squared distance of the contact points
  const int32_t* sign;    // (B,n)
  const float* onrm;      // (B,n,3) unit (p - closest)/|.|
  const float* closest;   // (B,n,3)
  const float* cpts;      // (B,n,3)
  const float* cnrm;      // (B,n,3) hand contact normals (world)
  int B, n;
  float w_dis;
  float* obj_normal; // (B,n,3) outward object normal = onrm * sign  (contact normals fed to E_fc)
  float* g_cpts;     // (B,n,3)  w_dis * dE_dis/dp   (E_fc part is added by the caller's fc backward)
  float* g_cnrm;     // (B,n,3)  w_dis * dE_dis/dnH
};

// stage 1 (before E_fc is known): per-contact quantities; one thread per (row, contact)
__global__ void gq_contact_terms_kernel(GqCombineArgs g) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)g.B * g.n) return;
  const gq3 on = gq_mk(g.onrm[t * 3], g.onrm[t * 3 + 1], g.onrm[t * 3 + 2]);
  const gq3 nH = gq_mk(g.cnrm[t * 3], g.cnrm[t * 3 + 1], g.cnrm[t * 3 + 2]);
  const gq3 p = gq_mk(g.cpts[t * 3], g.cpts[t * 3 + 1], g.cpts[t * 3 + 2]);
  const gq3 cl = gq_mk(g.closest[t * 3], g.closest[t * 3 + 1], g.closest[t * 3 + 2]);
  const GqContactTerm c = gq_contact_term(g.dist_sq[t], (float)g.sign[t], on, nH, p, cl, g.w_dis);
  gq_contact_term_store(c, (size_t)t, g.obj_normal, g.g_cpts, g.g_cnrm);
}

__global__ void gq_fill_kernel(float* __restrict__ y, float a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = a;
}

// ---- MALA* --------------------------------------------------------------------------------------------------------
// column mean of grad^2 over ALL rows (optimizer.py:231); one block per column, fixed-order tree reduction
__global__ __launch_bounds__(256) void gq_colsq_mean_kernel(const float* __restrict__ grad, int B, int D, int clip,
                                                            float* __restrict__ g2) {
  __shared__ float red[256];
  const int col = blockIdx.x, tid = threadIdx.x;
  float acc = 0.0f;
  for (int r = tid; r < B; r += 256) {
    float v = grad[(size_t)r * D + col];
    if (clip) {
      v = (v != v) ? 0.0f : fminf(fmaxf(v, -100.0f), 100.0f);  // NaN -> 0 first: fmaxf(NaN, -100) would be -100
    }
    acc = fmaf(v, v, acc);
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) g2[col] = red[0] / (float)B;
}

// same means for batches <= 512 rows and D <= 64 in the canonical order of loop_dev.h: wavefront u = unit u
__global__ __launch_bounds__(GQ_COLSQ_UNITS * GQ_WAVE) void gq_colsq_units_kernel(const float* __restrict__ grad, int B, int D,
                                                                              int clip, float* __restrict__ g2) {
  __shared__ float sPart[GQ_COLSQ_UNITS * GQ_WAVE];
  const int lane = gq_lane(), unit = (int)threadIdx.x / GQ_WAVE;
  if (lane < D) sPart[unit * D + lane] = gq_colsq_unit(grad, B, D, clip, unit, lane);
  __syncthreads();
  if (unit == 0 && lane < D) g2[lane] = gq_colsq_finish(sPart, B, D, lane);
}

__global__ __launch_bounds__(GQ_WAVE) void gq_mala_propose_kernel(GqProposeArgs g) {
  gq_propose_body(g, (int)blockIdx.x, gq_lane());
}

__global__ __launch_bounds__(GQ_WAVE) void gq_mala_accept_kernel(GqAcceptArgs g) {
  gq_accept_body(g, (int)blockIdx.x, gq_lane());
}

int gq_colsq_launch_(const float* grad, int B, int D, int clip, float* g2, void* stream) {
  if (B <= 512 && D <= GQ_WAVE)
    hipLaunchKernelGGL(gq_colsq_units_kernel, dim3(1), dim3(GQ_COLSQ_UNITS * GQ_WAVE), 0, (hipStream_t)stream, grad, B, D, clip, g2);
  else
    hipLaunchKernelGGL(gq_colsq_mean_kernel, dim3((unsigned)D), dim3(256), 0, (hipStream_t)stream, grad, B, D, clip, g2);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

extern "C" {

// The per-contact terms of core/energy.py:25-28.  Outputs see GqCombineArgs.
int gq_contact_terms(const float* dist_sq, const int32_t* sign, const float* onrm, const float* closest,
                     const float* contact_pts, const float* contact_normals, int64_t batch, int n_contact, float w_dis,
                     float* obj_normal, float* g_contact_pts, float* g_contact_normals, void* stream) {
  GQ_REQUIRE(dist_sq && sign && onrm && closest && contact_pts && contact_normals && obj_normal && g_contact_pts &&
                 g_contact_normals && batch > 0 && n_contact > 0,
             "contact_terms: bad arguments");
  GqCombineArgs a{};
  a.dist_sq = dist_sq;
  a.sign = sign;
  a.onrm = onrm;
  a.closest = closest;
  a.cpts = contact_pts;
  a.cnrm = contact_normals;
  a.B = (int)batch;
  a.n = n_contact;
  a.w_dis = w_dis;
  a.obj_normal = obj_normal;
  a.g_cpts = g_contact_pts;
  a.g_cnrm = g_contact_normals;
  const int64_t tot = batch * n_contact;
  hipLaunchKernelGGL(gq_contact_terms_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

int gq_fill(float* y, float a, int64_t n, void* stream) {
  if (n == 0) return GQ_OK;
  GQ_REQUIRE(y && n > 0, "fill: bad arguments");
  hipLaunchKernelGGL(gq_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, a, n);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

// MalaStar.try_step (optimizer.py:199-273) with the draws injected; g2_scratch: (D) floats
int gq_mala_propose(const float* hand_pose, const float* grad, const int64_t* contact_idx, const float* u_switch,
                    const int64_t* new_idx, int64_t batch, int pose_dim, int n_contact, float step_size,
                    int stepsize_period, float decay, float mu, float switch_possibility, int clip_grad, float* ema,
                    int64_t* step, float* pose_out, int64_t* idx_out, float* step_size_out, float* g2_scratch,
                    const float* energy, int64_t batch_each, float* z_out, void* stream) {
  GQ_REQUIRE(batch > 0 && pose_dim > 9 && n_contact > 0, "mala_propose: bad arguments");
  gqProposeDesc d{};
  d.hand_pose = hand_pose;
  d.grad = grad;
  d.contact_idx = contact_idx;
  d.u_switch = u_switch;
  d.new_idx = new_idx;
  d.ema = ema;
  d.step = step;
  d.step_size_out = step_size_out;
  d.g2_scratch = g2_scratch;
  d.energy = energy;
  d.batch_each = batch_each;
  d.z_out = z_out;
  d.step_size = step_size;
  d.stepsize_period = stepsize_period;
  d.decay = decay;
  d.mu = mu;
  d.switch_possibility = switch_possibility;
  d.clip_grad = clip_grad;
  GqProposeArgs a{};
  int rc = gq_propose_fill(d, "mala_propose", batch, pose_dim, n_contact, pose_out, idx_out, &a);
  if (rc) return rc;
  rc = gq_colsq_launch_(grad, (int)batch, pose_dim, clip_grad, g2_scratch, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(gq_mala_propose_kernel, dim3((unsigned)batch), dim3(GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

// MalaStar.accept_step + the masked state update of fit.py:454-458
int gq_mala_accept(const float* new_energy, const float* u_accept, const float* z, const uint8_t* reset_mask,
                   const int64_t* step, const float* pose_new, const int64_t* idx_new, const float* grad_new,
                   int64_t batch, int pose_dim, int n_contact, float starting_temperature, float decay,
                   int annealing_period, float* energy, float* pose, int64_t* idx, float* grad, uint8_t* accept,
                   float* temperature, int n_terms, const float* terms_new, float* terms, void* stream) {
  GQ_REQUIRE(batch > 0, "mala_accept: bad arguments");
  gqAcceptDesc d{};
  d.u_accept = u_accept;
  d.z = z;
  d.reset_mask = reset_mask;
  d.step = step;
  d.starting_temperature = starting_temperature;
  d.decay = decay;
  d.annealing_period = annealing_period;
  d.energy = energy;
  d.pose = pose;
  d.idx = idx;
  d.grad = grad;
  d.accept = accept;
  d.temperature = temperature;
  d.n_terms = n_terms;
  d.terms_new = terms_new;
  d.terms = terms;
  GqAcceptArgs a{};
  const int rc = gq_accept_fill(d, "mala_accept", new_energy, pose_new, idx_new, grad_new, batch, pose_dim, n_contact, &a);
  if (rc) return rc;
  hipLaunchKernelGGL(gq_mala_accept_kernel, dim3((unsigned)batch), dim3(GQ_WAVE), 0, (hipStream_t)stream, a);
  GQ_LAUNCH_CHECK();
  return GQ_OK;
}

}  // extern "C"
