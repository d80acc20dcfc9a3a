// The part of the fused rollout step that rollout_post_kernel (rollout.hip) and the merged env-step forward
// (step_merge.h, compiled into mlp.hip) share: the launch's argument block and the device functions that derive the new
// running maxima / the merged observation normaliser from the exchange record(s).  Both translation units are compiled
// with -ffp-contract=off (build.py), and both call THESE functions: the state either kernel derives is the same bits.
#pragma once

#include "terms_eval.h"
#include "xwg.h"

namespace rpost {

using terms::kMaxTerms;
constexpr int kPostRows = 32;           // envs per tile (= rows per workgroup of the 32-row rollout forwards)
constexpr int kMaxObsPerThread = 2;     // rollout_post_kernel: D <= 512

struct TermMetaS {
  int32_t off[kMaxTerms + 1];
  float dp[kMaxTerms];
};

struct PostArgs {
  int64_t N;
  int A, D, K, n_terms;
  const float* cstr;
  float min_p, tau, one_minus_tau;
  int first_call;
  float* rm;
  float* reward;
  const uint8_t* reset;
  const uint8_t* time_outs;
  float* cstr_prob;
  float* dones;
  float* ep_viol;
  float* ep_prob;
  float* probs;
  int64_t* ep_len;
  float* action;
  float* prev_action;
  int zero_action;
  const float* log_prev;
  float* log_out;
  void* rewards_t;
  void* dones_t1;
  void* true_dones_t1;
  int planes_f16;
  const float* obs_raw;
  int64_t obs_ld;
  float* obs_mean;
  float* obs_var;
  float* obs_count;
  float obs_eps;
  double obs_n;
  float* obs_out;
  int64_t obs_out_ld;
  const float* x_colmax;
  const double* x_sums;
  int x_records;          // > 1: x_colmax / x_sums point at record 0 of `x_records` gathered records, x_stride bytes apart
  int64_t x_stride;
  double* reset_part;     // [grid][2 n_terms + 1]: per term {sum violation, sum probability}, then the reset count
  unsigned int* ticket;
  int defer;              // 1: no tail in this launch (post_tail_deferred runs it from a later launch)
  uint32_t d_magic, k_magic;   // catppo_div_magic(D), (K)
};
static_assert(sizeof(PostArgs) <= sizeof(catppo_ctx::post_tail_args), "catppo_ctx::post_tail_args too small");
static_assert(sizeof(PostArgs) <= sizeof(catppo_ctx::step_args), "catppo_ctx::step_args too small");
static_assert(sizeof(TermMetaS) <= sizeof(catppo_ctx::step_meta), "catppo_ctx::step_meta too small");

__device__ __forceinline__ void store_plane(void* p, int64_t i, float v, int f16) {
  if (f16) reinterpret_cast<_Float16*>(p)[i] = (_Float16)v;
  else reinterpret_cast<float*>(p)[i] = v;
}

// new running maximum of column c (constraint_manager.py:58-61) from the exchange record(s) and the state of the previous
// step (every workgroup of rollout_post_kernel, into LDS; the last one to arrive - or the deferred tail - writes it back).
// Split into the loads and the arithmetic so that rollout_post_kernel can request the operands up front.
__device__ __forceinline__ float load_colmax(const PostArgs& a, int c) {
  float m = a.x_colmax[c];
  for (int w = 1; w < a.x_records; ++w)     // gathered records of the other ranks: MAX is exact and order independent
    m = nanmax(m, reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.x_colmax) + w * a.x_stride)[c]);
  return m;
}
__device__ __forceinline__ float running_max_from(const PostArgs& a, float m, float rm_c) {
  if (a.first_call) return m;
  const float x = rm_c * a.tau;              // rm.mul_(tau)
  const float y = a.one_minus_tau * m;       // (1-tau) * cmax
  return x + y;                              // .add_()
}
__device__ __forceinline__ float derive_running_max(const PostArgs& a, int c) {
  return running_max_from(a, load_colmax(a, c), a.first_call ? 0.0f : a.rm[c]);
}
// merged observation normaliser of column c (cleanrl/ppo.py:48-62, the op order of rms.hip): new mean / variance
__device__ __forceinline__ void load_sums(const PostArgs& a, int c, double* sx_out, double* sxx_out) {
  const int D = a.D;
  double sx = a.x_sums[c], sxx = a.x_sums[D + c];
  for (int w = 1; w < a.x_records; ++w) {   // rank order: the same sums on every rank
    const double* xs = reinterpret_cast<const double*>(reinterpret_cast<const char*>(a.x_sums) + w * a.x_stride);
    sx += xs[c], sxx += xs[D + c];
  }
  *sx_out = sx, *sxx_out = sxx;
}
__device__ __forceinline__ void normaliser_from(const PostArgs& a, double sx, double sxx, float mean, float var, float cnt,
                                                float nf, float tot, float* new_mean, float* new_var) {
  const double m = sx / a.obs_n;
  double v = sxx / a.obs_n - m * m;
  if (v < 0.0) v = 0.0;
  const float bm = (float)m, bv = (float)v;
  const float delta = bm - mean;
  float t = delta * nf;
  t = t / tot;
  *new_mean = mean + t;
  const float m_a = var * cnt;
  const float m_b = bv * nf;
  float d2 = delta * delta;
  d2 = d2 * cnt;
  d2 = d2 * nf;
  d2 = d2 / tot;
  float M2 = m_a + m_b;
  M2 = M2 + d2;
  *new_var = M2 / tot;
}
__device__ __forceinline__ void derive_normaliser(const PostArgs& a, int c, float cnt, float nf, float tot, float* new_mean,
                                                  float* new_var) {
  double sx, sxx;
  load_sums(a, c, &sx, &sxx);
  normaliser_from(a, sx, sxx, a.obs_mean[c], a.obs_var[c], cnt, nf, tot, new_mean, new_var);
}

}  // namespace rpost
