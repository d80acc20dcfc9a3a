// Env step in three launches: rollout_post's work rides in the 32-row rollout forward (rows_fwd_kernel<32, false, 1, NL>).
//
// Between catppo_rollout_post and the next catppo_policy_step nothing runs, and the two tile the batch the same way (32
// envs / rows per workgroup).  The forward needs only the normalised observation rows of the post step; the rest of the
// post step needs nothing from the forward.  So, per (tile, network) workgroup:
//   entry   first weight slabs + bias of layer 0 (as rows_fwd_kernel), the tile's RAW observation rows and the operands
//           of the normaliser merge - and, critic workgroup, every operand of the post step's bookkeeping - are
//           requested together: one memory round trip where the two launches paid a boundary, a write of the normalised
//           tile and its re-read;
//   derive  the merged normaliser statistics (rollout_post.h: the functions rollout_post_kernel calls, on the same
//           exchange record), the normalised rows go straight into the LDS activation tile;
//   layers  rows_fwd_kernel's loop, unchanged: same contraction order, same heads, same Philox counters;
//   post    CRITIC workgroup only, BEHIND its value head: CaT probabilities, episode / reset statistics, reward, dones,
//           rollout-buffer rows, accumulator zeroing, and the normalised rows -> obs_out (held in registers since
//           `derive`).  The actor workgroup of the tile still runs its sampling epilogue (Philox, Box-Muller, log-prob)
//           at that point, so this part overlaps it; in front of the critic's first layer it would stand in front of
//           19 us of matrix work with its stores ahead of the first weight-slab waits (loads and stores share one
//           in-order counter).  Its LDS lies behind the weight rings: nothing aliases.
// The one-workgroup tail (publish the state, fold the reset statistics) stays deferred: it rides in the next rollout_pre
// launch, which re-derives the state from the same record.  The host side (try_step_merge) takes this launch only when
// the recorded step and the policy step agree; everything else goes through catppo_internal_flush_step.
#pragma once

namespace stepmerge {

using rpost::kPostRows;
using rpost::PostArgs;
using rpost::TermMetaS;

constexpr int kT = rowsfwd::kThreads;   // 512
constexpr int kC = 4;                   // constraint elements per thread: 32 rows x K <= 2048
constexpr int kO = 8;                   // observation elements per thread: 32 rows x D <= 4096
constexpr int kRedDoubles = 2 * rpost::kMaxTerms * kPostRows;

// floats of the post step's LDS area (behind tile + rings), in front of the fp64 reset-statistics rows
__host__ __device__ inline int post_floats(int K, int D, int nt) {
  return (2 * K + kPostRows * K + nt * kPostRows + 2 * D + 3) / 4 * 4 + 4;
}
inline size_t lds_bytes(size_t fwd_bytes, int K, int D, int nt) {
  return fwd_bytes + sizeof(float) * post_floats(K, D, nt) + sizeof(double) * kRedDoubles;
}

template <int NL>
__global__ __launch_bounds__(kT) void step_fwd_kernel(const FusedFwdArgs a, const PostArgs p, const TermMetaS meta) {
  using gemm::f32x16;
  constexpr int R = kPostRows;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* tile = smem;                                         // [R][ld]
  const int ld = a.ld0;
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* wring = smem + R * ld + wave * rowsfwd::kRingWave;
  const int K = p.K, D = p.D, nt = p.n_terms, Dp = a.Dp;
  float* col_rm = smem + R * ld + 8 * rowsfwd::kRingWave;     // [K]
  float* col_dp = col_rm + K;                                 // [K]
  float* ptile = col_dp + K;                                  // [R*K]
  float* tmax = ptile + R * K;                                // [nt*R]
  float* s_mean = tmax + nt * R;                              // [D]
  float* s_den = s_mean + D;                                  // [D]
  double* red = reinterpret_cast<double*>(col_rm + post_floats(K, D, nt));     // [2*nt*R] (16-byte aligned)
  __shared__ int s_off[rpost::kMaxTerms + 1];

  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int rows = (int)((p.N - r0) < R ? (p.N - r0) : R);
  const int net = a.net0 + (int)blockIdx.y;
  const bool critic = net == 0;                               // workgroup-uniform

  // ---- requests at entry: layer 0's first weight slabs, raw observation rows, operands of everything below
  rowsfwd::Layer<R> ly;
  float bias = a.params[a.off_b[net][0] + wave * 32 + l31];
  ly.stage(a.params + a.off_w[net][0], Dp, wave, lane);
  float po[kO];
#pragma unroll
  for (int j = 0; j < kO; ++j) {
    const int e = tid + j * kT;
    po[j] = 0.0f;
    if (e < rows * D) {
      const int r = fast_div(e, p.d_magic), c = e - r * D;
      po[j] = p.obs_raw[(r0 + r) * p.obs_ld + c];
    }
  }
  // padding columns [D, Dp) of the observation rows: the post step never writes them, the forward multiplies them
  const int npad = Dp - D;
  float xpad = 0.0f;
  int pad_r = 0, pad_c = 0;
  if (npad > 0 && tid < R * npad) {
    pad_r = tid / npad, pad_c = D + (tid - pad_r * npad);
    if (pad_r < rows) xpad = a.x[(r0 + pad_r) * Dp + pad_c];
  }
  const float pn_cnt = p.obs_count[0];
  double pn_sx = 0.0, pn_sxx = 0.0;
  float pn_mean = 0.0f, pn_var = 0.0f;
  if (tid < D) {
    rpost::load_sums(p, tid, &pn_sx, &pn_sxx);
    pn_mean = p.obs_mean[tid], pn_var = p.obs_var[tid];
  }
  float pc[kC], pk_m = 0.0f, pk_rm = 0.0f, pw_v = 0.0f, pw_p = 0.0f, pw_L = 1.0f, pe_reward = 0.0f;
  bool pw_rs = false, pe_rs = false, pe_to = false;
  const int n_el = rows * K;
#pragma unroll
  for (int j = 0; j < kC; ++j) pc[j] = 0.0f;
  if (critic) {
    const float* src = p.cstr + r0 * K;
#pragma unroll
    for (int j = 0; j < kC; ++j) {
      const int e = tid + j * kT;
      if (e < n_el) pc[j] = src[e];
    }
    {
      const int w = tid;
      const int t = w / kPostRows, e = w - t * kPostRows;
      if (w < nt * kPostRows && e < rows) {
        const int64_t i = r0 + e;
        const int64_t gi = (int64_t)t * p.N + i;
        pw_v = p.ep_viol[gi];
        pw_p = p.ep_prob[gi];
        pw_rs = p.reset[i] != 0;
        pw_L = (float)p.ep_len[i];
      }
    }
    if (tid < K) {
      pk_m = rpost::load_colmax(p, tid);
      if (!p.first_call) pk_rm = p.rm[tid];
    }
    if (tid < rows) {
      const int64_t i = r0 + tid;
      pe_reward = p.reward[i];
      pe_rs = p.reset[i] != 0;
      pe_to = p.time_outs[i] != 0;
    }
    if (tid <= nt) s_off[tid] = meta.off[tid];
  }
  __syncthreads();
  // ---- merged observation normaliser (cleanrl/ppo.py:48-62, the op order of rms.hip), identical in every workgroup;
  //      critic: the new running maxima (constraint_manager.py:58-61)
  {
    const float cnt = pn_cnt;
    const float nf = (float)p.obs_n;
    const float tot = cnt + nf;
    if (tid < D) {
      float new_mean, new_var;
      rpost::normaliser_from(p, pn_sx, pn_sxx, pn_mean, pn_var, cnt, nf, tot, &new_mean, &new_var);
      s_mean[tid] = new_mean;
      s_den[tid] = sqrtf(new_var + p.obs_eps);
    }
  }
  if (critic && tid < K) {
    int t = 0;
    while (t + 1 < nt && tid >= s_off[t + 1]) ++t;
    col_rm[tid] = rpost::running_max_from(p, pk_m, pk_rm);
    col_dp[tid] = meta.dp[t];
  }
  __syncthreads();
  // ---- normalised observation rows -> activation tile (rows past N: zeros, like the buffer loads of rows_fwd_kernel)
  float pv[kO];
#pragma unroll
  for (int j = 0; j < kO; ++j) {
    const int e = tid + j * kT;
    pv[j] = 0.0f;
    if (e < R * D) {
      const int r = fast_div(e, p.d_magic), c = e - r * D;
      if (r < rows) {
        const float v = po[j] - s_mean[c];
        pv[j] = v / s_den[c];
      }
      tile[r * ld + c] = pv[j];
    }
  }
  if (npad > 0 && tid < R * npad) tile[pad_r * ld + pad_c] = xpad;
  __syncthreads();

  // ---- the layers and the head: rows_fwd_kernel<32, false, 1, NL>
  ly.begin(wring, lane);
  int Kc = Dp;
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    f32x16 acc[1];
    ly.loop(tile, ld, wring, Kc, acc, lane);
    const bool more_layers = l + 1 < NL;
    float bias_next = 0.0f;
    if (more_layers) {
      bias_next = a.params[a.off_b[net][l + 1] + wave * 32 + l31];
      ly.stage(a.params + a.off_w[net][l + 1], rowsfwd::kWidth, wave, lane);
    }
    __syncthreads();                                          // every wave is done reading the tile: overwrite it
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      tile[row * ld + wave * 32 + l31] = gemm::elu_f(acc[0][r] + bias);
    }
    __syncthreads();
    if (more_layers) ly.begin(wring, lane);
    bias = bias_next;
    Kc = rowsfwd::kWidth;
  }
  fused_head<rowsfwd::kWidth>(a, tile, ld, net, r0, smem + R * ld);
  if (!critic) return;

  // ---- the post step's bookkeeping (statements and order of rollout_post_kernel), behind the value head
  float* pdst = p.probs ? p.probs + r0 * K : nullptr;
  auto prob_of = [&](const float x, const int c) {
    float q_ = 0.0f;
    if (x > 0.0f) {
      float q = x / col_rm[c];
      q = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
      const float s = q * col_dp[c];
      q_ = p.min_p + s;
    }
    return q_;
  };
#pragma unroll
  for (int j = 0; j < kC; ++j) {
    const int e = tid + j * kT;
    if (e < n_el) {
      const float pr = prob_of(pc[j], e - fast_div(e, p.k_magic) * K);
      ptile[e] = pr;
      if (pdst) pdst[e] = pr;
    }
  }
  __syncthreads();
  // per (term, env): max over the term's columns, episode statistics, reset statistics
  if (tid < nt * kPostRows) {
    const int w = tid;
    const int t = w / kPostRows, e = w - t * kPostRows;
    double ra = 0.0, rb = 0.0;
    if (e < rows) {
      const float* row = ptile + e * K;
      float m = row[s_off[t]];
      for (int c = s_off[t] + 1; c < s_off[t + 1]; ++c) m = nanmax(m, row[c]);
      tmax[t * kPostRows + e] = m;
      const int64_t gi = (int64_t)t * p.N + r0 + e;
      float v = pw_v + (m > 0.0f ? 1.0f : 0.0f);
      float q = pw_p + m;
      if (pw_rs) {       // ConstraintManager.reset (constraint_manager.py:190-211) for the envs that reset
        ra = (double)(v / pw_L);
        rb = (double)(q / pw_L);
        v = 0.0f, q = 0.0f;
      }
      p.ep_viol[gi] = v;
      p.ep_prob[gi] = q;
    }
    red[w] = ra;
    red[nt * kPostRows + w] = rb;
  }
  __syncthreads();
  if (tid < nt) {
    const int t = tid;
    double sa = 0.0, sb = 0.0;
    for (int e = 0; e < kPostRows; ++e) sa += red[t * kPostRows + e], sb += red[nt * kPostRows + t * kPostRows + e];
    xwg_store(p.reset_part + (int64_t)blockIdx.x * (2 * nt + 1) + 2 * t, sa);
    xwg_store(p.reset_part + (int64_t)blockIdx.x * (2 * nt + 1) + 2 * t + 1, sb);
  }
  // per env: probability, reward, dones (cat_env.py:102-107,118-121), rollout rows, reset bookkeeping
  if (tid < rows) {
    const int e = tid;
    float pr = tmax[e];
    for (int t = 1; t < nt; ++t) pr = nanmax(pr, tmax[t * kPostRows + e]);
    const int64_t i = r0 + e;
    p.cstr_prob[i] = pr;
    const float omp = 1.0f - pr;
    float r = pe_reward * omp;
    r = (r < 0.0f) ? 0.0f : r;
    p.reward[i] = r;
    const bool rs = pe_rs;
    {   // envs of this tile that reset: rows <= 32 live in the first half of wave 0
      const unsigned long long mask = __ballot(rs);
      if (tid == 0) xwg_store(p.reset_part + (int64_t)blockIdx.x * (2 * nt + 1) + 2 * nt, (double)__popcll(mask));
    }
    const float dn = rs ? 1.0f : pr;
    if (p.dones) p.dones[i] = dn;
    if (p.rewards_t != nullptr) {
      rpost::store_plane(p.rewards_t, i, r, p.planes_f16);
      rpost::store_plane(p.dones_t1, i, dn, p.planes_f16);
      rpost::store_plane(p.true_dones_t1, i, pe_to ? 1.0f : 0.0f, p.planes_f16);
    }
    if (rs) {
      p.ep_len[i] = 0;
      if (p.zero_action) {
        for (int k = 0; k < p.A; ++k) p.action[i * p.A + k] = 0.0f, p.prev_action[i * p.A + k] = 0.0f;
      }
    }
  }
  // normalised next observation rows (the rollout buffer's obs[step + 1]: what this launch's forward has just consumed)
#pragma unroll
  for (int j = 0; j < kO; ++j) {
    const int e = tid + j * kT;
    if (e < rows * D) {
      const int r = fast_div(e, p.d_magic), c = e - r * D;
      p.obs_out[(r0 + r) * p.obs_out_ld + c] = pv[j];
    }
  }
}

}  // namespace stepmerge

// Does the policy step (call, nets) continue the post step recorded in the context?  Then ONE launch does both, and the
// step's deferred tail is registered exactly as catppo_rollout_post would have.  false: nothing was launched, the caller
// flushes the recorded step and goes on as without it.
bool try_step_merge(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const FusedFwdArgs& call,
                    int nets, hipStream_t s) {
  using namespace stepmerge;
  PostArgs p;
  TermMetaS meta;
  memcpy(&p, ctx->step_args, sizeof(p));
  memcpy(&meta, ctx->step_meta, sizeof(meta));
  const MlpSwitches& sw = switches();
  const int64_t N = call.M;
  FusedFwdArgs a = call;
  size_t fwd_lds = 0;
  // (policy_core's order: the 16-row kernel comes first where it applies)
  const bool step16_first = sw.step16_fwd && N <= sw.step16_fwd_max_rows && step16_applies(shape, L, N);
  const bool fwd_ok = !step16_first && sw.rows_fwd_rollout && N <= sw.fused_fwd_max_rows && N >= sw.fused_fwd_min_rows &&
                      shape->n_hidden <= 3 && rows_fwd_plan(shape, L, shape->n_hidden, 32, &a, &fwd_lds);
  // the same step: rows, stream, and the rows the forward reads are the rows the post step writes
  const bool same = ctx->step_stream == (void*)s && p.N == N && p.obs_out == call.x && p.obs_out_ld == L.obs_pad &&
                    p.D >= 1 && p.D <= L.obs_pad && call.given == nullptr;
  // what the kernel holds per thread / per workgroup
  const bool fits = (int64_t)kPostRows * p.K <= kC * kT && p.K <= kT && (int64_t)kPostRows * p.D <= kO * kT &&
                    p.n_terms * kPostRows <= kT && kPostRows * (L.obs_pad - p.D) <= kT;
  // the two halves run side by side now: what the heads write must not be what the post step reads or writes
  auto apart = [](const void* x, const void* y) { return x == nullptr || x != y; };
  const bool disjoint = apart(call.action, p.action) && apart(call.action, p.prev_action) &&
                        apart(call.logprob, p.reward) && apart(call.value_out, p.reward) &&
                        apart(call.eps_out, p.action) && apart(call.logprob, p.cstr_prob) &&
                        apart(call.value_out, p.cstr_prob) && apart(call.value_out, p.rewards_t) &&
                        apart(call.value_out, p.dones_t1) && apart(call.value_out, p.true_dones_t1);
  if (!(fwd_ok && same && fits && disjoint)) return false;
  const size_t lds = lds_bytes(fwd_lds, p.K, p.D, p.n_terms);
  if (lds > 160 * 1024) return false;
  a.nets_per_wg = 1;
  const int64_t tiles = cdiv64(N, 32);
  dispatch_value<1, 2, 3>(a.n_hidden, [&](auto nl) {
    launch_lds(step_fwd_kernel<decltype(nl)::value>, dim3((unsigned)tiles, nets), dim3(kT), lds, s, a, p, meta);
  });
  ctx->step_pending = false;
  memcpy(ctx->post_tail_args, &p, sizeof(p));               // (p.defer == 1: a step is only recorded in deferred mode)
  ctx->post_tail_nblk = (int)tiles;
  ctx->post_tail_stream = s;
  ctx->post_tail_pending = true;
  catppo_plan_note(ctx, "env step + rollout forward, %lld rows: step_fwd_kernel (rows_fwd_kernel<32> + heads with the "
                   "post step of the recorded env step: normalised rows straight into the tile, bookkeeping behind the "
                   "critic's value head), %lld tiles x %d networks, ONE launch in place of rollout_post_kernel + forward",
                   (long long)N, (long long)tiles, nets);
  return true;
}
