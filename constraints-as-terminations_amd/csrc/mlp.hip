// Actor-critic MLP on MI355X: rollout policy step, PPO minibatch forward/loss/backward.
//
// Replaces cleanrl/ppo.py:71-123 (Agent) and :298-352 (minibatch update up to backward()).
// Hidden layers run on the fp32 MFMA GEMM of gemm_f32.h (critic + actor grouped in one launch,
// bias+ELU / ELU' fused in the epilogue).  The A-wide / 1-wide output heads, the Gaussian
// log-prob / entropy, the clipped PPO losses AND their analytic gradients w.r.t. the last
// hidden activations are one wave-per-row VALU kernel (head_loss) - or, from 4096 rows up and a
// last layer of 128 / 256 columns, the epilogue of the last forward GEMM itself (fwd_head_kernel:
// the activated tile stays in LDS, the head products run on the MFMA): no autograd graph, no
// (M,12) temporaries, no host sync.  Weight gradients are split-K over the batch with
// deterministic two-stage reduction (no float atomics => run-to-run reproducible); a layer's
// weight-gradient and data-gradient GEMMs share one launch (gemm_pair_kernel), the minibatch is
// gathered once per epoch (catppo_ppo_gather) and every partial is folded by one launch.
// The hidden layers below the last one run as ONE row-resident launch where the shape allows (rows_fwd_kernel,
// rows_fwd_wide_kernel), the same kernels with heads are the rollout forward, small batches take 16-row tiles (step16.h),
// and the first layer's weight-gradient launch carries the fold of the layers above it (dw_fold_kernel).
// This file: the C ABI and the two cores behind it - policy_core walks the rollout-forward candidates, minibatch_grad_core
// lists the stages of an optimiser step.  Kernels, switches, plans and launch functions: the headers below (map: mlp_common.h).
#include "common.h"
#include "gemm_f32.h"
#include "rng.h"
#include "rollout_post.h"

#include <cassert>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace {
#include "mlp_common.h"
#include "mlp_forward.h"
#include "mlp_loss.h"
#include "mlp_wide.h"
#include "step16.h"
#include "step_merge.h"
#include "mlp_step.h"
#include "mlp_backward.h"
#include "mlp_optim.h"

}  // namespace

// =============================================================================== C ABI
extern "C" int catppo_mlp_layout_of(const catppo_mlp_shape* shape, catppo_mlp_layout* out) {
  return layout_of(shape, out);
}

extern "C" uint64_t catppo_mlp_workspace_bytes(const catppo_mlp_shape* shape, int64_t rows) {
  catppo_mlp_layout L;
  if (layout_of(shape, &L) != CATPPO_OK || rows < 1) return 0;
  MlpWs w{};
  carve(shape, L, rows, true, nullptr, 0, &w);
  return w.bytes + 4096;
}

static int mlp_prologue(catppo_ctx* ctx, const catppo_mlp_shape* shape, int64_t M, bool training,
                        catppo_mlp_layout* L, MlpWs* w, const char* fn) {
  if (!ctx) return CATPPO_E_ARG;
  if (layout_of(shape, L) != CATPPO_OK) return catppo_fail(ctx, CATPPO_E_ARG, "%s: unsupported MLP shape", fn);
  if (M < 1 || M > (int64_t(1) << 30)) return catppo_fail(ctx, CATPPO_E_ARG, "%s: bad row count", fn);
  if (!carve(shape, *L, M, training, static_cast<char*>(ctx->ws), ctx->ws_bytes, w))
    return catppo_fail(ctx, CATPPO_E_WORKSPACE, "%s: workspace too small (%llu < %llu B); call catppo_reserve", fn,
                       (unsigned long long)ctx->ws_bytes, (unsigned long long)w->bytes);
  return CATPPO_OK;
}

namespace {
// layer-wise rollout forward, the form that takes every shape: one GEMM launch per hidden layer, then the head launch.
// bf16 operands, large batches (BASELINE configs[4]: 32768 envs): bf16-stored activations between the launches
// (gemm_f32.h "act16"); the last hidden layer writes fp32 for the head kernel.  CATPPO_ACT16=0: fp32-stored.
int rollout_layers(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w,
                   const FusedFwdArgs& call, bool critic_only, hipStream_t s) {
  const int64_t N = call.M;
  const int nets = critic_only ? 1 : 2;
  const bool fwd16 = switches().act16 && shape->mfma_bf16 == 1 && shape->n_hidden >= 2 && N >= 4096 && w.w16 != nullptr;
  if (fwd16) forward_hidden16(shape, L, call.params, call.x, N, w, nets, s, shape->n_hidden, true);
  else forward_hidden(shape, L, call.params, call.x, N, w, 0, nets, s);
  if (fwd16) catppo_plan_note(ctx, "rollout forward, %lld rows: bf16-stored activations between the layer-wise launches", (long long)N);
  if (shape->act_dim >= kMaxA)
    catppo_plan_note(ctx, "rollout forward, %lld rows: %d layer-wise GEMM launches (%s) + head_act_wide_kernel%s "
                     "[act_dim %d >= %d: no one-launch forward has wide heads]", (long long)N, shape->n_hidden,
                     fwd16 ? "bf16-stored activations" : "gemm_f32_kernel", critic_only ? " (critic only)" : "",
                     shape->act_dim, kMaxA);
  else
    catppo_plan_note(ctx, "rollout forward, %lld rows: %d layer-wise GEMM launches (gemm_f32_kernel) + head_act_kernel "
                     "[outside the one-launch window %s, or operand precision %d != fp32]", (long long)N, shape->n_hidden,
                     "CATPPO_FUSED_FWD_MIN_ROWS..MAX_ROWS (2049..4096)", shape->mfma_bf16);
  CATPPO_CHECK_LAUNCH(ctx);
  launch_head_act(shape, L, call, w, critic_only, s);
  return CATPPO_OK;
}

// rollout policy step behind catppo_policy_step
int policy_core(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* params, const float* x, int64_t N,
                const float* eps, const float* given_action, float* action, float* logprob, void* value,
                int value_dtype, const catppo_iter_state* rng_state, int rng_step, float* eps_out, bool critic_only,
                void* stream, const char* fn) {
  catppo_mlp_layout L;
  MlpWs w{};
  if (int rc = mlp_prologue(ctx, shape, N, false, &L, &w, fn)) return rc;
  CATPPO_CHECK_ARG(ctx, params && x && value && (critic_only || (action && logprob)));
  CATPPO_CHECK_ARG(ctx, value_dtype == CATPPO_F32 || value_dtype == CATPPO_F16);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // what every forward form gets from the call; Dp / ld0 / ld1 / hidden / offsets belong to each form's plan
  FusedFwdArgs call{};
  call.x = x, call.params = params, call.M = N, call.net0 = 0;
  call.logstd = params + L.off_logstd, call.eps = eps, call.given = given_action, call.A = shape->act_dim;
  call.action = action, call.logprob = logprob, call.value_out = value, call.value_f16 = (int)(value_dtype == CATPPO_F16);
  call.rng_state = rng_state, call.rng_step = rng_step, call.eps_out = eps_out, call.do_head = 1;
  const int nets = critic_only ? 1 : 2;
  // a post step recorded by catppo_rollout_post (catppo_rollout_defer_tail mode 2): this forward carries it when it
  // continues that step; otherwise the step runs as its own launch first, and the forward goes on as without it
  if (ctx->step_pending) {
    if (try_step_merge(ctx, shape, L, call, nets, s)) {
      CATPPO_CHECK_LAUNCH(ctx);
      return CATPPO_OK;
    }
    if (int rc = catppo_internal_flush_step(ctx, s)) return rc;
  }
  // the one-launch forms in the order they are preferred; the first that applies launches
  if (!(rollout_step16(ctx, shape, L, call, nets, s) || rollout_rows_fwd(ctx, shape, L, call, nets, s) ||
        rollout_rows_wide(ctx, shape, L, call, nets, s) || rollout_fused_fwd(ctx, shape, L, call, nets, s)))
    if (int rc = rollout_layers(ctx, shape, L, w, call, critic_only, s)) return rc;
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}
}  // namespace

// ABI 0.6: the one rollout-forward entry (catppo_policy_act / _ex / _rng, catppo_value / _ex of ABI <= 0.5 are inline
// wrappers in include/catppo_compat.h).  action == NULL: critic only.  Action noise: `eps` (supplied N(0,1)), or `state`
// (Philox counter {env, dim / 4, step, iteration}, eps_out receives it), or `given_action` (evaluate these actions).
extern "C" int catppo_policy_step(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* params, const float* x,
                                  int64_t N, const float* eps, const float* given_action, const catppo_iter_state* state,
                                  int32_t step, float* eps_out, float* action, float* logprob, void* value, int value_dtype,
                                  void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  CATPPO_CHECK_ARG(ctx, state == nullptr || (step >= 0 && eps == nullptr));
  const bool critic_only = action == nullptr;
  CATPPO_CHECK_ARG(ctx, !critic_only || (logprob == nullptr && eps == nullptr && given_action == nullptr && state == nullptr));
  return policy_core(ctx, shape, params, x, N, eps, given_action, action, logprob, value, value_dtype, state, step, eps_out,
                     critic_only, stream, __func__);
}

namespace {
// forward + losses + backward on an ALREADY GATHERED minibatch: xmb [M,Dp], act [M,A], scal [4][M]
// {old log-prob, advantage, normalised return, normalised value}, adv_part [nbg][2] fp64 advantage moments.  Stream order of
// the exchange: buckets right after their layer's launch (backward_layers), the tail's side-stream part right after dw_fold_kernel.
int minibatch_grad_core(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, MlpWs& w,
                        const catppo_ppo_hparams* hp, const float* params, int64_t M, const float* vrms_mean,
                        const float* vrms_var, const float* adv_stats, float* grad, float* diag, hipStream_t s,
                        NormEmit* ne = nullptr) {
  // 1. decide
  const StepPlan plan = decide_step(ctx, shape, L, w, M);
  if (ne != nullptr && plan.exch != Exchange::None)
    return catppo_fail(ctx, CATPPO_E_ARG, "%s: the one-call optimiser step cannot run with the gradient buckets "
                       "(something reduces the gradient between fold and clip)", __func__);
  if (ne != nullptr) ne->n_slots = 0;
  // 2. forward + heads + loss + head backward
  const HeadArgs g = head_args(shape, L, w, hp, params, M, vrms_mean, vrms_var, adv_stats, ctx->branch_out);
  if (int rc = step_forward_heads(ctx, shape, L, w, plan, params, g, s)) return rc;
  // 3. backward through the hidden layers; split-K partials for every weight gradient (Exchange::Buckets: folded and
  //    reduced per layer on the way, after which `s` has joined the side stream in front of the last bucket)
  Fold f{};
  f.grad = grad, f.diag = diag, f.ne = ne;
  if (plan.fwd == FwdForm::Step16) {
    if (int rc = backward_step16(ctx, shape, L, w, plan, hp, M, f, s)) return rc;
  } else {
    if (int rc = backward_layers(ctx, shape, L, w, plan, hp, params, M, f, s)) return rc;
  }
  if (plan.exch == Exchange::Buckets) return CATPPO_OK;
  // 4. fold what is not folded yet (+ the rest of the tail exchange)
  if (int rc = fold_final(ctx, hp, f, s)) return rc;
  if (plan.exch == Exchange::Tail) return exchange_tail_join(ctx, L, f, s);
  return CATPPO_OK;
}
}  // namespace

extern "C" int catppo_ppo_minibatch_grad(catppo_ctx* ctx, const catppo_mlp_shape* shape,
                                         const catppo_ppo_hparams* hp, const float* params, const float* b_obs,
                                         const float* b_actions, const float* b_logprobs,
                                         const float* b_advantages, const float* b_returns_n,
                                         const float* b_values_n, const int64_t* mb_inds, int64_t M,
                                         const float* vrms_mean, const float* vrms_var, const float* adv_stats,
                                         float* grad, float* diag, void* stream) {
  catppo_mlp_layout L;
  MlpWs w{};
  if (int rc = mlp_prologue(ctx, shape, M, true, &L, &w, __func__)) return rc;
  CATPPO_CHECK_ARG(ctx, hp && params && b_obs && b_actions && b_logprobs && b_advantages && b_returns_n &&
                            b_values_n && mb_inds && vrms_mean && vrms_var && grad && diag);
  CATPPO_CHECK_ARG(ctx, !hp->adv_stats_external || adv_stats != nullptr);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 1. gather the minibatch (ppo.py:300-302,314,331-337 index with mb_inds)
  hipLaunchKernelGGL(ppo_gather_kernel, dim3((unsigned)cdiv64(M, kGatherRows), 1), dim3(256), 0, s, b_obs, b_actions,
                     b_logprobs, b_advantages, b_returns_n, b_values_n, mb_inds, M, M, L.obs_pad, shape->act_dim,
                     w.xmb, w.act, w.scal, w.adv_part, (const catppo_iter_state*)nullptr, 0, 0, (int64_t*)nullptr);
  CATPPO_CHECK_LAUNCH(ctx);
  return minibatch_grad_core(ctx, shape, L, w, hp, params, M, vrms_mean, vrms_var, adv_stats, grad, diag, s);
}

extern "C" int catppo_ppo_gather_ex(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* b_obs,
                                    const float* b_actions, const float* b_logprobs, const void* b_advantages,
                                    int adv_dtype, const float* b_returns_n, const float* b_values_n,
                                    const int64_t* inds, const catppo_iter_state* state, int32_t epoch, int64_t total,
                                    int64_t M, float* x_g, float* act_g, float* scal_g, double* adv_part_g,
                                    int64_t* inds_out, void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  catppo_mlp_layout L;
  CATPPO_CHECK_ARG(ctx, shape && catppo_mlp_layout_of(shape, &L) == CATPPO_OK);
  CATPPO_CHECK_ARG(ctx, b_obs && b_actions && b_logprobs && b_advantages && b_returns_n && b_values_n);
  CATPPO_CHECK_ARG(ctx, (inds != nullptr) != (state != nullptr));    // exactly one source of the permutation
  if (inds != nullptr) state = nullptr;
  CATPPO_CHECK_ARG(ctx, adv_dtype == CATPPO_F32 || adv_dtype == CATPPO_F16);
  CATPPO_CHECK_ARG(ctx, x_g && act_g && scal_g && adv_part_g && total >= 1 && total < (int64_t(1) << 31) && M >= 1);
  const int64_t n_mb = cdiv64(total, M);
  CATPPO_CHECK_ARG(ctx, n_mb <= 65535);
  hipLaunchKernelGGL(ppo_gather_kernel, dim3((unsigned)cdiv64(M, kGatherRows), (unsigned)n_mb), dim3(256), 0,
                     static_cast<hipStream_t>(stream), b_obs, b_actions, b_logprobs,
                     static_cast<const float*>(b_advantages), b_returns_n, b_values_n, inds, total,
                     M, L.obs_pad, shape->act_dim, x_g, act_g, scal_g, adv_part_g, state, (int)epoch,
                     (int)(adv_dtype == CATPPO_F16), inds_out);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}

extern "C" int catppo_ppo_minibatch_grad_packed(catppo_ctx* ctx, const catppo_mlp_shape* shape,
                                                const catppo_ppo_hparams* hp, const float* params,
                                                const float* x_mb, const float* act_mb, const float* scal_mb,
                                                const double* adv_part_mb, int64_t M, const float* vrms_mean,
                                                const float* vrms_var, const float* adv_stats, float* grad,
                                                float* diag, void* stream) {
  catppo_mlp_layout L;
  MlpWs w{};
  if (int rc = mlp_prologue(ctx, shape, M, true, &L, &w, __func__)) return rc;
  CATPPO_CHECK_ARG(ctx, hp && params && x_mb && act_mb && scal_mb && adv_part_mb && vrms_mean && vrms_var && grad &&
                            diag);
  CATPPO_CHECK_ARG(ctx, !hp->adv_stats_external || adv_stats != nullptr);
  CATPPO_CHECK_ARG(ctx, (reinterpret_cast<uintptr_t>(x_mb) & 15) == 0);
  // the kernels only read these: point the workspace view at the caller's gathered slices
  w.xmb = const_cast<float*>(x_mb), w.act = const_cast<float*>(act_mb), w.scal = const_cast<float*>(scal_mb);
  w.adv_part = const_cast<double*>(adv_part_mb);
  return minibatch_grad_core(ctx, shape, L, w, hp, params, M, vrms_mean, vrms_var, adv_stats, grad, diag,
                             static_cast<hipStream_t>(stream));
}

extern "C" int catppo_clip_adam(catppo_ctx* ctx, float* params, float* grad, float* exp_avg, float* exp_avg_sq,
                                int64_t n_flat, float max_grad_norm, double lr, double beta1, double beta2,
                                double eps, int64_t step, void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  CATPPO_CHECK_ARG(ctx, params && grad && exp_avg && exp_avg_sq && n_flat >= 1 && step >= 1);
  hipStream_t s = static_cast<hipStream_t>(stream);
  WsCarver ws(ctx);
  double* part = ws.take<double>(kNormBlocks);
  CATPPO_NEED_WS(ctx, part);
  int nb = (int)cdiv64(n_flat, 256 * 4);
  if (nb > kNormBlocks) nb = kNormBlocks;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nb), dim3(256), 0, s, (const float*)grad, n_flat, part);
  CATPPO_CHECK_LAUNCH(ctx);
  // bias corrections in double on the host, like torch.optim.Adam's Python scalars
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  int nblk = (int)cdiv64(n_flat, 256 * 4);
  if (nblk > 1024) nblk = 1024;
  hipLaunchKernelGGL(clip_adam_kernel, dim3(nblk), dim3(256), 0, s, params, grad, exp_avg, exp_avg_sq, n_flat,
                     (const double*)part, nb, max_grad_norm, (float)beta1, (float)beta2, (float)(1.0 - beta1),
                     (float)(1.0 - beta2), (float)eps, step_size, bc2_sqrt);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}

extern "C" int catppo_clip_adam_dev(catppo_ctx* ctx, float* params, float* grad, float* exp_avg, float* exp_avg_sq,
                                    int64_t n_flat, float max_grad_norm, double beta1, double beta2, double eps,
                                    catppo_iter_state* state, void* stream) {
  CATPPO_CHECK_ARG(ctx, ctx != nullptr);
  CATPPO_CHECK_ARG(ctx, params && grad && exp_avg && exp_avg_sq && n_flat >= 1 && state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  WsCarver ws(ctx);
  double* part = ws.take<double>(kNormBlocks);
  CATPPO_NEED_WS(ctx, part);
  int nb = (int)cdiv64(n_flat, 256 * 4);
  if (nb > kNormBlocks) nb = kNormBlocks;
  hipLaunchKernelGGL(sqnorm_partial_step_kernel, dim3(nb), dim3(256), 0, s, (const float*)grad, n_flat, part, state, beta1,
                     beta2);
  CATPPO_CHECK_LAUNCH(ctx);
  int nblk = (int)cdiv64(n_flat, 256 * 4);
  if (nblk > 1024) nblk = 1024;
  hipLaunchKernelGGL(clip_adam_dev_kernel, dim3(nblk), dim3(256), 0, s, params, grad, exp_avg, exp_avg_sq, n_flat,
                     (const double*)part, nb, max_grad_norm, beta1, beta2, (float)eps,
                     (const catppo_iter_state*)state);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}

// One optimiser step of a single process in one call (ABI 0.4): catppo_ppo_minibatch_grad_packed + catppo_clip_adam_dev
// with the squared gradient norm emitted by the fold launches (NormEmit) instead of a launch that re-reads the gradient.
extern "C" int catppo_ppo_minibatch_step_packed(catppo_ctx* ctx, const catppo_mlp_shape* shape,
                                                const catppo_ppo_hparams* hp, float* params, const float* x_mb,
                                                const float* act_mb, const float* scal_mb, const double* adv_part_mb,
                                                int64_t M, const float* vrms_mean, const float* vrms_var,
                                                const float* adv_stats, float* grad, float* diag, float* exp_avg,
                                                float* exp_avg_sq, float max_grad_norm, double beta1, double beta2,
                                                double eps, catppo_iter_state* state, void* stream) {
  catppo_mlp_layout L;
  MlpWs w{};
  if (int rc = mlp_prologue(ctx, shape, M, true, &L, &w, __func__)) return rc;
  CATPPO_CHECK_ARG(ctx, hp && params && x_mb && act_mb && scal_mb && adv_part_mb && vrms_mean && vrms_var && grad &&
                            diag && exp_avg && exp_avg_sq && state);
  CATPPO_CHECK_ARG(ctx, !hp->adv_stats_external || adv_stats != nullptr);
  CATPPO_CHECK_ARG(ctx, (reinterpret_cast<uintptr_t>(x_mb) & 15) == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  w.xmb = const_cast<float*>(x_mb), w.act = const_cast<float*>(act_mb), w.scal = const_cast<float*>(scal_mb);
  w.adv_part = const_cast<double*>(adv_part_mb);
  NormEmit ne;
  ne.part = w.norm_part, ne.st = state, ne.beta1 = beta1, ne.beta2 = beta2;
  if (int rc = minibatch_grad_core(ctx, shape, L, w, hp, params, M, vrms_mean, vrms_var, adv_stats, grad, diag, s, &ne))
    return rc;
  if (ne.n_slots < 1 || ne.n_slots > kNormSlots)
    return catppo_fail(ctx, CATPPO_E_ARG, "%s: %d squared-norm slots", __func__, ne.n_slots);
  int nblk = (int)cdiv64(L.n_flat, 256 * 4);
  if (nblk > 1024) nblk = 1024;
  hipLaunchKernelGGL(clip_adam_dev_kernel, dim3(nblk), dim3(256), 0, s, params, grad, exp_avg, exp_avg_sq,
                     (int64_t)L.n_flat, (const double*)ne.part, ne.n_slots, max_grad_norm, beta1, beta2, (float)eps,
                     (const catppo_iter_state*)state);
  catppo_plan_note(ctx, "clip + Adam: clip_adam_dev_kernel, %d workgroups, norm from %d slots of the fold launches", nblk, ne.n_slots);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}

// Test hook (tests/test_gpu_parity_sizes.py): buf != NULL - [2][M] int32 - makes the head / loss kernel of
// every following catppo_ppo_minibatch_* call write the clip branch each sample took (surrogate codes [0, M), value-loss codes
// [M, 2 M): 0 inside, 1 below, 2 above the clip range; cleanrl/ppo.py:320-341); NULL switches it off.  Costs nothing when off.
extern "C" int catppo_debug_clip_branches(catppo_ctx* ctx, int32_t* buf) {
  if (!ctx) return CATPPO_E_ARG;
  ctx->branch_out = buf;
  return CATPPO_OK;
}

#ifdef STEP16_TL
extern "C" int catppo_debug_step16_tl(void* buf) {     // timeline builds only: not part of include/catppo.h
  unsigned long long* pbuf = static_cast<unsigned long long*>(buf);
  return hipMemcpyToSymbol(HIP_SYMBOL(step16::g_s16tl), &pbuf, sizeof(pbuf)) == hipSuccess ? 0 : -1;
}
#endif

#ifdef FUSED_TL
// timeline builds only (tools/rows_fwd_timeline.py): the training launch of rows_fwd_kernel on its own
extern "C" int catppo_debug_rows_fwd(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* params, const float* x,
                                     int64_t M, int n_layers, void* stream) {
  catppo_mlp_layout L;
  MlpWs w{};
  if (int rc = mlp_prologue(ctx, shape, M, true, &L, &w, __func__)) return rc;
  FusedFwdArgs ra{};
  size_t rlds = 0;
  if (!rows_fwd_plan(shape, L, n_layers, 64, &ra, &rlds)) return CATPPO_E_ARG;
  ra.x = x, ra.params = params, ra.M = M, ra.net0 = 0, ra.do_head = 0;
  for (int net = 0; net < 2; ++net)
    for (int l = 0; l < n_layers; ++l) ra.Hout[net][l] = w.H[net][l];
  rows_launch_train(ra, rlds, 0, M, ctx->n_cu, static_cast<hipStream_t>(stream));
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}
#endif
