/*
 * catppo.h - C ABI of libcatppo.so: the MI355X (gfx950) kernels underneath the
 * CaT + CleanRL-PPO hot path.
 *
 * The reference (Gepetto/constraints-as-terminations) has no FFI: the path sits behind
 * Python interfaces.  Each entry point below replaces a sequence of eager
 * torch ops of the reference; the citation after "replaces:" is the reference location,
 * relative to /root/reference/exts/cat_envs/cat_envs/tasks/utils/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All tensor memory is
 *     caller-owned DEVICE memory (fp32 unless stated), row-major, densely packed unless a
 *     leading dimension `ld*` is given.  The library owns only its workspace.
 *   - every call ENQUEUES on `stream` (a hipStream_t passed as void*) and never
 *     synchronises; no allocation after catppo_create / catppo_reserve.
 *   - return value: 0 = ok, <0 = error (CATPPO_E_*); text via catppo_last_error(ctx).
 *   - a ctx is bound to one device and is not thread-safe (one host thread per ctx,
 *     like the reference's single-threaded loop).
 *   - scalars that the reference computes in Python double and then applies to an fp32
 *     tensor (tau, 1-tau, max_p-min_p, gamma, gamma*lambda) are passed ALREADY ROUNDED to
 *     fp32 by the caller; the kernels use unfused IEEE fp32 (no FMA contraction, correctly
 *     rounded division / sqrt) so that termination masks are bit-exact.
 */
#ifndef CATPPO_H
#define CATPPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CATPPO_VERSION 600 /* 0.6.0: the _ex families collapsed into one entry each (58 exports, 77 in 0.5); the
                              names of ABI <= 0.5 are static inline wrappers in catppo_compat.h */

#define CATPPO_OK 0
#define CATPPO_E_ARG (-1)     /* bad argument */
#define CATPPO_E_HIP (-2)     /* HIP runtime error (launch, alloc) */
#define CATPPO_E_NODEV (-3)   /* no gfx950 device / device index out of range */
#define CATPPO_E_WORKSPACE (-4) /* workspace too small: call catppo_reserve first */
#define CATPPO_E_COMM (-5)    /* RCCL error / communicator not initialised */

/* element types of the buffers that exist in more than one precision (rollout planes, collectives) */
#define CATPPO_F32 0
#define CATPPO_F16 1
#define CATPPO_F64 2

typedef struct catppo_ctx catppo_ctx;

/* ---- lifecycle ------------------------------------------------------------------- */
int catppo_version(void);
/* ABI 0.5: which kernels does a shape get?  enable > 0 starts recording (clears the log), 0 stops, < 0 only reads; returns
 * the text recorded so far: one line per launch decision of catppo_policy_act* / catppo_value* /
 * catppo_ppo_minibatch_grad* / _step_packed (kernel, grid shape, the rule that selected it), written at the decision
 * sites themselves.  tools/explain_plan.py prints it for a (obs_dim, hidden, rows) triple. */
const char* catppo_plan_log(catppo_ctx* ctx, int enable);
int catppo_create(int device, catppo_ctx** out);
void catppo_destroy(catppo_ctx* ctx);
const char* catppo_last_error(catppo_ctx* ctx);
/* make sure the internal workspace holds at least `bytes` (never called implicitly while
 * a stream capture is active; returns CATPPO_E_WORKSPACE from compute calls otherwise). */
int catppo_reserve(catppo_ctx* ctx, uint64_t bytes);

/* ---- CaT: constraints -> termination probability ------------------------------------
 * cstr        [N,K]   constraint values of ALL terms side by side (positive = violated;
 *                     bool terms already converted to 0/1), term t owns the columns
 *                     [term_off[t], term_off[t+1]).
 * term_off    [n_terms+1] int32, HOST array: column offsets, term_off[0]==0, term_off[n_terms]==K
 * term_dp     [n_terms]  fp32, HOST array: fl32(max_p_t - min_p); the curriculum rewrites max_p
 *                        on the host at every reset, so both arrays travel in the kernel arguments
 *                        (n_terms <= 64)
 * rm          [K]     running maxima (state, in/out)
 * reward      [N]     in/out, may be NULL      r <- max(fl(r * fl(1-p)), 0)
 * reset_mask  [N]     uint8/bool, may be NULL  dones[i] = reset ? 1 : p
 * cstr_prob   [N]     out    p_i = max_j prob_ij
 * dones       [N]     out, may be NULL
 * ep_viol     [n_terms,N] in/out   += (max_{j in t} prob_ij > 0)
 * ep_prob     [n_terms,N] in/out   += max_{j in t} prob_ij
 * probs       [N,K]   out, may be NULL (per column probabilities, CaT.probs)
 *
 * replaces: cat/constraint_manager.py:39-82 (CaT.add per term, CaT.get_probs),
 *           :213-229 (ConstraintManager.compute statistics),
 *           cat/cat_env.py:102-107,118-121 (reward scaling, float dones, hard resets).
 */
int catppo_cat_step(catppo_ctx* ctx, const float* cstr, int64_t N, int K,
                    const int32_t* term_off, int n_terms, const float* term_dp,
                    float min_p, float tau, float one_minus_tau, int first_call,
                    float* rm, float* reward, const uint8_t* reset_mask,
                    float* cstr_prob, float* dones, float* ep_viol, float* ep_prob,
                    float* probs, void* stream);

/* Two-phase form for env-sharded runs (a MAX all-reduce of `colmax` goes in between):
 *   catppo_cat_colmax : colmax[j] = max(max_i cstr[i,j], 1e-6)        (:55)
 *   catppo_cat_apply  : running-max EMA from (all-reduced) colmax, then everything else. */
int catppo_cat_colmax(catppo_ctx* ctx, const float* cstr, int64_t N, int K, float* colmax,
                      void* stream);
int catppo_cat_apply(catppo_ctx* ctx, const float* cstr, int64_t N, int K,
                     const int32_t* term_off, int n_terms, const float* term_dp,
                     float min_p, float tau, float one_minus_tau, int first_call,
                     const float* colmax, float* rm, float* reward,
                     const uint8_t* reset_mask, float* cstr_prob, float* dones,
                     float* ep_viol, float* ep_prob, float* probs, void* stream);

/* ConstraintManager.reset: per-term episode statistics of the envs selected by `mask`
 * (uint8/bool [N]; NULL = all envs), then zero their accumulators:
 *   out[2t]   = mean_i(ep_viol[t,i] / len_i) * 100      "Episode_Constraint_violation/<term>"
 *   out[2t+1] = mean_i(ep_prob[t,i] / len_i)            "Episode_Constraint_probability/<term>"
 * If no env is selected `out` receives `prev` (may be NULL: `out` untouched) - the reference keeps the
 * last log dict in env.extras until the next reset.  episode_length: int64 [N] (IsaacLab's
 * episode_length_buf); a zero length gives NaN/inf exactly like the reference's first reset.
 * replaces: cat/constraint_manager.py:190-211. */
int catppo_cat_reset(catppo_ctx* ctx, float* ep_viol, float* ep_prob, const int64_t* episode_length,
                     const uint8_t* mask, int n_terms, int64_t N, const float* prev, float* out, void* stream);

/* Solo12 constraint terms evaluated straight from sim-state tensors into the cstr matrix.
 * `desc` is a host array of n_terms descriptors (see catppo_term_desc).
 * replaces: cat/constraints.py:23-235 (C1..C15). */
enum catppo_term_kind {
  CATPPO_TERM_ABS_LIMIT = 0,      /* |x[:,ids]| - limit                    C1,C3,C4,C5 */
  CATPPO_TERM_ABS_DIFF_LIMIT = 1, /* |x[:,ids]-y[:,ids]| - limit           C11 */
  CATPPO_TERM_ABS_DIFF_LIMIT_GATE_CMDY = 2, /* (|x-y|-limit)*[|cmd_y|<dz]  C2 */
  CATPPO_TERM_GREATER = 3,        /* x[:,col] > limit  (bool -> 0/1)       C6 */
  CATPPO_TERM_CONTACT_ANY = 4,    /* any_b(max_h |F_hb| > thr)             C7 */
  CATPPO_TERM_NORM2_LIMIT = 5,    /* ||x[:, :2]|| - limit                  C8 */
  CATPPO_TERM_AIR_TIME = 6,       /* (limit-last_air)*touchdown*[|cmd|>dz] C9 */
  CATPPO_TERM_N_FOOT_CONTACT = 7, /* |#contacts - n| * [|cmd|>minc]        C10 */
  CATPPO_TERM_ACTION_RATE = 8,    /* |a-a_prev|/dt - limit                 C12 */
  CATPPO_TERM_FORCE_LIMIT = 9,    /* max_h |F_hb| - limit                  C13 */
  CATPPO_TERM_LIMIT_MINUS = 10,   /* limit - x[:,col]                      C14 */
  CATPPO_TERM_ABS_LIMIT_GATE_CMDNORM_LT = 11 /* (|x|-limit)*[|cmd|<dz]     C15 */
};

#define CATPPO_TERM_MAX_IDS 32
typedef struct catppo_term_desc {
  int32_t kind;          /* catppo_term_kind */
  int32_t width;         /* output columns */
  int32_t n_ids;         /* number of joint/body ids used (<= CATPPO_TERM_MAX_IDS) */
  int32_t ids[CATPPO_TERM_MAX_IDS]; /* joint ids, body ids, or ids[0] = column (Solo12: 12 joints, 17 bodies) */
  float limit;           /* limit / threshold */
  float aux;             /* dead-zone / min command / desired feet / step_dt */
  const float* x;        /* primary state tensor (N, x_ld) */
  const float* y;        /* secondary (default_joint_pos, prev_action, first_contact as 0/1) */
  int32_t x_ld, y_ld;
} catppo_term_desc;

/* forces: (N,H,B,3) net_forces_w_history, env i at forces + i*forces_env_stride (= H*B*3 when
 * dense); command: (N,3) with leading dimension command_ld.  Either may be NULL if no term uses
 * it.  cstr [N,K] out, K = sum of widths. */
int catppo_cat_terms(catppo_ctx* ctx, const catppo_term_desc* desc, int n_terms, int64_t N,
                     const float* forces, int64_t forces_env_stride, int H, int B,
                     const float* command, int command_ld, float* cstr, int K, void* stream);

/* catppo_cat_terms + catppo_cat_step in three launches: the term kernel also emits the per-workgroup column
 * maxima, so the CaT step does not re-read cstr for them.  Same arguments as the two calls (n_terms is both
 * the descriptor count and the term count of term_off / term_dp).  Single-process runs only: env-sharded runs
 * need the all-reduce point between catppo_cat_colmax and catppo_cat_apply. */
int catppo_cat_terms_step(catppo_ctx* ctx, const catppo_term_desc* desc, int n_terms, int64_t N,
                          const float* forces, int64_t forces_env_stride, int H, int B, const float* command,
                          int command_ld, float* cstr, int K, const int32_t* term_off, const float* term_dp,
                          float min_p, float tau, float one_minus_tau, int first_call, float* rm, float* reward,
                          const uint8_t* reset_mask, float* cstr_prob, float* dones, float* ep_viol,
                          float* ep_prob, float* probs, void* stream);

/* Env-sharded variant of the same fusion: terms -> cstr plus the local (floored) column maxima in two launches;
 * all-reduce `colmax` with MAX, then catppo_cat_apply. */
int catppo_cat_terms_colmax(catppo_ctx* ctx, const catppo_term_desc* desc, int n_terms, int64_t N,
                            const float* forces, int64_t forces_env_stride, int H, int B, const float* command,
                            int command_ld, float* cstr, int K, float* colmax, void* stream);

/* ---- env-step bookkeeping, fused ------------------------------------------------------------
 * catppo_env_pre_step: process_action (prev <- action, action <- action_in, [N,A]); episode_length += 1;
 *   time_outs = episode_length >= max_episode_length; terminated = hard_reset > 0.5; reset = either;
 *   reward_out = reward_src (the reward manager's output, strided view allowed).  time_outs /
 *   terminated / reset are uint8 (torch.bool) [N].   replaces: cat/cat_env.py:62,92-97.
 * catppo_rollout_store: rewards[step] = reward, dones[step+1] = dones, true_dones[step+1] =
 *   float(time_outs).   replaces: cleanrl/ppo.py:215-216,226. */
int catppo_env_pre_step(catppo_ctx* ctx, const float* action_in, float* action, float* prev_action, int A,
                        int64_t* episode_length, int64_t max_episode_length, const float* hard_reset,
                        int64_t hard_reset_stride, const float* reward_src, int64_t reward_stride,
                        uint8_t* time_outs, uint8_t* terminated, uint8_t* reset, float* reward_out,
                        int64_t N, void* stream);

/* env-sharded exact mode: advantage moments of every minibatch of a (multi-)epoch permutation in one
 * launch, moments[m] = {sum, sum of squares, count} (fp64) over adv[inds[m*mb : (m+1)*mb]]; after ONE
 * SUM all-reduce catppo_adv_stats turns them into {mean, unbiased std + 1e-8} per minibatch, the
 * `adv_stats` input of catppo_ppo_minibatch_grad.   replaces: cleanrl/ppo.py:314-318 across ranks. */
int catppo_adv_stats(catppo_ctx* ctx, const double* moments, int n_minibatches, float* stats, void* stream);
/* the same moments from the per-chunk partial sums catppo_ppo_gather[_ex] already wrote (`adv_part_g`:
 * [n_mb][parts_per_mb][2] fp64, parts_per_mb = ceil(minibatch / 64)) - no index array, any advantage plane
 * precision (the gather widened fp16 exactly).  moments[m] = {sum, sum of squares, rows of minibatch m}. */
int catppo_adv_moments_parts(catppo_ctx* ctx, const double* adv_part_g, int parts_per_mb, int64_t total,
                             int64_t minibatch, double* moments, void* stream);

/* ---- GAE -------------------------------------------------------------------------------
 * time-major (T,N) buffers; float dones in [0,1]; separate time-out mask.
 *   nn = 1-d_{t+1}, tn = 1-td_{t+1}
 *   delta = fl(fl(r_t + fl(fl(fl(gamma*v_{t+1})*nn)*tn)) - v_t)
 *   A_t   = fl(delta + fl(fl(fl(gl*nn)*tn)*A_{t+1})),  ret_t = fl(A_t + v_t)
 * replaces: cleanrl/ppo.py:251-277.  Algorithmic HBM traffic: 24 B per env-step. */

/* The float-done recurrences of the reference's other two trainers, same buffers and launch shape:
 *   CATPPO_GAE_RL_GAMES  rl_games/cat_common.py:96-103 -> rl_games A2CBase.discount_values(fdones float):
 *       the CleanRL recurrence without the time-out channel (true_dones / next_true_done ignored, may
 *       be NULL); gamma_lambda = fl32(gamma*tau).  18 B per env-step.
 *   CATPPO_GAE_SKRL      skrl/ppo.py:397-442 compute_gae with `not_dones = 1 - dones`:
 *       A_t = fl(fl(r_t - v_t) + fl(fl(gamma*(1-d_t)) * fl(v_{t+1} + fl(lambda*A_{t+1}))));
 *       `dones` is indexed at t (not t+1), next_done / true_dones unused (may be NULL) and the
 *       `gamma_lambda` argument carries lambda itself.  18 B per env-step.
 * ONE entry since ABI 0.6: catppo_gae_planes(kind, mode, dtype, ...) - kind as above, mode CATPPO_GAE_SERIAL | _SCAN (below),
 * dtype CATPPO_F32 | CATPPO_F16 = element type of EVERY plane and row (fp16 rollout planes, BASELINE config 5: values are
 * widened to fp32, the recurrence runs in the same fp32 op order, advantages and returns = fl32(A + v) are rounded to half
 * (RNE) when stored; 12 B (CleanRL) / 10 B per env-step).  The scan mode exists for the CleanRL recurrence on fp32 planes. */
typedef enum { CATPPO_GAE_CLEANRL = 0, CATPPO_GAE_RL_GAMES = 1, CATPPO_GAE_SKRL = 2 } catppo_gae_kind;
enum { CATPPO_GAE_SERIAL = 0, CATPPO_GAE_SCAN = 1 };
int catppo_gae_planes(catppo_ctx* ctx, int kind, int mode, int dtype, const void* rewards, const void* values,
                      const void* dones, const void* true_dones, const void* next_value, const void* next_done,
                      const void* next_true_done, float gamma, float gamma_lambda, void* advantages, void* returns,
                      int T, int64_t N, void* stream);

/* skrl whole-batch advantage normalisation (skrl/ppo.py:436): out = (A - mean(A)) / (std_unbiased(A) + 1e-8),
 * moments in fp64 (deterministic); out may alias advantages; stats (NULL ok) receives {mean, std + 1e-8}. */
int catppo_adv_normalize(catppo_ctx* ctx, const float* advantages, int64_t n, float* out, float* stats,
                         void* stream);

/* rl_games `value_bootstrap` (rl_games/cat_common.py:59-64): rewards_i += fl(fl(gamma*values_i) * time_out_i),
 * in place, time_outs as uint8 {0,1}. */
int catppo_value_bootstrap(catppo_ctx* ctx, float* rewards, const float* values, const uint8_t* time_outs,
                           float gamma, int64_t N, void* stream);

/* ---- RunningMeanStd ----------------------------------------------------------------------
 * x [N,D] with leading dimension ldx.  mean/var [D], count [1] fp32 state.
 *   catppo_rms_moments : sums[0:D] = sum_i x, sums[D:2D] = sum_i x^2   (fp64, deterministic)
 *   catppo_rms_merge   : batch mean / biased var from (all-reduced) sums and total row
 *                        count n, then the Chan merge in the reference's fp32 op order
 *   catppo_rms_update  : moments + merge (single GPU)
 *   catppo_rms_normalize: out = (x-mean)/sqrt(var+eps)   (out may alias x)
 * replaces: cleanrl/ppo.py:12-62. */
int catppo_rms_merge(catppo_ctx* ctx, const double* sums, double n, int D, float* mean,
                     float* var, float* count, void* stream);

/* ---- actor-critic MLP ---------------------------------------------------------------------
 * Two independent MLPs (critic then actor, the reference's registration order) with L
 * hidden layers, ELU(alpha=1).  All parameters, gradients and Adam moments live in flat
 * fp32 buffers laid out by catppo_mlp_layout (segments 16-byte aligned, weight matrices
 * 128-byte aligned, first-layer rows padded from D to Dp = round_up(D,16) with zeros; the
 * padding between segments is never read as a parameter and never written by a gradient).
 * replaces: cleanrl/ppo.py:71-123 (Agent), :300-354 (minibatch update). */
#define CATPPO_MAX_HIDDEN 4

typedef struct catppo_mlp_shape {
  int32_t obs_dim;                  /* D  */
  int32_t act_dim;                  /* A  (1..63): A <= 15 runs the 16-slot head kernels (one-launch forwards, step16,
                                       fused last layer); 16..63 the wide heads (64 lanes: A actor outputs + the critic)
                                       behind the layer-wise hidden-layer launches */
  int32_t n_hidden;                 /* L  (1..CATPPO_MAX_HIDDEN) */
  int32_t hidden[CATPPO_MAX_HIDDEN]; /* widths, each a multiple of 64 */
  int32_t mfma_bf16;                /* 0: fp32-input MFMA (reference numerics, default).  1: the hidden-layer GEMMs
                                       (forward, data gradient, weight gradient) round their operands to bf16
                                       (RNE) and use v_mfma_f32_32x32x16_bf16 with fp32 accumulation; parameters,
                                       gradients and the optimiser stay fp32 (BASELINE config 5).  Round 6: from 4096 rows
                                       up the hidden activations and dZ live in the workspace AS bf16 (rounded where they
                                       are produced instead of where a GEMM consumes them: same operands; elu' and the bias
                                       gradients see the rounded values) - CATPPO_ACT16=0 keeps them fp32-stored.
                                       2: split-bf16 ("bf16x3"): every operand is split x = hi + lo (two bf16 values,
                                       16 mantissa bits) and a.b = a_hi.b_hi + a_hi.b_lo + a_lo.b_hi on the bf16
                                       matrix pipe - meets the fp32 parity tolerances at 5x less matrix-pipe time;
                                       finer than the TF32 the reference enables (scripts/clean_rl/train.py:86-87). */
} catppo_mlp_shape;

typedef struct catppo_mlp_layout {
  int32_t obs_pad;                  /* Dp */
  int64_t n_flat;                   /* total floats in the flat buffer (incl. padding) */
  int64_t n_params;                 /* true parameter count (377,241 for the reference) */
  int64_t off_logstd;               /* [A] */
  /* per net (0 = critic, 1 = actor), per layer l = 0..L (L = output layer) */
  int64_t off_w[2][CATPPO_MAX_HIDDEN + 1]; /* [out_l, in_pad_l] row-major */
  int64_t off_b[2][CATPPO_MAX_HIDDEN + 1]; /* [out_l] */
  int32_t in_dim[CATPPO_MAX_HIDDEN + 1];   /* padded input width of layer l */
  int32_t out_dim[2][CATPPO_MAX_HIDDEN + 1];
} catppo_mlp_layout;

int catppo_mlp_layout_of(const catppo_mlp_shape* shape, catppo_mlp_layout* out);

/* workspace bytes needed by the MLP calls for a batch of `rows` samples */
uint64_t catppo_mlp_workspace_bytes(const catppo_mlp_shape* shape, int64_t rows);

/* Rollout policy step (no grad):  x [N,Dp] normalised obs ->
 *   action = mu + exp(logstd)*eps  (eps [N,A] supplied N(0,1) noise; NULL -> action = mu;
 *            given_action [N,A] non-NULL -> that action is scored instead, ppo.py:109-113)
 *   logprob [N], value [N].   replaces: ppo.py:104-119,208-212. */

/* critic only (bootstrap value, ppo.py:252) */

typedef struct catppo_ppo_hparams {
  float clip_coef, ent_coef, vf_coef;
  int32_t norm_adv, clip_vloss;
  float inv_global_batch;   /* 1 / (minibatch size summed over all ranks) */
  /* advantage normalisation statistics: if adv_stats_external != 0 the kernel reads
   * {mean, 1/(std+1e-8)} from adv_stats (device, 2 floats; env-sharded exact mode),
   * otherwise it computes them over this minibatch. */
  int32_t adv_stats_external;
} catppo_ppo_hparams;

/* One minibatch: gather rows `mb_inds` of the flattened rollout buffers, forward both nets,
 * PPO losses, backward.  Writes the flat gradient (same layout as params) and 8 diagnostics
 * {pg_loss, v_loss, entropy, loss, approx_kl, old_approx_kl, clipfrac, 0} which are
 * ACCUMULATED into diag[8] (zeroed by the caller once per iteration).
 *   b_obs [B,Dp], b_actions [B,A], b_logprobs/b_advantages/b_returns_n/b_values_n [B]
 *   mb_inds [M] int64;   value_rms {mean,var} device scalars for newvalue normalisation.
 * replaces: ppo.py:298-352. */
int catppo_ppo_minibatch_grad(catppo_ctx* ctx, const catppo_mlp_shape* shape,
                              const catppo_ppo_hparams* hp, const float* params,
                              const float* b_obs, const float* b_actions,
                              const float* b_logprobs, const float* b_advantages,
                              const float* b_returns_n, const float* b_values_n,
                              const int64_t* mb_inds, int64_t M, const float* vrms_mean,
                              const float* vrms_var, const float* adv_stats, float* grad,
                              float* diag, void* stream);

/* Epoch-level gather: ONE launch copies the samples of a whole permutation into packed buffers so that minibatch
 * m (M samples, the last one possibly shorter) is the contiguous slice
 *   x_g[m*M*Dp ..], act_g[m*M*A ..], scal_g[4*m*M ..] = {old log-prob, advantage, returns_n, values_n}[M_m],
 *   adv_part_g[m*CATPPO_GATHER_PARTS(M)*2 ..] = fp64 {sum, sum of squares} of the advantages per 64-row chunk,
 * and catppo_ppo_minibatch_grad_packed runs forward / losses / backward on such a slice without gathering again
 * (5 gathers per iteration instead of 30).  Same arithmetic and results as catppo_ppo_minibatch_grad. */
#define CATPPO_GATHER_ROWS 64
#define CATPPO_GATHER_PARTS(M) (((M) + CATPPO_GATHER_ROWS - 1) / CATPPO_GATHER_ROWS)
int catppo_ppo_minibatch_grad_packed(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_ppo_hparams* hp,
                                     const float* params, const float* x_mb, const float* act_mb,
                                     const float* scal_mb, const double* adv_part_mb, int64_t M,
                                     const float* vrms_mean, const float* vrms_var, const float* adv_stats,
                                     float* grad, float* diag, void* stream);

/* Global-norm clip + Adam on the flat buffers (after the gradient all-reduce if sharded).
 *   g <- g * min(1, max_norm/(||g||+1e-6));  Adam(beta1,beta2,eps), bias-corrected, `step`
 *   counted from 1.   replaces: ppo.py:353-354 (clip_grad_norm_, optim.Adam.step). */
int catppo_clip_adam(catppo_ctx* ctx, float* params, float* grad, float* exp_avg,
                     float* exp_avg_sq, int64_t n_flat, float max_grad_norm, double lr,
                     double beta1, double beta2, double eps, int64_t step, void* stream);

/* ---- device-resident iteration state --------------------------------------------------------------------
 * Everything that changes from one optimiser step / rollout step / iteration to the next and that a kernel needs
 * (learning rate, Adam step count, RNG counters) lives in ONE small device struct instead of kernel arguments, so
 * that the launches of an iteration are identical from one iteration to the next and can be replayed from a
 * hipGraph (catppo_graph_*), and so that a KL-adaptive schedule can change the learning rate without a host
 * round trip.  The struct is caller-owned device memory (sizeof(catppo_iter_state) bytes); only the library's
 * kernels write it. */
typedef struct catppo_iter_state {
  uint64_t seed;      /* key of the counter-based RNG (Philox4x32-10 action noise, minibatch permutation) */
  int64_t iteration;  /* 1-based PPO iteration, incremented by catppo_iter_begin */
  int64_t adam_step;  /* optimiser steps taken, incremented by catppo_clip_adam_dev */
  double lr;          /* learning rate used by catppo_clip_adam_dev */
  double kl_mark;     /* diag[4] (approx-KL sum) at the last catppo_kl_adaptive_lr of this iteration */
  double n_mark;      /* diag[7] (minibatch count) at that point */
  double last_kl;     /* KL the schedule last saw (diagnostics) */
  float adam_step_size;  /* lr / (1 - beta1^step) of the step catppo_clip_adam_dev is taking (written by its first launch, */
  float adam_bc2_sqrt;   /* sqrt(1 - beta2^step)                      read by its second; scratch, not an input)     */
} catppo_iter_state;

/* state <- {seed, iteration 0, adam_step 0, lr} */
int catppo_iter_init(catppo_ctx* ctx, catppo_iter_state* state, uint64_t seed, double lr, void* stream);
/* start of an iteration: iteration += 1, KL marks <- 0, and the learning-rate schedule
 *   CATPPO_LR_FIXED   lr = lr0
 *   CATPPO_LR_LINEAR  lr = (1 - (iteration-1)/num_iterations) * lr0   in double, the reference's expression
 *                     (cleanrl/ppo.py:196-199)
 *   CATPPO_LR_KEEP    lr unchanged (it is driven by catppo_kl_adaptive_lr) */
enum { CATPPO_LR_FIXED = 0, CATPPO_LR_LINEAR = 1, CATPPO_LR_KEEP = 2 };
int catppo_iter_begin(catppo_ctx* ctx, catppo_iter_state* state, double lr0, int64_t num_iterations, int schedule,
                      void* stream);

/* catppo_clip_adam with lr and the step count taken from (and the step count advanced in) the device state.
 * Same arithmetic: the bias corrections 1-beta^step are evaluated in double on the device. */
int catppo_clip_adam_dev(catppo_ctx* ctx, float* params, float* grad, float* exp_avg, float* exp_avg_sq,
                         int64_t n_flat, float max_grad_norm, double beta1, double beta2, double eps,
                         catppo_iter_state* state, void* stream);

/* ABI 0.4: one optimiser step of a single process in ONE call = catppo_ppo_minibatch_grad_packed followed by
 * catppo_clip_adam_dev (same arguments, same results up to the summation order of the fp64 squared norm), for callers
 * with nothing to do between the two - no gradient all-reduce.  The workgroups that fold the split-K partials into the
 * flat gradient also emit the sum of squares of what they write, so the clip needs no launch that re-reads the
 * gradient: one launch fewer per step (7 instead of 8 at 16384 x 3 x 256).
 * replaces: cleanrl/ppo.py:298-356 (minibatch losses, backward, clip_grad_norm_, optimizer.step) of a non-distributed run. */
int catppo_ppo_minibatch_step_packed(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_ppo_hparams* hp,
                                     float* params, const float* x_mb, const float* act_mb, const float* scal_mb,
                                     const double* adv_part_mb, int64_t M, const float* vrms_mean,
                                     const float* vrms_var, const float* adv_stats, float* grad, float* diag,
                                     float* exp_avg, float* exp_avg_sq, float max_grad_norm, double beta1, double beta2,
                                     double eps, catppo_iter_state* state, void* stream);

/* KL-adaptive learning rate, device side (no host sync).  Two calls so that an env-sharded run can put its
 * all-reduce between them:
 *   catppo_kl_mean        kl_out[0] = (diag[4] - kl_mark) / (diag[7] - n_mark): the mean approx-KL of the minibatches
 *                         processed since the previous call of this iteration (the marks then advance).  With
 *                         inv_global_batch = 1/(M*world) in the minibatch calls the per-rank values SUM to the
 *                         global mean, which is what skrl's all_reduce(kl, SUM)/world_size computes.
 *   catppo_kl_adaptive_lr kl > threshold*kl_factor : lr = max(lr / lr_factor, min_lr)
 *                         kl < threshold/kl_factor : lr = min(lr * lr_factor, max_lr)
 * replaces: skrl/ppo.py:558-567 (scheduler.step(kl) after the KL all-reduce) with skrl's published KLAdaptiveLR rule
 * (kl_factor 2, lr_factor 1.5, min_lr 1e-6, max_lr 1e-2; threshold skrl_ppo_cfg.yaml:49-51 = 0.01) - rl_games'
 * `lr_schedule: adaptive` (rl_games_cat_solo.yaml:64-66, kl_threshold 0.008) is the same rule.  Neither library
 * is vendored in the reference: the rule itself is PARITY UNPINNED, the call site and the reduction are pinned. */
int catppo_kl_mean(catppo_ctx* ctx, catppo_iter_state* state, const float* diag, float* kl_out, void* stream);
int catppo_kl_adaptive_lr(catppo_ctx* ctx, catppo_iter_state* state, const float* kl, double kl_threshold,
                          double kl_factor, double lr_factor, double min_lr, double max_lr, void* stream);

/* ---- rollout forward: policy step + value (ONE entry since ABI 0.6) ------------------------------------------------
 * catppo_policy_step: both networks' forward on x [N, Dp] + the Gaussian head (replaces Agent.get_action_and_value /
 * get_value, cleanrl/ppo.py:104-119,186-189; the bootstrap value of :251 is the critic-only form, action == NULL).
 * Where the action comes from - exactly one of:
 *   eps          supplied N(0,1) noise [N, A]: a = mu + sigma * eps (Normal.sample(), cleanrl/ppo.py:111)
 *   state, step  on-device noise: Philox4x32-10 + Box-Muller inside the head kernel; element (env i, dim k) of rollout
 *                step `step` of iteration state->iteration uses counter {i, k/4, step, iteration}, key = state->seed,
 *                lane k%4 of the block (independent of A: dimension k draws the same noise at every action width);
 *                eps_out ([N, A], may be NULL) receives it, so a parity test can replay it
 *   given_action evaluate these actions (log-prob / value of stored actions)
 * value_dtype: CATPPO_F32, or CATPPO_F16 to store `value` as IEEE half (fp16 rollout planes).
 * Kernels by batch size (catppo_plan_log names them): <= 2048 rows step16_fwd_kernel (16-row tiles), 2049-4096 the 32-row
 * row-resident kernels, else layer-wise GEMM launches + head_act_kernel.  act_dim >= 16: always the layer-wise hidden-layer
 * launches (fp32-stored, or bf16-stored in the bf16-operand mode from 4096 rows) + head_act_wide_kernel, the critic-only
 * form included (its values equal the full call's bit for bit); the optimiser step of such a shape runs the layer-wise
 * forward + head_loss_wide_kernel in place of head_loss_kernel. */
int catppo_policy_step(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* params, const float* x, int64_t N,
                       const float* eps, const float* given_action, const catppo_iter_state* state, int32_t step,
                       float* eps_out, float* action, float* logprob, void* value, int value_dtype, void* stream);

/* The epoch gather (one launch for every minibatch of an epoch: minibatch m = contiguous slice m of the packed buffers)
 * with (a) either an index array `inds` (state == NULL) or a permutation computed on the fly
 * (inds == NULL; replaces torch.randperm, cleanrl/ppo.py:295): sample j of the epoch reads row P(j), P = a keyed
 * bijection of [0,total) (6-round Feistel network on the next power of four with cycle walking, round keys from
 * Philox(seed; iteration, epoch)) - no index array, no sort; inds_out ([total] int64, may be NULL) receives P for
 * parity tests - and (b) adv_dtype: element type of b_advantages (CATPPO_F16 for fp16 rollout planes; widened on
 * the way into the packed buffers). */
int catppo_ppo_gather_ex(catppo_ctx* ctx, const catppo_mlp_shape* shape, const float* b_obs, const float* b_actions,
                         const float* b_logprobs, const void* b_advantages, int adv_dtype, const float* b_returns_n,
                         const float* b_values_n, const int64_t* inds, const catppo_iter_state* state, int32_t epoch,
                         int64_t total, int64_t M, float* x_g, float* act_g, float* scal_g, double* adv_part_g,
                         int64_t* inds_out, void* stream);
/* ABI 0.5: the moments of ALL `n_epochs` keyed permutations of an iteration (catppo_ppo_gather_ex with `state`) in one
 * call, before the first gather: moments[(e * n_mb + m)] = {sum, sum of squares, rows} of minibatch m of epoch e, so an
 * env-sharded run exchanges the advantage statistics of an iteration with ONE all-reduce instead of one per epoch.
 * `parts_scratch`: n_epochs * n_mb * ceil(minibatch / 64) * 2 doubles.  Chunking and summation order are the
 * gather's: bit-identical to catppo_adv_moments_parts on the partials of the epoch's own gather.  `advantages`: the
 * (total,) plane, CATPPO_F32 or CATPPO_F16.   replaces: cleanrl/ppo.py:314-318 across ranks and epochs. */
int catppo_adv_moments_keyed(catppo_ctx* ctx, const void* advantages, int adv_dtype, const catppo_iter_state* state,
                             int32_t n_epochs, int64_t total, int64_t minibatch, double* parts_scratch,
                             double* moments, void* stream);

/* ---- fp16 rollout planes (BASELINE config 5) ------------------------------------------------------------------
 * catppo_rollout_store_ex: catppo_rollout_store with the three destination rows in `dtype`.
 * catppo_rms_moments_ex / _update_ex / _normalize_ex: RunningMeanStd over an input of `x_dtype` (widened exactly;
 * statistics, state and output stay fp32). */
int catppo_rollout_store_ex(catppo_ctx* ctx, const float* reward, const float* dones, const uint8_t* time_outs,
                            void* rewards_t, void* dones_t1, void* true_dones_t1, int dtype, int64_t N, void* stream);
int catppo_rms_moments_ex(catppo_ctx* ctx, const void* x, int x_dtype, int64_t N, int D, int64_t ldx, double* sums,
                          void* stream);
int catppo_rms_update_ex(catppo_ctx* ctx, const void* x, int x_dtype, int64_t N, int D, int64_t ldx, float* mean,
                         float* var, float* count, void* stream);
int catppo_rms_normalize_ex(catppo_ctx* ctx, const void* x, int x_dtype, int64_t N, int D, int64_t ldx,
                            const float* mean, const float* var, float eps, float* out, int64_t ldo, void* stream);

/* ---- GAE scan mode -----------------------------------------------------------------------------------------------
 * mode CATPPO_GAE_SERIAL : one lane per env walks t = T-1..0 (catppo_gae_ex; bit-exact with the reference loop).
 * mode CATPPO_GAE_SCAN   : the time axis of an env is split over the 2^k lanes of a lane group; every lane composes
 *   the affine maps A -> delta_t + c_t * A of its chunk, the group combines them with a wavefront-shuffle suffix
 *   scan, then every lane replays its chunk from the incoming value.  Fills the chip at small N (4096 envs: 64 waves
 *   serial, up to 1024 in scan mode); the composition reassociates the recurrence, so results agree with the serial
 *   mode to ~1e-6 relative (tests hold 1e-5), not bit for bit.  CleanRL recurrence (kind 0), fp32 planes. */
/* ---- fused rollout step ------------------------------------------------------------------------------------------
 * Everything between the simulator's state update and the next policy forward, in TWO launches instead of ten:
 *   launch 1 (16-env tiles)  process_action, episode counters, terminations, reward pick-up (catppo_env_pre_step);
 *                            all constraint terms -> cstr (catppo_cat_terms); per-workgroup column maxima and fp64
 *                            observation moments; the last workgroup to finish folds them (fixed order) into
 *                            xchg = {colmax[K] floored at 1e-6 | sum x [D] | sum x^2 [D]}
 *   [env-sharded: MAX / SUM all-reduce of xchg here]
 *   launch 2 (32-env tiles)  running-max EMA, probabilities, per-env / per-term maxima, episode statistics, reward
 *                            scaling, float dones (catppo_cat_apply); ConstraintManager.reset statistics of the envs
 *                            that reset + zeroing (catppo_cat_reset), episode_length / action history reset;
 *                            rollout-buffer rows (catppo_rollout_store); Chan merge of the observation normaliser
 *                            and normalised observation row obs[step+1] (catppo_rms_update + _normalize).  Every
 *                            workgroup derives the new running maxima / normaliser state redundantly from xchg; the
 *                            last one to finish writes them back and folds the reset statistics into `log_out`.
 * Same arithmetic and results as the separate calls (bit-exact: CaT, rewards, dones, statistics; normaliser: same
 * fp64 sums folded in a different fixed order, <= 1 ulp of the fp32 state). */
typedef struct catppo_rollout_step {
  /* sizes */
  int64_t N;
  int32_t A, D, K, n_terms;
  /* pre-step (catppo_env_pre_step) */
  const float* action_in; float* action; float* prev_action;
  int64_t* episode_length; int64_t max_episode_length;
  const float* hard_reset; int64_t hard_reset_stride;
  const float* reward_src; int64_t reward_stride;
  uint8_t* time_outs; uint8_t* terminated; uint8_t* reset; float* reward;
  /* constraint terms (catppo_cat_terms) */
  const catppo_term_desc* desc;       /* HOST array [n_terms] */
  const float* forces; int64_t forces_env_stride; int32_t H, B;
  const float* command; int32_t command_ld;
  float* cstr;
  /* CaT (catppo_cat_apply) */
  const int32_t* term_off; const float* term_dp;   /* HOST arrays */
  float min_p, tau, one_minus_tau; int32_t first_call;
  float* rm; float* cstr_prob; float* dones; float* ep_viol; float* ep_prob; float* probs;
  /* ConstraintManager.reset statistics: log_out[2*n_terms] <- means over the envs that reset (log_prev if none) */
  const float* log_prev; float* log_out;
  int32_t zero_action_on_reset;
  /* rollout rows */
  void* rewards_t; void* dones_t1; void* true_dones_t1; int32_t plane_dtype;
  /* observation normaliser + next observation row */
  const float* obs_raw; int64_t obs_ld;
  float* obs_mean; float* obs_var; float* obs_count; float obs_eps; double obs_rows_total;
  float* obs_out; int64_t obs_out_ld;
  /* exchange buffer, device: K floats (as doubles' storage is separate) - see catppo_rollout_xchg_layout */
  void* xchg;
  /* env-sharded, ONE collective per env step (ABI 0.3): catppo_rollout_pre writes this rank's record into `xchg`; the
   * caller all-gathers the records of all ranks (catppo_allgather, `bytes` of catppo_rollout_xchg_layout each, rank order) into
   * `xchg_gathered`, and catppo_rollout_post folds them itself - column maxima by MAX (exact), moment sums in rank order
   * (identical on every rank).  xchg_records = number of records (0 / 1: read `xchg`, e.g. after MAX / SUM all-reduces). */
  const void* xchg_gathered;
  int32_t xchg_records;
  /* ABI 0.4: the simulator's state advance inside catppo_rollout_pre.  A simulator whose new state already exists as
   * one contiguous [N, sim_row_bytes] block somewhere else (here: the synthetic stream's next slab; the reference's
   * `scene.update`, cat/cat_env.py:60-90, is that copy) hands it over as `sim_src`: every input of THIS call that points
   * into the state block [sim_state, sim_state + N * sim_row_bytes) - term tensors, forces, command, hard_reset,
   * reward_src, obs_raw - is read from `sim_src` at the same offset, and the launch copies the rows to `sim_state`
   * (each workgroup its own envs), so that after it every view of the state block is current (catppo_rollout_post and
   * everybody else read it as before).  One launch and a 5 us copy kernel less per env step.  sim_src == NULL: the
   * caller has updated the state block itself.  sim_row_bytes % 16 == 0. */
  const void* sim_src; void* sim_state; int64_t sim_row_bytes;
} catppo_rollout_step;
/* bytes of one exchange record and the byte offset of its fp64 sums (K constraint columns, D observation width) */
int catppo_rollout_xchg_layout(int K, int D, uint64_t* bytes, uint64_t* sum_offset);
uint64_t catppo_rollout_step_sizeof(void);   /* sizeof(catppo_rollout_step): lets a binding check its struct layout */
/* phase 1 (two launches: the per-tile kernel and the fold of its partial rows into `xchg`) and phase 2 (one launch); call
 * both back to back on one GPU; all-reduce xchg in between when env-sharded:
 * floats [0,K) with MAX, doubles at byte offset `sum_offset` of catppo_rollout_xchg_layout [2*D] with SUM) */
int catppo_rollout_pre(catppo_ctx* ctx, const catppo_rollout_step* a, void* stream);
int catppo_rollout_post(catppo_ctx* ctx, const catppo_rollout_step* a, void* stream);
/* ABI 0.5: the tail of catppo_rollout_post - ONE workgroup that, after all others, publishes the new running maxima (rm)
 * and observation-normaliser state (obs_mean / obs_var / obs_count) and folds the reset statistics into log_out - off the
 * chain forward -> pre -> fold -> post -> forward of an env step.  With on = 1 a post launch ends without that tail (and
 * without the "last workgroup arrives" hand-shake in front of it); the tail runs as one more workgroup of the NEXT
 * catppo_rollout_pre launch on the same stream (nothing in between reads what it writes: the policy forward consumes
 * obs_out, the simulator its own state), or as a launch of its own from catppo_rollout_defer_tail(ctx, -1, stream) (flush,
 * the mode stays) / the next catppo_rollout_post / catppo_rollout_defer_tail(ctx, 0, stream).  CONTRACT while on: rm, obs_mean, obs_var, obs_count
 * and log_out of a step are valid (in stream order) only after one of those calls; every other output of the step is
 * valid after catppo_rollout_post as before.  Values are bit-identical either way: the tail derives the state with the same
 * device functions from the same exchange record(s) - which must stay untouched until then (they are: the next writer is
 * the fold behind the next catppo_rollout_pre / the next all-gather).  The rollout loop of cleanrl/ppo.py's PPOTrainer
 * switches it on around its env steps and off (= flush) before GAE.  One stream per context while it is on: the pending
 * tail and its reset-statistics rows belong to the context; a call that flushes the tail from ANOTHER stream is ordered
 * behind the tail's launch by an event (round 6).  Reference: the statistics concerned are
 * ConstraintManager's running maxima (cat/constraint_manager.py:58-61), RunningMeanStd's state (cleanrl/ppo.py:48-62)
 * and the episode log of ConstraintManager.reset (cat/constraint_manager.py:190-211).
 *
 * on = 2 (env step in three launches): deferred tail as with 1, and catppo_rollout_post itself launches NOTHING - it
 * records its argument block in the context (a step with obs_raw; the caller's all-reduce / all-gather of the exchange
 * record has been enqueued by then, as before).  The next catppo_policy_step of that context carries the step in its
 * own launch (step_fwd_kernel: every workgroup of the 32-row forward normalises its observation rows from the raw rows
 * straight into its LDS tile, the critic workgroup of a tile does the step's bookkeeping behind its value head) when it
 * continues the step: same stream, same N, x == obs_out with obs_out_ld == the padded observation width, a shape and a
 * row count the 32-row forward rows_fwd_kernel<32> takes (fp32, every hidden layer 256 wide, act_dim < 16, 2049..4096
 * rows unless the window is overridden), eps / state noise or the critic-only form (no given_action), K <= 64 constraint
 * columns, D <= 128, and head outputs that are none of the step's buffers.  Anything else - another size or shape,
 * bf16 or wide heads, given_action, another catppo_rollout_pre / _post, any catppo_rollout_defer_tail call (-1 included)
 * - first launches the recorded step as the rollout_post_kernel launch it would have been, on the stream it was recorded
 * for, and then proceeds as without it.  CONTRACT while on = 2: NO output of a step (obs_out, reward, dones, the
 * rollout-buffer planes, episode statistics; and, as with 1, rm / normaliser state / log_out) is valid before the next
 * catppo_policy_step or one of those calls; nothing the step reads may be written in between.  Results are bit-identical
 * in every mode.  PPOTrainer.rollout arms it beside the tail deferral and flushes in its `finally`. */
int catppo_rollout_defer_tail(catppo_ctx* ctx, int on, void* stream);    /* on: 1 | 2 | 0 (= off + flush) | -1 (flush only) */

/* ---- rl_games front end: episode bookkeeping with float dones ---------------------------------------
 * One env step of CaTA2CAgent.play_steps' bookkeeping (rl_games/cat_common.py:71-92), one launch, no host sync:
 *   current_rewards += rewards; current_shaped_rewards += shaped_rewards; current_lengths += 1
 *   done_i = dones_i >= 1.0;  the three AverageMeters are updated with current_*[done]
 *   current_rewards *= (1 - dones); current_shaped_rewards *= (1 - dones)   (FLOAT not_dones);  current_lengths[done] = 0
 * rewards / shaped_rewards / current_*rewards: [N, value_size]; dones, current_lengths: [N] (fp32, rl_games keeps the
 * lengths in fp32); done_mask_out: optional [N] bytes (what `dones.ge(1.0)` was), for an observer that wants indices.
 * catppo_rlg_meters (device memory, initialised by catppo_rlg_meters_init) restates rl_games' torch_ext.AverageMeter
 * (rl_games 1.6.1 is not vendored in the reference tree: published rule, parity unpinned against rl_games itself):
 *   update(values): n = rows; if n == 0 return; new_mean = mean(values); size = min(n, max_size);
 *                   old = min(max_size - size, current_size); current_size = old + size;
 *                   mean = (mean * old + new_mean * size) / (old + size)                                            */
#define CATPPO_RLG_MAX_VALUE_SIZE 4
typedef struct catppo_rlg_meters {
  float mean_rewards[CATPPO_RLG_MAX_VALUE_SIZE];
  float mean_shaped_rewards[CATPPO_RLG_MAX_VALUE_SIZE];
  float mean_lengths;
  int32_t size_rewards, size_shaped, size_lengths;   /* AverageMeter.current_size */
  int32_t max_size;                                   /* games_to_track */
  int32_t last_done_count;                            /* episodes that ended in the latest step */
} catppo_rlg_meters;
int catppo_rlg_meters_init(catppo_ctx* ctx, catppo_rlg_meters* meters, int max_size, void* stream);
int catppo_rlg_episode_step(catppo_ctx* ctx, const float* rewards, const float* shaped_rewards, const float* dones,
                            int value_size, float* current_rewards, float* current_shaped_rewards,
                            float* current_lengths, int64_t N, catppo_rlg_meters* meters, uint8_t* done_mask_out,
                            void* stream);

/* ---- HIP graphs ------------------------------------------------------------------------------------------------
 * Capture every launch the library (or anything else) enqueues on `stream` between begin and end into a hipGraph,
 * instantiate it, and replay it with one call.  `stream` must not be the legacy default stream.  No library call
 * allocates or synchronises while a capture is active (catppo_reserve returns CATPPO_E_ARG then). */
int catppo_graph_begin(catppo_ctx* ctx, void* stream);
/* graph_id == NULL: end the capture WITHOUT keeping its graph (error path: something between begin and end failed, the
 * partial graph must never be replayed); a no-op when no capture is active */
int catppo_graph_end(catppo_ctx* ctx, void* stream, int* graph_id, int* n_nodes);
int catppo_graph_launch(catppo_ctx* ctx, int graph_id, void* stream);
int catppo_graph_destroy(catppo_ctx* ctx, int graph_id);
/* ---- collectives (RCCL over xGMI, one process per GPU) ---------------------------------------------------------
 * librccl is loaded at run time (dlopen) by the first of these calls; the library has no link-time dependency on it.
 * catppo_comm_unique_id: rank 0 creates the id (128 bytes) and ships it to the other ranks by any means (the host
 * code here uses the launcher's rendezvous store); every rank then calls catppo_comm_init.  The collectives are
 * in place, enqueue on `stream`, are capturable in a hipGraph, and reduce `count` elements of `dtype`
 * (CATPPO_F32 / CATPPO_F64).   semantics replaced: skrl/ppo.py:126-131 (parameter broadcast), :534-537 (gradient
 * reduction), :562-564 (KL all-reduce); the CleanRL path of the reference has no collective. */
enum { CATPPO_SUM = 0, CATPPO_MAX = 1 };
#define CATPPO_UNIQUE_ID_BYTES 128
/* ctx == NULL: can this process use the collectives at all (librccl loadable, every entry point present: CATPPO_OK /
 * CATPPO_E_COMM)?  No communicator, no bootstrap thread: what every rank checks BEFORE anybody enters the blocking
 * catppo_comm_init.  ctx != NULL: the world size of its communicator (>= 1), 0 = none. */
int catppo_comm_probe(catppo_ctx* ctx);
int catppo_comm_unique_id(uint8_t* out128);
int catppo_comm_init(catppo_ctx* ctx, int rank, int world, const uint8_t* unique_id128);
int catppo_comm_destroy(catppo_ctx* ctx);
int catppo_allreduce(catppo_ctx* ctx, void* buf, int64_t count, int dtype, int op, void* stream);
int catppo_broadcast(catppo_ctx* ctx, void* buf, int64_t count, int dtype, int root, void* stream);
/* recv[rank * bytes ...] = send of that rank, for every rank (ncclAllGather of raw bytes; send != recv) */
int catppo_allgather(catppo_ctx* ctx, const void* send, void* recv, int64_t bytes, void* stream);

/* ---- ABI 0.4: gradient all-reduce in per-layer buckets, overlapped with the backward pass ------------------------
 * semantics replaced: skrl/ppo.py:534-537 (every gradient reduced after backward()).  With the switch on AND a
 * communicator present, catppo_ppo_minibatch_grad / _packed fold the partials of hidden layer l (and, with the last
 * hidden layer, the heads and log-std) as soon as that layer's weight-gradient launch is enqueued - on the context's
 * side stream - and SUM-all-reduce that bucket of the flat gradient there, while the launches of the layers below
 * still run on `stream`; the side stream joins `stream` before the call returns its stream order, so `grad` is the
 * GLOBAL sum when the next operation on `stream` (catppo_clip_adam*) reads it and the caller must NOT all-reduce it
 * again.  Sums per element are those of the single fold launch (bit-identical on a world of one); the whole sequence
 * is capturable.  catppo_set_grad_overlap(ctx, -1) queries: 1 when the next gradient call will reduce the gradient itself. */
/* ABI 0.5: on == 2 selects the "tail" form - NO extra launch: once the launch that folds every layer above the first is
 * enqueued (dw_fold_kernel), those ranges of the flat gradient are all-reduced on the side stream under the final fold
 * launch of the first layer's own partials, which are reduced on the caller's stream behind a join.  Measured on a world of
 * one: see profiles/r5_grad_overlap_tail_world1.txt. */
int catppo_set_grad_overlap(catppo_ctx* ctx, int on);      /* on: 0 | 1 | 2 set (CATPPO_OK), -1 query (0 / 1) */

/* ---- Solo12 servo surrogate: a closed-loop stand-in simulator on the device -----------------------
 * One control step of N envs in one launch: (state row, action, command) -> next state row, for the packed sim-state
 * block the CaT env reads (cat_envs/tasks/utils/cat/cat_env.py, Solo12ServoSim).  Not physics: 12 clamped PD servo
 * joints integrated over `decimation` substeps, base velocity / roll / pitch as first-order lags of fixed joint
 * combinations, feet, contact forces and air times from the knee offsets, commands and first poses from Philox4x32-10
 * keyed on (seed; global env id, episode, resample index).  fp32, unfused, only + - * / sqrt min max abs compares and
 * selects, every reduction in a fixed order: tests/servo_twin.py restates it bit for bit in numpy.
 * A row is `row_floats` floats (multiple of 4; rows 16-byte aligned, `row_stride` floats apart); off_* are float
 * offsets into it.  off_servo names 14 floats of private state: v[3] | roll pitch | air[4] | contact[4] | episode.
 * reset[i] != 0: env i ended its episode in the previous step; the kernel then starts from the first state of the
 * episode in its row (re-derived from the counter) instead of the row.  A step that ends an episode (episode_length + 1
 * >= max_episode_length, or the model's own hard_reset) writes the terminal state, but its `obs` already shows the
 * first state of the next episode.  init != 0: write the first state of episode 0 (no integration; action and reset
 * are not read).  state_in and state_out are different buffers unless init.  Enqueues on `stream`, never allocates,
 * never synchronises.
 * fixed_command != NULL: env i's command is fixed_command[3 i .. 3 i + 2] in every step and every episode (the step's
 * command, the init row, the post-reset observation); no dead zone, no standing fraction - the table is the command.
 * eval != NULL: a per-env evaluation record of CATPPO_SERVO_EVAL_FLOATS fp32 sums, read, updated and written back by
 * the launch of every step (one unfused add per field and step, the kernel's own values of that step) and set to zero
 * by an init launch:  0 steps | 1 episodes ended | 2 falls (hard_reset) | 3 reward (raw) | 4 (cx - vx)^2 + (cy - vy)^2 |
 * 5 (cw - wz)^2 | 6 roll^2 + pitch^2 | 7 tree16 of applied_torque^2 | 8 feet in contact | 9 return of the running
 * episode (zero after the step that ends it) | 10 returns of the ended episodes | 11 lengths of the ended episodes.
 * Both NULL: the launch computes what it did before the two fields existed, bit for bit.  Neither may alias a state
 * buffer; the record never changes a float of the state row.
 * Step responses (trailing fields; a zero-filled tail is the behaviour described so far, exactly).
 * fixed_segments = S > 1: fixed_command is a schedule [S, N, 3].  A step that starts at episode length t uses row
 * min(t / fixed_segment_steps, S - 1) of env i; the same index serves the init row (t = the env's episode_length, zero in
 * an evaluation) and the post-reset observation (t = 0, segment 0).  The schedule is keyed on the episode length, like
 * command resampling: an episode that ends restarts its schedule.  No dead zone, no standing fraction.  S of 0 or 1 reads
 * [N, 3].  S > 1 needs fixed_segment_steps >= 1 and a table; S < 0 is an error.
 * trace != NULL ([trace_capacity, trace_envs, CATPPO_SERVO_TRACE_FLOATS] fp32, 16-byte aligned, zeroed by the caller):
 * every step writes one row for each of the envs 0 .. trace_envs - 1 of this simulator, at the slot that field 0 of the
 * env's evaluation record (steps counted so far) held before the step - no host counter, so it survives graph capture,
 * and it needs eval != NULL.  A step whose slot is >= trace_capacity writes nothing, and neither does an init launch.
 * Needs 1 <= trace_envs <= N and trace_capacity >= 1; may alias none of state_in, state_out, eval, fixed_command.
 * Row:  0 t (episode length the step started from) | 1 ends | 2 fallen | 3 reward (raw) | 4..6 the step's command |
 * 7..9 vx vy wz after the step | 10 roll | 11 pitch | 12 base height z | 13 feet in contact | 14 15 zero |
 * 16..19 contact flag per foot | 20..23 fz per foot | 24..35 q | 36..47 qd | 48..59 tau_w (applied_torque) |
 * 60..71 the action of this step.  The trace never changes a float of the state row or of the record.
 * Rewards (trailing fields after trace_capacity; a zero-filled tail is the behaviour described so far, exactly).
 * reward_terms = T in 1 .. CATPPO_SERVO_REWARD_MAX_TERMS: the row's off_reward field receives the sum of the T terms of
 * reward_table instead of the built-in expression - in table order k = 0 .. T - 1, value_k = (raw_k * weight_k) * step_dt
 * (two rounded fp32 multiplies, step_dt = dt * (float)decimation; IsaacLab's func * weight * dt) and reward = reward +
 * value_k from 0.f, unfused.  reward_table is a device array of T entries, 16-byte aligned, read by every launch (a weight
 * the host writes into it, in stream order, is in the next launch; by value the table would have grown the kernel
 * arguments past the size at which the compiler keeps the code of the launches without rewards as it was).  T = 0: the
 * built-in reward.  The evaluation record's field 3 (and 9, 10) and the trace's field 3 keep the built-in tracking
 * expression whatever T is: a fixed score, comparable across reward configurations.
 * raw by kind (symbols of csrc/servo_sim.hip; ex ey ew = command - velocity after the step; m = bit `lane` of joint_mask
 * as 0 / 1; tree16, tree4: the kernel's orders):
 *  1 expf(0 - (ex ex + ey ey) / param)       2 expf(0 - (ew ew) / param)         [param = std^2]
 *  3 1 / (1 + (ex ex + ey ey) / param)       4 1 / (1 + (ew ew) / param)
 *  5 ang0^2 + ang1^2                         6 g0^2 + g1^2 (after the roll-over override)
 *  7 tree16(m tau_w^2)    8 tree16(m acc^2), acc = tau_w / inertia    9 tree16(m qd^2)    10 tree16(m |q - default|)
 * 11 tree16((a - a_prev)^2), a_prev = state_in[off_obs + 33 + lane], 0 for an env that starts an episode: obs_dim >= 45
 * 12 tree16(a^2)         13 tree4((last_air - param) touch) * (sqrtf(cx cx + cy cy) > 0.1f)       14 (z - param)^2
 * 15 fallen ? 1 : 0      16 fallen ? 0 : 1
 * Kinds 1 - 4 need param > 0, kinds 7 - 10 a joint_mask in 1 .. 0xFFF, kind 11 obs_dim >= 45: the table is device memory,
 * so its writer checks the entries (Solo12ServoSim.set_reward_table); the entry point checks T, the record and the table
 * pointer.  Whatever the table holds the launch stays inside its buffers: an unknown kind contributes raw = 0, kind 11
 * with obs_dim < 45 reads a_prev = 0.
 * reward_rec ([N, CATPPO_SERVO_REWARD_FLOATS] fp32, 16-byte aligned, required when T > 0; may alias none of state_in,
 * state_out, eval, trace, fixed_command): floats 0 .. 14 the sums of the running episode per term, 16 .. 30 the sums of
 * the ended episodes per term since the caller last zeroed them, 31 the count of ended episodes, 15 zero.  Per step
 * s = rec[k] + value_k (one fp32 add); a step that ends the episode does rec[16 + k] += s, rec[k] = 0, rec[31] += 1, any
 * other rec[k] = s.  An init launch zeroes the whole record.  No atomics, no communication between envs. */
#define CATPPO_SERVO_EVAL_FLOATS 12
#define CATPPO_SERVO_TRACE_FLOATS 72
#define CATPPO_SERVO_REWARD_FLOATS 32
#define CATPPO_SERVO_REWARD_MAX_TERMS 15
typedef struct catppo_servo_reward_term {
  int32_t kind;
  uint32_t joint_mask;
  float weight, param;
} catppo_servo_reward_term;
typedef struct catppo_servo_sim {
  int64_t N, env_offset;                 /* env_offset: global env id of row 0 (env-sharded runs) */
  const float* state_in;
  float* state_out;
  int64_t row_stride;
  int32_t row_floats, obs_dim, H, B;     /* force history depth, bodies (17: base + 4 x {shoulder, upper, lower, foot}) */
  int32_t off_joint_pos, off_joint_vel, off_joint_acc, off_applied_torque, off_projected_gravity, off_root_pos,
      off_command, off_last_air_time, off_first_contact, off_forces, off_reward, off_hard_reset, off_obs, off_servo;
  const float* action;                   /* [N, 12] */
  const uint8_t* reset;                  /* [N] */
  const int64_t* episode_length;         /* [N], before this step's increment */
  int64_t max_episode_length;
  int32_t decimation, resample_steps, init, reserved;   /* reserved: 0 or one of CATPPO_SERVO_EXT_OBS / _EVENTS / _COMMANDS / _TERMINATIONS / _ACTIONS / _ACTUATORS / _RANDOMIZE / _HISTORY / _PLANT (see below) */
  uint64_t seed;
  float default_joint_pos[12];
  float dt, kp, kd, inertia, tau_max, action_scale, vel_alpha, tilt_beta, tilt_max, reward_scale, foot_clearance,
      contact_threshold, stand_height, height_drop, floor_height, min_height, base_stiffness, weight, impact_gain,
      init_noise, standing_fraction, command_deadzone;
  const float* fixed_command;            /* [N, 3], [fixed_segments, N, 3] or NULL */
  float* eval;                           /* [N, CATPPO_SERVO_EVAL_FLOATS] or NULL; 16-byte aligned */
  int32_t fixed_segments;                /* S > 1: fixed_command is a schedule [S, N, 3]; 0 or 1: [N, 3] */
  int32_t fixed_segment_steps;           /* control steps per segment of the schedule */
  float* trace;                          /* [trace_capacity, trace_envs, CATPPO_SERVO_TRACE_FLOATS] or NULL; 16-byte aligned */
  int32_t trace_envs, trace_capacity;    /* envs 0 .. trace_envs - 1 are traced, for trace_capacity steps */
  int32_t reward_terms;                  /* T in 0 .. 15; 0: the built-in reward */
  float* reward_rec;                     /* [N, CATPPO_SERVO_REWARD_FLOATS] or NULL; 16-byte aligned */
  const catppo_servo_reward_term* reward_table;   /* device, [reward_terms]; 16-byte aligned */
} catppo_servo_sim;
int catppo_servo_sim_step(catppo_ctx* ctx, const catppo_servo_sim* desc, void* stream);

/* Observations ("Observations").  desc->reserved == CATPPO_SERVO_EXT_OBS: `desc` is the head of a
 * catppo_servo_sim_obs, i.e. a second, small descriptor lies right behind the 368 bytes of catppo_servo_sim (which stays
 * what it is: the launches without it carry the same kernel argument as before).  reserved == 0: nothing lies behind it;
 * any other value is an error.  With it the row gets a second observation field, the POLICY observation - `width` = P
 * floats at off_policy_obs (multiple of 4; the field is padded with zeros to a multiple of 4 floats, lies inside row_floats
 * and is disjoint from [off_obs, off_obs + 45)).  The raw observation at off_obs stays exactly where and what it is
 * (obs_dim == 45 is required); every other float of the row, the records and the trace are what the launch without the
 * second descriptor writes.
 * A post-pass over the finished row computes, for output float j with entry E = table[j], in fp32, unfused, in the order of
 * IsaacLab's ObservationManager (noise, clip, scale):
 *   x = raw[clamp(E.src, 0, 44)]
 *   if (E.flags & 1) x = x + E.bias
 *   if (E.flags & 2) x = (x + u * E.noise_width) + E.noise_lo            u = uniform in (0, 1) from the Philox word below
 *   if (E.flags & 4) x = x < E.clip_lo ? E.clip_lo : x;  x = x > E.clip_hi ? E.clip_hi : x       (a NaN passes through)
 *   x = x * E.scale
 * u: word j & 3 of Philox4x32-10 with key = seed and counter {global env id, ep', (t' << 4) | (j >> 2), "OBSN"}, where
 * (ep', t') are the episode and the episode length of the state the observation describes: (0, 0) in an init launch,
 * (episode + 1, 0) in a step that ends its episode, (episode, episode_length + 1) otherwise; max_episode_length < 2^27.
 * It covers init launches and the post-reset observation of a step that ends an episode alike.
 * table is a DEVICE array of P entries, 16-byte aligned, read by every launch: entries the host rewrites in stream order
 * (the noise bits, say) are in the next launch, under graph replay too.  It may alias none of the state buffers, the
 * records, the trace, the command table or the reward table. */
#define CATPPO_SERVO_OBS_MAX_WIDTH 64
#define CATPPO_SERVO_EXT_OBS 0x4F425331   /* "OBS1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_obs */
typedef struct catppo_servo_obs_entry {   /* 32 bytes, one per float of the policy observation */
  int32_t src;                            /* index into the raw 45-float observation of the row (field off_obs) */
  uint32_t flags;                         /* bit 0 bias, bit 1 noise, bit 2 clip */
  float bias, noise_lo, noise_width, clip_lo, clip_hi, scale;
} catppo_servo_obs_entry;
typedef struct catppo_servo_obs {
  int32_t width;                          /* P in 1 .. CATPPO_SERVO_OBS_MAX_WIDTH: floats of the policy observation */
  int32_t off_policy_obs;                 /* row offset of the policy observation, multiple of 4 */
  const catppo_servo_obs_entry* table;    /* DEVICE array [P], 16-byte aligned */
} catppo_servo_obs;
typedef struct catppo_servo_sim_obs {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_OBS */
  catppo_servo_obs obs;
} catppo_servo_sim_obs;

/* Events ("Events").  desc->reserved == CATPPO_SERVO_EXT_EVENTS: `desc` is the head of a
 * catppo_servo_sim_events, i.e. the observation descriptor and an event descriptor lie behind the 368 bytes.  Under this
 * value obs.width == 0 with a NULL table means "no observation table" (the row has no policy field); otherwise `obs` is
 * checked and used exactly as under CATPPO_SERVO_EXT_OBS.  0 and CATPPO_SERVO_EXT_OBS keep their meaning.
 * ev.block is a DEVICE array of CATPPO_SERVO_EVENT_FLOATS fp32 words, 16-byte aligned, read by every launch (a flag the host
 * rewrites in stream order is in the next launch, under graph replay too).  It may alias none of the state buffers, the
 * records, the trace, the command table, the reward table or the observation table.  max_episode_length < 2^27.  Words:
 *   0 flags (uint32 bits: 1 push, 2 joint reset by scale, 4 joint reset by offset, 8 root reset, 16 friction)
 *   1 p (push probability per step)    2 num_buckets (int32)    3 zero
 *   4..13  push (lo, width) of vx vy wz roll-rate pitch-rate        14 15 joint position (lo, width)
 *   16 17  joint velocity (lo, width; offset mode)                  18..21 root pose (lo, width) of x y
 *   22..27 root velocity (lo, width) of x y yaw                     28 29 friction (lo, width)        30 31 zero
 * A sample is s = lo + u * width (two rounded fp32 operations), u = uniform in (0, 1) from a word of Philox4x32-10 with
 * key = seed and counter {global env id, episode, third, tag}:
 *   push         tag "PUSH", third = (t << 1) | b, t = episode length the step starts from.  Block 0: word 0 decides
 *                (pushed = u < p), words 1..3 sample vx vy wz; block 1 (pushed envs only): words 0 1 the roll and pitch rates.
 *                A push replaces the three velocities the step starts from (after the reset select) and adds rate * step_dt
 *                to roll and pitch; ang[0], ang[1] keep differentiating against the un-kicked values.
 *   joint reset  position from tag "INIT", block j / 4, word j % 4 (the built-in pose's words): q0 = def * s (scale) or
 *                def + s (offset); velocity 0.f (scale) or s from tag "JVEL", same block and word (offset).
 *   root reset   tag "ROOT": block 0 words 0 1 the first state's root x y, block 1 words 0 1 2 its vx vy wz.
 *   friction     tag "FRIC": bucket = clamp((int)(u * (float)num_buckets), 0, num_buckets - 1) from {gid, 0, 0, tag} word 0;
 *                mu = lo + u * width from {bucket, 0, 1, tag} word 0; m = mu < 1.f ? mu : 1.f; the three velocity rows of
 *                the base model become tree16((gain * m) * dq).  Recomputed by every launch, no state in the row.
 * The first state (joint and root terms) serves the init launch, the start of a step whose reset flag is set and the
 * post-reset observation of a step that ends its episode (obs 9..20, 21..32 and wz at obs 2) alike.
 * With the push flag set, float 14 of a trace row is 1.f in a step whose env was pushed.  The block's writer checks its
 * values (Solo12ServoSim.set_event_block); whatever it holds the launch stays inside its row.
 *
 * Disturbances ("Disturbances").  ev.floats may also be CATPPO_SERVO_EVENT_FLOATS_EXT: the block then has
 * 64 words, words 0..31 exactly as above, and three more flag bits count (in a 32-word block they are ignored):
 *   32 timed push    64 external wrench    128 the wrench is drawn per episode (clear: once per env, for all episodes)
 *   32 33  T (lo, width) of the timed push's interval, in seconds     34 35 force (lo, width), in N
 *   36 37  torque (lo, width), in N m                                 38..63 zero
 * ev.reserved is then off_ev_state: 0, or the row offset of a 4-float state field `ev_state` (float 0: the time left until
 * the env's next timed push, in seconds; floats 1..3 zero) under the rules of off_cmd_state: a multiple of 4, inside
 * row_floats, disjoint from every base field and every other field.  With a 32-word block it must be 0; 1 is refused under
 * either size.  The library cannot read the block: with the timed bit set while off_ev_state == 0 the kernel ignores the bit.
 *   timed push   IsaacLab's push_by_setting_velocity under the interval rule with is_global_time = False.  tag "PSHT".  First
 *                state of episode ep (init launch, or a step whose reset flag is set, which runs no update):
 *                tl = T_lo + u * T_width from {gid, ep, 0, tag} word 0.  Any other step, starting at episode length t:
 *                tl = tl - step_dt; fire = tl < 1e-6f; if fire, tl is redrawn from {gid, ep, t + 1, tag} word 0.  A fired step
 *                takes the push's samples (tag "PUSH", third = (t << 1) | b, words and ranges as above; word 0 of block 0 is not
 *                used) and ADDS them: v0[k] = xin[k] + s_k; tilt kick, ang and trace float 14 as for the push.  Every step
 *                writes tl into ev_state of its output row; with the bit cleared the field is carried over unchanged.  With
 *                both push bits set the per-step push wins and the timer keeps running.
 *   wrench       IsaacLab's apply_external_force_torque on the base.  tag "WRNC", e = ep with bit 128, else 0:
 *                {gid, e, 0, tag} words 0..2 sample F[0..2] from the force range, {gid, e, 1, tag} words 0..2 T[0..2] from the
 *                torque range.  With W the load the stance feet share (d.weight, or the env's drawn or pinned one) and
 *                L = W * d.stand_height, after the five reductions: red[0] += F[0] / W, red[1] += F[1] / W, red[2] += T[2] / L,
 *                red[3] += T[0] / L, red[4] += T[1] / L, and the stance feet share fmaxf(W - F[2], 0.f).  Stateless. */
#define CATPPO_SERVO_EXT_EVENTS 0x45565431   /* "EVT1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_events */
#define CATPPO_SERVO_EVENT_FLOATS 32
#define CATPPO_SERVO_EVENT_FLOATS_EXT 64     /* the second accepted value of catppo_servo_events.floats */
#define CATPPO_SERVO_EVENT_PUSH 1u
#define CATPPO_SERVO_EVENT_JOINT_SCALE 2u
#define CATPPO_SERVO_EVENT_JOINT_OFFSET 4u
#define CATPPO_SERVO_EVENT_ROOT 8u
#define CATPPO_SERVO_EVENT_FRICTION 16u
#define CATPPO_SERVO_EVENT_PUSH_TIMED 32u    /* this bit and the two below: in a block of CATPPO_SERVO_EVENT_FLOATS_EXT words only */
#define CATPPO_SERVO_EVENT_WRENCH 64u
#define CATPPO_SERVO_EVENT_WRENCH_RESET 128u
typedef struct catppo_servo_events {
  const float* block;                     /* DEVICE array [floats], 16-byte aligned */
  int32_t floats;                         /* CATPPO_SERVO_EVENT_FLOATS or CATPPO_SERVO_EVENT_FLOATS_EXT */
  int32_t reserved;                       /* off_ev_state: 0, or with CATPPO_SERVO_EVENT_FLOATS_EXT the row offset of ev_state */
} catppo_servo_events;
typedef struct catppo_servo_sim_events {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_EVENTS */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;
} catppo_servo_sim_events;

/* Commands ("Commands").  desc->reserved == CATPPO_SERVO_EXT_COMMANDS: `desc` is the head of a
 * catppo_servo_sim_commands, i.e. the observation, event and command descriptors lie behind the 368 bytes.  Under this
 * value obs.width == 0 with a NULL table means "no observation table" and ev.block == NULL with ev.floats == 0 means "no
 * events"; otherwise both are checked and used exactly as under CATPPO_SERVO_EXT_EVENTS.  0, CATPPO_SERVO_EXT_OBS and
 * CATPPO_SERVO_EXT_EVENTS keep their meaning.
 * cmd.block is a DEVICE array of CATPPO_SERVO_COMMAND_FLOATS fp32 words, 16-byte aligned, read by every launch (ranges the
 * host rewrites in stream order are in the next launch, under graph replay too).  It may alias none of the state buffers,
 * the records, the trace, the command table or the other tables and blocks.  max_episode_length < 2^27.  Words:
 *   0 flags (uint32 bits: 1 dead zone, 2 random resample, 4 yaw flip, 8 standing)      1 dz (dead zone)
 *   2 p_still    3 p_move    4..9 (lo, width) of the commands x y wz    10 rel_standing    11 12 T_lo T_width (seconds)
 *   13..15 zero
 * cmd.off_cmd_state names one more 16-byte field of the row (a multiple of 4, disjoint from every other field the kernel
 * writes): float 0 the time left until the timed resample in seconds, floats 1..3 zero.  The velocity command becomes a
 * stateful process on (off_command, off_cmd_state) of the input row; the built-in generator ("CMDS", resample_steps,
 * standing_fraction, command_deadzone) is not evaluated.  A sample is s = lo + u * width (two rounded fp32 operations),
 * u = uniform in (0, 1) from a word of Philox4x32-10 with key = seed and counter {global env id, episode, third, tag}:
 *   draw(third)  tag "CMDD": words 0..2 sample x y wz, word 3 gives standing = u <= rel_standing
 *   time(third)  tag "CMDT": word 0 samples T_lo + u * T_width; words 2 and 3 are the step's two decisions (below)
 * Rules: dead zone = no |c_i| > dz zeroes the command (+0.f); standing = `standing` zeroes it; each only with its flag.
 * First command of episode ep (third = 0): c = draw(0), dead zone, standing, tl = time(0).  It serves the init launch
 * (row, raw observation, cmd_state), a step whose reset flag is set (which runs no update) and the post-reset observation
 * of a step that ends its episode alike.
 * Update of a step that starts at episode length t and is not a reset step, third = ((t + 1) << 1) | b, c and tl from the
 * input row; D = time(b = 0), which every such step draws:
 *   1. tl = tl - step_dt; if tl <= 0: c = draw(b = 0), standing, tl = D word 0's sample
 *   2. dead zone
 *   3. (random resample) still = sqrt((c0 c0 + c1 c1) + c2 c2) < dz; p = still ? p_still : p_move; if u(D word 2) < p:
 *      c = draw(b = 1), tl = time(b = 1); this command meets the dead zone in the next step
 *   4. (yaw flip) if u(D word 3) < p_move: c2 = -c2
 * The update runs at the start of the step it applies to: reward, records, trace and observation of the step see it.
 * With a fixed-command table the generator is bypassed as without commands and cmd_state is written as zeros.
 * Float 15 of a trace row is 1.f when the command was redrawn in the step (1. or 3.) plus 2.f when the yaw flipped.
 * The block's writer checks its values (Solo12ServoSim.set_command_block); whatever it holds the launch stays inside its
 * row: the words are floats and one flag word, never addresses. */
#define CATPPO_SERVO_EXT_COMMANDS 0x434D4431   /* "CMD1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_commands */
#define CATPPO_SERVO_COMMAND_FLOATS 16
#define CATPPO_SERVO_COMMAND_DEADZONE 1u
#define CATPPO_SERVO_COMMAND_RANDOM_RESAMPLE 2u
#define CATPPO_SERVO_COMMAND_YAW_FLIP 4u
#define CATPPO_SERVO_COMMAND_STANDING 8u
typedef struct catppo_servo_commands {
  const float* block;                     /* DEVICE array [CATPPO_SERVO_COMMAND_FLOATS], 16-byte aligned */
  int32_t floats;                         /* CATPPO_SERVO_COMMAND_FLOATS */
  int32_t off_cmd_state;                  /* the row's 4-float field: time left | 0 0 0 */
} catppo_servo_commands;
typedef struct catppo_servo_sim_commands {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_COMMANDS */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;
} catppo_servo_sim_commands;

/* Terminations ("Terminations").  desc->reserved == CATPPO_SERVO_EXT_TERMINATIONS: `desc` is the head of a
 * catppo_servo_sim_terminations, i.e. the observation, event, command and termination descriptors lie behind the 368
 * bytes.  Under this value obs.width == 0 with a NULL table means "no observation table", ev.block == NULL with
 * ev.floats == 0 "no events" and cmd.block == NULL with cmd.floats == 0 "no commands"; otherwise the three are checked and
 * used exactly as under CATPPO_SERVO_EXT_COMMANDS.  Every older value of `reserved` keeps its meaning.
 * term.table is a DEVICE array of `terms` entries {kind, mask, p0, p1} (1 <= terms <= CATPPO_SERVO_TERM_MAX_TERMS; the
 * entry point reserves CATPPO_SERVO_TERM_MAX_TERMS entries behind the pointer when it checks for overlap), 16-byte aligned,
 * read by every launch that is no init launch (params the host rewrites in stream order are in the next launch, under graph
 * replay too).  Term k fires in a step when (symbols of csrc/servo_sim.hip, all after the step's integration; fp32, unfused):
 *   1 time_out                         t + 1 >= max_episode_length
 *   2 illegal_contact                  some body b with bit b of mask set (17 bodies, base_link = bit 0) and some history slot
 *                                      h < H has sqrt((fx fx + fy fy) + fz fz) > p0.  Slot 0 is this step's forces (fbase on
 *                                      body 0, fz on the feet 4 8 12 16, zero elsewhere), slot h >= 1 is slot h - 1 of the
 *                                      input row; a step whose reset flag is set has only slot 0
 *   3 upside_down                      sqrt(g0 g0 + g1 g1) > p0          g = (0 - pitch, roll, -1) / sqrt(tilt2 + 1), the
 *   4 bad_orientation                  (0 - g2) < p0                     projected gravity BEFORE the roll-over override;
 *                                                                        p0 = f32(cos(limit_angle)), computed by the host
 *   5 root_height_below_minimum        z < p0
 *   6 joint_pos_out_of_manual_limit    some joint j with bit j of mask set has q < p0 or q > p1
 *   7 joint_vel_out_of_manual_limit    some joint j with bit j of mask set has |qd| > p0
 *   8 rolled_over                      tilt2 > tilt_max * tilt_max       (the model's own flag)
 * "some" over joints or bodies is a max over the env's 16 lanes in the shape of tree16 (exact: the order cannot matter);
 * kind 2 gives lane l body l of the history slots and lane 0 body 16 as well.  terminated = some fired term of kind != 1.
 * It stands where the model's flag `fallen` stands without this descriptor: an episode ends on t + 1 >= max_episode_length
 * or terminated; the row's hard_reset, reward kinds 15 and 16, field 2 of the evaluation record and float 2 of a trace
 * row are `terminated`.  The written projected gravity is still overridden with (0, 0, 1) when tilt2 > tilt_max^2, which no
 * longer ends an episode by itself.
 * term.off_term_state names one more 16-byte field of the row (a multiple of 4, disjoint from every other field the kernel
 * writes): float 0 is the step's fired terms as a float, bit k = term k (exact: below 2^16), floats 1..3 zero; an init
 * launch writes zeros.
 * term.rec ([N, CATPPO_SERVO_TERM_FLOATS] fp32, 16-byte aligned; may alias none of the state buffers, the records, the
 * trace, the command table or the other tables and blocks): a step that ends its episode adds 1 to float k < 15 when term k
 * fired and 1 to float 15, the count of ended episodes; any other step leaves it alone; an init launch zeroes it.  No
 * atomics, no communication between envs.
 * The table's writer checks its entries (Solo12ServoSim.set_termination_table); whatever it holds the launch stays inside
 * its row and its record: an unknown kind never fires, masks select lanes, params are compared, nothing is an address. */
#define CATPPO_SERVO_EXT_TERMINATIONS 0x54524D31   /* "TRM1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_terminations */
#define CATPPO_SERVO_TERM_FLOATS 16
#define CATPPO_SERVO_TERM_MAX_TERMS 15
typedef struct catppo_servo_term_entry {
  int32_t kind;
  uint32_t mask;                          /* kinds 6, 7: joints (bits 0..11); kind 2: bodies (bits 0..16) */
  float p0, p1;
} catppo_servo_term_entry;
typedef struct catppo_servo_terminations {
  const catppo_servo_term_entry* table;   /* DEVICE array [terms], 16-byte aligned */
  float* rec;                             /* DEVICE [N, CATPPO_SERVO_TERM_FLOATS], 16-byte aligned */
  int32_t terms;                          /* 1 .. CATPPO_SERVO_TERM_MAX_TERMS */
  int32_t off_term_state;                 /* the row's 4-float field: fired terms | 0 0 0 */
} catppo_servo_terminations;
typedef struct catppo_servo_sim_terminations {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_TERMINATIONS */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;
} catppo_servo_sim_terminations;

/* Actions ("Actions").  desc->reserved == CATPPO_SERVO_EXT_ACTIONS: `desc` is the head of a
 * catppo_servo_sim_actions, i.e. the observation, event, command, termination and action descriptors lie behind the 368
 * bytes.  Under this value term.table == NULL with term.terms == 0 means "no terminations" (the three blocks before it are
 * marked absent as under CATPPO_SERVO_EXT_TERMINATIONS); otherwise the four are checked and used exactly as under that
 * value.  Every older value of `reserved` keeps its meaning.
 * act.table is a DEVICE array of 12 entries of 32 bytes, one per simulator joint j (lane j), 16-byte aligned, read by every
 * launch that is no init launch (values the host rewrites in stream order are in the next launch, under graph replay too).
 * act.width = A, 1 <= A <= 12, is the width of the action: sim.action is [N, A].  Entry j: col in -1 .. A - 1 is the action
 * column that drives joint j (-1: none; the kernel clamps it into 0 .. A - 1 before it is used, whatever the table holds),
 * flags & CATPPO_SERVO_ACTION_KIND_MASK the kind, flags & CATPPO_SERVO_ACTION_CLIP the clip bit.  fp32, unfused:
 *   raw = action[e * A + col]       p = raw * scale + offset       clip bit: p = p < clip_lo ? clip_lo : p, then
 *                                                                            p = p > clip_hi ? clip_hi : p
 * and per substep, before the clamp to +- tau_max (which, like qdd, the integration and the choice of the reported
 * substep, stays as it is):
 *   0 not driven                    tau = kp * (def - q) - kd * qd
 *   1 JointPositionAction           tau = kp * (p - q) - kd * qd
 *   2 RelativeJointPositionAction   tau = kp * ((p + q) - q) - kd * qd       (q of this substep; sum and difference rounded)
 *   3 JointVelocityAction           tau = kd * (p - qd)                      (no position gain on such a joint)
 *   4 JointEffortAction             tau = p
 * The raw action by column is what the rest of the step calls `a`: obs[33 + k], trace float 60 + k and reward kinds 11 / 12
 * read column k for k < A and zero for k >= A.  sim.action_scale is unused.  With col = j, kind 1, scale = action_scale,
 * offset = default_joint_pos[j] and no clip the launch computes the bits of the launch without the descriptor.
 * The table's writer checks its entries (Solo12ServoSim.set_action_table); whatever it holds the launch stays inside the
 * action's row: col is clamped, an unknown kind is "not driven", the rest are values. */
#define CATPPO_SERVO_EXT_ACTIONS 0x41435431        /* "ACT1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_actions */
#define CATPPO_SERVO_ACTION_KIND_MASK 0x7u
#define CATPPO_SERVO_ACTION_CLIP 0x8u
typedef struct catppo_servo_action_entry {
  int32_t col;                            /* -1 .. A - 1 */
  uint32_t flags;                         /* kind | CATPPO_SERVO_ACTION_CLIP */
  float scale, offset, clip_lo, clip_hi;
  uint32_t zero[2];
} catppo_servo_action_entry;
typedef struct catppo_servo_actions {
  const catppo_servo_action_entry* table; /* DEVICE array [12], 16-byte aligned */
  int32_t width;                          /* A: 1 .. 12 */
  int32_t reserved;                       /* 0 */
} catppo_servo_actions;
typedef struct catppo_servo_sim_actions {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_ACTIONS */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;         /* table NULL and terms 0: no terminations */
  catppo_servo_actions act;
} catppo_servo_sim_actions;

/* Actuators ("Actuators").  desc->reserved == CATPPO_SERVO_EXT_ACTUATORS: `desc` is the head of a
 * catppo_servo_sim_actuators, i.e. the catppo_servo_sim_actions above with an actuator descriptor behind it.  The five
 * descriptors before it are checked and used exactly as under CATPPO_SERVO_EXT_ACTIONS, except that act.table must not be
 * NULL: a launch without an ActionsCfg passes the identity action table (col j, kind 1, action_scale, default pose, no
 * clip), which computes the bits of the launch without one.  Every older value of `reserved` keeps its meaning.
 * actu.table is a DEVICE array of 12 entries of 32 bytes, one per simulator joint j (lane j), 16-byte aligned, read by every
 * launch that is no init launch (values the host rewrites in stream order are in the next launch, under graph replay too).
 * Entry j stands where sim.kp, sim.kd, sim.inertia and sim.tau_max stand for joint j - in the servo torque of every action
 * kind, the clamp, qdd, the row's joint_acc and reward kind 8 (tau_w / inertia) - which are unused under this value.
 * fp32, unfused, per substep s = 0 .. decimation - 1, with qd of that substep before its integration:
 *   tau as under "Actions", with kp_j, kd_j and the delayed processed action (below) in the place of p
 *   flags & CATPPO_SERVO_ACTUATOR_DC_MOTOR clear (ideal PD, delayed PD, implicit):
 *     tau = fminf(fmaxf(tau, -effort_limit), effort_limit)
 *   set (DC motor; IsaacLab's DCMotor._clip_effort):
 *     r  = qd / velocity_limit
 *     hi = saturation_effort * (1.f - r)         hi = fminf(fmaxf(hi, 0.f), effort_limit)
 *     lo = saturation_effort * (-1.f - r)        lo = fminf(fmaxf(lo, -effort_limit), 0.f)
 *     tau = fminf(fmaxf(tau, lo), hi)
 *   qdd = tau / inertia_j      (the integration and the choice of the reported substep stay as they are)
 * velocity_limit of a joint that is no DC motor is not read: the surrogate has no joint velocity clamp.
 * Delay.  delay = min | max << 8 | group << 16 (8 bits each).  The lag L of (env, episode, group), in physics steps:
 *   min == max: L = min; otherwise u = uniform_open(word 0 of Philox{gid, episode, group, "ADLY"}),
 *   L = min + (int)(u * (float)(max - min + 1)), at most max
 * (one draw per group: the joints of a group share it; re-derived in every step).  The row's field at off_act_hist, three
 * slots of 16 floats, holds in float j of slot k - 1 the processed action p of joint j of the control step k steps ago;
 * float 12 of slot 0 is 1.f in every row a step wrote and 0.f in the row of an init launch, floats 13 .. 15 of slot 0 and
 * 12 .. 15 of slots 1 and 2 are zero.  In a step that follows a reset or whose input row has float 12 of slot 0 equal to
 * 0.f all three slots count as holding this step's p.  In substep s
 *   k = s >= L ? 0 : (L - s + decimation - 1) / decimation, at most 3
 * and the target is this step's p for k == 0, else slot k - 1.  The output row's slots are p, slot 0, slot 1 (as counted).
 * obs[33 + k], the trace's action floats and reward kinds 11 / 12 keep reading the raw, undelayed columns.
 * With kp = sim.kp, kd = sim.kd, inertia = sim.inertia, effort_limit = sim.tau_max, flags 0 and delay 0 in every entry the
 * launch computes the bits of the launch without the descriptor, the field at off_act_hist excepted.
 * off_act_hist: 48 floats of the row on a 16-byte boundary that no other field the kernel writes touches.  The table's
 * writer checks its entries (Solo12ServoSim.set_actuator_table); whatever it holds the launch stays inside its rows: the
 * entries are values, never addresses, and k is clamped. */
#define CATPPO_SERVO_EXT_ACTUATORS 0x41435531      /* "ACU1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_actuators */
#define CATPPO_SERVO_ACTUATOR_DC_MOTOR 0x1u
#define CATPPO_SERVO_ACT_HIST_FLOATS 48            /* 3 slots of 16 floats */
typedef struct catppo_servo_actuator_entry {
  float kp, kd, inertia, effort_limit;    /* stiffness, damping, sim.inertia + armature, effort limit of joint j */
  float saturation_effort, velocity_limit; /* read for a DC motor only */
  uint32_t flags;                         /* CATPPO_SERVO_ACTUATOR_DC_MOTOR */
  uint32_t delay;                         /* min | max << 8 | group << 16 */
} catppo_servo_actuator_entry;
typedef struct catppo_servo_actuators {
  const catppo_servo_actuator_entry* table; /* DEVICE array [12], 16-byte aligned */
  int32_t off_act_hist;                   /* float offset of the row's 48-float history field, a multiple of 4 */
  int32_t reserved;                       /* 0 */
} catppo_servo_actuators;
typedef struct catppo_servo_sim_actuators {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_ACTUATORS */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;         /* table NULL and terms 0: no terminations */
  catppo_servo_actions act;               /* table never NULL */
  catppo_servo_actuators actu;
} catppo_servo_sim_actuators;

/* Randomisation ("Randomisation").  desc->reserved == CATPPO_SERVO_EXT_RANDOMIZE: `desc` is the head of a
 * catppo_servo_sim_randomize, i.e. the catppo_servo_sim_actuators above with a randomisation descriptor behind it.  The six
 * descriptors before it are checked and used exactly as under CATPPO_SERVO_EXT_ACTUATORS (a launch without a robot passes
 * the identity actuator table and the identity action table).  Every older value of `reserved` keeps its meaning.
 * rnd.block is a DEVICE array of CATPPO_SERVO_RANDOMIZE_FLOATS (32) fp32 words, 16-byte aligned, read by every launch that
 * is no init launch (a word the host rewrites in stream order is in the next launch, under graph replay too; a device block
 * because a descriptor is copied into a captured graph's kernel arguments once).  Wave lane k < 32 loads word k, the body
 * reads through readlane: every branch on a flag is wave-uniform.
 *   word 0  flags (integer): CATPPO_SERVO_RANDOMIZE_ENABLE | _KP | _KD | _FRICTION | _ARMATURE | _MASS (one bit per
 *           quantity) | _GAINS_RESET | _JOINT_RESET | _MASS_RESET (the term draws per episode, not once per env)
 *   word 1  operations (integer): gains | joint parameters << 8 | mass << 16; 0 "scale" x * s, 1 "add" x + s, 2 "abs" s
 *   words 2 .. 4  12-bit joint masks (integers): gains, joint parameters, and the body mask of the mass term (bit 0 = base_link)
 *   word 5  zero
 *   words 6 .. 15  (lo, width) of stiffness, damping, friction, armature, mass: a sample is s = lo + u * width
 *   words 16 .. 18  m0 = f32(weight / 9.81), g = f32(9.81), servo_inertia        word 19  zero
 *   words 20 .. 31  the nominal armature of joint 0 .. 11
 * Draws: Philox4x32-10, key = sim.seed, counter {global env id, e, third, tag}, u = uniform_open(word); e = 0, or the row's
 * episode word under the term's _RESET bit.  Nothing is stored: lane j re-derives its values in every step.
 *   gains, tag "AGAN", third = j: kp' = op(entry.kp, s(word 0)), kd' = op(entry.kd, s(word 1)) for the joints of mask 0
 *   joint parameters, tag "JPAR", third = j, for the joints of mask 1: fr = op(0.f, s(word 0)) (a Coulomb torque, N m);
 *     armature' = op(armature_j, s(word 1)), inertia' = servo_inertia + armature' (without _ARMATURE: entry.inertia)
 *   mass, tag "MASS", third = 0: m' = op(m0, s(word 0)); the stance feet share m' * g where they shared sim.weight;
 *     rho = m' / m0 and the three velocity lags of the base use fminf(sim.vel_alpha / rho, 1.f) where they used sim.vel_alpha
 * kp', kd' and inertia' stand wherever entry.kp, entry.kd and entry.inertia stand under CATPPO_SERVO_EXT_ACTUATORS.  Per
 * substep, after the clamp (tau, tau_w and applied_torque keep the actuator's torque before friction):
 *   qd_free = qd + qdd * dt        df = (fr / inertia') * dt  (once per lane)
 *   qd = fr > 0.f ? qd_free - fminf(fmaxf(qd_free, -df), df) : qd_free        q = q + qd * dt
 * With _ENABLE clear, or no quantity bit set, the launch draws nothing and computes the bits of the launch under
 * CATPPO_SERVO_EXT_ACTUATORS.  The block's writer checks its values (Solo12ServoSim.set_randomize_block); whatever it holds
 * the launch stays inside its rows: samples are only ever floats, masks only select. */
#define CATPPO_SERVO_EXT_RANDOMIZE 0x524E4431      /* "RND1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_randomize */
#define CATPPO_SERVO_RANDOMIZE_FLOATS 32
#define CATPPO_SERVO_RANDOMIZE_ENABLE 0x1u
#define CATPPO_SERVO_RANDOMIZE_KP 0x2u
#define CATPPO_SERVO_RANDOMIZE_KD 0x4u
#define CATPPO_SERVO_RANDOMIZE_FRICTION 0x8u
#define CATPPO_SERVO_RANDOMIZE_ARMATURE 0x10u
#define CATPPO_SERVO_RANDOMIZE_MASS 0x20u
#define CATPPO_SERVO_RANDOMIZE_GAINS_RESET 0x100u
#define CATPPO_SERVO_RANDOMIZE_JOINT_RESET 0x200u
#define CATPPO_SERVO_RANDOMIZE_MASS_RESET 0x400u
typedef struct catppo_servo_randomize {
  const float* block;                     /* DEVICE array [32], 16-byte aligned */
  int32_t reserved[2];                    /* 0 */
} catppo_servo_randomize;
typedef struct catppo_servo_sim_randomize {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_RANDOMIZE */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;         /* table NULL and terms 0: no terminations */
  catppo_servo_actions act;               /* table never NULL */
  catppo_servo_actuators actu;            /* table never NULL */
  catppo_servo_randomize rnd;
} catppo_servo_sim_randomize;

/* Observation history ("History").  PARITY UNPINNED: the rule restates IsaacLab's ObservationManager and
 * CircularBuffer (history_length on a term or group) from their published form.  desc->reserved == CATPPO_SERVO_EXT_HISTORY:
 * `desc` is the head of a catppo_servo_sim_history, i.e. the catppo_servo_sim_randomize above with a history descriptor
 * behind it.  The seven descriptors before it are checked and used exactly as under CATPPO_SERVO_EXT_RANDOMIZE, except that
 * the observation descriptor is never empty (a launch without a robot passes the identity action and actuator tables and a
 * switched-off randomisation block).  Every older value of `reserved` keeps its meaning.
 * The row gets a second policy field, policy_obs_hist: hist.floats = T floats (1 .. CATPPO_SERVO_OBS_HISTORY_MAX_FLOATS) at
 * hist.off_hist, a multiple of 4 at or past sim.row_floats with off_hist + pad4(T) <= sim.row_stride: it lies outside the
 * part of the row that is staged in LDS and leaves with registers-to-memory dword stores.  A term of frame width w and depth
 * H owns H * w consecutive floats, oldest frame first, terms in table order; the current frame stays in obs.off_policy_obs.
 * hist.map is a DEVICE array of T 32-bit words, 16-byte aligned, read by every launch (a word the host rewrites in stream
 * order is in the next launch):  word i = cur | w << 8 | newest << 16
 *   cur     0 .. obs.width - 1: the float of the current frame that float i shows when it is new
 *   w       the frame width of float i's term: the float one slot later is float i + w
 *   newest  1: float i lies in the last slot of its term
 * After the observation post-pass, lane l of an env writes floats i = l, l + 16, ... < T of the output row:
 *   out[off_hist + i] = (fill || newest) ? policy_obs[cur] : in[off_hist + i + w]
 * fill: an init launch, or a step that ends its episode (policy_obs then shows the first state of the next one): the first
 * frame of an episode fills every slot.  A step after a reset shifts like any other: its input row holds the filled history.
 * The kernel clamps cur to 0 .. obs.width - 1 and i + w to < T: whatever the map holds the launch stays inside its row.  The
 * floats between T and pad4(T) are written as zeros.  The map's writer checks every word (Solo12ServoSim.set_history_table). */
#define CATPPO_SERVO_EXT_HISTORY 0x48535431        /* "HST1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_history */
#define CATPPO_SERVO_OBS_HISTORY_MAX_FLOATS 512
#define CATPPO_SERVO_OBS_HISTORY_MAX_DEPTH 16
#define CATPPO_SERVO_HISTORY_NEWEST 0x10000u
typedef struct catppo_servo_history {
  const uint32_t* map;                    /* DEVICE array [floats], 16-byte aligned */
  int32_t off_hist;                       /* the row's policy_obs_hist field: in [row_floats, row_stride), a multiple of 4 */
  int32_t floats;                         /* T */
} catppo_servo_history;
typedef struct catppo_servo_sim_history {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_HISTORY */
  catppo_servo_obs obs;                   /* never empty */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;         /* table NULL and terms 0: no terminations */
  catppo_servo_actions act;               /* table never NULL */
  catppo_servo_actuators actu;            /* table never NULL */
  catppo_servo_randomize rnd;             /* block never NULL */
  catppo_servo_history hist;
} catppo_servo_sim_history;

/* Pinned plants ("Robustness").  desc->reserved == CATPPO_SERVO_EXT_PLANT: `desc` is the head of a
 * catppo_servo_sim_plant, i.e. the catppo_servo_sim_history above with a plant descriptor behind it.  The eight descriptors
 * before it are checked and used exactly as under CATPPO_SERVO_EXT_HISTORY, except that an empty history descriptor (map NULL
 * and floats 0) is an absent one and the observation descriptor may then be empty, too; a history that is present still needs
 * its observations; act, actu and rnd are never absent.  Every older value of `reserved` keeps its meaning, and
 * catppo_servo_randomize.reserved stays reserved and zero.  A plant table is an evaluation input: at least one of
 * sim.fixed_command, sim.eval, sim.trace is set, and the launch is the step-response instance of its pack.
 * plant.table is a DEVICE array [N, CATPPO_SERVO_PLANT_FLOATS = 8] of fp32 words, 16-byte aligned, row i for local env i (like
 * fixed_command), read by every launch that is no init launch (a word the host rewrites in stream order is in the next launch).
 *   word 0  pin bits (integer): CATPPO_SERVO_PLANT_KP | _KD | _FRICTION | _ARMATURE | _MASS | _LAG; the other bits zero
 *   word 1  kp_scale            word 2  kd_scale
 *   word 3  joint friction, N m (a Coulomb torque)          word 4  armature, kg m^2
 *   word 5  mass_scale          word 6  lag in physics steps (integer)          word 7  zero
 * Lane k < 8 of an env's 16 lanes loads word k (one 32-byte read per env, up front); the body reads word k through a 16-wide
 * shuffle.  The spare lane groups past N read the row of the env they recompute, never a row >= N.
 * The pins apply after the lag draw ("Actuators") and after the randomisation block's draws ("Randomisation"), to all twelve
 * joints and all actuator groups, whatever the block's _ENABLE bit, quantity bits, masks and operations say.  fp32, unfused,
 * one rounded operation each; t_k is word k of the env's row, block word k the randomisation block's:
 *   _KP        kp' = entry.kp * t1
 *   _KD        kd' = entry.kd * t2
 *   _FRICTION  fr = t3
 *   _ARMATURE  inertia' = block word 18 (servo_inertia) + t4
 *   _FRICTION or _ARMATURE:  df = (fr / inertia') * dt, from the final fr and inertia'
 *   _MASS      m = m0 * t5, weight = m * g, av = fminf(sim.vel_alpha / (m / m0), 1.f)   (m0, g: block words 16, 17)
 *   _LAG       L = min(word 6, 255) for every joint (the substep's slot index is clamped as under "Actuators")
 * A row with no bit set leaves its env exactly as the launch under CATPPO_SERVO_EXT_HISTORY (or _RANDOMIZE, without a
 * history) computes it.  The row gets no new state.  The table's writer checks every row (Solo12ServoSim.set_fixed_plant);
 * whatever the table holds the launch stays inside its rows: the values are floats and one clamped integer. */
#define CATPPO_SERVO_EXT_PLANT 0x504C4E31          /* "PLN1": value of catppo_servo_sim.reserved that announces catppo_servo_sim_plant */
#define CATPPO_SERVO_PLANT_FLOATS 8
#define CATPPO_SERVO_PLANT_KP 0x1u
#define CATPPO_SERVO_PLANT_KD 0x2u
#define CATPPO_SERVO_PLANT_FRICTION 0x4u
#define CATPPO_SERVO_PLANT_ARMATURE 0x8u
#define CATPPO_SERVO_PLANT_MASS 0x10u
#define CATPPO_SERVO_PLANT_LAG 0x20u
typedef struct catppo_servo_plant {
  const float* table;                     /* DEVICE array [N, 8], 16-byte aligned */
  int32_t reserved[2];                    /* 0 */
} catppo_servo_plant;
typedef struct catppo_servo_sim_plant {
  catppo_servo_sim sim;                   /* sim.reserved = CATPPO_SERVO_EXT_PLANT */
  catppo_servo_obs obs;                   /* width 0 and table NULL: no observation table (only without a history) */
  catppo_servo_events ev;                 /* block NULL and floats 0: no events */
  catppo_servo_commands cmd;              /* block NULL and floats 0: no commands */
  catppo_servo_terminations term;         /* table NULL and terms 0: no terminations */
  catppo_servo_actions act;               /* table never NULL */
  catppo_servo_actuators actu;            /* table never NULL */
  catppo_servo_randomize rnd;             /* block never NULL */
  catppo_servo_history hist;              /* map NULL and floats 0: no history */
  catppo_servo_plant plant;
} catppo_servo_sim_plant;

/* ---- test hook (ABI 0.6) ------------------------------------------------------------------------------------------
 * buf != NULL ([2][M] int32, device): the head / loss kernel of every following catppo_ppo_minibatch_* call writes the clip
 * branch each sample of the minibatch took - surrogate codes in [0, M) (ratio against 1 +- clip_coef), value-loss codes in
 * [M, 2 M) (newvalue - old value against +- clip_coef): 0 inside, 1 below, 2 above; cleanrl/ppo.py:320-341.  NULL: off.
 * What tests/test_gpu_parity_sizes.py compares with the oracle's branches when two parameter trajectories part. */
int catppo_debug_clip_branches(catppo_ctx* ctx, int32_t* buf);

#ifdef __cplusplus
}
#endif
#endif /* CATPPO_H */
