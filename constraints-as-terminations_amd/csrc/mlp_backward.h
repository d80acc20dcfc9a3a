// Backward tail of a minibatch (cleanrl/ppo.py:352): the fixed-order fold of split-K / head partials into the flat gradient
// (seg_reduce_kernel) and the first layer's weight-gradient launch that carries the fold of the other layers (dw_fold_kernel).
// The per-layer weight + data gradient GEMMs are gemm_f32.h's gemm_pair_kernel.  At the end: the host side of the backward, the fold
// and the gradient exchange (stages 3 and 4 of minibatch_grad_core).  Part of mlp.hip's translation unit.
#pragma once

// ------------------------------------------------------------------------------- segmented partial reduction
// dst[e] (+)= scale * sum_{p<n_parts} src[p*stride + e]   in fixed order.  One launch handles every segment
// (all split-K weight/bias partials, the head partials and the diagnostics).
constexpr int kMaxSegs = 24;
struct Seg {
  const float* src;
  float* dst;
  int64_t count;
  int64_t stride;
  int n_parts;
  int mode;     // 0: dst = sum, 1: dst += sum * scale (diagnostics)
  float scale;
};
struct SegTable {
  int n;
  Seg s[kMaxSegs];
};

// block = EL lanes x G part-groups (EL*G = 256).  Thread (e,g) adds parts g, g+G, ... in order, the G group sums are
// then combined in LDS in fixed order => deterministic.  Aligned segments (every weight / bias partial): a lane owns FOUR
// consecutive elements (16-byte loads) and its parts are requested in batches of four or eight that are always full -
// a batch past the last part re-reads the last part and adds 0 - so the loads of a batch are in flight together
// whatever the split count (the unrolled loop of rounds 1-2 fell into its serial remainder for the 2-4 parts per thread
// of a small minibatch).  The order of the additions per element is unchanged: results are bit-identical.
template <int NB>
__device__ __forceinline__ float4 seg_sum4(const float* __restrict__ src, int64_t stride, int g, int G, int last) {
  float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int q0 = g; q0 <= last; q0 += NB * G) {
    float4 x[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int q = q0 + j * G;
      x[j] = *reinterpret_cast<const float4*>(src + (int64_t)(q < last ? q : last) * stride);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const bool on = q0 + j * G <= last;
      a.x += on ? x[j].x : 0.0f, a.y += on ? x[j].y : 0.0f, a.z += on ? x[j].z : 0.0f, a.w += on ? x[j].w : 0.0f;
    }
  }
  return a;
}

// one workgroup's share of one segment: workgroup bx of nbx walks the segment's elements (sm: 1024 floats of LDS)
// Returns the fp64 sum of squares of the gradient elements THIS thread wrote (mode 0 only): the launches that fold the
// gradient can emit the squared-norm partials of the clip on the way (NormEmit below).
__device__ __forceinline__ double seg_reduce_body(const Seg sg, const int bx, const int nbx, float* __restrict__ sm,
                                                  const float ent_coef, const float vf_coef) {
  double ss = 0.0;
  // few wide partials (split-K): 4 part groups x 64 lanes; many narrow ones (head): 16 x 16
  const int G = sg.n_parts >= 128 ? 16 : 4;
  const int EL = 256 / G;
  const int el = threadIdx.x % EL, g = threadIdx.x / EL;
  const bool vec = sg.mode == 0 && (reinterpret_cast<uintptr_t>(sg.src) & 15) == 0 && sg.stride % 4 == 0 &&
                   sg.count % 4 == 0 && (reinterpret_cast<uintptr_t>(sg.dst) & 15) == 0;
  if (vec) {
    const int last = sg.n_parts - 1;
    const bool few = (sg.n_parts + G - 1) / G <= 4;         // parts per thread
    float4* sm4 = reinterpret_cast<float4*>(sm);
    for (int64_t e0 = (int64_t)bx * EL * 4; e0 < sg.count; e0 += (int64_t)nbx * EL * 4) {
      const int64_t e = e0 + el * 4;
      float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (e < sg.count && g <= last) a = few ? seg_sum4<4>(sg.src + e, sg.stride, g, G, last)
                                              : seg_sum4<8>(sg.src + e, sg.stride, g, G, last);
      sm4[threadIdx.x] = a;
      __syncthreads();
      if (g == 0 && e < sg.count) {
        for (int gg = 1; gg < G; ++gg) {
          const float4 y = sm4[gg * EL + el];
          a.x += y.x, a.y += y.y, a.z += y.z, a.w += y.w;
        }
        *reinterpret_cast<float4*>(sg.dst + e) = a;
        ss += (double)a.x * (double)a.x;
        ss += (double)a.y * (double)a.y;
        ss += (double)a.z * (double)a.z;
        ss += (double)a.w * (double)a.w;
      }
      __syncthreads();
    }
    return ss;
  }
  for (int64_t e0 = (int64_t)bx * EL; e0 < sg.count; e0 += (int64_t)nbx * EL) {
    const int64_t e = e0 + el;
    float a = 0.0f;
    if (e < sg.count) {
#pragma unroll 8
      for (int p = g; p < sg.n_parts; p += G) a += sg.src[(int64_t)p * sg.stride + e];
    }
    sm[threadIdx.x] = a;
    __syncthreads();
    if (g == 0) {
      for (int gg = 1; gg < G; ++gg) a += sm[gg * EL + el];
    }
    __syncthreads();
    if (g == 0) sm[el] = a;          // combined sums, visible to the whole block
    __syncthreads();
    if (g == 0 && e < sg.count) {
      if (sg.mode == 0) {
        sg.dst[e] = a;
        ss += (double)a * (double)a;
      } else {
        // diagnostics block {pg, v, ent, loss, kl, old_kl, clipfrac, count} (count = 8 <= EL: one block)
        float v = a * sg.scale;
        if (e == 3) v = (sm[0] - ent_coef * sm[2] + sm[1] * vf_coef) * sg.scale;   // pg - ENT*entropy + v_loss*VF
        if (e == 7) v = 1.0f;                                                      // minibatches accumulated
        sg.dst[e] = sg.dst[e] + v;
      }
    }
    __syncthreads();
  }
  return ss;
}

// The clip of an optimiser step needs ||grad||^2 (cleanrl/ppo.py:354, clip_grad_norm_): a launch of its own that
// re-reads the gradient the fold launches have just written - 5 us per step for 1.2 MB.  With NormEmit.part set, every
// workgroup that folds a piece of the gradient also writes the fp64 sum of squares of that piece into its own slot
// (fixed slot per workgroup => the final sum has a fixed order), and one thread of the last fold launch advances the
// Adam step count and prepares the bias corrections (what sqnorm_partial_step_kernel does beside its loads).
// catppo_ppo_minibatch_step_packed then goes straight to the Adam launch.
struct NormEmit {
  double* part = nullptr;            // [kNormSlots]; nullptr: off
  catppo_iter_state* st = nullptr;
  double beta1 = 0.0, beta2 = 0.0;
  int n_slots = 0;                   // slots written so far by the launches of this step (host side)
};
static_assert(kNormSlots >= 256 * kMaxSegs, "one squared-norm slot per fold workgroup");

__device__ __forceinline__ void emit_norm_slot(double ss, double* __restrict__ slot, float* __restrict__ sm) {
  ss = wave_sum_d(ss);
  double* d = reinterpret_cast<double*>(sm);
  __syncthreads();                   // sm is free (seg_reduce_body ends behind a barrier; belt and braces)
  if ((threadIdx.x & 63) == 0) d[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) *slot = (d[0] + d[1]) + (d[2] + d[3]);
}

// torch.optim.Adam: bias_correction = 1 - beta ** step (Python doubles), step_size = lr / bias_correction1
__device__ __forceinline__ void adam_advance_step(catppo_iter_state* __restrict__ st, double beta1, double beta2) {
  const int64_t step_i = st->adam_step + 1;
  const double step = (double)step_i;
  const double bc1 = 1.0 - pow(beta1, step);
  const double bc2 = 1.0 - pow(beta2, step);
  st->adam_step = step_i;
  st->adam_step_size = (float)(st->lr / bc1);
  st->adam_bc2_sqrt = (float)sqrt(bc2);
}

__global__ __launch_bounds__(256) void seg_reduce_kernel(const SegTable t, float ent_coef, float vf_coef,
                                                         double* __restrict__ norm_slots, catppo_iter_state* st,
                                                         double beta1, double beta2) {
  __shared__ __attribute__((aligned(16))) float sm[1024];
  if (st != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 64) adam_advance_step(st, beta1, beta2);
  const double ss = seg_reduce_body(t.s[blockIdx.y], blockIdx.x, gridDim.x, sm, ent_coef, vf_coef);
  if (norm_slots != nullptr) emit_norm_slot(ss, norm_slots + blockIdx.y * gridDim.x + blockIdx.x, sm);
}

// The first layer's weight-gradient GEMM and the fold of every OTHER layer's partials in one launch (round 4).  dW_0 is
// the last GEMM of an optimiser step (it needs dZ_0, the output of the last paired launch) and a light one (0.8 GFLOP,
// 37 MB); the partials of the layers above it have been complete since their own launches.  Their fold (43 MB of
// streaming reads, no matrix work) used to wait behind it in a launch of its own; here its workgroups fill the CUs
// beside the GEMM's, the way the paired launches mix long and short workgroups.  Workgroups [0, n_gemm) run the GEMM
// (launch order first: they are resident from the start), the rest fold: kFoldX workgroups per segment.
constexpr int kFoldX = 256;
template <int PREC = 0>      // operand precision of the GEMM workgroups (round 5: the bf16 / split-bf16 modes take this launch too)
__global__ __launch_bounds__(256) void dw_fold_kernel(const gemm::Params p, const SegTable t, const int gemm_tiles,
                                                      const int n_gemm, float ent_coef, float vf_coef,
                                                      double* __restrict__ norm_slots) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x;
  if (b < n_gemm) {
    const gemm::TileId id = gemm::xcd_tile_of(b, gemm_tiles, n_gemm / gemm_tiles, p.xcd_legacy);
    gemm::gemm_body<64, 64, false, false, gemm::EPI_PARTIAL, gemm::BK, PREC>(p, id.tile, id.bz, smem);
  } else {
    const int f = b - n_gemm;
    const double ss = seg_reduce_body(t.s[f / kFoldX], f % kFoldX, kFoldX, smem, ent_coef, vf_coef);
    if (norm_slots != nullptr) emit_norm_slot(ss, norm_slots + f, smem);
  }
}

// Every hidden layer's split-K weight gradient in ONE launch (round 6, the small-minibatch step of step16.h: all dZ are in
// memory when the backward chain's launch ends, so nothing orders the weight gradients against each other).  All
// problems use gemm_body's 64x64 EPI_PARTIAL tile - one instruction stream, the problem picked by workgroup index; the
// partial sums per element are those of the per-layer launches (same splits, same slab order).
struct DwMulti {
  gemm::Params p[CATPPO_MAX_HIDDEN];
  int first[CATPPO_MAX_HIDDEN + 1];    // first workgroup of problem i (launch order); first[n] = grid size
  int tiles[CATPPO_MAX_HIDDEN];        // 64x64 tiles of one (network, split) slice
  int n;
};
__global__ __launch_bounds__(256) void dw_multi_kernel(const DwMulti m) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int b = blockIdx.x;
  int i = 0;
  while (i + 1 < m.n && b >= m.first[i + 1]) ++i;
  const gemm::TileId id = gemm::xcd_tile_of(b - m.first[i], m.tiles[i], (m.first[i + 1] - m.first[i]) / m.tiles[i], m.p[i].xcd_legacy);
  gemm::gemm_body<64, 64, false, false, gemm::EPI_PARTIAL>(m.p[i], id.tile, id.bz, smem);
}

// =============================================================================== host side: backward, fold, exchange
#define CATPPO_HIP_OK(call)                                                                          \
  do {                                                                                               \
    hipError_t e__ = (call);                                                                         \
    if (e__ != hipSuccess)                                                                           \
      return catppo_fail(ctx, CATPPO_E_HIP, "%s: %s failed: %s", __func__, #call, hipGetErrorString(e__)); \
  } while (0)

// What the partials of a step are folded into: the segment table of the NEXT fold launch (emptied by every launch that
// folds), the flat gradient and the diagnostics it writes, the squared-norm slots of the one-call optimiser step.
struct Fold {
  SegTable segs;
  float *grad, *diag;
  NormEmit* ne;            // null: no squared-norm slots
  bool tail_forked;        // Exchange::Tail: the side stream carries the ranges that dw_fold_kernel completed
};

void add_seg(SegTable& t, const float* src, float* dst, int64_t count, int64_t stride, int n_parts, int mode, float scale) {
  t.s[t.n++] = Seg{src, dst, count, stride, n_parts, mode, scale};
}
// split-K partials of hidden layer l: [split][net][out*in] weights, [net][split][out] biases
void add_layer_segs(Fold& f, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w, int l, int splits) {
  const int out = shape->hidden[l], in = L.in_dim[l];
  for (int net = 0; net < 2; ++net) {
    add_seg(f.segs, w.wpart[l] + (int64_t)net * out * in, f.grad + L.off_w[net][l], (int64_t)out * in, 2 * (int64_t)out * in,
            splits, 0, 1.0f);
    add_seg(f.segs, w.bpart[l] + (int64_t)net * splits * out, f.grad + L.off_b[net][l], out, out, splits, 0, 1.0f);
  }
}
// head partials + diagnostics ride along with the reduction launch
void add_head_segs(Fold& f, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w, const StepPlan& plan,
                   const catppo_ppo_hparams* hp) {
  const int nl = shape->n_hidden, A = shape->act_dim, HL = shape->hidden[nl - 1], nbh = plan.nbh;
  const int NS = head_scalars(A);
  const int64_t wrow = (int64_t)(A + 1) * HL;
  const float* cw = w.head_w + (plan.head_by_net ? (int64_t)nbh * wrow : 0);
  const float* cs = w.head_s + (plan.head_by_net ? (int64_t)nbh * NS : 0);
  add_seg(f.segs, w.head_w, f.grad + L.off_w[1][nl], (int64_t)A * HL, wrow, nbh, 0, 1.0f);
  add_seg(f.segs, cw + (int64_t)A * HL, f.grad + L.off_w[0][nl], HL, wrow, nbh, 0, 1.0f);
  add_seg(f.segs, w.head_s, f.grad + L.off_b[1][nl], A, NS, nbh, 0, 1.0f);
  add_seg(f.segs, cs + A, f.grad + L.off_b[0][nl], 1, NS, nbh, 0, 1.0f);
  add_seg(f.segs, w.head_s + A + 1, f.grad + L.off_logstd, A, NS, nbh, 0, 1.0f);
  add_seg(f.segs, w.head_s + 2 * A + 1, f.diag, kHeadDiag, NS, plan.head_by_net ? 2 * nbh : nbh, 1, hp->inv_global_batch);
}

// split-K weight-gradient problem of hidden layer l: dW[out,in] = dZ^T . Xin, contraction over the M rows (tiling rule
// shared by every backward path)
Params dw_params(const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w, int64_t M, bool act16, int l) {
  const int out = shape->hidden[l], in = L.in_dim[l];
  Params pw{};
  pw.nets = 2;
  pw.I = out, pw.J = in, pw.Kc = (int)M;
  pw.lda = out, pw.ldb = in, pw.ldc = in;
  // contraction rows per split for `tiles` output tiles (both networks): ~512 workgroups, at most max_splits splits
  auto rows_per_split = [&](int tiles, int max_splits) {
    int splits = 512 / (tiles > 0 ? tiles : 1);
    if (splits > max_splits) splits = max_splits;
    if (splits > split_cap(out, in)) splits = split_cap(out, in);
    if (splits < 1) splits = 1;
    return (int)(cdiv64(cdiv64(M, splits), gemm::BK) * gemm::BK);
  };
  int per = rows_per_split(((out + 127) / 128) * ((in + 127) / 128) * 2, (int)cdiv64(M, 4 * gemm::BK));
  if (!(out >= 128 && in >= 128 && per >= 256)) {
    // 64x64 tiles will be used (narrow layer, or a minibatch too small for 256-row contraction chunks): size the
    // split for ~512 workgroups with at least 128 contraction rows each.  At 2048 samples the old rule cut a
    // 256x512 layer into 2048 workgroups of 64 rows - four slabs of work between a prologue and a 33 MB partial store.
    // (512 workgroups: 256 / 384 / 1024 measured, profiles/r6_ab_dw_target.txt)
    per = rows_per_split(((out + 63) / 64) * ((in + 63) / 64) * 2, (int)(M / 128));
  }
  if (act16) per = (per + 31) / 32 * 32;            // 32-k slabs of the bf16-stored weight-gradient loop
  const int splits = (int)cdiv64(M, per);
  pw.splits = splits;
  pw.kc_per_split = per;
  pw.c_split_stride = 2 * (int64_t)out * in;    // [split][net][out*in]
  for (int net = 0; net < 2; ++net) {
    pw.op[net].A = w.dZ[net][l];
    pw.op[net].B = l == 0 ? w.xmb : w.H[net][l - 1];
    pw.op[net].C = w.wpart[l] + (int64_t)net * out * in;
    pw.op[net].dbias = w.bpart[l] + (int64_t)net * splits * out;   // [net][split][out]
  }
  return pw;
}

// ------------------------------------------------------------------------------- stage 4: fold + gradient exchange
// Exchange::Buckets, called right after the launch that completes layer l's partials.  Bucket l = {W_l, b_l of both
// networks} (+ heads and log-std with the last hidden layer): its fold and its all-reduce go to the side stream NOW and
// run under the launches of layers l-1 .. 0.  Per element the sums are those of the single fold launch (seg_reduce treats
// every segment independently), the ranges of a bucket are contiguous per network in the flat layout
// (W_l | b_l | W_l+1 ...) and travel as one grouped RCCL operation.
// (the first layer's bucket has nothing left to hide behind - its weight gradient is the last GEMM of the step -
// so it stays on `s`: one fork / join pair less, measured 24 us per step for three forks on a world of one)
int exchange_bucket(catppo_ctx* ctx, const catppo_mlp_layout& L, const catppo_ppo_hparams* hp, Fold& f, int l, int nl,
                    hipStream_t s) {
  hipStream_t bs = l > 0 ? ctx->side : s;
  if (l > 0) {
    CATPPO_HIP_OK(hipEventRecord(ctx->ev_fork[l], s));
    CATPPO_HIP_OK(hipStreamWaitEvent(ctx->side, ctx->ev_fork[l], 0));
  }
  hipLaunchKernelGGL(seg_reduce_kernel, dim3(256, f.segs.n), dim3(256), 0, bs, f.segs, hp->ent_coef, hp->vf_coef,
                     (double*)nullptr, (catppo_iter_state*)nullptr, 0.0, 0.0);
  CATPPO_CHECK_LAUNCH(ctx);
  f.segs.n = 0;
  int64_t off[3], cnt[3];
  int nr = 0;
  const bool last = l == nl - 1;
  for (int net = 0; net < 2; ++net) {
    // end of this network's (W_l, b_l) = start of its next layer; the bucket of the last hidden layer runs on
    // through the head layer to the end of the network's block
    const int64_t end = last ? (net == 0 ? L.off_w[1][0] : L.n_flat) : L.off_w[net][l + 1];
    off[nr] = L.off_w[net][l], cnt[nr] = end - L.off_w[net][l], ++nr;
  }
  if (last) off[nr] = L.off_logstd, cnt[nr] = L.off_w[0][0] - L.off_logstd, ++nr;
  // join BEFORE the first layer's own all-reduce: every operation on the communicator is then ordered by stream
  // dependencies (no two of them concurrently in flight on different streams), inside a captured graph too
  if (l == 0 && nl > 1) CATPPO_HIP_OK(hipStreamWaitEvent(s, ctx->ev_join, 0));
  if (int rc = catppo_internal_allreduce_ranges(ctx, f.grad, off, cnt, nr, bs)) return rc;
  if (l == 1) CATPPO_HIP_OK(hipEventRecord(ctx->ev_join, ctx->side));   // the last forked bucket
  return CATPPO_OK;
}

// Exchange::Tail, called right after dw_fold_kernel: every range of the flat gradient except the first layer's (W0 | b0 of
// both networks) is final now and travels on the side stream under the final fold launch
int exchange_tail_fork(catppo_ctx* ctx, const catppo_mlp_layout& L, Fold& f, hipStream_t s) {
  CATPPO_HIP_OK(hipEventRecord(ctx->ev_fork[0], s));
  CATPPO_HIP_OK(hipStreamWaitEvent(ctx->side, ctx->ev_fork[0], 0));
  int64_t off[3] = {L.off_logstd, L.off_w[0][1], L.off_w[1][1]};      // log-std | critic layers 1.. | actor layers 1..
  int64_t cnt[3] = {L.off_w[0][0] - L.off_logstd, L.off_w[1][0] - L.off_w[0][1], L.n_flat - L.off_w[1][1]};
  if (int rc = catppo_internal_allreduce_ranges(ctx, f.grad, off, cnt, 3, ctx->side)) return rc;
  CATPPO_HIP_OK(hipEventRecord(ctx->ev_join, ctx->side));
  f.tail_forked = true;
  return CATPPO_OK;
}

// Exchange::Tail, behind the final fold launch on `s`: the first layer's own ranges, or the whole gradient
int exchange_tail_join(catppo_ctx* ctx, const catppo_mlp_layout& L, const Fold& f, hipStream_t s) {
  if (f.tail_forked) {      // join first: two operations on one communicator are never in flight on two streams at once
    CATPPO_HIP_OK(hipStreamWaitEvent(s, ctx->ev_join, 0));
    int64_t off[2] = {L.off_w[0][0], L.off_w[1][0]}, cnt[2] = {L.off_w[0][1] - L.off_w[0][0], L.off_w[1][1] - L.off_w[1][0]};
    return catppo_internal_allreduce_ranges(ctx, f.grad, off, cnt, 2, s);
  }
  // shapes whose first-layer weight gradient does not share its launch with the fold: one all-reduce
  int64_t off[1] = {0}, cnt[1] = {L.n_flat};
  return catppo_internal_allreduce_ranges(ctx, f.grad, off, cnt, 1, s);
}

// every split-K / head partial of the minibatch not folded yet is folded into the flat gradient by one launch
int fold_final(catppo_ctx* ctx, const catppo_ppo_hparams* hp, Fold& f, hipStream_t s) {
  NormEmit* ne = f.ne;
  hipLaunchKernelGGL(seg_reduce_kernel, dim3(256, f.segs.n), dim3(256), 0, s, f.segs, hp->ent_coef, hp->vf_coef,
                     ne ? ne->part + ne->n_slots : (double*)nullptr, ne ? ne->st : (catppo_iter_state*)nullptr,
                     ne ? ne->beta1 : 0.0, ne ? ne->beta2 : 0.0);
  catppo_plan_note(ctx, "final fold: seg_reduce_kernel, %d segments x 256 workgroups%s", f.segs.n,
                   ne ? " + squared-norm slots and Adam step advance (one-call optimiser step)" : "");
  CATPPO_CHECK_LAUNCH(ctx);
  if (ne) ne->n_slots += 256 * f.segs.n;
  return CATPPO_OK;
}

// ------------------------------------------------------------------------------- stage 3: backward through the hidden layers
// After step16_kernel every dZ is in memory: all weight gradients in ONE grouped launch of 64x64-tile split-K
// workgroups, the layer with the longest contraction chunks first
int backward_step16(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w,
                    const StepPlan& plan, const catppo_ppo_hparams* hp, int64_t M, Fold& f, hipStream_t s) {
  const int nl = shape->n_hidden;
  DwMulti dm{};
  int order[CATPPO_MAX_HIDDEN];
  for (int l = 0; l < nl; ++l) order[l] = l;
  Params pws[CATPPO_MAX_HIDDEN];
  for (int l = 0; l < nl; ++l) pws[l] = dw_params(shape, L, w, M, plan.act16, l);
  for (int i = 0; i < nl; ++i)
    for (int j = i + 1; j < nl; ++j)
      if (pws[order[j]].kc_per_split > pws[order[i]].kc_per_split) { const int t = order[i]; order[i] = order[j]; order[j] = t; }
  int total = 0;
  for (int i = 0; i < nl; ++i) {
    const Params& pw = pws[order[i]];
    dm.p[i] = pw;
    dm.tiles[i] = tiles_of<64, 64>(pw);
    dm.first[i] = total;
    total += dm.tiles[i] * pw.nets * pw.splits;
  }
  dm.first[nl] = total, dm.n = nl;
  constexpr size_t dw_lds = gemm::smem_bytes<64, 64, false, false>();
  hipLaunchKernelGGL(dw_multi_kernel, dim3((unsigned)total), dim3(256), dw_lds, s, dm);
  catppo_plan_note(ctx, "weight gradients of all %d hidden layers: dw_multi_kernel, %d workgroups of 64x64 split-K tiles, ONE launch", nl, total);
  CATPPO_CHECK_LAUNCH(ctx);
  for (int l = nl - 1; l >= 0; --l) {
    add_layer_segs(f, shape, L, w, l, pws[l].splits);
    if (l == nl - 1) add_head_segs(f, shape, L, w, plan, hp);
  }
  return CATPPO_OK;
}

// data-gradient problem of hidden layer l > 0: dZ_{l-1} = (dZ_l . W_l) * elu'(H_{l-1})
Params dx_params(const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w, const float* params, int64_t M,
                 bool act16, int l) {
  const int out = shape->hidden[l], in = L.in_dim[l];
  Params px{};
  px.nets = 2, px.splits = 1;
  px.I = (int)M, px.J = in, px.Kc = out;
  px.lda = out, px.ldb = in, px.ldc = in, px.ldaux = in;
  for (int net = 0; net < 2; ++net) {
    px.op[net].A = w.dZ[net][l];
    px.op[net].B = params + L.off_w[net][l];
    px.op[net].C = w.dZ[net][l - 1];
    px.op[net].aux = w.H[net][l - 1];
  }
  if (act16) {
    // dZ_l (A) and the transposed bf16 weight copy (B, [in][out]) are K-contiguous: contraction sizes in FLOAT units;
    // aux (H_{l-1}) and the output dZ_{l-1} are bf16-stored: ldaux / ldc in bf16 elements
    px.Kc = out / 2, px.lda = out / 2, px.ldb = out / 2;
    for (int net = 0; net < 2; ++net) px.op[net].B = reinterpret_cast<const float*>(w.w16t + L.off_w[net][l]);
  }
  return px;
}

// The first layer's weight gradient: the last GEMM of the step.  It shares its launch with the fold of the layers above
// it (dw_fold_kernel) when it is the plain 64x64-tile launch; CATPPO_DW0_FOLD=0 keeps GEMM and fold apart (A/B).
// (measured and removed: a 256 x 64 tile for the narrow first layer - one workgroup per CU owning all 256
// output rows of a network for its slice of the batch, dZ_0 and the observations read once - was 3.5 us per step
// SLOWER than the 64x64 tiling, 9.48 vs 9.39 ms of update phase, profiles/r4_ab_dw0_tile.txt: twice the partial
// bytes for the fold and 64 single-dword write-through stores per lane in the epilogue of a workgroup that only
// multiplies 8 slabs)
// (measured and removed, again: 128x64 tiles for this GEMM - two accumulators per wave, the observations read once per 128 rows, partials
//  through the staged 16-byte stores the first attempt did not have - measured 3 us per step SLOWER at cfg2 and at the reference shapes)
int backward_first_layer(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const StepPlan& plan,
                         const catppo_ppo_hparams* hp, const Params& pw, Fold& f, hipStream_t s) {
  const int out = shape->hidden[0], in = L.in_dim[0], splits = pw.splits, per = pw.kc_per_split, bf16 = shape->mfma_bf16;
  const bool dw_with_fold = switches().dw0_fold && plan.exch != Exchange::Buckets && f.segs.n > 0 &&
                            (plan.act16 || !(pw.I >= 128 && pw.J >= 128 && pw.kc_per_split >= 256));      // launch_gemm_auto's 128x128 rule
  if (!dw_with_fold) {
    if (plan.act16) launch_gemm_prec<64, 64, false, false, gemm::EPI_PARTIAL, 5>(pw, s);     // bf16-stored dZ_0, fp32 observations
    else launch_gemm_auto<false, false, gemm::EPI_PARTIAL>(pw, s, bf16);
    catppo_plan_note(ctx, "layer %d weight gradient (%d x %d, %d splits of %d rows): gemm_f32_kernel, split-K partials "
                     "[own launch: first layer without the fold (precision %d / switches)]", 0, out, in, splits, per, bf16);
    CATPPO_CHECK_LAUNCH(ctx);
    return CATPPO_OK;
  }
  const int t64 = tiles_of<64, 64>(pw), n_gemm = t64 * pw.nets * pw.splits;
  constexpr size_t lds = gemm::smem_bytes<64, 64, false, false>();
  static_assert(lds >= 4096, "the fold workgroups use 1024 floats of the same allocation");
  const dim3 grid((unsigned)(n_gemm + kFoldX * f.segs.n));
  double* nslots = f.ne ? f.ne->part + f.ne->n_slots : (double*)nullptr;
  dispatch_value<0, 1, 2, 5>(plan.act16 ? 5 : bf16, [&](auto prec) {
    hipLaunchKernelGGL(dw_fold_kernel<decltype(prec)::value>, grid, dim3(256), lds, s, pw, f.segs, t64, n_gemm, hp->ent_coef,
                       hp->vf_coef, nslots);
  });
  CATPPO_CHECK_LAUNCH(ctx);
  catppo_plan_note(ctx, "layer 0 weight gradient (%d x %d, %d splits of %d rows) + fold of the %d partial segments of the other "
                   "layers / heads: dw_fold_kernel, %d + %d workgroups", out, in, splits, per, f.segs.n, n_gemm, kFoldX * f.segs.n);
  if (f.ne) f.ne->n_slots += kFoldX * f.segs.n;
  f.segs.n = 0;        // folded; what is added afterwards (this layer's own partials) goes to the final fold launch
  if (plan.exch == Exchange::Tail) return exchange_tail_fork(ctx, L, f, s);
  return CATPPO_OK;
}

// Per hidden layer above the first ONE launch holding the split-K weight-gradient GEMM and the data-gradient GEMM
// (gemm_pair_kernel), then the first layer's weight gradient; every layer with its own partial buffers.
int backward_layers(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w,
                    const StepPlan& plan, const catppo_ppo_hparams* hp, const float* params, int64_t M, Fold& f, hipStream_t s) {
  const int nl = shape->n_hidden, bf16 = shape->mfma_bf16;   // 0 fp32 MFMA, 1 bf16 operands, 2 split-bf16 (bf16x3)
  for (int l = nl - 1; l >= 0; --l) {
    const int out = shape->hidden[l], in = L.in_dim[l];
    const Params pw = dw_params(shape, L, w, M, plan.act16, l);
    const int splits = pw.splits, per = pw.kc_per_split;
    if (l == 0)
      if (int rc = backward_first_layer(ctx, shape, L, plan, hp, pw, f, s)) return rc;
    add_layer_segs(f, shape, L, w, l, splits);
    if (l == nl - 1) add_head_segs(f, shape, L, w, plan, hp);
    if (l > 0) {
      const Params px = dx_params(shape, L, w, params, M, plan.act16, l);
      if (plan.act16) {
        launch_dw_dx_pair<true>(pw, px, s, 3, ctx->n_cu);
        catppo_plan_note(ctx, "layer %d weight gradient (%d x %d, %d splits of %d rows) + data gradient (%lld x %d, k = %d): "
                         "gemm_pair_kernel on bf16-stored operands, ONE launch", l, out, in, splits, per, (long long)M, in, out);
      } else {
        launch_dw_dx_pair<false>(pw, px, s, bf16, ctx->n_cu);
        catppo_plan_note(ctx, "layer %d weight gradient (%d x %d, %d splits of %d rows) + data gradient (%lld x %d, k = %d): "
                         "gemm_pair_kernel, ONE launch%s", l, out, in, splits, per, (long long)M, in, out,
                         M <= kSmallRows ? " [<= 4096 rows: 64x64 weight-gradient tiles]" : "");
      }
      CATPPO_CHECK_LAUNCH(ctx);
    }
    // a bucket is enqueued right after the launch that completes its layer's partials
    if (plan.exch == Exchange::Buckets)
      if (int rc = exchange_bucket(ctx, L, hp, f, l, nl, s)) return rc;
  }
  return CATPPO_OK;
}
#undef CATPPO_HIP_OK
