// The optimiser step's launch plan: what a minibatch of a shape gets (decide_step, no HIP call in it) and the stage that
// runs its forward and heads.  The backward and the fold / gradient exchange are mlp_backward.h's host functions; mlp.hip's
// minibatch_grad_core is the list of stages.  Part of mlp.hip's translation unit (see mlp_common.h).
#pragma once

enum class FwdForm {      // forward of the hidden layers (below the last one when the head form computes that itself)
  Step16,                 // step16_kernel: the whole step up to the data gradients in one launch of 16-row tiles
  Act16,                  // layer-wise, bf16-STORED activations and weight copies (bf16 operands, gemm_f32.h "act16")
  Rows,                   // rows_fwd_kernel<64>: one row-resident launch, every layer 256 wide
  RowsWide,               // rows_fwd_wide_kernel<64>: the same for 128 / 256 / (512 first) wide layers
  Layers                  // one GEMM launch per layer
};
enum class HeadForm { Step16, FwdHead, HeadLoss, HeadLossWide };      // heads + PPO loss + head backward: inside step16_kernel |
                                                                      // with the last hidden layer | own launch | own launch, A >= 16
enum class Exchange { None = 0, Buckets, Tail };                          // gradient all-reduce inside the step (catppo_set_grad_overlap)

struct StepPlan {
  FwdForm fwd;
  HeadForm head;
  Exchange exch;
  bool act16;             // activations, dZ and weight copies stored as bf16 from the forward to the weight gradients
  int nbh;                // head partial rows (per network when head_by_net)
  bool head_by_net;       // head partial rows [0, nbh) actor, [nbh, 2 nbh) critic
  HeadLossTiling tile;    // HeadLoss
  FusedFwdArgs rows;      // Rows / RowsWide: the per-path fields and LDS bytes of their plan,
  size_t rows_lds;
  int rows_nch;           //   chunks of the first layer (RowsWide; 0: Rows)
};

StepPlan decide_step(const catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w, int64_t M) {
  const MlpSwitches& sw = switches();
  const int nl = shape->n_hidden, A = shape->act_dim, HL = shape->hidden[nl - 1];
  StepPlan p{};
  // Large minibatches: the last hidden layer, the heads, the loss and the backward through the heads are ONE
  // launch (fwd_head_kernel).  Needs the full last-layer width in one tile (128 or 256 columns), a 16-aligned
  // contraction, and enough 64-row tiles to fill the chip (otherwise the 64x64-tile GEMM + head_loss pair has more
  // workgroups).  CATPPO_FUSED_HEAD=0 keeps the two launches.
  const bool fused_head = sw.fused_head && (HL == 128 || HL == 256) && nl >= 2 && L.in_dim[nl - 1] % gemm::BK == 0 &&
                          2 * cdiv64(M, 64) >= sw.fused_head_min_wg && A <= 15;
  // bf16 operands (BASELINE configs[4]): activations and dZ STORED as bf16, bf16 weight copies (gemm_f32.h "act16").
  // Needs the fused head launch (the 64-row head_loss path reads fp32 activations) and no per-layer gradient buckets.
  // CATPPO_ACT16=0: fp32-stored activations rounded at every use (A/B).
  p.act16 = sw.act16 && shape->mfma_bf16 == 1 && fused_head && ctx->grad_overlap != 1 && w.w16 != nullptr;
  if (sw.step16 && M <= sw.step16_max_rows && step16_applies(shape, L, M)) {
    p.fwd = FwdForm::Step16, p.head = HeadForm::Step16;
    p.nbh = (int)cdiv64(M, step16::kR), p.head_by_net = true;
  } else if (fused_head) {
    // hidden layers below the last: ONE row-resident launch (fwd_rows.h) when the minibatch has enough 64-row tiles, else
    // the layer-wise GEMM launches.  CATPPO_ROWS_FWD=0 keeps the latter, CATPPO_ROWS_WIDE=0 for the wide kernel only (A/B).
    const bool rows_window = sw.rows_fwd && M >= sw.rows_fwd_min_rows && M <= (1 << 20);
    p.head = HeadForm::FwdHead;
    p.nbh = (int)cdiv64(M, 64), p.head_by_net = true;
    if (p.act16) {
      p.fwd = FwdForm::Act16;
    } else if (rows_window && nl - 1 <= 3 && rows_fwd_plan(shape, L, nl - 1, 64, &p.rows, &p.rows_lds)) {
      p.fwd = FwdForm::Rows;
    } else {
      p.rows = FusedFwdArgs{};
      p.fwd = sw.rows_wide && rows_window && rows_wide_plan(shape, L, nl - 1, 64, &p.rows, &p.rows_lds, &p.rows_nch)
                  ? FwdForm::RowsWide : FwdForm::Layers;
    }
  } else {
    p.fwd = FwdForm::Layers;
    if (A >= kMaxA) {
      p.head = HeadForm::HeadLossWide;
      p.nbh = (int)cdiv64(M, kWideHeadRows);
      if (p.nbh > kHeadMaxBlocks) p.nbh = kHeadMaxBlocks;
    } else {
      p.head = HeadForm::HeadLoss;
      p.tile = head_loss_tiling(HL, M);
      p.nbh = p.tile.blocks;
    }
  }
  // catppo_set_grad_overlap + a communicator.  Buckets: fold and all-reduce the gradient per layer on the side stream while
  // the backward launches of the layers below run (exchange_bucket).  Tail: no extra launch; the ranges that are final after
  // dw_fold_kernel travel on the side stream under the final fold launch, the first layer's own ranges behind it.  The
  // 16-row step has no per-layer launches to hide buckets behind: with either mode it folds once and reduces the whole
  // gradient in one grouped operation (the tail form without its fork).
  if (ctx->comm != nullptr && ctx->grad_overlap == 1 && p.fwd != FwdForm::Step16) p.exch = Exchange::Buckets;
  else if (ctx->comm != nullptr && (ctx->grad_overlap == 1 || ctx->grad_overlap == 2)) p.exch = Exchange::Tail;
  return p;
}

// Stage 2: forward, heads, PPO loss and the gradient w.r.t. the last hidden pre-activations (cleanrl/ppo.py:304-351)
int step_forward_heads(catppo_ctx* ctx, const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const MlpWs& w,
                       const StepPlan& plan, const float* params, const HeadArgs& g, hipStream_t s) {
  const MlpSwitches& sw = switches();
  const int nl = shape->n_hidden, A = shape->act_dim, HL = shape->hidden[nl - 1];
  const int64_t M = g.M;
  if (plan.fwd == FwdForm::Step16) {
    launch_step16(ctx, shape, L, w, params, g, s);
    CATPPO_CHECK_LAUNCH(ctx);
    return CATPPO_OK;
  }
  if (plan.head != HeadForm::FwdHead) {
    forward_hidden(shape, L, params, w.xmb, M, w, 0, 2, s);      // every hidden layer, both nets per launch
    CATPPO_CHECK_LAUNCH(ctx);
    if (plan.head == HeadForm::HeadLossWide) {
      launch_head_loss_wide(g, HL, plan.nbh, s);
      catppo_plan_note(ctx, "minibatch %lld rows: %d layer-wise forward GEMM launches + head_loss_wide_kernel (%d-row tiles, %d blocks) "
                       "[act_dim %d >= %d: the 16-slot head kernels do not apply]", (long long)M, nl, kWideHeadRows, plan.nbh, A, kMaxA);
    } else {
      launch_head_loss(g, HL, plan.tile, s);
      catppo_plan_note(ctx, "minibatch %lld rows: %d layer-wise forward GEMM launches + head_loss_kernel (%d-row tiles, %d blocks) "
                       "[fused last-layer launch needs a 128 / 256-wide last layer and >= %d workgroups = %d rows]",
                       (long long)M, nl, plan.tile.rows, plan.nbh, sw.fused_head_min_wg, sw.fused_head_min_wg * 32);
    }
    CATPPO_CHECK_LAUNCH(ctx);
    return CATPPO_OK;
  }
  if (plan.fwd == FwdForm::Act16) {
    // bf16 copies of W_1 .. W_{nl-1} (as stored and transposed) + the layer-wise forward with bf16-stored activations
    const int64_t tot = forward_hidden16(shape, L, params, w.xmb, M, w, 2, s, nl - 1, false);
    catppo_plan_note(ctx, "minibatch %lld rows, bf16-stored activations: fwd0_w16_kernel (layer 0 + %lld weights as bf16, stored + "
                     "transposed, in one launch) + %d layer-wise forward GEMM launch(es) on bf16-stored operands", (long long)M,
                     (long long)tot, nl - 2);
  } else if (plan.fwd == FwdForm::Rows || plan.fwd == FwdForm::RowsWide) {
    FusedFwdArgs a = plan.rows;
    a.x = w.xmb, a.params = params, a.M = M, a.net0 = 0, a.do_head = 0;
    for (int net = 0; net < 2; ++net)
      for (int l = 0; l < nl - 1; ++l) a.Hout[net][l] = w.H[net][l];
    rows_launch_train(a, plan.rows_lds, plan.rows_nch, M, ctx->n_cu, s);
    if (plan.fwd == FwdForm::Rows)
      catppo_plan_note(ctx, "minibatch %lld rows, forward of hidden layers 0..%d: rows_fwd_kernel<64>, %lld row tiles, %s "
                       "[all 256 wide, >= %d rows, fp32]", (long long)M, nl - 2, (long long)cdiv64(M, 64),
                       cdiv64(M, 64) >= ctx->n_cu ? "one workgroup walks both networks" : "one workgroup per (tile, network)",
                       sw.rows_fwd_min_rows);
    else
      catppo_plan_note(ctx, "minibatch %lld rows, forward of hidden layers 0..%d: rows_fwd_wide_kernel<64>, %lld row tiles "
                       "[first layer %d wide in %d chunk(s), other layers 128 / 256, padded observations <= 64, >= %d rows, fp32]",
                       (long long)M, nl - 2, (long long)cdiv64(M, 64), shape->hidden[0], plan.rows_nch, sw.rows_fwd_min_rows);
  } else {
    forward_hidden(shape, L, params, w.xmb, M, w, 0, 2, s, nl - 1);
    catppo_plan_note(ctx, "minibatch %lld rows, forward of hidden layers 0..%d: %d layer-wise GEMM launches "
                     "[not row-resident: < %d rows, operand precision %d, a width outside {128, 256, (512 first)}, or "
                     "padded observations > 64 with a non-256 layer]", (long long)M, nl - 2, nl - 1, sw.rows_fwd_min_rows, shape->mfma_bf16);
  }
  CATPPO_CHECK_LAUNCH(ctx);
  const int prec = plan.act16 ? 3 : shape->mfma_bf16;
  launch_fwd_head(shape, L, w, params, M, prec, g, s);
  catppo_plan_note(ctx, "last hidden layer + heads + PPO loss + head backward: fwd_head_kernel<%d, prec %d>, %d tiles x 2 networks "
                   "[last layer 128 / 256 wide and >= %d workgroups]", HL, prec, plan.nbh, sw.fused_head_min_wg);
  CATPPO_CHECK_LAUNCH(ctx);
  return CATPPO_OK;
}
