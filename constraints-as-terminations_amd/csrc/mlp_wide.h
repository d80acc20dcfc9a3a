// Wide heads: 16 <= A <= 63 action dimensions (kMaxAWide).  The kernels of mlp_forward.h / mlp_loss.h / step16.h keep the A
// actor outputs and the critic output in the 16 slots of reduce16; here the A + 1 outputs of a row live in the 64 lanes of
// ONE wave instead: lane k < A owns action dimension k, lane kVSW = 63 the critic output.  Rollout head (head_act_wide_kernel)
// and heads + PPO loss + head backward (head_loss_wide_kernel) on the activations the layer-wise forward stored; the hidden
// layers, the backward below the heads and the fold are the A-generic launches of the narrow path.  VALU / LDS only: the
// head is 2 * HL * (A + 1) FLOP per row against ~580k for both 3 x 256 networks.  Part of mlp.hip's translation unit.
#pragma once

constexpr int kVSW = 63;                 // lane of the critic output (A <= 62 actor lanes never reach it, A = 63 uses 0..62)

// 64 per-lane partial values -> their 64-lane totals with 63 cross-lane exchanges (reduce16's butterfly, six levels): every
// step halves the live values, the lane keeping the half selected by its own bit.  Afterwards lane l holds the total of value l.
__device__ __forceinline__ float reduce64(float (&v)[64], int lane) {
  float a[32], b[16], c[8], d[4], e[2];
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4, h1 = lane & 2, h0 = lane & 1;
#pragma unroll
  for (int j = 0; j < 32; ++j) a[j] = (h5 ? v[j + 32] : v[j]) + __shfl_xor(h5 ? v[j] : v[j + 32], 32, 64);
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = (h4 ? a[j + 16] : a[j]) + __shfl_xor(h4 ? a[j] : a[j + 16], 16, 64);
#pragma unroll
  for (int j = 0; j < 8; ++j) c[j] = (h3 ? b[j + 8] : b[j]) + __shfl_xor(h3 ? b[j] : b[j + 8], 8, 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = (h2 ? c[j + 4] : c[j]) + __shfl_xor(h2 ? c[j] : c[j + 4], 4, 64);
#pragma unroll
  for (int j = 0; j < 2; ++j) e[j] = (h1 ? d[j + 2] : d[j]) + __shfl_xor(h1 ? d[j] : d[j + 2], 2, 64);
  return (h0 ? e[1] : e[0]) + __shfl_xor(h0 ? e[0] : e[1], 1, 64);
}

// the A actor dot products of one row (lane-owned CPL columns of the row in ha), slots >= A zero; W: [A][HL] in LDS or global
template <int CPL>
__device__ __forceinline__ void wide_actor_dots(const float* __restrict__ W, const float (&ha)[CPL], int A, int lane,
                                                float (&part)[64]) {
  constexpr int HL = CPL * 64;
#pragma unroll
  for (int k = 0; k < kVSW; ++k) {
    float d = 0.0f;
    if (k < A) {                          // wave-uniform
      float wk[CPL];
      load_vec<CPL>(W + k * HL + lane * CPL, wk);
#pragma unroll
      for (int c = 0; c < CPL; ++c) d = fmaf(ha[c], wk[c], d);
    }
    part[k] = d;
  }
}

// actor head weights: staged in LDS up to HL = 256 (A x HL <= 64.5 KB), read through the caches at HL = 512 (up to 129 KB)
template <int CPL>
constexpr bool wide_w_lds() { return CPL <= 4; }

// ------------------------------------------------------------------------------- rollout head, A >= 16
// One wave per row, as head_act_kernel; Philox convention of catppo.h (counter {env, k / 4, step, iteration}, lane k % 4), so
// dimension k draws the same noise whatever A is.  Ha == nullptr: critic only (the bootstrap value), the same critic sum
// order as the full call (lane 63's total in reduce64 does not depend on the other lanes' values): bit-identical values.
template <int CPL>
__global__ __launch_bounds__(256) void head_act_wide_kernel(const float* __restrict__ Hc, const float* __restrict__ Ha,
                                                            const float* __restrict__ W4c, const float* __restrict__ b4c,
                                                            const float* __restrict__ W4a, const float* __restrict__ b4a,
                                                            const float* __restrict__ logstd,
                                                            const float* __restrict__ eps,
                                                            const float* __restrict__ given, int64_t M, int A,
                                                            float* __restrict__ action, float* __restrict__ logprob,
                                                            void* __restrict__ value_out, int value_f16,
                                                            const catppo_iter_state* __restrict__ rng_state, int rng_step,
                                                            float* __restrict__ eps_out) {
  constexpr int HL = CPL * 64;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [A*HL] actor head weights (wide_w_lds)
  const int lane = threadIdx.x & 63;
  const int64_t wave_id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * 4;
  const bool actor = Ha != nullptr;
  if (!actor) A = 0;
  const float* W = W4a;
  if constexpr (wide_w_lds<CPL>()) {
    for (int o = threadIdx.x; o < A * HL; o += 256) lds[o] = W4a[o];
    __syncthreads();
    W = lds;
  }
  float wc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) wc[c] = W4c[lane * CPL + c];
  const float bc = b4c[0];
  const bool mine = lane < A;
  const float sd = mine ? expf(logstd[lane]) : 1.0f;
  const float var = sd * sd, lsd = logf(sd);
  const float ba = mine ? b4a[lane] : 0.0f;
  uint32_t rk0 = 0, rk1 = 0, rit = 0;
  if (rng_state != nullptr) {
    const uint64_t sd64 = rng_state->seed;
    rk0 = (uint32_t)sd64, rk1 = (uint32_t)(sd64 >> 32), rit = (uint32_t)rng_state->iteration;
  }
  for (int64_t i = wave_id; i < M; i += n_waves) {
    float ha[CPL], part[64];
    if (actor) load_vec<CPL>(Ha + i * HL + lane * CPL, ha);
    wide_actor_dots<CPL>(W, ha, A, lane, part);      // (A = 0: zeros)
    {
      float hc[CPL], dc = 0.0f;
      load_vec<CPL>(Hc + i * HL + lane * CPL, hc);
#pragma unroll
      for (int c = 0; c < CPL; ++c) dc = fmaf(hc[c], wc[c], dc);
      part[kVSW] = dc;
    }
    const float tot = reduce64(part, lane);
    const float v = lane_bcast(tot, kVSW) + bc;
    if (lane == 0) {
      if (value_f16) reinterpret_cast<_Float16*>(value_out)[i] = (_Float16)v;
      else reinterpret_cast<float*>(value_out)[i] = v;
    }
    if (!actor) continue;
    const float mu = tot + ba;
    float a = mu;
    if (mine && given != nullptr) {
      a = given[i * A + lane];
    } else if (mine && rng_state != nullptr) {
      const rng::u32x4 blk = rng::philox4x32_10(rng::u32x4{(uint32_t)i, (uint32_t)(lane >> 2), (uint32_t)rng_step, rit},
                                                rk0, rk1);
      const float e = rng::box_muller_pick(blk, lane & 3);
      a = mu + sd * e;
      if (eps_out != nullptr) eps_out[i * A + lane] = e;
    } else if (mine && eps != nullptr) {
      a = mu + sd * eps[i * A + lane];
    }
    const float diff = a - mu;
    const float term = mine ? (-(diff * diff) / (2.0f * var) - lsd - kHalfLog2Pi) : 0.0f;
    const float lp = wave_sum(term);
    if (mine) action[i * A + lane] = a;
    if (lane == 0) logprob[i] = lp;
  }
}

// ------------------------------------------------------------------------------- heads + PPO loss + head backward, A >= 16
// head_loss_kernel's contract and arithmetic (HeadArgs, per-block partials [nblk][(A+1)*HL] / [nblk][2A+1+8], clip-branch codes)
// with the A + 1 outputs of a row in the 64 lanes of its wave:
//   phase 1 (wave per row)  A + 1 dot products (reduce64), log-prob, clipped losses, d loss/d mu, d loss/d v; dZ of the last
//           hidden layer of both networks stored; the row's head gradients to an LDS [TR][64] tile (lane k -> column k)
//   phase 2 (thread per weight column and a group of KPG slots)  dW4 += G^T . H over the tile's rows, in registers
//           across the tiles of the block
constexpr int kWideHeadThreads = 512;
constexpr int kWideScal = 2 * (kMaxAWide - 1) + 1 + kHeadDiag + 1;   // LDS floats for the NS <= 135 block scalars
constexpr int kWideHeadRows = 16;       // row tile: 16-row tiles keep 128+ workgroups busy from 2048 rows up
template <int CPL>
inline size_t wide_head_lds_bytes(int A) {
  constexpr int HL = CPL * 64, TR = kWideHeadRows;
  const size_t w = wide_w_lds<CPL>() ? (size_t)A * HL : 0;
  return sizeof(float) * (w + 2 * (size_t)TR * HL + (size_t)TR * 64 + kWideScal + 4);
}

template <int CPL>
__global__ __launch_bounds__(kWideHeadThreads, 1) void head_loss_wide_kernel(const HeadArgs g) {
  constexpr int HL = CPL * 64;
  constexpr int NT = kWideHeadThreads, NW = NT / 64;
  constexpr int TR = kWideHeadRows;
  constexpr int RPW = TR / NW;                          // rows per wave and tile
  constexpr int NG = NT / HL;                           // phase-2 thread groups (HL <= 512)
  constexpr int KPG = 64 / NG;                          // head outputs per group (64 lanes)
  static_assert(NG >= 1 && KPG % 4 == 0 && RPW >= 1, "tile shape");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int A = g.A;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NS = 2 * A + 1 + kHeadDiag;
  constexpr int WF = wide_w_lds<CPL>() ? 1 : 0;
  float* s_wa = lds;                                    // [A*HL]  actor head weights (WF)
  float* sHa = s_wa + WF * A * HL;                      // [TR*HL] actor last-hidden tile   (16-B aligned: A*HL % 64 == 0)
  float* sHc = sHa + TR * HL;                           // [TR*HL] critic last-hidden tile
  float* sG = sHc + TR * HL;                            // [TR*64] per-row head gradients: d mu_k (k<A), 0, ..., d v at kVSW
  float* ls = sG + TR * 64;                             // [NS]    scalars: db4a[A], db4c, dlogstd[A], diag[8]
  float* s_adv = ls + kWideScal;                        // [2]     advantage mean, std + 1e-8

  const float* W = g.W4a;
  if constexpr (WF) {
    for (int o = tid; o < A * HL; o += NT) s_wa[o] = g.W4a[o];
    W = s_wa;
  }
  if (wave == 0) {                                      // advantage statistics (ppo.py:314-318), as head_loss_kernel
    if (g.hp.norm_adv && g.adv_stats == nullptr) {
      double a1 = 0.0, a2 = 0.0;
      for (int b = lane; b < g.n_adv_part; b += 64) {
        a1 += g.adv_part[2 * b];
        a2 += g.adv_part[2 * b + 1];
      }
      a1 = wave_sum_d(a1);
      a2 = wave_sum_d(a2);
      if (lane == 0) {
        const double n = (double)g.M;
        const double mean = a1 / n;
        double var = (a2 - n * mean * mean) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        s_adv[0] = (float)mean;
        s_adv[1] = (float)sqrt(var) + 1e-8f;
      }
    } else if (lane == 0) {
      s_adv[0] = g.adv_stats ? g.adv_stats[0] : 0.0f;
      s_adv[1] = g.adv_stats ? g.adv_stats[1] : 1.0f;
    }
  }
  __syncthreads();
  const float adv_mean = s_adv[0], adv_den = s_adv[1];
  const float clipc = g.hp.clip_coef, invM = g.hp.inv_global_batch;
  const float vden = sqrtf(g.vrms_var[0] + 1e-8f), vmean = g.vrms_mean[0];
  const bool norm_adv = g.hp.norm_adv != 0, clip_vloss = g.hp.clip_vloss != 0;
  const float ent_coef_m = g.hp.ent_coef * invM, vf_half = g.hp.vf_coef * 0.5f;

  const bool mine = lane < A;                           // lane k owns action dimension k
  const float sd = mine ? expf(g.logstd[lane]) : 1.0f;
  const float var = sd * sd, lsd = logf(sd);
  const float ba = mine ? g.b4a[lane] : 0.0f;
  const float ent_row = wave_sum(mine ? kEntConst + lsd : 0.0f);   // entropy is state independent
  float gls = 0.0f;                                     // d loss / d logstd_k (lane k)
  float d_pg = 0.0f, d_v = 0.0f, d_ent = 0.0f, d_kl = 0.0f, d_okl = 0.0f, d_cf = 0.0f;
  float wc[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) wc[c] = g.W4c[lane * CPL + c];
  const float bc = g.b4c[0];

  // phase-2 ownership: weight column c2, slots [k0, k0 + KPG) (a wave lies inside one group: HL >= 64)
  const int c2 = tid % HL, k0 = (tid / HL) * KPG;
  float acc[KPG];
#pragma unroll
  for (int kk = 0; kk < KPG; ++kk) acc[kk] = 0.0f;
  float accb = 0.0f;                                    // bias gradients: threads 0..63 (one per slot)

  const int64_t n_tiles = (g.M + TR - 1) / TR;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = tile * TR;
    const int rows = (int)((g.M - row0) < TR ? (g.M - row0) : TR);
    // ------------------------------------------------------------------ phase 1
    for (int rr = 0; rr < RPW; ++rr) {
      const int r = wave * RPW + rr;
      if (r >= rows) break;                             // wave-uniform
      const int64_t i = row0 + r;
      float hc[CPL], ha[CPL], part[64];
      load_vec<CPL>(g.Hc + i * HL + lane * CPL, hc);
      load_vec<CPL>(g.Ha + i * HL + lane * CPL, ha);
      const float a_taken = mine ? g.act[i * A + lane] : 0.0f;
      const float oldlogp = g.oldlogp[i], adv_raw = g.adv[i], R = g.ret_n[i], Vo = g.val_n[i];
      store_vec<CPL>(sHc + r * HL + lane * CPL, hc);
      store_vec<CPL>(sHa + r * HL + lane * CPL, ha);
      wide_actor_dots<CPL>(W, ha, A, lane, part);
      {
        float d = 0.0f;
#pragma unroll
        for (int c = 0; c < CPL; ++c) d = fmaf(hc[c], wc[c], d);
        part[kVSW] = d;
      }
      const float tot = reduce64(part, lane);           // lane k < A: mu_k - bias; lane kVSW: critic output - bias
      const float mu = tot + ba;
      const float v = lane_bcast(tot, kVSW) + bc;

      const float diff = mine ? a_taken - mu : 0.0f;
      const float term = mine ? -(diff * diff) / (2.0f * var) - lsd - kHalfLog2Pi : 0.0f;
      const float newlogp = wave_sum(term);
      const float logratio = newlogp - oldlogp;
      const float ratio = expf(logratio);
      d_okl += -logratio;
      d_kl += (ratio - 1.0f) - logratio;
      d_cf += fabsf(ratio - 1.0f) > clipc ? 1.0f : 0.0f;

      const float adv = norm_adv ? (adv_raw - adv_mean) / adv_den : adv_raw;
      const float rc = ratio < 1.0f - clipc ? 1.0f - clipc : (ratio > 1.0f + clipc ? 1.0f + clipc : ratio);
      const float pg1 = -adv * ratio, pg2 = -adv * rc;
      const bool inside = ratio >= 1.0f - clipc && ratio <= 1.0f + clipc;
      const float dr_tie = 0.5f * -adv + (inside ? 0.5f * -adv : 0.0f);
      const float dr = pg1 > pg2 ? -adv : (pg1 < pg2 ? (inside ? -adv : 0.0f) : dr_tie);
      d_pg += pg1 > pg2 ? pg1 : pg2;
      const float g_logp = dr * ratio * invM;

      const float nv = (v - vmean) / vden;
      const float e1 = nv - R;
      const float vl1 = e1 * e1;
      const float dl = nv - Vo;
      const float cl = dl < -clipc ? -clipc : (dl > clipc ? clipc : dl);
      const float e2 = (Vo + cl) - R;
      const float vl2 = e2 * e2;
      const bool in2 = dl >= -clipc && dl <= clipc;
      const float dnv_c = vl1 > vl2 ? 2.0f * e1 : (vl1 < vl2 ? (in2 ? 2.0f * e2 : 0.0f) : e1 + (in2 ? e2 : 0.0f));
      const float vl = clip_vloss ? (vl1 > vl2 ? vl1 : vl2) : vl1;
      const float dnv = clip_vloss ? dnv_c : 2.0f * e1;
      d_v += 0.5f * vl;
      d_ent += ent_row;
      if (g.branch_out != nullptr && lane == 0) {
        g.branch_out[i] = clip_code(ratio, 1.0f, clipc);
        g.branch_out[g.M + i] = clip_code(dl, 0.0f, clipc) | ((vl1 > vl2 ? 1 : (vl1 < vl2 ? 2 : 0)) << 2);
      }
      const float g_v = vf_half * dnv * invM / vden;

      // ---- backward through the heads
      const float gm = mine ? g_logp * diff / var : 0.0f;
      if (mine) gls += g_logp * (diff * diff / var - 1.0f) - ent_coef_m;
      sG[r * 64 + lane] = lane == kVSW ? g_v : gm;
      float dha[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) dha[c] = 0.0f;
#pragma unroll
      for (int k = 0; k < kVSW; ++k) {
        if (k < A) {                                    // wave-uniform
          const float gmk = lane_bcast(gm, k);
          float wk[CPL];
          load_vec<CPL>(W + k * HL + lane * CPL, wk);
#pragma unroll
          for (int c = 0; c < CPL; ++c) dha[c] = fmaf(gmk, wk[c], dha[c]);
        }
      }
      float oa[CPL], oc[CPL];
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        oa[c] = dha[c] * (ha[c] > 0.0f ? 1.0f : ha[c] + 1.0f);
        oc[c] = (g_v * wc[c]) * (hc[c] > 0.0f ? 1.0f : hc[c] + 1.0f);
      }
      store_vec_wt<CPL>(g.dZa + i * HL + lane * CPL, oa);
      store_vec_wt<CPL>(g.dZc + i * HL + lane * CPL, oc);
    }
    __syncthreads();
    // ------------------------------------------------------------------ phase 2: dW4 += G^T . H
    const bool grp_live = k0 < A || k0 + KPG > kVSW;   // wave-uniform: a group of unused slots only adds zeros
    if (grp_live) {
      for (int r = 0; r < rows; ++r) {
        const float ha2 = sHa[r * HL + c2], hc2 = sHc[r * HL + c2];
#pragma unroll
        for (int q = 0; q < KPG / 4; ++q) {
          const float4 gk = *reinterpret_cast<const float4*>(sG + r * 64 + k0 + 4 * q);
          const int k = k0 + 4 * q;
          acc[4 * q] = fmaf(gk.x, ha2, acc[4 * q]);
          acc[4 * q + 1] = fmaf(gk.y, ha2, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(gk.z, ha2, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(gk.w, k + 3 == kVSW ? hc2 : ha2, acc[4 * q + 3]);
        }
      }
    }
    if (tid < 64) {
      for (int r = 0; r < rows; ++r) accb += sG[r * 64 + tid];
    }
    __syncthreads();
  }

  // ---- per-block partials: weight gradients straight from the phase-2 registers, scalars through LDS
  float* pw = g.part_w + (int64_t)blockIdx.x * (A + 1) * HL;   // rows 0..A-1 = dW4a, row A = dW4c
#pragma unroll
  for (int kk = 0; kk < KPG; ++kk) {
    const int k = k0 + kk;
    if (k < A) pw[k * HL + c2] = acc[kk];
    else if (k == kVSW) pw[A * HL + c2] = acc[kk];
  }
  for (int w = 0; w < NW; ++w) {                        // fixed wave order => deterministic
    if (wave == w) {
      if (mine) ls[A + 1 + lane] = w == 0 ? gls : ls[A + 1 + lane] + gls;
      if (lane == kVSW) {
        float* dg = ls + 2 * A + 1;
        const float vals[kHeadDiag] = {d_pg, d_v, d_ent, 0.0f, d_kl, d_okl, d_cf, 0.0f};
#pragma unroll
        for (int q = 0; q < kHeadDiag; ++q) dg[q] = w == 0 ? vals[q] : dg[q] + vals[q];
      }
    }
    __syncthreads();
  }
  if (tid < A) ls[tid] = accb;                          // db4a[0..A-1]
  if (tid == kVSW) ls[A] = accb;                        // db4c
  __syncthreads();
  float* ps = g.part_s + (int64_t)blockIdx.x * NS;
  for (int o = tid; o < NS; o += NT) ps[o] = ls[o];
}

// =============================================================================== host side
// Heads of the layer-wise rollout forward, one wave per row.  A <= 15 (head_act_kernel): 4 rows per workgroup, up to 2048
// workgroups - measured 9.5 us at 4096 rows against 13.7 us with 16 rows per workgroup: the parallelism of many short
// workgroups beats amortising the 16 x HL head-weight staging.  16 <= A <= 63 (head_act_wide_kernel): the heads of a row in
// the 64 lanes of its wave; 8 rows per workgroup amortise the staging of the A x HL actor weights, and the critic-only
// call takes the same kernel with the actor's weights in place: its values equal the full call's bit for bit.
void launch_head_act(const catppo_mlp_shape* shape, const catppo_mlp_layout& L, const FusedFwdArgs& call, const MlpWs& w,
                     bool critic_only, hipStream_t s) {
  const int nl = shape->n_hidden, HL = shape->hidden[nl - 1], A = critic_only ? 0 : shape->act_dim;
  const bool wide = shape->act_dim >= kMaxA;
  const float *nul = nullptr, *Hc = w.H[0][nl - 1], *Ha = critic_only ? nul : w.H[1][nl - 1];
  const float *W4c = call.params + L.off_w[0][nl], *b4c = call.params + L.off_b[0][nl];
  const float *W4a = call.params + L.off_w[1][nl], *b4a = call.params + L.off_b[1][nl];
  const catppo_iter_state* rng = critic_only ? nullptr : call.rng_state;
  const bool actor = wide || !critic_only;      // the 16-slot kernel takes null actor operands on a critic-only call
  int64_t nblk = cdiv64(call.M, wide ? 8 : 4);
  if (nblk > 2048) nblk = 2048;
  dispatch_cpl(HL, [&](auto cpl) {      // layout_of admits only these widths
    constexpr int CPL = decltype(cpl)::value;
    auto launch = [&](auto kernel, size_t lds) {
      launch_lds(kernel, dim3((unsigned)nblk), dim3(256), lds, s, Hc, Ha, W4c, b4c, actor ? W4a : nul, actor ? b4a : nul,
                 actor ? call.logstd : nul, actor ? call.eps : nul, actor ? call.given : nul, call.M, A, call.action,
                 call.logprob, call.value_out, call.value_f16, rng, call.rng_step, call.eps_out);
    };
    if (wide) launch(head_act_wide_kernel<CPL>, wide_w_lds<CPL>() ? sizeof(float) * A * HL : 0);
    else launch(head_act_kernel<CPL>, sizeof(float) * 16 * HL);
  });
}

// head_loss_kernel's contract with the heads of a row in the 64 lanes of its wave: `nbw` blocks of kWideHeadRows-row tiles
void launch_head_loss_wide(const HeadArgs& g, int HL, int nbw, hipStream_t s) {
  dispatch_cpl(HL, [&](auto cpl) {
    constexpr int CPL = decltype(cpl)::value;
    launch_lds(head_loss_wide_kernel<CPL>, dim3(nbw), dim3(kWideHeadThreads), wide_head_lds_bytes<CPL>(g.A), s, g);
  });
}
