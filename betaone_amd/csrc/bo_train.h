// betaone_amd/csrc/bo_train.h -- the training loss of train.calculate_loss (/root/reference/train.py:222-249) with a SPARSE target.
//
// The reference's loss takes a dense pi row: F.cross_entropy(logits, target) + F.mse_loss(value, z).  A ply's pi has at most pi_width
// non-zeros (2 with this engine's search), and the replay buffer keeps exactly those (bo_replay.h: bo_k_replay_encode_sparse), so the
// loss and its gradient read them directly and the dense [B,4672] target is never built:
//   policy_loss = (1/B) sum_b -sum_e t_be (x_b[i_be] - lse(x_b))    over the valid entries e of row b (0 <= i_be < 4672)
//   value_loss  = (1/B) sum_b (v_b - z_b)^2
//   dlogits[b,a] = g_p/B (softmax(x_b)_a sum_e t_be - t_ba),  dvalue[b] = 2/B (v_b - z_b) g_v
//
//   bo_k_loss_fwd     one wave per row.  A row is 4672 = 64 x 73 logits: lane s holds actions s, s + 64, ... in 73 registers, so the
//                     row is read once and max / sum exp are wave butterflies (bo_wave.h, fixed order) -- no LDS, no barrier.  One
//                     workgroup per row would add an LDS reduction and barriers for a row that one wave already holds, and a batch has
//                     hundreds of rows to spread over the CUs.  Per row: [max, log sum exp(x - max), policy term, value term].
//   bo_k_loss_reduce  one wave: lane s sums rows s, s + 64, ... in row order, then a butterfly -- the three losses in a fixed order
//                     (bit-reproducible; no float atomics).  loss3 = [total, policy, value].
//   bo_k_loss_bwd     one wave per row: the logits again, the gradient of loss3 from a DEVICE pointer (a GradScaler scale never
//                     needs the host), softmax from the stored row statistics; dlogits / dvalue in the inputs' dtype.
//
// Arithmetic is float32 inside for every storage type, with expf / logf (strict libm, not exp2 approximations): parity with
// PyTorch's float32 log_softmax.  fp16 and bf16 outputs are rounded once, to nearest even, so a value beyond the fp16 range
// becomes inf where PyTorch's cast of its float32 gradient would (GradScaler skips the step on it).
// Non-finite logits are not masked: a NaN or +inf logit makes the row's max NaN / inf, and its softmax and gradient NaN, as in
// PyTorch; any non-finite logit makes the row's policy term NaN (PyTorch's dense target multiplies the -inf by a zero; with the -inf
// under a target entry PyTorch's term is +inf, here it is NaN all the same).  A -inf logit leaves the max and the sum alone: its
// softmax is 0 and the row's gradient finite, -g_p/B t at that action if it is a target, as in PyTorch (a row of nothing but
// -inf has max -inf, x - max NaN, and a NaN gradient throughout).  A row with no valid entries adds 0 to the policy loss and gets
// a zero policy gradient.  Entries whose index is not an action (-1 or anything else outside 0..4671) are skipped, values
// included; an action twice in a row is not defined.
//
// The value head on a mix of the game's outcome and the search's root value (bo_k_loss_fwd_mix / _reduce_mix / _bwd_mix):
//   t_b = (1 - a) z_b + a q_b,   value_mix = (1/B) sum_b (v_b - t_b)^2,   dvalue[b] = 2/B (v_b - t_b) g_v
// q_b is the record's root value (bo_replay.h; q = z where the record has none), a one float32 ON THE DEVICE, read by the kernels as
// grad_out is: a schedule changes it under a captured step.  z and q are both from the side to move's point of view: no sign flips.
// a == 0 SELECTS t = z (no 0 * q: q may be NaN, and z = -0.0 has to stay -0.0), so the policy term, the value term and both
// gradients are then the bits of the kernels above; a outside [0, 1] or NaN is not clamped: every entry of loss5 and dvalue are NaN.
// The same wave-per-row layout and the same operations in the same order on the policy side.  Per row
// [max, log sum exp, policy term, (v - t)^2, (v - z)^2, (v - q)^2]; loss5 = [policy + value_mix, policy, value_mix, value_vs_z,
// value_vs_q], the last two diagnostics with no gradient (grad_out stays [3]).
#pragma once
#include "bo_wave.h"

#define BO_LOSS_PER_LANE (BO_NUM_ACTIONS / 64)   // 73
#define BO_LOSS_STATS 4                          // row_stats floats per row
#define BO_LOSS_STATS_MIX 6                      // ... of the mix entry points

#if defined(BO_WAVE_EMU)
#define BO_LOSS_KERNEL static
#else
#define BO_LOSS_KERNEL __global__ __launch_bounds__(64)
#endif

struct bo_bf16 { uint16_t u; };

BO_DEV float bo_ld_f(const float *p) { return *p; }
BO_DEV void bo_st_f(float *p, float v) { *p = v; }
BO_DEV float bo_ld_f(const bo_bf16 *p) { return __builtin_bit_cast(float, (uint32_t)p->u << 16); }
BO_DEV void bo_st_f(bo_bf16 *p, float v) {  // round to nearest even; NaN -> the canonical quiet NaN (c10::BFloat16's rounding)
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    p->u = v != v ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
#if !defined(BO_WAVE_EMU)
BO_DEV float bo_ld_f(const _Float16 *p) { return (float)*p; }
BO_DEV void bo_st_f(_Float16 *p, float v) { *p = (_Float16)v; }  // v_cvt_f16_f32: round to nearest even, inf beyond the range
#endif

BO_DEV bool bo_loss_valid(int i) { return (unsigned)i < (unsigned)BO_NUM_ACTIONS; }

// A row into the wave's registers: lane s gets the logits of actions s, s + 64, ... and returns the largest of them; nan / nonfinite:
// the lane saw a NaN / a NaN or an infinity.
template <typename TL>
BO_DEV float bo_loss_row_load(const TL *xr, float (&x)[BO_LOSS_PER_LANE], bool &nan, bool &nonfinite) {
    const int s = bo_lane();
    float m = -__builtin_inff();
    nan = nonfinite = false;
#pragma unroll
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) {
        x[j] = bo_ld_f(xr + s + 64 * j);
        nan |= x[j] != x[j];
        nonfinite |= !(x[j] - x[j] == 0.0f);
        m = x[j] > m ? x[j] : m;
    }
    return m;
}

// A row's logits once through the wave: st[0..2] = max, log sum exp(x - max), the policy term (written by lane 0).
template <typename TL>
BO_DEV void bo_loss_row_policy(int W, const TL *xr, const int *ix, const float *vx, float *st) {
    const int s = bo_lane();
    float x[BO_LOSS_PER_LANE];
    bool nan, nonfinite;
    const float m = bo_loss_row_load(xr, x, nan, nonfinite);
    float mx = bo_wave_max_f(m);
    if (bo_ballot(nan)) mx = __builtin_nanf("");  // (PyTorch's max propagates NaN; the butterfly compare would drop it)
    float se = 0.0f;
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) se += expf(x[j] - mx);
    const float logsum = logf(bo_wave_sum_f(se));
    float acc = 0.0f;
    for (int e = s; e < W; e += 64) {
        const int i = ix[e];
        if (bo_loss_valid(i)) acc += vx[e] * ((bo_ld_f(xr + i) - mx) - logsum);
    }
    acc = bo_wave_sum_f(acc);
    const bool bad = bo_ballot(nonfinite) != 0;
    if (s == 0) {
        st[0] = mx;
        st[1] = logsum;
        st[2] = bad ? __builtin_nanf("") : -acc;
    }
}

// dlogits of one row from its stored statistics; gp = the gradient that reaches the policy term
template <typename TL>
BO_DEV void bo_loss_row_dlogits(int n, int W, const TL *xr, TL *dr, const int *ix, const float *vx, float gp, float mx, float logsum) {
    const int s = bo_lane();
    const float gb = gp / (float)n;
    float S = 0.0f;
    for (int e = 0; e < W; e++) S += bo_loss_valid(ix[e]) ? vx[e] : 0.0f;  // (pi is normalised in float32: S need not be 1)
    const float sgb = S * gb;
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) {
        const int a = s + 64 * j;
        float t = 0.0f;
        for (int e = 0; e < W; e++) t = ix[e] == a ? vx[e] : t;  // one writer per address: the lane of the action looks it up
        const float sm = expf((bo_ld_f(xr + a) - mx) - logsum);
        bo_st_f(dr + a, sm * sgb - t * gb);
    }
}

BO_DEV bool bo_mix_ok(float a) { return a >= 0.0f && a <= 1.0f; }  // (false for NaN)
BO_DEV float bo_mix_target(float a, float z, float q) {
    if (a == 0.0f) return z;                        // a select, not 0 * q
    if (!bo_mix_ok(a)) return __builtin_nanf("");
    return (1.0f - a) * z + a * q;
}

// the value target of row b: z, or under MIX the mix of z and q
template <bool MIX>
BO_DEV float bo_loss_value_target(int b, const float *z, const float *q, const float *mix) {
    if constexpr (MIX) return bo_mix_target(mix[0], z[b], q[b]);
    else return z[b];
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------------------
// One body each for the forward, the reduce and the backward.  MIX is a compile-time switch: the stride of row_stats, the value target
// (z, or bo_mix_target) and the value columns that lane 0 writes.  The named kernels below are the instantiations; the plain ones pass
// no q and no mix.  bo_k_metrics_rows (bo_metrics.h) shares bo_loss_row_load and repeats bo_loss_row_policy's operations in its order
// for its CE column.
template <bool MIX, typename TL, typename TV>
BO_DEV void bo_loss_fwd_row(int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z, const float *q,
                            const float *mix, float *row_stats) {
    const int b = bo_block();
    float *st = row_stats + (size_t)b * (MIX ? BO_LOSS_STATS_MIX : BO_LOSS_STATS);
    bo_loss_row_policy(W, logits + (size_t)b * BO_NUM_ACTIONS, pi_idx + (size_t)b * W, pi_val + (size_t)b * W, st);
    if (bo_lane() == 0) {
        const float v = bo_ld_f(value + b), dz = v - z[b];
        if constexpr (MIX) {
            const float d = v - bo_mix_target(mix[0], z[b], q[b]), dq = v - q[b];
            st[3] = d * d;
            st[4] = dz * dz;
            st[5] = dq * dq;
        } else {
            st[3] = dz * dz;
        }
    }
}

// One wave: lane s sums rows s, s + 64, ... of every column from 2 on, then a butterfly per column.  out is loss3, or loss5 under MIX.
template <bool MIX>
BO_DEV void bo_loss_reduce_cols(int n, const float *row_stats, const float *mix, float *out) {
    constexpr int STRIDE = MIX ? BO_LOSS_STATS_MIX : BO_LOSS_STATS, COLS = STRIDE - 2;
    const int s = bo_lane();
    float a[COLS];
    for (int c = 0; c < COLS; c++) a[c] = 0.0f;
    for (int b = s; b < n; b += 64)
        for (int c = 0; c < COLS; c++) a[c] += row_stats[(size_t)b * STRIDE + 2 + c];
    for (int c = 0; c < COLS; c++) a[c] = bo_wave_sum_f(a[c]);
    if (s == 0) {
        const float pl = a[0] / (float)n, vl = a[1] / (float)n;
        const bool ok = !MIX || bo_mix_ok(mix[0]);
        const float nan = __builtin_nanf("");
        out[0] = ok ? pl + vl : nan;
        out[1] = ok ? pl : nan;
        out[2] = vl;                                 // (under an invalid mix NaN already: every row's target is)
        if constexpr (MIX) {
            out[3] = ok ? a[2] / (float)n : nan;
            out[4] = ok ? a[3] / (float)n : nan;
        }
    }
}

template <bool MIX, typename TL, typename TV>
BO_DEV void bo_loss_bwd_row(int n, int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                            const float *q, const float *mix, const float *row_stats, const float *grad3, TL *dlogits, TV *dvalue) {
    constexpr int STRIDE = MIX ? BO_LOSS_STATS_MIX : BO_LOSS_STATS;
    const int b = bo_block();
    // the gradient of [total, policy, value]: the policy term feeds total and policy, the value term total and value (loss5's two
    // diagnostics have none).  It is read first, the statistics are indexed in the call and the target is one expression: in this
    // order the scalar loads of the prologue come out as profiles/loss_refactor.md has measured them.
    const float gp = grad3[0] + grad3[1], gv = grad3[0] + grad3[2];
    bo_loss_row_dlogits(n, W, logits + (size_t)b * BO_NUM_ACTIONS, dlogits + (size_t)b * BO_NUM_ACTIONS, pi_idx + (size_t)b * W,
                        pi_val + (size_t)b * W, gp, row_stats[(size_t)b * STRIDE], row_stats[(size_t)b * STRIDE + 1]);
    if (bo_lane() == 0) bo_st_f(dvalue + b, (2.0f / (float)n) * (bo_ld_f(value + b) - bo_loss_value_target<MIX>(b, z, q, mix)) * gv);
}

template <typename TL, typename TV>
BO_LOSS_KERNEL void bo_k_loss_fwd(int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                                  float *row_stats) {
    bo_loss_fwd_row<false>(W, logits, value, pi_idx, pi_val, z, nullptr, nullptr, row_stats);
}
template <typename TL, typename TV>
BO_LOSS_KERNEL void bo_k_loss_fwd_mix(int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                                      const float *q, const float *mix, float *row_stats) {
    bo_loss_fwd_row<true>(W, logits, value, pi_idx, pi_val, z, q, mix, row_stats);
}
BO_LOSS_KERNEL void bo_k_loss_reduce(int n, const float *row_stats, float *loss3) { bo_loss_reduce_cols<false>(n, row_stats, nullptr, loss3); }
BO_LOSS_KERNEL void bo_k_loss_reduce_mix(int n, const float *row_stats, const float *mix, float *loss5) {
    bo_loss_reduce_cols<true>(n, row_stats, mix, loss5);
}
template <typename TL, typename TV>
BO_LOSS_KERNEL void bo_k_loss_bwd(int n, int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                                  const float *row_stats, const float *grad3, TL *dlogits, TV *dvalue) {
    bo_loss_bwd_row<false>(n, W, logits, value, pi_idx, pi_val, z, nullptr, nullptr, row_stats, grad3, dlogits, dvalue);
}
template <typename TL, typename TV>
BO_LOSS_KERNEL void bo_k_loss_bwd_mix(int n, int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                                      const float *q, const float *mix, const float *row_stats, const float *grad3, TL *dlogits, TV *dvalue) {
    bo_loss_bwd_row<true>(n, W, logits, value, pi_idx, pi_val, z, q, mix, row_stats, grad3, dlogits, dvalue);
}
