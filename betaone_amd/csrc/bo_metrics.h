// betaone_amd/csrc/bo_metrics.h -- held-out validation: what a net's logits and value say about records it was not trained on.
//
// The loss kernels (bo_train.h) give one number per batch.  These give, per row and summed per bucket, how good the policy's ranking of
// the search's best move is, how the probability mass lies, and how the value head does -- without a gradient, so a whole validation
// pass is two launches per batch and ONE device -> host copy at its end.
//
//   bo_k_metrics_rows    one wave per row, the layout of bo_k_loss_fwd: lane s holds actions s, s + 64, ... in 73 registers.  The row is
//                        read from memory once; the logit under a target entry and the one under the target's top move come out of
//                        the registers (a shuffle from the lane that holds the action, selected by the register that does), not out of
//                        memory again.  No LDS, no barrier, no atomics.  Writes row[b][BO_METRIC_ROW_COLS] float32.
//   bo_k_metrics_reduce  one wave per bucket: lane s adds, in float64, rows s, s + 64, ... (row order) whose bucket is the wave's, then a
//                        fixed butterfly; lane 0 ADDS the sums into accum[bucket][BO_METRIC_COLS] (float64, device).  One wave owns a
//                        bucket and calls on one stream are ordered, so no atomics; the counts are sums of small integers in float64,
//                        exact whatever the split into batches.
//
// Per row, with the valid entries e of the row (bo_loss_valid), t_e = pi_val, i_e = pi_idx, mx = max x, lse = log sum exp(x - mx),
// p_a = exp((x_a - mx) - lse), and i* the valid entry with the largest t (ties: the lowest ACTION, not the first slot):
//   bad                1 if a logit is NaN, +inf or -inf or the value NaN: every other column of the record is then 0
//   has_policy         1 if the row has a valid entry; without one the policy columns are 0
//   decisive           z != 0
//   rank               actions a with x_a > x_i*, or x_a == x_i* and a < i* -- stored values compared, exact in every dtype
//   top1, top3, top5   rank < 1, 3, 5
//   argmax_in_support  the net's argmax (lowest index among equal maxima, torch.argmax's rule) is one of the i_e
//   ce                 -sum_e t_e ((x_ie - mx) - lse): the operations of bo_k_loss_fwd in its order, so the bits of its row_stats[b][2]
//                      in every row that is not bad (-0.0 where the row has no valid entry)
//   target_entropy     -sum_e t_e log t_e over t_e > 0
//   net_entropy        -sum_a p_a ((x_a - mx) - lse), a term 0 where p_a == 0
//   p_top, p_support   p_i*, sum_e p_ie
//   se_z, se_q, abs_v  (v - z)^2, (v - q)^2 (0 without q), |v|
//   sign_ok            decisive and v z > 0
//   z, v               for the reliability table (mean outcome against mean prediction per bucket)
// Arithmetic is float32 with expf / logf, as in bo_train.h.  Entries whose index is no action are skipped, values included; an action
// twice in a row is not defined.
#pragma once
#include "bo_train.h"

// The logit of action a (wave-uniform, an action) out of the row that the wave holds: every lane picks its register a >> 6 (a
// compile-time index per step, so the row stays in registers), and lane a & 63 has the answer.
BO_DEV float bo_row_pick(const float (&x)[BO_LOSS_PER_LANE], int a) {
    float cand = 0.0f;
#pragma unroll
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) cand = (a >> 6) == j ? x[j] : cand;
    return __builtin_bit_cast(float, bo_readlane(__builtin_bit_cast(int, cand), a & 63));
}

static_assert(BO_METRIC_COLS == BO_METRIC_ROW_COLS + 1 && BO_METRIC_ROW_RANK + 1 == BO_METRIC_SUM_RANK && BO_METRIC_ROW_CE + 1 == BO_METRIC_SUM_CE &&
                  BO_METRIC_ROW_V + 1 == BO_METRIC_SUM_V,
              "include/betaone_engine.h: accum column c >= 1 is the sum of row column c - 1");

template <typename TL, typename TV>
BO_LOSS_KERNEL void bo_k_metrics_rows(int W, const TL *logits, const TV *value, const int *pi_idx, const float *pi_val, const float *z,
                                      const float *q, float *rows) {
    const int b = bo_block(), s = bo_lane();
    const TL *xr = logits + (size_t)b * BO_NUM_ACTIONS;
    float x[BO_LOSS_PER_LANE];
    bool nan, nonfinite;
    const float m = bo_loss_row_load(xr, x, nan, nonfinite);
    const bool nonfinite_row = bo_ballot(nonfinite) != 0;   // (here, not at the end: the test would keep the logits alive to there)
    float mx = bo_wave_max_f(m);
    if (bo_ballot(nan)) mx = __builtin_nanf("");  // (as bo_k_loss_fwd)
    // the net's argmax: the lowest action whose logit is the maximum (the lane's lowest register first, then the lowest lane's)
    int mj = BO_LOSS_PER_LANE;
#pragma unroll
    for (int j = BO_LOSS_PER_LANE - 1; j >= 0; j--) mj = x[j] == mx ? j : mj;
    int amax = mj < BO_LOSS_PER_LANE ? s + 64 * mj : 0x7fffffff;
    for (int k = 1; k < 64; k <<= 1) { const int o = bo_shfl_xor(amax, k); amax = o < amax ? o : amax; }

    // The order below keeps ONE copy of the row alive: everything that compares logits (the rank) comes first, then x turns into
    // x - mx in place, which is all the exponentials and the policy term need.  Each wave-wide step stands right behind its loop: the
    // compiler moves a lane-local computation down to its use, and a use at the end of the kernel keeps 73 registers alive to there
    // (243 VGPRs and one wave per SIMD with the non-finite ballot at the end; 104 and four waves with it here).
    // the entries, 64 at a time (lane s has entry e0 + s): the target's top move and its entropy
    float tent = 0.0f, bt = -__builtin_inff();
    int bi = 0x7fffffff;
    bool any = false, hit = false;
    for (int e0 = 0; e0 < W; e0 += 64) {
        const int e = e0 + s;
        const int i = e < W ? pi_idx[(size_t)b * W + e] : -1;
        if (bo_loss_valid(i)) {
            const float t = pi_val[(size_t)b * W + e];
            if (t > 0.0f) tent += t * logf(t);
            if ((t > bt) | ((t == bt) & (i < bi))) { bt = t; bi = i; }
            any = true;
            hit |= i == amax;
        }
    }
    tent = bo_wave_sum_f(tent);
    const bool has = bo_ballot(any) != 0, in_support = bo_ballot(hit) != 0;
    bo_wave_argmax_f(bt, bi);
    const int istar = has ? bi : 0;
    const float xs = bo_row_pick(x, istar);
    // (branch-free, and the action s + 64 j < i* as 64 j < i* - s: one register, not 73 action numbers)
    const int dstar = istar - s;
    int above = 0;
#pragma unroll
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) above += (int)(x[j] > xs) + (int)((x[j] == xs) & (64 * j < dstar));
    const int rank = bo_wave_sum(above);   // (the last use of the logits themselves: from here on the registers hold x - mx)
    // sum exp and the policy term with the operations of bo_k_loss_fwd in its order
    float se = 0.0f;
#pragma unroll
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) {
        x[j] = x[j] - mx;
        se += expf(x[j]);
    }
    const float logsum = logf(bo_wave_sum_f(se));
    // the entries again: lane s takes x[i] - mx of entry e0 + s, picked entry by entry (a pi has 2 entries with this engine's search)
    float acc = 0.0f, psup = 0.0f;
    for (int e0 = 0; e0 < W; e0 += 64) {
        const int e = e0 + s, cnt = W - e0 < 64 ? W - e0 : 64;
        const int i = e < W ? pi_idx[(size_t)b * W + e] : -1;
        float xe = 0.0f;
        for (int k = 0; k < cnt; k++) {
            const int ik = bo_readlane(i, k);
            if (!bo_loss_valid(ik)) continue;   // (wave-uniform)
            const float o = bo_row_pick(x, ik);
            xe = s == k ? o : xe;
        }
        if (bo_loss_valid(i)) {
            const float d = xe - logsum;
            acc += pi_val[(size_t)b * W + e] * d;
            psup += expf(d);
        }
    }
    acc = bo_wave_sum_f(acc);
    psup = bo_wave_sum_f(psup);
    float nent = 0.0f;
#pragma unroll
    for (int j = 0; j < BO_LOSS_PER_LANE; j++) {
        const float d = x[j] - logsum;
        const float p = expf(d);
        nent += p == 0.0f ? 0.0f : p * d;
    }
    nent = bo_wave_sum_f(nent);
    const float v = bo_ld_f(value + b), zb = z[b];
    const bool bad = nonfinite_row || v != v;
    if (s == 0) {
        float *r = rows + (size_t)b * BO_METRIC_ROW_COLS;
        const bool pol = has && !bad;
        const float dz = v - zb, dq = q ? v - q[b] : 0.0f;
        const bool decisive = zb != 0.0f;
        r[BO_METRIC_ROW_BAD] = bad ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_HAS_POLICY] = pol ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_DECISIVE] = !bad && decisive ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_RANK] = pol ? (float)rank : 0.0f;
        r[BO_METRIC_ROW_TOP1] = pol && rank < 1 ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_TOP3] = pol && rank < 3 ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_TOP5] = pol && rank < 5 ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_ARGMAX_IN_SUPPORT] = pol && in_support ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_CE] = bad ? 0.0f : -acc;   // (-0.0 in a row without entries, as in row_stats)
        r[BO_METRIC_ROW_TARGET_ENTROPY] = pol ? -tent : 0.0f;
        r[BO_METRIC_ROW_NET_ENTROPY] = pol ? -nent : 0.0f;
        r[BO_METRIC_ROW_P_TOP] = pol ? expf((xs - mx) - logsum) : 0.0f;
        r[BO_METRIC_ROW_P_SUPPORT] = pol ? psup : 0.0f;
        r[BO_METRIC_ROW_SE_Z] = bad ? 0.0f : dz * dz;
        r[BO_METRIC_ROW_SE_Q] = bad ? 0.0f : dq * dq;
        r[BO_METRIC_ROW_ABS_V] = bad ? 0.0f : __builtin_fabsf(v);
        r[BO_METRIC_ROW_SIGN_OK] = !bad && decisive && v * zb > 0.0f ? 1.0f : 0.0f;
        r[BO_METRIC_ROW_Z] = bad ? 0.0f : zb;
        r[BO_METRIC_ROW_V] = bad ? 0.0f : v;
    }
}

// accum[k][0] += rows of bucket k that are not bad; accum[k][c] += sum of row column c - 1 (c >= 1).  bucket == NULL: every row is
// bucket 0.  A row whose bucket is outside [0, gridDim) belongs to no wave.
BO_LOSS_KERNEL void bo_k_metrics_reduce(int n, const float *rows, const int *bucket, double *accum) {
    const int k = bo_block(), s = bo_lane();
    double a[BO_METRIC_COLS];
#pragma unroll
    for (int c = 0; c < BO_METRIC_COLS; c++) a[c] = 0.0;
    for (int b = s; b < n; b += 64) {
        if ((bucket ? bucket[b] : 0) != k) continue;
        const float *r = rows + (size_t)b * BO_METRIC_ROW_COLS;
        a[0] += 1.0 - (double)r[BO_METRIC_ROW_BAD];
#pragma unroll
        for (int c = 1; c < BO_METRIC_COLS; c++) a[c] += (double)r[c - 1];
    }
#pragma unroll
    for (int c = 0; c < BO_METRIC_COLS; c++) a[c] = bo_wave_sum_d(a[c]);
    if (s == 0) {
#pragma unroll
        for (int c = 0; c < BO_METRIC_COLS; c++) accum[(size_t)k * BO_METRIC_COLS + c] += a[c];
    }
}
