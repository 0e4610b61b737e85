// betaone_amd/csrc/bo_replay.h -- GPU-resident replay buffer: finished games as compact records in HBM, training batches expanded on
// the device.
//
// The reference hands self-play results to training through pickles of DENSE tuples (49.4 KB per ply, self_play.py:220-231), reads
// them all back into one Python list (train.load_recent_data, train.py:187-219) and lets a DataLoader index it
// (ChessDataset.__getitem__, train.py:179-184; the loop that consumes the batches: train_network, train.py:252-262).  Here a ply is
// its position (80 B), its repetition count under the END-of-game tracker (self_play.py:200-208: the training planes of ply i are
// encoded with the tracker of the finished game), its sparse pi and its z: ~110 B per ply resident in HBM (100 M plies = 11 GB of the
// 288), and a batch is made where it is consumed -- one wave per sampled ply writes the 120 planes, the dense pi row and z.
//   bo_k_replay_counts   once per added game: repetition count of every position of the game (a position's count is the number of
//                        key-equal positions in the WHOLE game minus one: what bo_k_encode_positions recomputes per encoded ply)
//   bo_k_replay_encode   one wave per sample: 8 history blocks from the ply's own game (positions are stored game-contiguous),
//                        scalar planes, dense pi row (zero fill + scatter), z
//   bo_k_replay_encode_sparse  the same planes and z, pi as the record keeps it ([W] indices and values): for the sparse-target
//                        loss of bo_train.h, which never needs the dense row
//   bo_k_replay_encode_sparse_q  the same launch with the record's root value q beside z (bo_train.h: the value target as a mix of the
//                        two).  A slot keeps one float32 q next to its z: the search's root value at that ply from the side to
//                        move's point of view, like z -- or z itself where the game was recorded without root values.
//   bo_k_replay_encode_sym / _sparse_sym / _sparse_q_sym  the same three bodies with SYM = true: sample b is handed out under the board
//                        symmetry s_sym[b] (bo_sym.h): every DPos is transformed in registers before encode_block / encode_scalars
//                        write it, the pi indices go through sym_action; entry order, values, z and q are untouched.  applied[b]
//                        (may be NULL) = the code that was applied: the mirror bit is dropped while the record's current position
//                        has a castling right.  The kernels above are the instantiation with SYM = false.
#pragma once
#include "bo_sym.h"
#include "bo_tree.h"

BO_KERNEL void bo_k_replay_counts(const DPos *pos, int n_pos, int *rep) {
    const int i = bo_block(), s = bo_lane();
    const DPos H = pos[i];
    int c = 0;
    for (int j = s; j < n_pos; j += 64) c += key_equal(pos[j], H) ? 1 : 0;
    c = bo_wave_sum(c);
    if (s == 0) rep[i] = c > 1 ? c - 1 : 0;
}

// the 120 planes of sample b: the record in ring slot `slot`, the k-th ply of its game (so slots slot - min(7, k) .. slot are its
// history).  Shared by both samplers, so their states cannot drift apart.
// rep_of(h) = the repetition count of the board in slot h (the PGN sampler of bo_pgn.h counts it live).
// SYM: every board under the symmetry t (wave-uniform; the code sym_applied gave for the sample).
template <bool SYM = false, class RepOf> BO_DEV void replay_planes_rep(float *states, int b, const DPos *pos, int slot, int k, RepOf rep_of, int t = 0) {
    const int s = bo_lane();
    float *row = states + (size_t)b * BO_ROW;
    const int nb = k < 7 ? k + 1 : 8, h0 = slot - (nb - 1);
    for (int pl = 0; pl < (8 - nb) * 14; pl++) row[pl * 64 + s] = 0.0f;
    if constexpr (SYM) {
        for (int j = 0; j < nb; j++) encode_block(row, 8 - nb + j, sym_pos(pos[h0 + j], t), rep_of(h0 + j));
        encode_scalars(row, sym_pos(pos[slot], t));
    } else {
        for (int j = 0; j < nb; j++) encode_block(row, 8 - nb + j, pos[h0 + j], rep_of(h0 + j));
        encode_scalars(row, pos[slot]);
    }
}
BO_DEV void replay_planes(float *states, int b, const DPos *pos, const int *rep, int slot, int k) {
    replay_planes_rep(states, b, pos, slot, k, [rep](int h) { return rep[h]; });
}
// the planes of sample b under s_sym[b]; returns the applied code (and stores it where the caller asked for it)
BO_DEV int replay_planes_sym(float *states, int b, const DPos *pos, const int *rep, int slot, int k, const int *s_sym, int *applied) {
    const int t = sym_applied(pos[slot].flags, s_sym[b]);
    replay_planes_rep<true>(states, b, pos, slot, k, [rep](int h) { return rep[h]; }, t);
    if (applied && bo_lane() == 0) applied[b] = t;
    return t;
}

// sample i = the record in ring slot s_slot[i], the s_k[i]-th ply of its game
template <bool SYM>
BO_DEV void replay_encode_dense(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val, const float *z,
                                int W, const int *s_slot, const int *s_k, const int *s_sym, float *states, float *pis, float *zs,
                                int *applied) {
    const int b = bo_block(), s = bo_lane();
    const int slot = s_slot[b];
    int t = 0;
    if constexpr (SYM) t = replay_planes_sym(states, b, pos, rep, slot, s_k[b], s_sym, applied);
    else replay_planes(states, b, pos, rep, slot, s_k[b]);
    // dense pi row: every address has ONE writer (lane = action mod 64), which looks its action up among the ply's few entries
    float *pr = pis + (size_t)b * BO_NUM_ACTIONS;
    const int n = pi_n[slot];
    const int *ix = pi_idx + (size_t)slot * W;
    const float *vx = pi_val + (size_t)slot * W;
    if constexpr (SYM) {
        // the entries' indices are mapped ONCE, entry e by lane e & 63 (n <= W <= BO_RES_CAP), and read back lane by lane in the loop
        int m[BO_RES_CAP / 64];
#pragma unroll
        for (int r = 0; r < BO_RES_CAP / 64; r++) m[r] = s + 64 * r < n ? sym_action(ix[s + 64 * r], t) : -1;
        for (int a = s; a < BO_NUM_ACTIONS; a += 64) {
            float v = 0.0f;
            for (int e = 0; e < n; e++) {
                const int r = e >> 6;  // (wave-uniform)
                v = bo_readlane(r == 0 ? m[0] : r == 1 ? m[1] : r == 2 ? m[2] : m[3], e & 63) == a ? vx[e] : v;
            }
            pr[a] = v;
        }
    } else {
        for (int a = s; a < BO_NUM_ACTIONS; a += 64) {
            float v = 0.0f;
            for (int e = 0; e < n; e++) v = ix[e] == a ? vx[e] : v;
            pr[a] = v;
        }
    }
    if (s == 0) zs[b] = z[slot];
}
BO_KERNEL void bo_k_replay_encode(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val, const float *z,
                                  int W, const int *s_slot, const int *s_k, float *states, float *pis, float *zs) {
    replay_encode_dense<false>(pos, rep, pi_n, pi_idx, pi_val, z, W, s_slot, s_k, nullptr, states, pis, zs, nullptr);
}
BO_KERNEL void bo_k_replay_encode_sym(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val,
                                      const float *z, int W, const int *s_slot, const int *s_k, const int *s_sym, float *states, float *pis,
                                      float *zs, int *applied) {
    replay_encode_dense<true>(pos, rep, pi_n, pi_idx, pi_val, z, W, s_slot, s_k, s_sym, states, pis, zs, applied);
}

// the same sample with its pi as stored: out_idx / out_val [n, W], the record's entries first, then (-1, 0) in the unused slots
template <bool WITH_Q, bool SYM = false>
BO_DEV void replay_encode_sparse(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val, const float *z,
                                 const float *q, int W, const int *s_slot, const int *s_k, float *states, int *out_idx, float *out_val,
                                 float *zs, float *qs, const int *s_sym = nullptr, int *applied = nullptr) {
    const int b = bo_block(), s = bo_lane();
    const int slot = s_slot[b];
    int t = 0;
    if constexpr (SYM) t = replay_planes_sym(states, b, pos, rep, slot, s_k[b], s_sym, applied);
    else replay_planes(states, b, pos, rep, slot, s_k[b]);
    const int n = pi_n[slot];
    for (int e = s; e < W; e += 64) {
        const bool used = e < n;
        const int a = used ? pi_idx[(size_t)slot * W + e] : -1;
        out_idx[(size_t)b * W + e] = SYM ? sym_action(a, t) : a;
        out_val[(size_t)b * W + e] = used ? pi_val[(size_t)slot * W + e] : 0.0f;
    }
    if (s == 0) {
        zs[b] = z[slot];
        if (WITH_Q) qs[b] = q[slot];
    }
}
BO_KERNEL void bo_k_replay_encode_sparse(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val,
                                         const float *z, int W, const int *s_slot, const int *s_k, float *states, int *out_idx,
                                         float *out_val, float *zs) {
    replay_encode_sparse<false>(pos, rep, pi_n, pi_idx, pi_val, z, nullptr, W, s_slot, s_k, states, out_idx, out_val, zs, nullptr);
}
BO_KERNEL void bo_k_replay_encode_sparse_q(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val,
                                           const float *z, const float *q, int W, const int *s_slot, const int *s_k, float *states,
                                           int *out_idx, float *out_val, float *zs, float *qs) {
    replay_encode_sparse<true>(pos, rep, pi_n, pi_idx, pi_val, z, q, W, s_slot, s_k, states, out_idx, out_val, zs, qs);
}
BO_KERNEL void bo_k_replay_encode_sparse_sym(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val,
                                             const float *z, int W, const int *s_slot, const int *s_k, const int *s_sym, float *states,
                                             int *out_idx, float *out_val, float *zs, int *applied) {
    replay_encode_sparse<false, true>(pos, rep, pi_n, pi_idx, pi_val, z, nullptr, W, s_slot, s_k, states, out_idx, out_val, zs, nullptr, s_sym,
                                      applied);
}
BO_KERNEL void bo_k_replay_encode_sparse_q_sym(const DPos *pos, const int *rep, const int *pi_n, const int *pi_idx, const float *pi_val,
                                               const float *z, const float *q, int W, const int *s_slot, const int *s_k, const int *s_sym,
                                               float *states, int *out_idx, float *out_val, float *zs, float *qs, int *applied) {
    replay_encode_sparse<true, true>(pos, rep, pi_n, pi_idx, pi_val, z, q, W, s_slot, s_k, states, out_idx, out_val, zs, qs, s_sym, applied);
}
