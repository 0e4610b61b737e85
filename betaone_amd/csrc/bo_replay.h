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
//   bo_k_replay_encode*  one wave per sample, eight one-line instantiations of ONE body, replay_encode<DENSE, WITH_Q, SYM>, over ONE
//                        argument struct, ReplayArgs: the 120 planes (8 history blocks from the ply's own game -- positions are stored
//                        game-contiguous -- and the scalar planes, replay_planes_rep), one target row, z.  The next sampler feature is
//                        a flag of the body, not another copy of it.
//     bo_k_replay_encode           DENSE: the pi row of 4672, every address written once (replay_row_dense)
//     bo_k_replay_encode_sparse    pi as the record keeps it ([W] indices and values, replay_row_sparse): for the sparse-target loss
//                                  of bo_train.h, which never needs the dense row
//     bo_k_replay_encode_sparse_q  WITH_Q: the record's root value q beside z (bo_train.h: the value target as a mix of the two).  A
//                                  slot keeps one float32 q next to its z: the search's root value at that ply from the side to
//                                  move's point of view, like z -- or z itself where the game was recorded without root values.
//     bo_k_replay_encode_merged    (bo_merge.h) the sparse row and z, q read from the sample's merge group instead of its ring slot
//     ..._sym                      SYM: sample b is handed out under the board symmetry s_sym[b] (bo_sym.h): every DPos is
//                                  transformed in registers before encode_block / encode_scalars write it, the pi indices go through
//                                  sym_action; entry order, values, z and q are untouched.  applied[b] (may be NULL) = the code that
//                                  was applied: the mirror bit is dropped while the record's current position has a castling right.
//                        DENSE, WITH_Q and SYM are compile-time: an instance without SYM carries nothing of sym_pos.
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
// history).  Shared by replay_encode and the PGN sampler, so their states cannot drift apart.
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

// One sampler launch, by value (as MergeArgs of bo_merge.h): sample b = the record in ring slot s_slot[b], the s_k[b]-th ply of its game.
struct ReplayArgs {
    const DPos *pos;                   // the ring and its repetition counts
    const int *rep;
    const int *s_slot, *s_k;           // [n] the staged batch: ring slot and ply of every sample
    const int *s_sym;                  // [n] SYM: the symmetry asked for (bo_sym.h)
    const int *s_grp;                  // [n] the target row of sample b; NULL (and always for the dense row): that of its own ring slot
    // the targets, W entries per row: the buffer's columns by ring slot, or a merge's by group (bo_merge.h: m_idx, m_val, m_z, m_q, Wm)
    const int *pi_n;                   // entries in use per row; NULL: rows are padded with (-1, 0) already (a merge's)
    const int *pi_idx;
    const float *pi_val, *z, *q;
    int W;
    float *states;                     // [n, 120, 8, 8]
    float *pis;                        // dense: [n, 4672]
    int *out_idx;                      // sparse: [n, W] the row's entries first, then (-1, 0) in the unused places
    float *out_val;
    float *zs, *qs;                    // [n]; qs with WITH_Q
    int *applied;                      // [n] SYM: the code that was applied (may be NULL)
};

// dense pi row: every address has ONE writer (lane = action mod 64), which looks its action up among the row's few entries
template <bool SYM> BO_DEV void replay_row_dense(const ReplayArgs &a, int b, int row, int t) {
    const int s = bo_lane();
    float *pr = a.pis + (size_t)b * BO_NUM_ACTIONS;
    const int n = a.pi_n[row];
    const int *ix = a.pi_idx + (size_t)row * a.W;
    const float *vx = a.pi_val + (size_t)row * a.W;
    if constexpr (SYM) {
        // the entries' indices are mapped ONCE, entry e by lane e & 63 (n <= W <= BO_RES_CAP), and read back lane by lane in the loop
        int m[BO_RES_CAP / 64];
#pragma unroll
        for (int r = 0; r < BO_RES_CAP / 64; r++) m[r] = s + 64 * r < n ? sym_action(ix[s + 64 * r], t) : -1;
        for (int c = s; c < BO_NUM_ACTIONS; c += 64) {
            float v = 0.0f;
            for (int e = 0; e < n; e++) {
                const int r = e >> 6;  // (wave-uniform)
                v = bo_readlane(r == 0 ? m[0] : r == 1 ? m[1] : r == 2 ? m[2] : m[3], e & 63) == c ? vx[e] : v;
            }
            pr[c] = v;
        }
    } else {
        for (int c = s; c < BO_NUM_ACTIONS; c += 64) {
            float v = 0.0f;
            for (int e = 0; e < n; e++) v = ix[e] == c ? vx[e] : v;
            pr[c] = v;
        }
    }
}

// the row as it is kept: a record's entries in the record's order, or a merge group's union
template <bool SYM> BO_DEV void replay_row_sparse(const ReplayArgs &a, int b, int row, int t) {
    const int n = a.pi_n ? a.pi_n[row] : a.W;
    for (int e = bo_lane(); e < a.W; e += 64) {
        const bool used = e < n;
        const int c = used ? a.pi_idx[(size_t)row * a.W + e] : -1;
        a.out_idx[(size_t)b * a.W + e] = SYM ? sym_action(c, t) : c;
        a.out_val[(size_t)b * a.W + e] = used ? a.pi_val[(size_t)row * a.W + e] : 0.0f;
    }
}

// SYM: sample b is handed out under the symmetry sym_applied gives for s_sym[b]: the boards are transformed in registers, the pi
// indices go through sym_action; entry order, values, z and q are untouched.
template <bool DENSE, bool WITH_Q, bool SYM> BO_DEV void replay_encode(const ReplayArgs &a) {
    const int b = bo_block();
    const int slot = a.s_slot[b];
    const int row = !DENSE && a.s_grp ? a.s_grp[b] : slot;  // (read in front of the planes: nothing waits for it behind them)
    int t = 0;
    if constexpr (SYM) t = sym_applied(a.pos[slot].flags, a.s_sym[b]);
    const int *rep = a.rep;
    replay_planes_rep<SYM>(a.states, b, a.pos, slot, a.s_k[b], [rep](int h) { return rep[h]; }, t);
    if (SYM && a.applied && bo_lane() == 0) a.applied[b] = t;
    if constexpr (DENSE) replay_row_dense<SYM>(a, b, row, t);
    else replay_row_sparse<SYM>(a, b, row, t);
    if (bo_lane() == 0) {
        a.zs[b] = a.z[row];
        if (WITH_Q) a.qs[b] = a.q[row];
    }
}
BO_KERNEL void bo_k_replay_encode(ReplayArgs a) { replay_encode<true, false, false>(a); }
BO_KERNEL void bo_k_replay_encode_sym(ReplayArgs a) { replay_encode<true, false, true>(a); }
BO_KERNEL void bo_k_replay_encode_sparse(ReplayArgs a) { replay_encode<false, false, false>(a); }
BO_KERNEL void bo_k_replay_encode_sparse_q(ReplayArgs a) { replay_encode<false, true, false>(a); }
BO_KERNEL void bo_k_replay_encode_sparse_sym(ReplayArgs a) { replay_encode<false, false, true>(a); }
BO_KERNEL void bo_k_replay_encode_sparse_q_sym(ReplayArgs a) { replay_encode<false, true, true>(a); }
