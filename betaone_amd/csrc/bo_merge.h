// betaone_amd/csrc/bo_merge.h -- merged targets for the replay buffer (records.GpuReplayBuffer.merge_duplicates): the records of a
// training window whose INPUTS coincide -- every game's ply 0, the shared opening plies -- are grouped, and each group gets one target:
// the mean of its members' sparse pi, z and q.  Both losses are linear in their targets, so the expected gradient is the one against
// the mean, and the mean has 1/n of the variance.  Positions stay where bo_replay.h keeps them; nothing is copied.
//
//   bo_k_replay_group          one lane per work item (a record: its ring slot and ply k).  The item is hashed and an open-addressing
//                              table of T slots (a power of two) is probed linearly, built the way bo_k_book_insert builds its own: ONE
//                              compare-and-swap on owner[slot] per probed slot either claims an empty slot (-1 -> the item) or returns
//                              the item that owns it, whose READ-ONLY ring entries are compared exactly.  At most T probes; then the
//                              item is an overflow.  The group's canonical id is the LOWEST record index among its members: an atomic
//                              min on canon[slot].  Which item owns a slot depends on the order of arrival; canon does not.
//   bo_k_replay_merge          one wave per group, members in ascending record index (the host's stable sort): the union of the
//                              members' actions in ascending order, per action the float64 sum of the members' values in member order,
//                              divided by the count and rounded once to float32; z and q the same.  A group of one is a copy.
//   bo_k_replay_encode_merged  the per-step sampler: the planes of the sampled record itself, the targets of its group, one launch --
//                              bo_replay.h's replay_encode with the group's row as the target row.  _sym: under a board symmetry.
//
// Key `input`: two records are equal iff replay_planes_rep writes the same 120 planes for them -- compared block by block on what
// encode_block and encode_scalars show: per history block the twelve piece-and-colour boards and min(rep, 2) (a block in front of the
// game's first ply is all zero), and of the current board the turn and castling bits, both counters and the en-passant square.
// Key `position`: key_equal of the current board alone.
// The probe start mixes EVERY compared word (all blocks and the counters): one position reached with many histories or move numbers
// spreads over the table.  It is computed here from the boards: a ring entry of the replay buffer carries khash = 0 (dpos_from_abi),
// and the key bits of a history board (castling, en passant) are not in the planes, so key_hash of it would split equal inputs.
//
// Nothing waits: no flag, no spin, no plain store another workgroup reads.  owner is only touched by the compare-and-swap, canon only
// by the atomic min (relaxed, agent scope; bo_perft.h's wrappers); gid[i] is the item's own word.
#pragma once
#include "bo_perft.h"   // the atomic wrappers
#include "bo_replay.h"  // ReplayArgs, replay_encode

#define MERGE_KEY_INPUT 0
#define MERGE_KEY_POSITION 1
#define MERGE_CANON_NONE 0x7f7f7f7f  // canon[] before the launch (a memset of 0x7f): above every record index

BO_DEV uint64_t merge_mix(uint64_t h, uint64_t v) {
    h ^= v;
    h *= 0xBF58476D1CE4E5B9ULL;
    h ^= h >> 29;
    return h;
}
BO_DEV int merge_rep2(int rep) { return rep >= 2 ? 2 : rep >= 1 ? 1 : 0; }
BO_DEV int merge_ep(const DPos &P) { const int ep = pos_ep(P); return (ep >= 0 && ep < 64) ? ep : -1; }  // (the plane compares it with a square)

// block j (0 = the oldest, 7 = the current board) of the record (slot, k): ring entry slot - 7 + j, present from block 8 - nb on
BO_DEV bool merge_block_in(int k, int j) { return j >= 8 - (k < 7 ? k + 1 : 8); }

BO_DEV uint64_t merge_hash_input(const DPos *pos, const int *rep, int slot, int k) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    for (int j = 0; j < 8; j++) {
        if (!merge_block_in(k, j)) { h = merge_mix(h, 0x5bd1e995u); continue; }
        const DPos &H = pos[slot - 7 + j];
#pragma unroll
        for (int t = 0; t < 6; t++) {
            h = merge_mix(h, H.bb[t] & H.bb[BB_WHITE]);
            h = merge_mix(h, H.bb[t] & H.bb[BB_BLACK]);
        }
        h = merge_mix(h, (uint64_t)merge_rep2(rep[slot - 7 + j]) + 1);
    }
    const DPos &P = pos[slot];
    h = merge_mix(h, (uint64_t)(P.flags & (F_TURN | F_CASTLE_MASK)) | ((uint64_t)(merge_ep(P) + 1) << 8));
    h = merge_mix(h, ((uint64_t)(uint32_t)P.halfmove << 32) | (uint32_t)P.fullmove);
    return h ^ (h >> 32);
}

BO_DEV bool merge_block_equal(const DPos *pos, const int *rep, int ha, bool ina, int hb, bool inb) {
    if (!ina || !inb) return ina == inb;  // an absent block is 14 zero planes; a present one has its kings
    const DPos &A = pos[ha], &B = pos[hb];
    uint64_t d = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        d |= (A.bb[t] & A.bb[BB_WHITE]) ^ (B.bb[t] & B.bb[BB_WHITE]);
        d |= (A.bb[t] & A.bb[BB_BLACK]) ^ (B.bb[t] & B.bb[BB_BLACK]);
    }
    return d == 0 && merge_rep2(rep[ha]) == merge_rep2(rep[hb]);
}

BO_DEV bool merge_equal_input(const DPos *pos, const int *rep, int sa, int ka, int sb, int kb) {
    const DPos &A = pos[sa], &B = pos[sb];
    if (((A.flags ^ B.flags) & (F_TURN | F_CASTLE_MASK)) != 0 || A.halfmove != B.halfmove || A.fullmove != B.fullmove ||
        merge_ep(A) != merge_ep(B))
        return false;
    for (int j = 7; j >= 0; j--)  // the current board first: most unequal pairs end here
        if (!merge_block_equal(pos, rep, sa - 7 + j, merge_block_in(ka, j), sb - 7 + j, merge_block_in(kb, j))) return false;
    return true;
}

struct MergeGroupArgs {
    const DPos *pos;       // the ring and its repetition counts
    const int *rep;
    const int *slot, *k;   // [n] the work list: ring slot and ply of every item
    const int *rec;        // [n] the item's record index
    int64_t n, T;
    int key;
    int32_t *owner;        // [T] -1
    int32_t *canon;        // [T] MERGE_CANON_NONE
    int32_t *gid;          // [n] the item's table slot, -2 = overflow
    int32_t *status;       // [1] overflow items
};

BO_KERNEL void bo_k_replay_group(MergeGroupArgs a) {
    const int lane = bo_lane();
    const int64_t i = (int64_t)bo_block() * 64 + lane;
    const bool in = i < a.n;
    int32_t gid = -2;
    if (in) {
        const int slot = a.slot[i], k = a.k[i];
        const bool by_input = a.key == MERGE_KEY_INPUT;
        const uint64_t h = by_input ? merge_hash_input(a.pos, a.rep, slot, k) : (uint64_t)key_hash(a.pos[slot]);
        const int64_t mask = a.T - 1;
        int64_t s = (int64_t)h & mask;
        for (int64_t p = 0; p < a.T; p++, s = (s + 1) & mask) {
            const int32_t o = bo_atomic_cas_i32(&a.owner[s], -1, (int32_t)i);
            if (o == -1) { gid = (int32_t)s; break; }
            if (o < 0 || o >= a.n) continue;  // (not an item of this call: a column that was not set to -1)
            const int so = a.slot[o];
            const bool same = by_input ? merge_equal_input(a.pos, a.rep, slot, k, so, a.k[o]) : key_equal(a.pos[slot], a.pos[so]);
            if (same) { gid = (int32_t)s; break; }
        }
        if (gid >= 0) bo_atomic_min_i32(&a.canon[gid], a.rec[i]);
        a.gid[i] = gid;
    }
    const int n_over = bo_popc64(bo_ballot(in && gid == -2));
    if (lane == 0 && n_over) bo_atomic_add_i32(&a.status[0], n_over);
}

struct MergeArgs {
    const int *pi_n, *pi_idx;   // the buffer's columns, by ring slot; W entries per slot
    const float *pi_val, *z, *q;
    int W;
    const int *off;             // [G + 1] group g's members are mslot[off[g] .. off[g + 1])
    const int *mslot;           // [n] ring slots, ascending record index inside a group
    int Wm;
    int32_t *usz;               // [G] the size of the group's union (may exceed BO_RES_CAP: the host refuses the merge)
    int *out_idx;               // [G, Wm]; NULL: the counting pass, only usz is written
    float *out_val, *out_z, *out_q;
};

BO_DEV float merge_readlane_f(float v, int src) { return __builtin_bit_cast(float, bo_readlane(__builtin_bit_cast(int, v), src)); }

// The largest group (every game's ply 0) is walked by ONE wave, 64 members per round: the lanes load the round's slots, counts, z, q
// and each member's first two entries (all of a pi of the reference's search), then the wave goes through them in member order
// reading lanes; entries beyond the second are wave-uniform loads.  Its time is linear in the group's size.
BO_KERNEL void bo_k_replay_merge(MergeArgs a) {
    BO_SHARED int s_act[BO_RES_CAP], s_srt[BO_RES_CAP];
    const int g = bo_block(), lane = bo_lane();
    const int m0 = a.off[g], m1 = a.off[g + 1], cnt = m1 - m0;
    const bool write = a.out_idx != nullptr;
    if (cnt == 1) {  // a copy: the record's entries in the record's order, z and q bit for bit
        const int slot = a.mslot[m0];
        int n = a.pi_n[slot];
        n = n < 0 ? 0 : n > a.W ? a.W : n;
        if (!write) {
            if (lane == 0) a.usz[g] = n;
            return;
        }
        for (int e = lane; e < a.Wm; e += 64) {
            const bool used = e < n;
            a.out_idx[(size_t)g * a.Wm + e] = used ? a.pi_idx[(size_t)slot * a.W + e] : -1;
            a.out_val[(size_t)g * a.Wm + e] = used ? a.pi_val[(size_t)slot * a.W + e] : 0.0f;
        }
        if (lane == 0) { a.out_z[g] = a.z[slot]; a.out_q[g] = a.q[slot]; }
        return;
    }
    // the union of the members' actions, in order of first appearance (U is wave-uniform)
    int U = 0;
    for (int base = m0; base < m1; base += 64) {
        const bool have = base + lane < m1;
        const int my_slot = have ? a.mslot[base + lane] : 0;
        int my_n = have ? a.pi_n[my_slot] : 0;
        my_n = my_n < 0 ? 0 : my_n > a.W ? a.W : my_n;
        const int my_i0 = my_n > 0 ? a.pi_idx[(size_t)my_slot * a.W] : 0, my_i1 = my_n > 1 ? a.pi_idx[(size_t)my_slot * a.W + 1] : 0;
        const int round = m1 - base < 64 ? m1 - base : 64;
        for (int j = 0; j < round; j++) {
            const int slot = bo_readlane(my_slot, j), n = bo_readlane(my_n, j);
            for (int e = 0; e < n; e++) {
                const int act = e == 0 ? bo_readlane(my_i0, j) : e == 1 ? bo_readlane(my_i1, j) : a.pi_idx[(size_t)slot * a.W + e];
                bool f = false;
#pragma unroll
                for (int r = 0; r < BO_RES_CAP / 64; r++) f = f || (lane + 64 * r < U && s_act[lane + 64 * r] == act);
                if (bo_ballot(f) == 0) {
                    if (lane == 0 && U < BO_RES_CAP) s_act[U] = act;
                    U++;
                    bo_wave_sync();
                }
            }
        }
    }
    if (!write) {
        if (lane == 0) a.usz[g] = U;
        return;
    }
    if (U > BO_RES_CAP) return;  // (refused by the host after the counting pass)
    // ascending order: the entries are distinct, an entry's rank is the number of smaller ones
    bo_wave_sync();
#pragma unroll
    for (int r = 0; r < BO_RES_CAP / 64; r++) {
        const int i = lane + 64 * r;
        if (i < U) {
            const int v = s_act[i];
            int rank = 0;
            for (int j = 0; j < U; j++) rank += s_act[j] < v ? 1 : 0;
            s_srt[rank] = v;
        }
    }
    bo_wave_sync();
    int mine[BO_RES_CAP / 64];
    double acc[BO_RES_CAP / 64];
#pragma unroll
    for (int r = 0; r < BO_RES_CAP / 64; r++) {
        mine[r] = lane + 64 * r < U ? s_srt[lane + 64 * r] : 0;
        acc[r] = 0.0;
    }
    double zs = 0.0, qs = 0.0;
    for (int base = m0; base < m1; base += 64) {
        const bool have = base + lane < m1;
        const int my_slot = have ? a.mslot[base + lane] : 0;
        int my_n = have ? a.pi_n[my_slot] : 0;
        my_n = my_n < 0 ? 0 : my_n > a.W ? a.W : my_n;
        const float my_z = have ? a.z[my_slot] : 0.0f, my_q = have ? a.q[my_slot] : 0.0f;
        const int my_i0 = my_n > 0 ? a.pi_idx[(size_t)my_slot * a.W] : 0, my_i1 = my_n > 1 ? a.pi_idx[(size_t)my_slot * a.W + 1] : 0;
        const float my_v0 = my_n > 0 ? a.pi_val[(size_t)my_slot * a.W] : 0.0f, my_v1 = my_n > 1 ? a.pi_val[(size_t)my_slot * a.W + 1] : 0.0f;
        const int round = m1 - base < 64 ? m1 - base : 64;
        for (int j = 0; j < round; j++) {  // member order: the sums are the same whatever built the table
            const int slot = bo_readlane(my_slot, j), n = bo_readlane(my_n, j);
            zs += (double)merge_readlane_f(my_z, j);
            qs += (double)merge_readlane_f(my_q, j);
            for (int e = 0; e < n; e++) {
                const int act = e == 0 ? bo_readlane(my_i0, j) : e == 1 ? bo_readlane(my_i1, j) : a.pi_idx[(size_t)slot * a.W + e];
                const double v = (double)(e == 0 ? merge_readlane_f(my_v0, j) : e == 1 ? merge_readlane_f(my_v1, j) : a.pi_val[(size_t)slot * a.W + e]);
#pragma unroll
                for (int r = 0; r < BO_RES_CAP / 64; r++)
                    if (lane + 64 * r < U && mine[r] == act) acc[r] += v;
            }
        }
    }
    const double dn = (double)cnt;
#pragma unroll
    for (int r = 0; r < BO_RES_CAP / 64; r++) {
        const int i = lane + 64 * r;
        if (i < a.Wm) {
            const bool used = i < U;
            a.out_idx[(size_t)g * a.Wm + i] = used ? mine[r] : -1;
            a.out_val[(size_t)g * a.Wm + i] = used ? (float)(acc[r] / dn) : 0.0f;
        }
    }
    if (lane == 0) { a.out_z[g] = (float)(zs / dn); a.out_q[g] = (float)(qs / dn); }
}

// The per-step sampler is bo_replay.h's body with the target rows of a merge: s_grp[b] = the group of sample b, the columns m_idx / m_val
// [G, Wm], m_z / m_q [G], rows padded already.  SYM: the group's mean targets are transformed on the way out; the grouping knows
// nothing of it.
BO_KERNEL void bo_k_replay_encode_merged(ReplayArgs a) { replay_encode<false, true, false>(a); }
BO_KERNEL void bo_k_replay_encode_merged_sym(ReplayArgs a) { replay_encode<false, true, true>(a); }
