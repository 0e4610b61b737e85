// betaone_amd/csrc/bo_mate.h -- forced mates on the GPU: an AND/OR backup over the perft frontier (bo_perft.h).
//
// The attacker is the root's side to move.  dtm = plies to mate with best play by both sides: odd at attacker nodes, 0 = no mate within
// the budget.  Draw rules are IGNORED, as in perft and the tablebases: only a position without legal moves ends a line (a repetition or
// the 50-move rule never saves the defender, and a stalemate is never a mate).
//
// A search for mate in at most n moves is a full-width walk to depth D = 2n - 1, level by level on the frontier in HBM, one wavefront
// per entry.  Level l holds positions l plies below the roots: even levels are attacker entries, odd levels defender entries, the last
// level (D - 1) is an attacker level.  Every level keeps one value byte per entry.
//   bo_k_mate_roots      per root: key fields as bo_k_perft_roots leaves them, its move list, and two bits: the side to move is in
//                        check; the side NOT to move is in check (not a position)
//   bo_k_mate_attack     attacker level.  The wave generates the entry's moves, makes each in turn and runs the generator on the
//                        child (wave-uniform, as perft_count<true>).  A child in check without moves: the entry is a mate in 1, value 1,
//                        never expanded.  A child without moves and without check is a stalemate: dropped.  Otherwise the value is 0
//                        for now, and above the last level the count is the number of LIVE children (at least one move).  The 256-bit
//                        live mask goes to HBM so the expand kernel places the live children without generating their moves again; at
//                        the root level the mask of mating moves goes to the roots' key mask.
//   bo_k_mate_expand     attacker level: live child i of entry e at out[off[e] - off[a] + rank of i among the live children]
//   (defender levels)    every entry has a move by construction: bo_k_perft_count writes the move count, bo_k_perft_expand the children
//   bo_k_mate_backup     one wave per parent of a chunk, after the chunk below has been taken to the bottom.  The children's values are
//                        the contiguous run off[p] - off[a] .. off[p + 1] - off[a] of the next level's value bytes.  Attacker: the
//                        minimum of v + 1 over children with v > 0, else 0.  Defender: 0 if any child is 0, else the maximum of v + 1.
//   bo_k_mate_backup_root  the same for the roots, and per root the key moves (the root moves of the shortest mate, a mask over the
//                        generated move list), their number and the lowest-index key move's word
// Offsets come from bo_perft.h's scan kernels, so placement is deterministic; the reductions are integer min / max butterflies.  No
// atomics: every value, mask and count is one plain vector store by one lane, and the results do not depend on the chunking.
#pragma once
#include "bo_perft.h"

#define MT_LAST 0x1u  // the entries are at the walk's last level: nothing below them is counted
#define MT_ROOT 0x2u  // the entries are the roots: the mask of mating moves is kept

BO_DEV int bo_wave_min_i(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = bo_shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
BO_DEV int bo_wave_max_i(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = bo_shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}

// root_chk: bit 0 = the side to move is in check, bit 1 = the side not to move is in check
BO_KERNEL void bo_k_mate_roots(DPos *roots, int32_t *root_moves, int32_t *root_n, int32_t *root_chk) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int r = bo_block(), s = bo_lane();
    DPos P = roots[r];
    P.flags |= F_IRREV;
    finish_key(P);
    if (s == 0) roots[r] = P;
    bool chk;
    const int n = bo_movegen(P, mv, &chk);
    for (int i = s; i < BO_MAX_MOVES; i += 64) root_moves[(size_t)r * BO_MAX_MOVES + i] = i < n ? (int32_t)mv[i] : -1;
    const int us = pos_turn(P);
    const uint64_t ok = P.bb[BB_K] & pos_their(P);
    const bool bad = ok != 0 && attackers_of(P, !us, bo_lsb64(ok), pos_all(P), 0) != 0;
    if (s == 0) {
        root_n[r] = n;
        root_chk[r] = (chk ? 1 : 0) | (bad ? 2 : 0);
    }
}

// entry `block` of an attacker level: cnt, val, live[4 words]; MT_ROOT: keymask[4 words] = the mating moves
BO_KERNEL void bo_k_mate_attack(const DPos *pos, int32_t *cnt, uint8_t *val, uint64_t *live, uint64_t *keymask, uint32_t mode) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    BO_SHARED bo_mv mv2[BO_MAX_MOVES];
    const int s = bo_lane();
    const int64_t e = bo_block();
    const DPos P = pos[e];
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    uint64_t l = 0, m = 0;  // lane w < 4 keeps word w of the masks
    for (int i = 0; i < n; i++) {  // wave-uniform: every lane holds the same child
        const DPos c = make_move(P, mv[i]);
        bool chk2;
        const int n2 = bo_movegen_inline(c, mv2, &chk2);
        const uint64_t b = s == (i >> 6) ? BIT(i & 63) : 0;
        if (n2) l |= b;
        else if (chk2) {
            m |= b;
            if (!(mode & MT_ROOT)) break;  // value 1: below the roots nobody asks which moves mate
        }
    }
    const bool mated = bo_ballot(m != 0) != 0;
    const int n_live = bo_wave_sum(bo_popc64(l));
    if (s < 4) {
        live[e * 4 + s] = l;
        if (mode & MT_ROOT) keymask[e * 4 + s] = m;
    }
    if (s == 0) {
        cnt[e] = (mated || (mode & MT_LAST)) ? 0 : n_live;
        val[e] = mated ? 1 : 0;
    }
}

// live children of entry a + block at out[off[entry] - off[a] + rank]; nothing is stored at or beyond out_cap
BO_KERNEL void bo_k_mate_expand(const DPos *pos, const uint64_t *off, const uint64_t *live, int64_t a, DPos *out_pos, int32_t *out_tag,
                                int64_t out_cap) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    if (off[e + 1] == off[e]) return;  // (wave-uniform) a mate in 1, or nothing live
    const DPos P = pos[e];
    const int64_t o = (int64_t)(off[e] - off[a]);
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    int base = 0;
    for (int w = 0; w < 4; w++) {
        const uint64_t L = live[e * 4 + w];
        const int i = 64 * w + s;
        if (((L >> s) & 1) && i < n) {
            const int64_t at = o + base + bo_popc64(L & (BIT(s) - 1));
            if (at < out_cap) {
                out_pos[at] = make_move(P, mv[i]);
                out_tag[at] = 0;
            }
        }
        base += bo_popc64(L);
    }
}

// parents a .. a + grid of a level, children's values in child_val[0 .. off[a + grid] - off[a])
BO_KERNEL void bo_k_mate_backup(const int32_t *cnt, const uint64_t *off, int64_t a, const uint8_t *child_val, uint8_t *val, uint32_t attacker) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const int c = cnt[e];
    if (c == 0) return;  // (wave-uniform) an attacker entry that keeps the count kernel's value
    const int64_t o = (int64_t)(off[e] - off[a]);
    int lo = 255, hi = 0, zero = 0;
    for (int i = s; i < c; i += 64) {
        const int v = child_val[o + i];
        if (v > 0) {
            lo = v + 1 < lo ? v + 1 : lo;
            hi = v + 1 > hi ? v + 1 : hi;
        } else zero = 1;
    }
    lo = bo_wave_min_i(lo);
    hi = bo_wave_max_i(hi);
    zero = bo_wave_max_i(zero);
    const int r = attacker ? (lo == 255 ? 0 : lo) : (zero ? 0 : hi);
    if (s == 0) val[e] = (uint8_t)r;
}

// the roots a .. a + grid (attacker entries): value, key mask, number of keys, lowest-index key.  act[e] = the root's row in moves.
BO_KERNEL void bo_k_mate_backup_root(const int32_t *cnt, const uint64_t *off, int64_t a, const uint8_t *child_val, uint8_t *val,
                                     const uint64_t *live, uint64_t *keymask, const int32_t *act, const int32_t *moves, int32_t *n_keys,
                                     int32_t *key) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const int c = cnt[e];
    uint64_t k[4];
    if (c) {  // (wave-uniform)
        const int64_t o = (int64_t)(off[e] - off[a]);
        int v[4], lo = 255, base = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {  // lane s looks at move 64 w + s
            const uint64_t L = live[e * 4 + w];
            v[w] = ((L >> s) & 1) ? (int)child_val[o + base + bo_popc64(L & (BIT(s) - 1))] : 0;
            if (v[w] > 0 && v[w] + 1 < lo) lo = v[w] + 1;
            base += bo_popc64(L);
        }
        lo = bo_wave_min_i(lo);
        const int d = lo == 255 ? 0 : lo;
#pragma unroll
        for (int w = 0; w < 4; w++) k[w] = bo_ballot(d > 0 && v[w] > 0 && v[w] + 1 == d);
        if (s == 0) {
            val[e] = (uint8_t)d;
#pragma unroll
            for (int w = 0; w < 4; w++) keymask[e * 4 + w] = k[w];
        }
    } else {  // mate in 1 (the count kernel left the mating moves) or nothing: its mask is empty
#pragma unroll
        for (int w = 0; w < 4; w++) k[w] = keymask[e * 4 + w];
    }
    if (s == 0) {
        int first = -1;
#pragma unroll
        for (int w = 3; w >= 0; w--)
            if (k[w]) first = 64 * w + bo_lsb64(k[w]);
        n_keys[e] = bo_popc64(k[0]) + bo_popc64(k[1]) + bo_popc64(k[2]) + bo_popc64(k[3]);
        key[e] = first < 0 ? -1 : moves[(size_t)act[e] * BO_MAX_MOVES + first];
    }
}

// one lane per line: out[i] = pos[i] after move[i] (the principal variation's attacker moves)
BO_KERNEL void bo_k_mate_play(const DPos *pos, const int32_t *move, int64_t n, DPos *out, int32_t *out_tag) {
    const int64_t i = (int64_t)bo_block() * 64 + bo_lane();
    if (i >= n) return;
    out[i] = make_move(pos[i], (bo_mv)move[i]);
    out_tag[i] = 0;
}
