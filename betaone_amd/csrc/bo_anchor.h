// betaone_amd/csrc/bo_anchor.h -- the anchor opponent: a fixed-depth full-width negamax with an integer static evaluation, run for
// whole batches of roots over the perft frontier (bo_perft.h), in the way bo_mate.h runs its AND/OR backup.
//
// val(P, p) of a position p plies below its root, searched to depth D (DESIGN.md "Anchor opponent"): without a legal move
// -(MATE - p) in check and 0 otherwise; at p == D the static evaluation ev(P); else the maximum over the moves of -val(child, p + 1).
// Draw rules are IGNORED, as in perft and mate: only a position without legal moves ends a line.  Everything is integer and fits an
// int16; level l of the walk keeps one int16 per entry.
//   bo_k_anchor_count        inner level l < D - 1: what bo_k_perft_count writes (the move count, for the scan), and for an entry
//                            without moves its terminal value.  The children are placed by bo_k_perft_expand.
//   bo_k_anchor_leaf         level D - 1.  The wave generates the entry's moves, makes each in turn and runs the generator on the
//                            child (wave-uniform, as bo_k_mate_attack): the child is mated, stalemated, or evaluated -- one lane per
//                            square, summed over the wave.  The entry's value is the maximum of the negated child values.  AN_ROOT
//                            (D == 1, the entries are the roots): the per-move scores go to HBM.
//   bo_k_anchor_backup       one wave per parent of a chunk, after the chunk below has been taken to the bottom: the maximum of -v over
//                            the contiguous run off[p] - off[a] .. off[p + 1] - off[a] of the next level's values.
//   bo_k_anchor_backup_root  the same for the roots; also the row of per-move scores, the number of moves that reach the maximum and
//                            the lowest-index one's word.  With child_val == nullptr the scores are the leaf kernel's (D == 1).
//   bo_k_anchor_eval         ev alone, one wave per position.
//
// Quiescence Q > 0 (bo_anchor_q; DESIGN.md "Anchor opponent", quiescence): at p == D a position with a legal move gets qs(P, D, Q) in
// place of ev(P).  The TACTICAL moves of P are all its legal moves when it is in check, else the legal moves that capture (the
// destination holds an enemy man, or en passant: PF_CAPTURES' test) or promote, in the generator's order.
//   qs(P, p, q) = -(MATE - p) / 0 without a legal move, as val;  ev(P) if q == 0;  else the maximum of the FLOOR -- ev(P), or -MATE in
//                 check: no standing pat there -- and of -qs(P.m, p + 1, q - 1) over the tactical moves m.
// The walk then has D + Q levels: 0 .. D - 1 full width (bo_k_anchor_count, bo_k_perft_expand; bo_k_anchor_leaf is the Q == 0 kernel),
// and p <= D + Q <= 16, so every value still fits the int16.
//   bo_k_anchor_qcount       levels D .. D + Q - 2: the number of tactical moves (for the scan), and the terminal value or the floor.
//   bo_k_anchor_qexpand      tactical child of rank r (among the tactical moves, by ballot and popcount over the four 64-move words)
//                            at off[e] - off[a] + r.
//   bo_k_anchor_qleaf        level D + Q - 1, one quiescence ply left: shaped like bo_k_anchor_leaf, over the tactical moves only,
//                            starting from the terminal value or the floor.  The children are never stored.
//   bo_k_anchor_backup_q     as bo_k_anchor_backup for a quiescence level: starts from the entry's own value instead of -MATE.
// Offsets come from bo_perft.h's scan kernels, so placement is deterministic; the reductions are integer butterflies.  No atomics:
// every value is one plain vector store by one lane, and nothing depends on the chunking.
#pragma once
#include "bo_mate.h"

#define AN_MATE 30000
#define AN_NONE INT32_MIN  // a score beyond the root's move list
#define AN_ROOT 0x1u       // bo_k_anchor_leaf: the entries are the roots, the per-move scores are kept

// The term of the man on this lane's square, signed for the side to move; the wave's sum is ev(P).
BO_DEV int anchor_ev(const DPos &P) {
    const int s = bo_lane();
    const uint64_t b = BIT(s);
    const bool white = (P.bb[BB_WHITE] & b) != 0, black = (P.bb[BB_BLACK] & b) != 0;
    const int f = s & 7, rank = s >> 3;
    const int r = white ? rank : 7 - rank;  // counted from the owner's back rank
    const int e = f < 7 - f ? f : 7 - f;
    const int d = e + (r < 7 - r ? r : 7 - r);
    int t = 0;
    if (P.bb[BB_P] & b) t = 100 + 2 * (r - 1) * (r - 1) + 3 * e;
    else if (P.bb[BB_N] & b) t = 300 + 8 * d;
    else if (P.bb[BB_B] & b) t = 320 + 4 * d;
    else if (P.bb[BB_R] & b) t = 500 + (r == 6 ? 20 : 0);
    else if (P.bb[BB_Q] & b) t = 900 + 2 * d;
    else if (P.bb[BB_K] & b) t = P.bb[BB_Q] == 0 ? 8 * d : -6 * r;
    if (!(white || black)) t = 0;
    const bool ours = pos_turn(P) ? white : black;
    return bo_wave_sum(ours ? t : -t);
}

BO_KERNEL void bo_k_anchor_eval(const DPos *pos, int32_t *out) {
    const int64_t e = bo_block();
    const DPos P = pos[e];
    const int v = anchor_ev(P);
    if (bo_lane() == 0) out[e] = v;
}

// entry `block` of an inner level `ply` plies below the roots: cnt, and the terminal value of an entry without moves
BO_KERNEL void bo_k_anchor_count(const DPos *pos, int32_t *cnt, int16_t *val, int32_t ply) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int64_t e = bo_block();
    const DPos P = pos[e];
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    if (bo_lane() == 0) {
        cnt[e] = n;
        if (n == 0) val[e] = (int16_t)(chk ? -(AN_MATE - ply) : 0);
    }
}

// entry `block` of the last level, `ply` = D - 1 plies below the roots: val; AN_ROOT: scores[block][256]
BO_KERNEL void bo_k_anchor_leaf(const DPos *pos, int32_t *cnt, int16_t *val, int32_t *scores, int32_t ply, uint32_t mode) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    BO_SHARED bo_mv mv2[BO_MAX_MOVES];
    const int s = bo_lane();
    const int64_t e = bo_block();
    const DPos P = pos[e];
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    int best = chk ? -(AN_MATE - ply) : 0;  // (kept only when there is no move)
    if (n) best = -AN_MATE;
    for (int i = 0; i < n; i++) {  // wave-uniform: every lane holds the same child
        const DPos c = make_move(P, mv[i]);
        bool chk2;
        const int n2 = bo_movegen_inline(c, mv2, &chk2);
        const int cv = n2 ? anchor_ev(c) : chk2 ? -(AN_MATE - (ply + 1)) : 0;
        best = -cv > best ? -cv : best;
        if ((mode & AN_ROOT) && s == 0) scores[e * BO_MAX_MOVES + i] = -cv;
    }
    if (mode & AN_ROOT)
        for (int i = n + s; i < BO_MAX_MOVES; i += 64) scores[e * BO_MAX_MOVES + i] = AN_NONE;
    if (s == 0) {
        cnt[e] = 0;  // nothing below the last level
        val[e] = (int16_t)best;
    }
}

// parents a .. a + grid of a level, the children's values in child_val[0 .. off[a + grid] - off[a])
BO_KERNEL void bo_k_anchor_backup(const int32_t *cnt, const uint64_t *off, int64_t a, const int16_t *child_val, int16_t *val) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const int c = cnt[e];
    if (c == 0) return;  // (wave-uniform) an entry without moves keeps the count kernel's value
    const int64_t o = (int64_t)(off[e] - off[a]);
    int hi = -AN_MATE;
    for (int i = s; i < c; i += 64) {
        const int v = -(int)child_val[o + i];
        hi = v > hi ? v : hi;
    }
    hi = bo_wave_max_i(hi);
    if (s == 0) val[e] = (int16_t)hi;
}

// the roots a .. a + grid (each has a move): scores row, value, number of best moves, the lowest-index best move's word.
// child_val: child i of a root is its move i (bo_k_perft_expand places every move); nullptr: the row is the leaf kernel's.
// n_moves[e] = the root's move count; act[e] = the root's row in moves.
BO_KERNEL void bo_k_anchor_backup_root(const int32_t *n_moves, const uint64_t *off, int64_t a, const int16_t *child_val, int32_t *scores,
                                       int32_t *score, int32_t *n_best, int32_t *best, const int32_t *act, const int32_t *moves) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const int c = n_moves[e];
    const int64_t o = child_val ? (int64_t)(off[e] - off[a]) : 0;
    int v[4], hi = AN_NONE;
#pragma unroll
    for (int w = 0; w < 4; w++) {  // lane s looks at move 64 w + s
        const int i = 64 * w + s;
        if (child_val) {
            v[w] = i < c ? -(int)child_val[o + i] : AN_NONE;
            scores[e * BO_MAX_MOVES + i] = v[w];
        } else v[w] = i < c ? scores[e * BO_MAX_MOVES + i] : AN_NONE;
        hi = v[w] > hi ? v[w] : hi;
    }
    hi = bo_wave_max_i(hi);
    uint64_t k[4];
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = bo_ballot(c > 0 && v[w] == hi);
    if (s == 0) {
        int first = -1;
#pragma unroll
        for (int w = 3; w >= 0; w--)
            if (k[w]) first = 64 * w + bo_lsb64(k[w]);
        score[e] = hi;
        n_best[e] = bo_popc64(k[0]) + bo_popc64(k[1]) + bo_popc64(k[2]) + bo_popc64(k[3]);
        best[e] = first < 0 ? -1 : moves[(size_t)act[e] * BO_MAX_MOVES + first];
    }
}

// ---- quiescence -----------------------------------------------------------------------------------------------------------------------
// move m of P (in check: chk) is tactical
BO_DEV bool anchor_tactical(const DPos &P, bo_mv m, bool chk) {
    const int from = MV_FROM(m), to = MV_TO(m);
    const bool pawn = (P.bb[BB_P] & BIT(from)) != 0;
    const bool ep = pawn && to == pos_ep(P) && (from & 7) != (to & 7) && !(pos_all(P) & BIT(to));
    return chk || (pos_their(P) & BIT(to)) != 0 || ep || MV_PROMO(m) != 0;
}
// t[w] bit s: move 64 w + s of the n in mv is tactical (wave-uniform control flow; every lane gets the four words)
BO_DEV void anchor_tactical_mask(const DPos &P, const bo_mv *mv, int n, bool chk, uint64_t t[4]) {
    const int s = bo_lane();
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int i = 64 * w + s;
        t[w] = bo_ballot(i < n && anchor_tactical(P, mv[i], chk));
    }
}
// what qs(P, ply, q > 0) starts from: the terminal value of a position without moves, else the floor
BO_DEV int anchor_qfloor(int n, bool chk, int ev, int ply) { return n == 0 ? (chk ? -(AN_MATE - ply) : 0) : chk ? -AN_MATE : ev; }

// entry `block` of a quiescence level `ply` >= D plies below the roots, two or more quiescence plies left: cnt, val
BO_KERNEL void bo_k_anchor_qcount(const DPos *pos, int32_t *cnt, int16_t *val, int32_t ply) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int64_t e = bo_block();
    const DPos P = pos[e];
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    uint64_t t[4];
    anchor_tactical_mask(P, mv, n, chk, t);
    const int ev = anchor_ev(P);
    if (bo_lane() == 0) {
        cnt[e] = bo_popc64(t[0]) + bo_popc64(t[1]) + bo_popc64(t[2]) + bo_popc64(t[3]);
        val[e] = (int16_t)anchor_qfloor(n, chk, ev, ply);
    }
}

// tactical children of entry a + block at out[off[entry] - off[a] + rank]; nothing is stored at or beyond out_cap
BO_KERNEL void bo_k_anchor_qexpand(const DPos *pos, const uint64_t *off, int64_t a, DPos *out_pos, int32_t *out_tag, int64_t out_cap) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    if (off[e + 1] == off[e]) return;  // (wave-uniform) no tactical move
    const DPos P = pos[e];
    const int64_t o = (int64_t)(off[e] - off[a]);
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    uint64_t t[4];
    anchor_tactical_mask(P, mv, n, chk, t);
    int base = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if ((t[w] >> s) & 1) {
            const int64_t at = o + base + bo_popc64(t[w] & (BIT(s) - 1));
            if (at < out_cap) {
                out_pos[at] = make_move(P, mv[64 * w + s]);
                out_tag[at] = 0;
            }
        }
        base += bo_popc64(t[w]);
    }
}

// entry `block` of the last level, `ply` = D + Q - 1 plies below the roots, one quiescence ply left: val
BO_KERNEL void bo_k_anchor_qleaf(const DPos *pos, int32_t *cnt, int16_t *val, int32_t ply) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    BO_SHARED bo_mv mv2[BO_MAX_MOVES];
    const int64_t e = bo_block();
    const DPos P = pos[e];
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    int best = anchor_qfloor(n, chk, anchor_ev(P), ply);
    for (int i = 0; i < n; i++) {  // wave-uniform: every lane holds the same move and the same child
        const bo_mv m = (bo_mv)bo_readlane((int)mv[i], 0);
        if (!anchor_tactical(P, m, chk)) continue;
        const DPos c = make_move(P, m);
        bool chk2;
        const int n2 = bo_movegen_inline(c, mv2, &chk2);
        const int cv = n2 ? anchor_ev(c) : chk2 ? -(AN_MATE - (ply + 1)) : 0;
        best = -cv > best ? -cv : best;
    }
    if (bo_lane() == 0) {
        cnt[e] = 0;  // nothing below the last level
        val[e] = (int16_t)best;
    }
}

// bo_k_anchor_backup for the parents of a quiescence level: the maximum of the entry's own value and -v over its run
BO_KERNEL void bo_k_anchor_backup_q(const int32_t *cnt, const uint64_t *off, int64_t a, const int16_t *child_val, int16_t *val) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const int c = cnt[e];
    if (c == 0) return;  // (wave-uniform) an entry without tactical moves keeps its value
    const int64_t o = (int64_t)(off[e] - off[a]);
    int hi = (int)val[e];
    for (int i = s; i < c; i += 64) {
        const int v = -(int)child_val[o + i];
        hi = v > hi ? v : hi;
    }
    hi = bo_wave_max_i(hi);
    if (s == 0) val[e] = (int16_t)hi;
}
