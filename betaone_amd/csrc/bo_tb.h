// betaone_amd/csrc/bo_tb.h -- endgame tablebases built and probed on the device (distance to mate in plies, 2 to 4 men).
//
// A table is a flat uint16 array in HBM over a piece list K, strong pieces, k, weak pieces (the strong side is WHITE in the table's
// frame); the colour-swapped material is served by the mirror (ranks flipped = bitboards byte-swapped, colours and the side to move
// swapped).  No castling rights; pawns on one side only, so en passant cannot occur; the 50-move rule is ignored (the Nalimov metric).
//   index        idx = ((stm * 64 + sq[0]) * 64 + sq[1]) ... over the list; stm 0 = the strong side moves.  No symmetry reduction:
//                2 * 64^n entries.  The host mirror is betaone_amd/tablebase.py.
//   code         0 not a position | 1 draw (while building: also unresolved) | 2 + k mate in k plies: k even = the side to move is
//                mated in k (k = 0 checkmate), k odd = the side to move mates in k.
//   code 0       two men on one square, adjacent kings, the side NOT to move in check, a pawn on rank 1 or 8, and of two identical
//                men the ordering with the larger square first.
//   bo_k_tb_init     one lane per index: legality.  A legal entry whose king has a safe step is unresolved; the few others are
//                    balloted and get one wave each (bo_movegen_inline): checkmate 2, stalemate 1, else unresolved.
//   bo_k_tb_pass     a workgroup owns TB_RUN consecutive indices.  Its wave loads 64 codes, ballots the unresolved ones, and takes them
//                    one by one: decode (wave-uniform), bo_movegen_inline into LDS, move j on lane j in rounds of 64, make_move, the
//                    child's code from the child's table (tb_lookup: this table, a sub-table after a capture or a promotion, mirrored
//                    where the strong side is black, or an insufficient-material draw), two reductions over the wave.
//                    EXACT-PASS RULE: pass i assigns an entry only the value i -- a win when the smallest child loss + 1 == i, a loss
//                    when every child is a win and the largest + 1 == i.  A child code written in the same pass reads as i (or as
//                    unresolved): as a lost child it would make a win in i + 1, as a won child a loss in i + 1; both are ignored, so the
//                    in-place update is deterministic.  One 64-bit atomic per workgroup counts the assignments.
//   bo_k_tb_verify   the same walk over every entry with the final codes and without the restriction (a Bellman check), and the
//                    legality of every index again; counts the mismatches.
//   bo_k_tb_probe    one lane per bo_position: status and code.
// make_move indexes the position's bitboards by the side to move and the promoted piece, so the child lives in scratch memory (DESIGN,
// "PGN export"); the parent is wave-uniform.
#pragma once
#include "bo_perft.h"
#include "bo_tb_probe.h"  // TbTable, tb_lookup and the constants: shared with the tree kernels

// index -> position in the table's frame (no castling bits, no e.p., clocks 0).  false: two men on one square.
BO_DEV bool tb_decode(const TbTable &T, int64_t idx, DPos *out) {
    DPos d;
#pragma unroll
    for (int i = 0; i < 8; i++) d.bb[i] = 0;
    bool ok = true;
    for (int s = 0; s < T.n_men; s++) {
        const int sq = (int)((idx >> (6 * (T.n_men - 1 - s))) & 63);
        const uint64_t b = BIT(sq);
        ok = ok && !((d.bb[BB_WHITE] | d.bb[BB_BLACK]) & b);
#pragma unroll
        for (int i = 0; i < 6; i++) d.bb[i] |= T.pt[s] == i + 1 ? b : 0;
        d.bb[BB_WHITE] |= T.strong[s] ? b : 0;
        d.bb[BB_BLACK] |= T.strong[s] ? 0 : b;
    }
    d.flags = ((idx >> (6 * T.n_men)) & 1) ? 0u : F_TURN;
    d.halfmove = 0;
    d.fullmove = 0;
    d.khash = 0;
    *out = d;
    return ok;
}
// is idx a position (code != 0)?  P = its decoded men
BO_DEV bool tb_legal(const TbTable &T, int64_t idx, const DPos &P, bool distinct) {
    if (!distinct) return false;
    if (P.bb[BB_P] & (RANK_1 | RANK_8)) return false;
    for (int s = 0; s + 1 < T.n_men; s++) {  // identical men: ascending squares only
        const int a = (int)((idx >> (6 * (T.n_men - 1 - s))) & 63), b = (int)((idx >> (6 * (T.n_men - 2 - s))) & 63);
        if (T.pt[s] == T.pt[s + 1] && T.strong[s] == T.strong[s + 1] && a > b) return false;
    }
    const int us = pos_turn(P);
    const uint64_t ok_k = P.bb[BB_K] & pos_our(P), tk = P.bb[BB_K] & pos_their(P);
    if (!ok_k || !tk) return false;
    const int tks = bo_lsb64(tk);
    if (king_att(tks) & ok_k) return false;
    return attackers_of(P, !us, tks, pos_all(P), 0) == 0;  // the side not to move may not be in check
}
// the king of the side to move has a step to a square that is not attacked: the position is neither mate nor stalemate
BO_DEV bool tb_king_can_step(const DPos &P) {
    const int us = pos_turn(P);
    const uint64_t kbb = P.bb[BB_K] & pos_our(P);
    const int ksq = bo_lsb64(kbb);
    const uint64_t occ = pos_all(P) ^ kbb;
    for (uint64_t t = king_att(ksq) & ~pos_our(P); t; t &= t - 1) {
        if (!attackers_of(P, us, bo_lsb64(t), occ, 0)) return true;
    }
    return false;
}

// ---- build -------------------------------------------------------------------------------------------------------------------------
BO_KERNEL void bo_k_tb_init(const TbTable *tabs) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const TbTable T = tabs[0];
    const int lane = bo_lane();
    const int64_t i0 = (int64_t)bo_block() * TB_RUN;
    for (int r = 0; r < TB_RUN / 64; r++) {
        const int64_t idx = i0 + r * 64 + lane;
        DPos P;
        const bool distinct = tb_decode(T, idx, &P);
        const bool legal = tb_legal(T, idx, P, distinct);
        uint16_t code = legal ? 1 : 0;
        uint64_t stuck = bo_ballot(legal && !tb_king_can_step(P));
        while (stuck) {  // wave-uniform
            const int src = bo_lsb64(stuck);
            stuck &= stuck - 1;
            DPos Q;
            (void)tb_decode(T, i0 + r * 64 + src, &Q);
            bool chk;
            const int n = bo_movegen_inline(Q, mv, &chk);
            if (lane == src && n == 0 && chk) code = 2;
            bo_wave_sync();
        }
        T.codes[idx] = code;  // (each entry is written once, by its own lane)
    }
}

BO_DEV int tb_wave_min(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = bo_shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
BO_DEV int tb_wave_max(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = bo_shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
#define TB_INF 0x7fff
// The value of the legal position P from its children's codes: the code (1 draw / unresolved, 2 + k).  *bad: a child without a code.
BO_DEV uint32_t tb_value(const TbTable *tabs, int n_tabs, const DPos &P, bo_mv *mv, int *bad) {
    const int lane = bo_lane();
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    *bad = 0;
    if (n == 0) return chk ? 2u : 1u;
    int min_loss = TB_INF, worst = -1;  // worst: the largest child win, TB_INF when a child is a draw / unresolved
    int nbad = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        if (j < n) {
            const DPos c = make_move(P, mv[j]);
            const uint32_t code = tb_lookup(tabs, n_tabs, c.bb, pos_turn(c));
            if (code == 0u || code == TB_NO_TABLE) nbad++;
            else if (code == 1u) worst = TB_INF;
            else {
                const int k = (int)code - 2;
                if (k & 1) worst = k > worst ? k : worst;
                else min_loss = k < min_loss ? k : min_loss;
            }
        }
    }
    min_loss = tb_wave_min(min_loss);
    worst = tb_wave_max(worst);
    *bad = tb_wave_max(nbad);
    bo_wave_sync();  // the move list is read before the next position's is written
    if (min_loss != TB_INF) return (uint32_t)(2 + min_loss + 1);
    if (worst == TB_INF || worst < 0) return 1u;
    return (uint32_t)(2 + worst + 1);
}

// counter[0] += the entries assigned the value pass_i; counter[1] += children without a code (must stay 0)
BO_KERNEL void bo_k_tb_pass(const TbTable *tabs, int n_tabs, int pass_i, uint64_t *counter) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const TbTable T = tabs[0];
    const int lane = bo_lane();
    const int64_t i0 = (int64_t)bo_block() * TB_RUN;
    int assigned = 0, nbad = 0;
    for (int r = 0; r < TB_RUN / 64; r++) {
        uint64_t todo = bo_ballot(T.codes[i0 + r * 64 + lane] == 1);
        while (todo) {  // wave-uniform
            const int64_t e = i0 + r * 64 + bo_lsb64(todo);
            todo &= todo - 1;
            DPos P;
            (void)tb_decode(T, e, &P);
            int bad;
            const uint32_t v = tb_value(tabs, n_tabs, P, mv, &bad);
            nbad += bad;
            if (v == (uint32_t)(2 + pass_i)) {
                if (lane == 0) T.codes[e] = (uint16_t)v;
                assigned++;
            }
        }
    }
    if (lane == 0 && assigned) bo_atomic_add_u64(&counter[0], (uint64_t)assigned);
    if (lane == 0 && nbad) bo_atomic_add_u64(&counter[1], (uint64_t)nbad);
}

// counter[0] += mismatches (legality of an index, or a legal entry's code against its children's final codes)
BO_KERNEL void bo_k_tb_verify(const TbTable *tabs, int n_tabs, uint64_t *counter) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const TbTable T = tabs[0];
    const int lane = bo_lane();
    const int64_t i0 = (int64_t)bo_block() * TB_RUN;
    int wrong = 0;
    for (int r = 0; r < TB_RUN / 64; r++) {
        const int64_t idx = i0 + r * 64 + lane;
        const uint32_t code = T.codes[idx];
        DPos L;
        const bool distinct = tb_decode(T, idx, &L);
        const bool legal = tb_legal(T, idx, L, distinct);
        wrong += bo_popc64(bo_ballot(legal != (code != 0)));
        uint64_t todo = bo_ballot(legal && code != 0);
        while (todo) {  // wave-uniform
            const int src = bo_lsb64(todo);
            todo &= todo - 1;
            DPos P;
            (void)tb_decode(T, i0 + r * 64 + src, &P);
            int bad;
            const uint32_t v = tb_value(tabs, n_tabs, P, mv, &bad);
            if (bad || v != (uint32_t)bo_shfl((int)code, src)) wrong++;
        }
    }
    if (lane == 0 && wrong) bo_atomic_add_u64(&counter[0], (uint64_t)wrong);
}

// ---- probe -------------------------------------------------------------------------------------------------------------------------
// status values of bo_tb_probe (include/betaone_engine.h BO_TB_*)
enum { TB_ST_COVERED = 0, TB_ST_NO_TABLE = 1, TB_ST_TOO_MANY = 2, TB_ST_CASTLING = 3, TB_ST_PAWNS = 4, TB_ST_NOT_A_POSITION = 5 };
BO_KERNEL void bo_k_tb_probe(const TbTable *tabs, int n_tabs, const bo_position *pos, int n, uint16_t *codes, int32_t *status) {
    const int i = bo_block() * 64 + bo_lane();
    if (i >= n) return;
    uint64_t bb[8];
#pragma unroll
    for (int k = 0; k < 8; k++) bb[k] = pos[i].bb[k];
    int st = TB_ST_COVERED;
    uint32_t code = 0;
    if (bo_popc64(bb[BB_WHITE] | bb[BB_BLACK]) > TB_MAX_MEN) st = TB_ST_TOO_MANY;
    else if (pos[i].castling & 0xFu) st = TB_ST_CASTLING;
    else if ((bb[BB_P] & bb[BB_WHITE]) && (bb[BB_P] & bb[BB_BLACK])) st = TB_ST_PAWNS;
    else if (bo_popc64(bb[BB_K] & bb[BB_WHITE]) != 1 || bo_popc64(bb[BB_K] & bb[BB_BLACK]) != 1) st = TB_ST_NOT_A_POSITION;
    else {
        code = tb_lookup(tabs, n_tabs, bb, pos[i].turn != 0);
        if (code == TB_NO_TABLE) { st = TB_ST_NO_TABLE; code = 0; }
        else if (code == 0) st = TB_ST_NOT_A_POSITION;
    }
    codes[i] = (uint16_t)code;
    status[i] = st;
}
