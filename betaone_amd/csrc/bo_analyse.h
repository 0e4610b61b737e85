// betaone_amd/csrc/bo_analyse.h -- analysis of games that are already on the device (betaone_amd/analyse.py): device code at both ends
// of a search whose roots are positions of a PGN file.
//
//   bo_k_setup_dev   one wave per game slot: what bo_k_setup does for a self-play context, from positions that bo_k_pgn_replay left in
//                    HBM instead of a FEN and a list of moves: the game's stack gpos[0..ply] and its tracker are COPIED, 64 positions
//                    per pass (lane j takes positions j, j + 64, ...), where bo_k_setup replays the moves one by one on lane 0.  Every
//                    argument is device memory: the host enqueues a batch's set-up behind the previous batch's result kernel and
//                    waits for nothing.
//   bo_k_analysis    one wave per game slot, behind bo_k_result: one fixed-size record per slot -- the root's state, the searched
//                    root's value, how the move that was played in the game fared, and the principal variation.
//   bo_k_pgn_after   one lane per item: the move that an action index of the ring names and the position after it (the position
//                    after a game's LAST move is not in the ring: the PGN writer needs it for that move's check / mate suffix).
//
// No atomics; every loop is bounded: the copy by ply, which is checked against PLY_CAP first, the walk by BO_PV_CAP.  That a node has at
// most 64 children -- one lane each -- is an invariant of the tree (BO_CH_CAP = 32 per expansion, twice that at the root), as in
// bo_k_result; it is not checked here.  Control flow is wave-uniform apart from lane-predicated stores.
#pragma once
#include "bo_tree.h"

#define BO_PV_CAP 16
#define BO_ANALYSIS_WORDS 32
#define ST_BAD_RANGE 128  // bo_k_setup_dev: the slot's positions are not inside the array it was given

// the move that leads from P to C = make_move(P, m): the square our piece left and the one it arrived on (the king's, when it moved:
// castling moves a rook as well), the promotion piece where a pawn became something else
BO_DEV bo_mv move_between(const DPos &P, const DPos &C) {
    const int us = pos_turn(P) ? BB_WHITE : BB_BLACK;
    uint64_t left = P.bb[us] & ~C.bb[us], arrived = C.bb[us] & ~P.bb[us];
    if (left & P.bb[BB_K]) { left &= P.bb[BB_K]; arrived &= C.bb[BB_K]; }
    if (!left || !arrived) return 0;
    const int from = bo_lsb64(left), to = bo_lsb64(arrived);
    int promo = 0;
    if ((P.bb[BB_P] & BIT(from)) && !(C.bb[BB_P] & BIT(to))) promo = piece_type_at(C, to);
    return MV(from, to, promo);
}

struct SetupDevArgs {
    const int *slots;         // [n] game slots to set up
    const DPos *pos;          // [capacity] positions, a game's plies in consecutive entries (bo_k_pgn_replay's ring)
    long long capacity;
    const long long *first;   // [n] the entry of the game's ply 0
    const int *ply;           // [n] the root's ply: entries first .. first + ply are the game so far
};

BO_KERNEL void bo_k_setup_dev(Eng e, SetupDevArgs a) {
    BO_SHARED StepShared sh;
    const int i = bo_block(), lane = bo_lane();
    const int g = a.slots[i];
    if (g < 0 || g >= e.c.G) return;
    const long long f = a.first[i];
    const int ply = a.ply[i];
    int st = 0;
    if (ply < 0 || f < 0 || f + (long long)ply >= a.capacity) st = ST_BAD_RANGE;
    else if (ply + 1 > e.c.PLY_CAP) st = ST_PLY_OVERFLOW;
    else if (ply + 1 > e.c.TRK_CAP) st = ST_TRK_OVERFLOW;
    if (lane == 0) {
        e.status[g] = st;
        e.ctx_mode[g] = 0;
        e.stat_evals[g] = e.stat_flushes[g] = e.stat_term_sims[g] = e.stat_levels[g] = e.stat_children_scanned[g] = 0;
        e.resign_cnt[2 * g] = e.resign_cnt[2 * g + 1] = 0;
    }
    if (st) {  // refused: nothing is copied, the slot holds an empty game whose root is never searched (root_term -1)
        if (lane == 0) {
            const size_t no = NOFF(e, g);
            e.ply[g] = 0; e.trk_n[g] = 0; e.n_hist[g] = 0;
            e.n_nodes[g] = 1; e.n_children[no] = 0; e.n_visits[no] = 0; e.q[no] = 0.0f;
            e.sims_done[g] = 0; e.rows[g] = 0; e.n_runs[g] = 0; e.n_ul[g] = 0; e.req_node[g] = -1; e.phase[g] = PH_IDLE; e.root_nch[g] = 0;
            e.root_nlegal[g] = 0; e.req_nlegal[g] = 0; e.root_term[g] = -1;
        }
        return;
    }
    DPos *gp = e.gpos + (size_t)g * e.c.PLY_CAP;
    DPos *tk = e.trk + (size_t)g * e.c.TRK_CAP;
    int *tc = e.trk_cnt + (size_t)g * e.c.TRK_CAP;
    bo_mv *pl = e.played + (size_t)g * e.c.PLY_CAP;
    for (int k0 = 0; k0 <= ply; k0 += 64) {
        const int k = k0 + lane;
        if (k <= ply) {
            DPos p = a.pos[f + k];
            if (k == 0) { p.flags |= F_IRREV; finish_key(p); }
            gp[k] = p;
            tk[k] = p;  // utils.RepetitionTracker.add_board after every real move (self_play.py:93,182): the live tracker
            tc[k] = 1;
            if (k < ply) pl[k] = move_between(p, a.pos[f + k + 1]);
        }
    }
    if (lane == 0) { e.ply[g] = ply; e.trk_n[g] = ply + 1; }
    bo_sync();
    root_prepare(e, g, sh);
}

// One record per slot (BO_ANALYSIS_WORDS words, include/betaone_engine.h: bo_analysis).  Lane l holds word l and stores it once: `out`
// may be pinned host memory.  Words: 0 terminal, 1 n_legal, 2 total_visits, 3 best_move, 4 root_value, 5 played_is_child,
// 6 played_visits, 7 played_q, 8 pv_len, 9..24 pv, 25 phase, 26 status, 27 ply, 28 simulations done, 29 the evaluate stage's watched fault word as
// bo_k_result left it (bo_engine_watch).
BO_KERNEL void bo_k_analysis(Eng e, const int *played, int *out) {
    const int g = bo_block(), lane = bo_lane();
    const size_t no = NOFF(e, g);
    const int ph = e.phase[g];
    const bool done = ph == PH_DONE && e.root_term[g] == 0;
    int w = 0;
    if (lane == 0) w = e.root_term[g];
    if (lane == 1) w = e.root_nlegal[g];
    if (lane == 3) w = done ? e.res_best_mv[g] : -1;
    if (lane == 25) w = ph;
    if (lane == 26) w = e.status[g];
    if (lane == 27) w = e.ply[g];
    if (lane == 28) w = e.sims_done[g];
    if (lane == 29) w = e.res_watch[0];
    if (done) {
        const int *rank = e.root_child_rank + (size_t)g * 2 * BO_CH_CAP;
        const int pm = played ? played[g] : -1;
        int node = 0, pv_len = 0;
        for (int d = 0; d < BO_PV_CAP; d++) {
            const int nch = e.n_children[no + node], fc = e.first_child[no + node];
            if (nch <= 0) break;
            const bool in = lane < nch;
            const int v = in ? e.n_visits[no + fc + lane] : -1;
            if (d == 0) {  // the root: total visits and the played move's child
                const int total = bo_wave_sum(in ? v : 0);
                const uint64_t hit = bo_ballot(in && pm >= 0 && (int)e.move[no + fc + lane] == pm);
                const int hl = hit ? bo_lsb64(hit) : 0;
                const int hv = bo_shfl(v, hl);
                const float hq = bo_shfl_f(in ? e.q[no + fc + lane] : 0.0f, hl);
                if (lane == 2) w = total;
                if (lane == 5) w = hit ? 1 : 0;
                if (lane == 6) w = hit ? hv : 0;
                if (lane == 7) w = hit ? __builtin_bit_cast(int, hq) : 0;
            }
            // the child with the most visits, the first maximum in child order (at the root: in legal-move order, as bo_k_result)
            int bv = v, bk = in ? (node == 0 ? rank[lane] : lane) : 0x7fffffff, bl = lane;
            for (int m = 1; m < 64; m <<= 1) {
                const int ov = bo_shfl_xor(bv, m), ok = bo_shfl_xor(bk, m), ol = bo_shfl_xor(bl, m);
                if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; bl = ol; }
            }
            if (bo_uniform(bv) <= 0) break;
            node = bo_uniform(fc + bl);
            const int mv = (int)e.move[no + node];
            if (lane == 9 + d) w = mv;
            pv_len++;
        }
        if (lane == 4) w = __builtin_bit_cast(int, e.q[no]);
        if (lane == 8) w = pv_len;
    }
    if (lane < BO_ANALYSIS_WORDS) out[(size_t)g * BO_ANALYSIS_WORDS + lane] = w;
}

// item i: entry idx[i] of the ring -- move_out[i] = the move its action index names there (-1: none), pos_out[i] = the position
// after it (either may be NULL).  One lane per item; an entry outside [0, capacity) gives -1 and a zeroed position.
BO_KERNEL void bo_k_pgn_after(const DPos *pos, const int *act, long long capacity, int n, const long long *idx, DPos *pos_out, int *move_out) {
    const int i = bo_block() * 64 + bo_lane();
    if (i >= n) return;
    const long long s = idx[i];
    DPos C;
    for (int k = 0; k < 8; k++) C.bb[k] = 0;
    C.flags = 0; C.halfmove = 0; C.fullmove = 0; C.khash = 0;
    int mo = -1;
    if (s >= 0 && s < capacity) {
        const DPos P = pos[s];
        bo_mv m;
        if (index_to_move(act[s], P, &m)) { mo = (int)m; C = make_move(P, m); }
    }
    if (move_out) move_out[i] = mo;
    if (pos_out) pos_out[i] = C;
}
