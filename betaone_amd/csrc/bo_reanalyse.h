// betaone_amd/csrc/bo_reanalyse.h -- reanalysis of self-play records (betaone_amd/reanalyse.py): the stored positions of a .bog file
// are searched again with a newer net, and the records get that search's pi and root value.  Device code at both ends of the search;
// the search itself is bo_analyse.h's path (bo_k_setup_dev, bo_search_begin_dev, the evaluate -> step graph).
//
//   dpos_from_abi       bo_position (the ABI form, 88 B) -> DPos: the ONE place that packs the flag word.  The host's from_abi
//                       (bo_engine.cpp) is this function; the kernel below calls it on the device.
//   bo_k_records_ring   one lane per position: the concatenated positions of a file's games, as they sit in the .bog body, become ring
//                       entries -- what bo_k_pgn_replay writes for the same positions, byte for byte.  A ring entry carries one bit a
//                       bo_position does not: F_IRREV, "the move that led here was irreversible", which cuts the repetition chain of
//                       a search.  It is a property of the previous position and the move; lane i recovers it from entry i - 1: when
//                       entry i is the child of entry i - 1 by the move between them (move_between + make_move, every field compared),
//                       the child's F_IRREV is taken.  A game's first position is the child of nothing in front of it (the position
//                       after a game's last move is part of the record), and bo_k_setup_dev sets the root's bit itself.
//   bo_k_reanalysis     one wave per game slot, behind bo_k_result, where bo_k_analysis sits in the analysis path: one 16-word record per
//                       slot, the first W entries of the slot's pi row, and the comparison with the pi the record held before.
//
// Vector stores only, no atomics; every loop is bounded (by BO_RES_CAP, by the old pi's length, which the host bounds).  Control flow is
// wave-uniform apart from lane-predicated loads and stores.
#pragma once
#include "bo_analyse.h"

#define BO_REANALYSIS_WORDS 16
#define ST_PI_OVERFLOW 256  // bo_k_reanalysis: the search produced more pi entries than the rows hold (the record's status word only)

#if defined(BO_WAVE_EMU)
#define BO_HOST_DEV static inline
#else
#define BO_HOST_DEV __host__ __device__ __forceinline__
#endif

BO_HOST_DEV DPos dpos_from_abi(const bo_position &p) {
    DPos d;
    for (int i = 0; i < 8; i++) d.bb[i] = p.bb[i];
    d.flags = (p.turn ? F_TURN : 0u) | ((p.castling & 0xFu) << F_CASTLE_SHIFT) | ((uint32_t)(p.ep_square + 1) << F_EP_SHIFT);
    if (p.ep_key >= 0) d.flags |= (uint32_t)(p.ep_key + 1) << F_EPKEY_SHIFT;
    // ep_key == -1 ("no ep component in the key") with a raw ep square present is re-derived on the device by
    // finish_key(); that is deterministic and gives -1 again.  Tracker keys taken from python-chess key tuples
    // carry ep_square == ep_key.
    d.halfmove = p.halfmove_clock;
    d.fullmove = p.fullmove_number;
    d.khash = 0;
    return d;
}

BO_KERNEL void bo_k_records_ring(const bo_position *pos, long long n, DPos *out) {
    const long long i = (long long)bo_block() * 64 + bo_lane();
    if (i >= n) return;
    DPos d = dpos_from_abi(pos[i]);
    finish_key(d);
    if (i > 0) {
        DPos p = dpos_from_abi(pos[i - 1]);
        finish_key(p);
        const bo_mv m = move_between(p, d);
        // (a move between two consistent positions lifts a piece: anything else is no predecessor, and make_move is not asked)
        if (MV_FROM(m) != MV_TO(m) && piece_type_at(p, MV_FROM(m)) != 0) {
            const DPos c = make_move(p, m);
            bool same = ((c.flags ^ d.flags) & ~F_IRREV) == 0 && c.halfmove == d.halfmove && c.fullmove == d.fullmove;
#pragma unroll
            for (int k = 0; k < 8; k++) same = same && c.bb[k] == d.bb[k];
            if (same) d.flags |= c.flags & F_IRREV;
        }
    }
    out[i] = d;
}

struct ReanalysisArgs {
    const int *played;     // [G] the action index the game played from the slot's root (-1 none), or NULL
    const long long *root; // [G] the root's index into old_ptr (-1: no old pi), or NULL with the three below
    const int *old_ptr;    // [roots + 1]
    const int *old_idx;    // the file's pi entries
    const float *old_val;
    int W;                 // entries per output row, 1 .. BO_RES_CAP
    int *out;              // [G][BO_REANALYSIS_WORDS]
    int *pi_idx;           // [G][W]
    float *pi_val;         // [G][W]
};

BO_DEV double bo_shfl_d(double v, int src) { return __builtin_bit_cast(double, bo_shfl_u64(__builtin_bit_cast(uint64_t, v), src)); }

// the first maximum of val[b .. e) in stored order -> its idx (-1: empty); every lane walks the same entries
BO_DEV int first_max_action(const int *idx, const float *val, int b, int e) {
    int a = -1;
    float best = 0.0f;
    for (int k = b; k < e; k++) {
        const float v = val[k];
        if (k == b || v > best) { best = v; a = idx[k]; }
    }
    return a;
}

// One record per slot (include/betaone_engine.h: bo_reanalysis).  Lane l holds word l and stores it once: `out` and the rows may be
// pinned host memory.  Words: 0 terminal, 1 n_legal, 2 total_visits, 3 best_idx, 4 root_value, 5 pi_n, 6 played_prob, 7 has_old,
// 8 agree, 9 tv, 10 phase, 11 status, 12 ply, 13 simulations done, 14 the evaluate stage's watched fault word as bo_k_result left it.
// The rows of a slot whose search has not finished (or never began) are not touched.
BO_KERNEL void bo_k_reanalysis(Eng e, ReanalysisArgs a) {
    const int g = bo_block(), lane = bo_lane();
    const size_t no = NOFF(e, g);
    const int ph = e.phase[g];
    const bool done = ph == PH_DONE && e.root_term[g] == 0;
    int w = 0;
    if (lane == 0) w = e.root_term[g];
    if (lane == 1) w = e.root_nlegal[g];
    if (lane == 3) w = -1;
    if (lane == 10) w = ph;
    if (lane == 11) w = e.status[g];
    if (lane == 12) w = e.ply[g];
    if (lane == 13) w = e.sims_done[g];
    if (lane == 14) w = e.res_watch[0];
    if (done) {
        const int n = e.res_n[g] < BO_RES_CAP ? e.res_n[g] : BO_RES_CAP;
        const int *ridx = e.res_idx + (size_t)g * BO_RES_CAP;
        const float *rval = e.res_val + (size_t)g * BO_RES_CAP;
        const int keep = n < a.W ? n : a.W;
        for (int j = lane; j < a.W; j += 64) {
            a.pi_idx[(size_t)g * a.W + j] = j < keep ? ridx[j] : -1;
            a.pi_val[(size_t)g * a.W + j] = j < keep ? rval[j] : 0.0f;
        }
        const int pa = a.played ? a.played[g] : -1;
        const long long r = a.root ? a.root[g] : -1;
        const int o0 = r >= 0 ? a.old_ptr[r] : 0, o1 = r >= 0 ? a.old_ptr[r + 1] : 0;
        float pp = 0.0f;
        bool pp_found = false;
        double acc = 0.0;
        // the new entries in row order: |new - old(a)|, old(a) = the first old entry with the same action (0 when there is none)
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane, cnt = n - j0 < 64 ? n - j0 : 64;
            const bool in = j < n;
            const int act = in ? ridx[j] : -1;
            const float nv = in ? rval[j] : 0.0f;
            const uint64_t hit = bo_ballot(in && pa >= 0 && act == pa);
            if (hit && !pp_found) { pp = bo_shfl_f(nv, bo_lsb64(hit)); pp_found = true; }
            float ov = 0.0f;
            bool seen = false;
            for (int k = o0; k < o1; k++)
                if (in && !seen && a.old_idx[k] == act) { ov = a.old_val[k]; seen = true; }
            const double t = fabs((double)nv - (double)ov);
            for (int k = 0; k < cnt; k++) acc = acc + bo_shfl_d(t, k);
        }
        // the old entries the new pi does not have, in stored order
        for (int k0 = o0; k0 < o1; k0 += 64) {
            const int k = k0 + lane, cnt = o1 - k0 < 64 ? o1 - k0 : 64;
            const bool in = k < o1;
            const int act = in ? a.old_idx[k] : -1;
            bool absent = in;
            for (int j = 0; j < n; j++) absent = absent && ridx[j] != act;
            const double t = absent ? (double)a.old_val[k] : 0.0;  // (acc is never -0.0: adding the 0.0 of a present entry changes no bit)
            for (int q = 0; q < cnt; q++) acc = acc + bo_shfl_d(t, q);
        }
        const int has_old = r >= 0 ? 1 : 0;
        const int new_arg = first_max_action(ridx, rval, 0, n);
        const int old_arg = has_old ? first_max_action(a.old_idx, a.old_val, o0, o1) : -1;
        if (lane == 2) w = e.res_total[g];
        if (lane == 3) w = e.res_best_idx[g];
        if (lane == 4) w = __builtin_bit_cast(int, e.q[no]);
        if (lane == 5) w = e.res_n[g];
        if (lane == 6) w = __builtin_bit_cast(int, pp);
        if (lane == 7) w = has_old;
        if (lane == 8) w = has_old && old_arg >= 0 && old_arg == new_arg ? 1 : 0;
        if (lane == 9) w = has_old ? __builtin_bit_cast(int, (float)(0.5 * acc)) : 0;
        if (lane == 11 && e.res_n[g] > a.W) w |= ST_PI_OVERFLOW;
    }
    if (lane < BO_REANALYSIS_WORDS) a.out[(size_t)g * BO_REANALYSIS_WORDS + lane] = w;
}
