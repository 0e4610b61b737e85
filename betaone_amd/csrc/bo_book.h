// betaone_amd/csrc/bo_book.h -- opening books from games (betaone_amd/book.py): every position of every game inside a ply window is
// grouped by its exact transposition key, and each group gets integer aggregates -- games, results, evals, the lowest ply, the first
// entry that reaches it.  The positions are ring entries that bo_k_pgn_replay / bo_k_records_ring left in HBM; nothing is copied.
//
//   bo_k_book_insert    one lane per work item.  The item's entry is read from the ring; the `back` entries in front of it (the same
//                       game's earlier window plies) are compared first: an equal key there means the game has been counted for this
//                       position already, and the item is skipped.  Then an open-addressing table of T slots (a power of two) is probed
//                       linearly from khash & (T - 1): ONE compare-and-swap on owner[slot] per probed slot either claims an empty slot
//                       (-1 -> the item's index) or returns the item that owns it, whose entry is read from the READ-ONLY ring and
//                       compared (khash first, then key_equal).  At most T probes; then the item is an overflow.
//
// Nothing waits: there is no flag, no spin, and no plain store another workgroup reads.  Everything workgroups share is an atomic
// read-modify-write (relaxed, agent scope) -- owner is only ever touched by the compare-and-swap, whose returned word is the only read
// of it; the columns are only added to / minimised.  What an owner index leads to (entry[], pos[]) was written before the launch.  All
// aggregates are integers: the columns do not depend on the order the items arrive in.  (Which slot a group lands in, and which of
// its items owns it, does depend on it: compare tables by `first`.)
//
// khash is read from the entry, never recomputed: it is the probe start and a filter, equality is key_equal.  Two entries with an
// equal key and DIFFERENT khash words (a caller's error: the kernels that write entries derive khash from the key) are never merged,
// wherever they probe: the filter rejects the pair.
//
// Contention: with a window near ply 0 nearly every game adds to the same few slots.  The lanes of a wave that found the same slot
// combine through LDS first (the slot's low six bits pick one of 64 cells; the cell's last writer leads, lanes of another slot that
// fell on the same cell go on alone), so a wave issues one set of global atomics per distinct slot.  BO_BOOK_NO_COMBINE turns it off.
#pragma once
#include "bo_perft.h"  // the atomic wrappers

#define BOOK_NO_COMBINE 1u
#define BOOK_EVAL_ONE (1 << 20)  // an eval of 1.0 in sum_eval

struct BookArgs {
    const DPos *pos;       // [capacity] the ring
    int64_t capacity, n, T;
    const int64_t *entry;  // [n]
    const int32_t *ply, *result, *back;
    const float *eval;     // [n] or NULL
    int32_t *owner;        // [T] the table's columns
    int64_t *first;
    int32_t *cnt, *w, *d, *l, *n_eval, *min_ply;
    int64_t *sum_eval;
    int32_t *gid;          // [n]
    int32_t *status;       // [2] overflow items, bad entries
    uint32_t flags;
};

BO_KERNEL void bo_k_book_insert(BookArgs a) {
    BO_SHARED int32_t s_lead[64], s_n[64], s_w[64], s_d[64], s_l[64], s_ne[64], s_ply[64];
    BO_SHARED int64_t s_first[64], s_sum[64];
    const int lane = bo_lane();
    const int64_t i = (int64_t)bo_block() * 64 + lane;
    const bool in = i < a.n;
    const int64_t e = in ? a.entry[i] : 0;
    const bool bad = in && (e < 0 || e >= a.capacity);
    bool live = in && !bad;
    DPos P = {};
    if (live) P = a.pos[e];
    // once per game: an equal key among the game's window entries directly in front (never before entry 0)
    if (live) {
        int64_t b = a.back[i];
        if (b > e) b = e;
        for (int64_t j = 1; j <= b; j++) {
            const DPos &Q = a.pos[e - j];
            if (Q.khash == P.khash && key_equal(Q, P)) { live = false; break; }
        }
    }
    int32_t gid = -1;
    if (live) {
        const int64_t mask = a.T - 1;
        int64_t s = (int64_t)P.khash & mask;
        gid = -2;
        for (int64_t k = 0; k < a.T; k++, s = (s + 1) & mask) {
            const int32_t o = bo_atomic_cas_i32(&a.owner[s], -1, (int32_t)i);
            if (o == -1) { gid = (int32_t)s; break; }
            if (o < 0 || o >= a.n) continue;  // (not an item of this call: a column the caller did not set to -1)
            const int64_t oe = a.entry[o];
            if (oe < 0 || oe >= a.capacity) continue;
            const DPos &Q = a.pos[oe];
            if (Q.khash == P.khash && key_equal(Q, P)) { gid = (int32_t)s; break; }
        }
    }
    const bool over = gid == -2;
    live = live && !over;
    if (in) a.gid[i] = gid;
    const int n_over = bo_popc64(bo_ballot(over)), n_bad = bo_popc64(bo_ballot(bad));
    if (lane == 0 && n_over) bo_atomic_add_i32(&a.status[0], n_over);
    if (lane == 0 && n_bad) bo_atomic_add_i32(&a.status[1], n_bad);

    // the item's contribution
    const int32_t r = live ? a.result[i] : 0;
    int32_t cw = r == 1, cd = r == 2, cl = r == 3, cne = 0, cn = 1, cply = live ? a.ply[i] : 0;
    int64_t csum = 0, cfirst = e;
    if (live && a.eval) {
        float v = a.eval[i];
        if (v == v) {  // NaN: no eval
            v = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
            const int64_t q = (int64_t)lrintf(v * (float)BOOK_EVAL_ONE);
            csum = (P.flags & F_TURN) ? q : -q;  // white's view
            cne = 1;
        }
    }
    bool flush = live;
    if (!(a.flags & BOOK_NO_COMBINE)) {
        s_lead[lane] = -1;
        s_n[lane] = s_w[lane] = s_d[lane] = s_l[lane] = s_ne[lane] = 0;
        s_ply[lane] = 0x7fffffff;
        s_first[lane] = 0x7fffffffffffffffLL;
        s_sum[lane] = 0;
        bo_wave_sync();
        const int cell = gid & 63;
        if (live) s_lead[cell] = lane;  // (several lanes may store here: the last one leads the cell)
        bo_wave_sync();
        const int lead = live ? s_lead[cell] : lane;
        const int32_t lead_gid = bo_shfl(gid, lead);  // (every lane shuffles: no && in front of it)
        const bool join = live && lead_gid == gid;
        if (join) {
            bo_atomic_add_i32(&s_n[cell], 1);
            if (cw) bo_atomic_add_i32(&s_w[cell], 1);
            if (cd) bo_atomic_add_i32(&s_d[cell], 1);
            if (cl) bo_atomic_add_i32(&s_l[cell], 1);
            if (cne) { bo_atomic_add_i32(&s_ne[cell], 1); bo_atomic_add_i64(&s_sum[cell], csum); }
            bo_atomic_min_i32(&s_ply[cell], cply);
            bo_atomic_min_i64(&s_first[cell], cfirst);
        }
        bo_wave_sync();
        if (join) {
            flush = lead == lane;
            cn = s_n[cell]; cw = s_w[cell]; cd = s_d[cell]; cl = s_l[cell]; cne = s_ne[cell];
            csum = s_sum[cell]; cply = s_ply[cell]; cfirst = s_first[cell];
        }
    }
    if (flush) {
        bo_atomic_add_i32(&a.cnt[gid], cn);
        if (cw) bo_atomic_add_i32(&a.w[gid], cw);
        if (cd) bo_atomic_add_i32(&a.d[gid], cd);
        if (cl) bo_atomic_add_i32(&a.l[gid], cl);
        if (cne) { bo_atomic_add_i32(&a.n_eval[gid], cne); bo_atomic_add_i64(&a.sum_eval[gid], csum); }
        bo_atomic_min_i32(&a.min_ply[gid], cply);
        bo_atomic_min_i64(&a.first[gid], cfirst);
    }
}
