// betaone_amd/csrc/bo_perft.h -- perft on the GPU: the move generator and make_move of bo_chess.h walked over whole trees.
//
// perft(d) = the number of move sequences of length d from a root (python-chess Board perft, oracle/bo_rules.c:bo_perft): draw rules
// are ignored, only a position without legal moves ends a line.  The tree is walked level by level on a frontier of DPos in HBM, one
// wavefront per frontier entry, with the SAME bo_movegen / make_move the searches run -- so what is counted (and hashed, for the move
// ORDER) is the rules code of the product.
//   entry tag            int32: root index * 256 + index of the root's move that leads to the entry (the root itself: root index * 256).
//                        Counts are accumulated per tag, so divide costs nothing extra.
//   bo_k_perft_roots     per root: key fields as bo_k_setup leaves them (finish_key), its move list for divide
//   bo_k_perft_count     one wave per entry: move list into LDS; an inner level writes the move count for the scan, the LAST level adds
//                        it to nodes[tag] (bulk counting: the positions of depth d are never made).  The list's hash goes to the
//                        root's checksum when asked.
//   bo_k_perft_count_stats   the last level in stats mode: the wave makes each move in turn, runs bo_movegen on the child and
//                        classifies the leaf
//   bo_k_perft_tile_sums / bo_k_perft_tile_scan / bo_k_perft_offsets   exclusive scan of the counts (tiles of 1024; 64-bit offsets)
//   bo_k_perft_split     the longest run of consecutive entries from `a` whose children fit the next level's buffer
//   bo_k_perft_expand    lane i (in rounds of 64) makes move i and stores the child and its tag at offset + i: placement is
//                        deterministic, the host reads one 8-byte total between levels
#pragma once
#include "bo_tree.h"

#define BO_PERFT_TILE 1024  // entries per scan tile: 16 rounds of one wave
#define BO_PERFT_FNV_BASIS 0xcbf29ce484222325ULL
#define BO_PERFT_FNV_PRIME 0x100000001b3ULL
enum { PF_CAPTURES = 0, PF_EP = 1, PF_CASTLES = 2, PF_PROMOTIONS = 3, PF_CHECKS = 4, PF_CHECKMATES = 5, PF_STALEMATES = 6, PF_NSTATS = 7 };
// mode bits of bo_k_perft_count
#define PF_LEAF 0x1u       // the entries are at depth d - 1: their moves are the leaves
#define PF_ORDER 0x4u      // add the move list's hash to the root's checksum
#define PF_ROOT_LEVEL 0x8u // the entries are the roots: a child's tag is tag + move index

#if defined(BO_WAVE_EMU)
BO_DEV void bo_atomic_add_u64(uint64_t *p, uint64_t v) { *p += v; }
// (bo_book.h) the emulator runs one lane at a time and one workgroup after another: plain operations
BO_DEV int32_t bo_atomic_cas_i32(int32_t *p, int32_t expect, int32_t v) { const int32_t o = *p; if (o == expect) *p = v; return o; }
BO_DEV void bo_atomic_add_i32(int32_t *p, int32_t v) { *p += v; }
BO_DEV void bo_atomic_min_i32(int32_t *p, int32_t v) { if (v < *p) *p = v; }
BO_DEV void bo_atomic_add_i64(int64_t *p, int64_t v) { *p += v; }
BO_DEV void bo_atomic_min_i64(int64_t *p, int64_t v) { if (v < *p) *p = v; }
#else
// global_atomic_add_x2 without a return value
BO_DEV void bo_atomic_add_u64(uint64_t *p, uint64_t v) { (void)atomicAdd((unsigned long long *)p, (unsigned long long)v); }
// (bo_book.h) relaxed, agent scope: read-modify-writes that every XCD sees at the same place; on an LDS address they become ds_* operations.
// The compare-and-swap returns the word it found (== expect: the swap happened).
BO_DEV int32_t bo_atomic_cas_i32(int32_t *p, int32_t expect, int32_t v) {
    (void)__hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}
BO_DEV void bo_atomic_add_i32(int32_t *p, int32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
BO_DEV void bo_atomic_min_i32(int32_t *p, int32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
BO_DEV void bo_atomic_add_i64(int64_t *p, int64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
BO_DEV void bo_atomic_min_i64(int64_t *p, int64_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

// inclusive prefix sum over lanes in ASCENDING lane order
BO_DEV int bo_wave_scan_asc(int v) {
    const int lane = bo_lane();
    for (int d = 1; d < 64; d <<= 1) {
        int o = bo_shfl(v, (lane - d) & 63);
        if (lane >= d) v += o;
    }
    return v;
}

BO_KERNEL void bo_k_perft_roots(DPos *roots, int32_t *root_moves, int32_t *root_n) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int r = bo_block(), s = bo_lane();
    DPos P = roots[r];  // (every lane resolves the key: the same value, one store)
    P.flags |= F_IRREV;
    finish_key(P);
    if (s == 0) roots[r] = P;
    bool chk;
    const int n = bo_movegen(P, mv, &chk);
    for (int i = s; i < BO_MAX_MOVES; i += 64) root_moves[(size_t)r * BO_MAX_MOVES + i] = i < n ? (int32_t)mv[i] : -1;
    if (s == 0) root_n[r] = n;
}

// entry a + block of the frontier (pos, tag).  STATS is a kernel of its own: it makes every child (make_move indexes the position's
// bitboards, which puts the position in scratch memory) and generates a second move list -- the bulk count, the hot kernel of the
// walk, keeps its position in registers (bo_movegen_inline) and uses no scratch.
template <bool STATS>
BO_DEV void perft_count(const DPos *pos, const int32_t *tag, int64_t a, int32_t *cnt, uint64_t *nodes, uint64_t *sums, uint64_t *stats,
                        uint32_t mode, bo_mv *mv, bo_mv *mv2) {
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const DPos P = pos[e];
    const int32_t tg = tag[e];
    const int root = tg >> 8;
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);  // the hot call of the walk: P stays in registers
    if ((mode & PF_ORDER) && s == 0) {
        uint64_t h = BO_PERFT_FNV_BASIS;
        for (int i = 0; i < n; i++) h = (h ^ (uint64_t)mv[i]) * BO_PERFT_FNV_PRIME;
        bo_atomic_add_u64(&sums[root], h);
    }
    if (!(mode & PF_LEAF)) {
        if (s == 0) cnt[e] = n;
        return;
    }
    if (mode & PF_ROOT_LEVEL) {  // depth 1: every move of the root is a leaf of its own
        for (int i = s; i < n; i += 64) bo_atomic_add_u64(&nodes[tg + i], 1);
    } else if (s == 0 && n) bo_atomic_add_u64(&nodes[tg], (uint64_t)n);
    if (!STATS) return;
    int st[PF_NSTATS];
#pragma unroll
    for (int k = 0; k < PF_NSTATS; k++) st[k] = 0;
    const uint64_t their = pos_their(P), all = pos_all(P);
    for (int i = 0; i < n; i++) {  // wave-uniform: every lane holds the same child
        const bo_mv m = mv[i];
        const int from = MV_FROM(m), to = MV_TO(m);
        const bool pawn = (P.bb[BB_P] & BIT(from)) != 0, king = (P.bb[BB_K] & BIT(from)) != 0;
        const bool ep = pawn && to == pos_ep(P) && (from & 7) != (to & 7) && !(all & BIT(to));
        const int df = (to & 7) - (from & 7);
        st[PF_CAPTURES] += ((their & BIT(to)) != 0 || ep) ? 1 : 0;
        st[PF_EP] += ep ? 1 : 0;
        st[PF_CASTLES] += (king && (df == 2 || df == -2)) ? 1 : 0;
        st[PF_PROMOTIONS] += MV_PROMO(m) ? 1 : 0;
        const DPos c = make_move(P, m);
        bool chk2;
        const int n2 = bo_movegen_inline(c, mv2, &chk2);
        st[PF_CHECKS] += chk2 ? 1 : 0;
        st[PF_CHECKMATES] += (chk2 && n2 == 0) ? 1 : 0;
        st[PF_STALEMATES] += (!chk2 && n2 == 0) ? 1 : 0;
    }
    if (s == 0) {
#pragma unroll
        for (int k = 0; k < PF_NSTATS; k++)
            if (st[k]) bo_atomic_add_u64(&stats[(size_t)root * PF_NSTATS + k], (uint64_t)st[k]);
    }
}
BO_KERNEL void bo_k_perft_count(const DPos *pos, const int32_t *tag, int64_t a, int32_t *cnt, uint64_t *nodes, uint64_t *sums, uint32_t mode) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    perft_count<false>(pos, tag, a, cnt, nodes, sums, nullptr, mode, mv, nullptr);
}
BO_KERNEL void bo_k_perft_count_stats(const DPos *pos, const int32_t *tag, int64_t a, uint64_t *nodes, uint64_t *sums, uint64_t *stats,
                                      uint32_t mode) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    BO_SHARED bo_mv mv2[BO_MAX_MOVES];
    perft_count<true>(pos, tag, a, nullptr, nodes, sums, stats, mode | PF_LEAF, mv, mv2);
}

// ---- exclusive scan of cnt[0..n) into off[0..n], off[n] = the total --------------------------------------------------------------
BO_KERNEL void bo_k_perft_tile_sums(const int32_t *cnt, int64_t n, int32_t *tsum) {
    const int b = bo_block(), s = bo_lane();
    const int64_t i0 = (int64_t)b * BO_PERFT_TILE;
    int v = 0;
    for (int r = 0; r < BO_PERFT_TILE / 64; r++) {
        const int64_t i = i0 + r * 64 + s;
        v += i < n ? cnt[i] : 0;
    }
    v = bo_wave_sum(v);
    if (s == 0) tsum[b] = v;
}
// one wave: tile bases (a tile holds at most 1024 * 256 children, 64 tiles fit an int), the total behind the last offset
BO_KERNEL void bo_k_perft_tile_scan(const int32_t *tsum, int n_tiles, uint64_t *tbase, uint64_t *off, int64_t n) {
    const int s = bo_lane();
    uint64_t carry = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += 64) {
        const int i = t0 + s;
        const int v = i < n_tiles ? tsum[i] : 0;
        const int incl = bo_wave_scan_asc(v);
        if (i < n_tiles) tbase[i] = carry + (uint64_t)(incl - v);
        carry += (uint64_t)bo_shfl(incl, 63);
    }
    if (s == 0) off[n] = carry;
}
BO_KERNEL void bo_k_perft_offsets(const int32_t *cnt, int64_t n, const uint64_t *tbase, uint64_t *off) {
    const int b = bo_block(), s = bo_lane();
    const int64_t i0 = (int64_t)b * BO_PERFT_TILE;
    uint64_t carry = tbase[b];
    for (int r = 0; r < BO_PERFT_TILE / 64; r++) {
        const int64_t i = i0 + r * 64 + s;
        const int v = i < n ? cnt[i] : 0;
        const int incl = bo_wave_scan_asc(v);
        if (i < n) off[i] = carry + (uint64_t)(incl - v);
        carry += (uint64_t)bo_shfl(incl, 63);
    }
}
// out[0] = the largest e in (a, n] with off[e] - off[a] <= cap, out[1] = off[e] - off[a].  An entry has at most 256 <= cap children,
// so e > a.
BO_KERNEL void bo_k_perft_split(const uint64_t *off, int64_t a, int64_t n, int64_t cap, int64_t *out) {
    if (bo_lane() != 0) return;
    const uint64_t base = off[a];
    int64_t lo = a + 1, hi = n;  // off[lo] - base <= cap holds
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] - base <= (uint64_t)cap) lo = mid;
        else hi = mid - 1;
    }
    out[0] = lo;
    out[1] = (int64_t)(off[lo] - base);
}

// children of entry a + block at out[off[entry] - off[a] + i]; nothing is stored at or beyond out_cap
BO_KERNEL void bo_k_perft_expand(const DPos *pos, const int32_t *tag, const uint64_t *off, int64_t a, DPos *out_pos, int32_t *out_tag,
                                 int64_t out_cap, uint32_t mode) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int s = bo_lane();
    const int64_t e = a + bo_block();
    const DPos P = pos[e];
    const int32_t tg = tag[e];
    const int64_t o = (int64_t)(off[e] - off[a]);
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    for (int i = s; i < n; i += 64) {
        if (o + i >= out_cap) break;
        out_pos[o + i] = make_move(P, mv[i]);
        out_tag[o + i] = (mode & PF_ROOT_LEVEL) ? tg + i : tg;
    }
}
