// betaone_amd/csrc/bo_tb_probe.h -- the probing half of the endgame tablebases (bo_tb.h): the table descriptor and the lookup of one
// position's code.  It needs the bitboards only (bo_chess.h), so the tree kernels (bo_tree.h) can probe a leaf without seeing the build,
// verify and perft kernels that bo_tb.h and bo_perft.h hold.  Layout, codes and the mirror: the head of bo_tb.h.
#pragma once
#include "bo_chess.h"

#define TB_MAX_MEN 4
#define TB_RUN 1024        // indices per workgroup: 16 rounds of one wave (2 * 64^n is a multiple for n >= 2)
#define TB_MAX_TABLES 64   // tables per probe set
#define TB_NO_TABLE 0xFFFFu

struct TbTable {
    uint16_t *codes;
    uint32_t sig;      // material: 3 bits per count, P N B R Q of the strong side from bit 0, of the weak side from bit 16
    int32_t n_men;
    uint8_t pt[TB_MAX_MEN];   // python-chess piece type 1..6 per slot
    uint8_t strong[TB_MAX_MEN];  // 1 = the strong side's (white in the table's frame)
};

BO_DEV uint32_t tb_sig_of(const uint64_t *bb, uint64_t strong, uint64_t weak) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) s |= (uint32_t)bo_popc64(bb[i] & strong) << (3 * i) | (uint32_t)bo_popc64(bb[i] & weak) << (16 + 3 * i);
    return s;
}
BO_DEV uint32_t tb_sig_swap(uint32_t s) { return (s >> 16) | ((s & 0xFFFFu) << 16); }
// KK, KBK, KNK: no table, a draw (the material-level part of Board.is_insufficient_material())
BO_DEV bool tb_insufficient(const uint64_t *bb) {
    const int men = bo_popc64(bb[BB_WHITE] | bb[BB_BLACK]);
    return men <= 2 || (men == 3 && (bb[BB_N] | bb[BB_B]) != 0);
}
BO_DEV uint64_t tb_pick(const uint64_t *bb, int pt) {  // bb[pt - 1] with constant indices
    uint64_t r = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) r = pt == i + 1 ? bb[i] : r;
    return r;
}
// The code of position P (any frame) in the set tabs[0..n): TB_NO_TABLE when no table has its material, 1 for insufficient material.
BO_DEV uint32_t tb_lookup(const TbTable *tabs, int n_tabs, const uint64_t *pbb, int white_to_move) {
    if (tb_insufficient(pbb)) return 1u;
    const int men = bo_popc64(pbb[BB_WHITE] | pbb[BB_BLACK]);
    const uint32_t sig = tb_sig_of(pbb, pbb[BB_WHITE], pbb[BB_BLACK]), sig_m = tb_sig_swap(sig);
    int t = -1;
    bool mir = false;
    for (int i = n_tabs - 1; i >= 0; i--) {  // (the first match wins; the plain frame before the mirror)
        if (tabs[i].n_men != men) continue;
        if (tabs[i].sig == sig_m) { t = i; mir = true; }
    }
    for (int i = n_tabs - 1; i >= 0; i--) {
        if (tabs[i].n_men == men && tabs[i].sig == sig) { t = i; mir = false; }
    }
    if (t < 0) return TB_NO_TABLE;
    uint64_t bb[8];
#pragma unroll
    for (int i = 0; i < 6; i++) bb[i] = mir ? __builtin_bswap64(pbb[i]) : pbb[i];
    bb[BB_WHITE] = mir ? __builtin_bswap64(pbb[BB_BLACK]) : pbb[BB_WHITE];
    bb[BB_BLACK] = mir ? __builtin_bswap64(pbb[BB_WHITE]) : pbb[BB_BLACK];
    const int strong_moves = mir ? !white_to_move : white_to_move;
    const TbTable &T = tabs[t];
    int64_t idx = strong_moves ? 0 : 1;
    uint64_t taken = 0;
    for (int s = 0; s < T.n_men; s++) {  // identical men take their squares in ascending order
        const uint64_t c = tb_pick(bb, T.pt[s]) & (T.strong[s] ? bb[BB_WHITE] : bb[BB_BLACK]) & ~taken;
        if (!c) return 0u;
        const int sq = bo_lsb64(c);
        taken |= BIT(sq);
        idx = idx * 64 + sq;
    }
    return T.codes[idx];
}
