// betaone_amd/csrc/bo_sym.h -- the two exact symmetries of chess for the replay samplers (bo_replay.h, bo_merge.h): a record is handed
// out as its twin at the moment a batch is made.  The input planes are absolute (encode_block / encode_scalars of bo_tree.h after the
// reference's encode_board: white and black planes of their own, plane 112 = who moves, nothing turned to the side to move), so the
// net sees a pattern once per colour and once per wing unless the sampler shows it the twins.
//
// A transform code t: bit 0 = COLOUR FLIP (swap the colours, mirror the ranks, toggle the turn; always valid; z and q are from the side
// to move's point of view and do not change), bit 1 = FILE MIRROR (a <-> h; valid when the position has no castling right left).
//   sym_applied(flags, t)  the code that is applied to a record whose CURRENT position has these flags: the mirror bit is dropped while
//                          any castling right is left.  All eight history boards of a sample get this one code (their own castling
//                          rights are not in the planes).
//   sym_pos(P, t)          the transformed position as far as encode_block, encode_scalars and pos_ep read it: the eight bitboards,
//                          the turn, the castling bits, the raw en-passant square.  halfmove and fullmove are kept.  khash, F_IRREV and
//                          the en-passant KEY field are LEFT AS THEY ARE: they belong to the untransformed position and no encoder reads
//                          them -- a transformed DPos is for the encoders only, never for key_equal or the move generator.
//   sym_action(a, t)       the policy index of the transformed move, closed form (no table in memory): with a = from * 73 + plane
//                          (utils.move_to_index, utils.py:221-281), the from square is mirrored and the plane's direction index goes
//                          through a reflection of the compass: queen directions N NE E SE S SW W NW (d -> (4 - d) & 7 for the rank
//                          mirror, (-d) & 7 for the file mirror), knight directions (k -> (3 - k) & 7, 7 - k), underpromotions are
//                          indexed relative to the pawn's colour already (unchanged by the colour flip; the capture side 0 <-> 2 under
//                          the file mirror).  An involution on all 4672 indices; -1 (an unused slot) stays -1.
#pragma once
#include "bo_chess.h"

#define SYM_COLOUR 1
#define SYM_MIRROR 2

BO_DEV int sym_applied(uint32_t flags, int t) { return (flags & F_CASTLE_MASK) ? (t & SYM_COLOUR) : t; }

// colour flip = byte swap (rank r <-> 7 - r); file mirror = the bits of every byte reversed = bit reverse, then byte swap; both = bit reverse
BO_DEV uint64_t sym_bb(uint64_t x, int t) {
    if (t & SYM_MIRROR) x = bo_bitrev64(x);
    if (t == SYM_COLOUR || t == SYM_MIRROR) x = __builtin_bswap64(x);
    return x;
}

BO_DEV DPos sym_pos(const DPos &P, int t) {
    DPos T = P;
#pragma unroll
    for (int i = 0; i < 6; i++) T.bb[i] = sym_bb(P.bb[i], t);
    const uint64_t w = sym_bb(P.bb[BB_WHITE], t), b = sym_bb(P.bb[BB_BLACK], t);
    T.bb[BB_WHITE] = (t & SYM_COLOUR) ? b : w;
    T.bb[BB_BLACK] = (t & SYM_COLOUR) ? w : b;
    uint32_t f = P.flags;
    if (t & SYM_COLOUR) f = ((f & ~F_CASTLE_MASK) | ((f & 0x06u) << 2) | ((f & 0x18u) >> 2)) ^ F_TURN;  // K<->k, Q<->q
    const uint32_t raw = (f & F_EP_MASK) >> F_EP_SHIFT;  // square + 1; 0 = none
    if (raw >= 1 && raw <= 64) {  // (anything else is no square and shows in no plane: kept)
        const uint32_t sq = (raw - 1) ^ ((t & SYM_COLOUR) ? 56u : 0u) ^ ((t & SYM_MIRROR) ? 7u : 0u);
        f = (f & ~F_EP_MASK) | ((sq + 1) << F_EP_SHIFT);
    }
    T.flags = f;
    return T;
}

BO_DEV int sym_action(int a, int t) {
    if (a < 0) return a;
    int from = a / 73, p = a - from * 73;
    if (t & SYM_COLOUR) {
        from ^= 56;
        if (p < 56) { const int d = p / 7; p += (((4 - d) & 7) - d) * 7; }
        else if (p < 64) p = 56 + ((3 - (p - 56)) & 7);
    }
    if (t & SYM_MIRROR) {
        from ^= 7;
        if (p < 56) { const int d = p / 7; p += (((8 - d) & 7) - d) * 7; }
        else if (p < 64) p = 56 + (7 - (p - 56));
        else { const int u = p - 64, piece = u / 3; p = 64 + 3 * piece + (2 - (u - 3 * piece)); }
    }
    return from * 73 + p;
}
