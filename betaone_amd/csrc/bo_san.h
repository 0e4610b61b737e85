// betaone_amd/csrc/bo_san.h -- PGN export: SAN rendered on the device, movetext assembled on the host (the inverse of bo_pgn.h).
//
//   bo_k_san_render      one wave per POSITION, not per game: every position of a game is known (P_0..P_n with P_{i+1} the position
//                        after m_i), so plies are independent.  The position is seen from the side to move (mirrored when black
//                        moves), so that every bitboard access has a constant index and nothing lives in scratch.
//                        bo_movegen_inline on P_i (move list in LDS); a ballot finds m_i in the list, the child (san_child: make_move
//                        with constant indices) must equal P_{i+1}; the SAN body of m_i (no suffix) goes to an 8-byte slot; a
//                        ballot over the legal moves of the same piece type to the same square gives python-chess's minimal
//                        disambiguation.  The state byte of P_i: in check, no legal move, and the ply's status.  The host appends
//                        '+' / '#' to m_{i-1} from the state of P_i, so no two waves write the same byte.
//   bo_k_san_status      one wave per game: the first ply whose status is not ok (a ballot over the game's state bytes).
//   pgn_movetext         host.  Move numbers ("N." / "N..."), SAN + suffix, "{book}" comments, the result token; lines of at most
//                        79 characters, no token split.
#pragma once
#include "bo_pgn.h"

// state byte of a position
#define SAN_ST_CHECK 0x1u      // the side to move is in check
#define SAN_ST_NO_MOVE 0x2u    // the side to move has no legal move
#define SAN_ST_PLY_SHIFT 4     // bits 4..7: BO_PGN_OK / BO_PGN_ILLEGAL / BO_PGN_MISMATCH of the move played from this position

// bo_position (the ABI form, include/betaone_engine.h) -> DPos with its key fields, as the host's from_abi + finish_key, seen from the
// side that moves in the ply being rendered: flip = black moves, and the board is mirrored (ranks reversed, colours swapped).  The side
// to move, `turn`, is then a constant of the call site, so every colour-indexed bitboard access of the chess helpers has a constant
// index and no position has to live in scratch.
BO_DEV DPos san_from_abi(const bo_position &a, bool flip, uint32_t turn) {
    DPos d;
#pragma unroll
    for (int i = 0; i < 6; i++) d.bb[i] = flip ? __builtin_bswap64(a.bb[i]) : a.bb[i];
    d.bb[BB_WHITE] = flip ? __builtin_bswap64(a.bb[BB_BLACK]) : a.bb[BB_WHITE];
    d.bb[BB_BLACK] = flip ? __builtin_bswap64(a.bb[BB_WHITE]) : a.bb[BB_BLACK];
    const uint32_t cr = a.castling & 0xFu, sq = flip ? 56u : 0u;
    // (selects, not branches: the side-to-move bit stays a known constant through every later use of the flags)
    d.flags = turn | ((flip ? (cr >> 2) | ((cr & 3u) << 2) : cr) << F_CASTLE_SHIFT) |
              (a.ep_square >= 0 ? (((uint32_t)a.ep_square ^ sq) + 1) << F_EP_SHIFT : 0u);
    d.halfmove = a.halfmove_clock;
    d.fullmove = a.fullmove_number;
    // finish_key (bo_tree.h): a given key e.p. square, else the raw one when an e.p. capture is legal
    const bool legal_ep = has_legal_ep(d);
    d.flags |= a.ep_key >= 0 ? (((uint32_t)a.ep_key ^ sq) + 1) << F_EPKEY_SHIFT
                             : legal_ep ? (uint32_t)(pos_ep(d) + 1) << F_EPKEY_SHIFT : 0u;
    d.khash = key_hash(d);
    return d;
}

// make_move (bo_chess.h) of a legal move with WHITE to move, as far as the key and the halfmove clock go (the caller counts the
// fullmove number on the board).  Every bitboard index is a constant: make_move indexes by the side to move and by the promoted piece,
// which would keep the child in scratch.
BO_DEV DPos san_child(const DPos &p, bo_mv m) {
    DPos c = p;
    const int from = MV_FROM(m), to = MV_TO(m), promo = MV_PROMO(m), pt = piece_type_at(p, from);
    const uint64_t fb = BIT(from), tb = BIT(to);
    c.halfmove = is_zeroing(p, m) ? 0 : p.halfmove + 1;
    uint32_t cr = (p.flags & F_CASTLE_MASK) & ~castle_bits_touched(fb | tb);
    cr &= pt == 6 ? ~0x06u : ~0u;
    const int ep_old = pos_ep(p), df = (to & 7) - (from & 7), diff = to - from;
#pragma unroll
    for (int i = 0; i < 6; i++) c.bb[i] &= ~fb;
    c.bb[BB_WHITE] &= ~fb;
    const bool castle = pt == 6 && (df == 2 || df == -2);
    const int rf = df < 0 ? 0 : 7, rt = df < 0 ? 3 : 5;  // (e1g1 / e1c1 form)
    const bool ep_cap = pt == 1 && to == ep_old && (diff == 7 || diff == 9) && !(pos_all(p) & tb);
    const uint64_t gone = castle ? 0 : tb | (ep_cap ? BIT(ep_old - 8) : 0);  // the black piece captured
    const int np = castle ? 6 : promo ? promo : pt;
#pragma unroll
    for (int i = 0; i < 6; i++) c.bb[i] = (c.bb[i] & ~gone) | (i == np - 1 ? tb : 0);
    c.bb[BB_R] = castle ? (c.bb[BB_R] & ~BIT(rf)) | BIT(rt) : c.bb[BB_R];
    c.bb[BB_WHITE] = (castle ? (c.bb[BB_WHITE] & ~BIT(rf)) | BIT(rt) : c.bb[BB_WHITE]) | tb;
    c.bb[BB_BLACK] &= ~gone;
    const int ep_new = pt == 1 && diff == 16 && (from >> 3) == 1 ? from + 8 : -1;
    c.flags = (cr | (uint32_t)(ep_new + 1) << F_EP_SHIFT);  // black to move
    const bool legal_ep = ep_new >= 0 && has_legal_ep(c);
    c.flags |= legal_ep ? (uint32_t)(ep_new + 1) << F_EPKEY_SHIFT : 0u;
    return c;
}

BO_DEV int san_letter(int pt) { return pt == 2 ? 'N' : pt == 3 ? 'B' : pt == 4 ? 'R' : pt == 5 ? 'Q' : 'K'; }

// positions pos[0, n_pos): game g holds pos[game_off[g] .. game_off[g + 1]), moves[k] is the move played from pos[k] (ignored for a
// game's last position).  Per position k: san[k] (the SAN body, NUL-padded; 0 when there is no move or it is bad) and state[k].
BO_KERNEL void bo_k_san_render(const int *game_off, int n_games, int n_pos, const bo_position *pos, const int *moves, uint64_t *san,
                               uint8_t *state) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int k = bo_block(), lane = bo_lane();
    int lo = 0, hi = n_games;  // the game of position k: game_off[lo] <= k < game_off[lo + 1]
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = (lo + hi) >> 1;
        if (game_off[mid] <= k) lo = mid;
        else hi = mid;
    }
    const bool last = k + 1 >= n_pos || k + 1 >= game_off[lo + 1];
    const bool flip = pos[k].turn == 0;  // (wave-uniform: one position per wave)
    const int sq = flip ? 56 : 0;        // square ^ sq: the mirrored frame <-> the board
    const DPos P = san_from_abi(pos[k], flip, F_TURN);
    bool chk;
    const int n = bo_movegen_inline(P, mv, &chk);
    bo_wave_sync();
    uint32_t st = (chk ? SAN_ST_CHECK : 0u) | (n == 0 ? SAN_ST_NO_MOVE : 0u);
    uint64_t out = 0;
    if (!last) {
        const int m = moves[k] ^ (sq | sq << 6);  // (a bijection: only a move of the board maps onto a legal move of the frame)
        int found = -1;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const uint64_t hit = bo_ballot(j < n && (int)mv[j] == m);
            if (hit && found < 0) found = j0 + bo_lsb64(hit);
        }
        int ply = BO_PGN_OK;
        if (found < 0) {
            ply = BO_PGN_ILLEGAL;
        } else if ((pos[k + 1].turn != 0) != flip) {
            ply = BO_PGN_MISMATCH;  // (the next position has the wrong side to move)
        } else {
            // the child in the frame has black to move; the fullmove number counts on after black's move on the board
            const DPos C = san_child(P, mv[found]), N = san_from_abi(pos[k + 1], flip, 0u);
            if (!key_equal(C, N) || C.halfmove != N.halfmove || P.fullmove + (flip ? 1 : 0) != N.fullmove) ply = BO_PGN_MISMATCH;
        }
        if (ply == BO_PGN_OK) {
            const bo_mv mm = mv[found];
            const int from = MV_FROM(mm), to = MV_TO(mm), promo = MV_PROMO(mm), pt = piece_type_at(P, from);
            const int ff = from & 7, tf = to & 7, fr = (from ^ sq) >> 3, tr = (to ^ sq) >> 3;
            int len = 0;
            auto put = [&](int c) { out |= (uint64_t)(uint8_t)c << (8 * len); len++; };
            if (pt == 6 && (tf - ff == 2 || ff - tf == 2)) {
                put('O'); put('-'); put('O');
                if (tf < ff) { put('-'); put('O'); }
            } else {
                const bool capture = piece_type_at(P, to) != 0 || (pt == 1 && ff != tf);
                if (pt == 1) {
                    if (capture) { put('a' + ff); put('x'); }
                } else {
                    // other legal moves of the same piece type to the same square (a wave-uniform ballot; the mirror keeps files and
                    // which ranks are equal)
                    bool any = false, same_file = false, same_rank = false;
                    for (int j0 = 0; j0 < n; j0 += 64) {
                        const int j = j0 + lane;
                        const int f2 = j < n ? MV_FROM(mv[j]) : from;
                        const bool o = j < n && MV_TO(mv[j]) == to && f2 != from && piece_type_at(P, f2) == pt;
                        const uint64_t bo = bo_ballot(o), bf = bo_ballot(o && (f2 & 7) == ff), br = bo_ballot(o && (f2 >> 3) == (from >> 3));
                        any = any || bo != 0;
                        same_file = same_file || bf != 0;
                        same_rank = same_rank || br != 0;
                    }
                    put(san_letter(pt));
                    if (any && (same_rank || !same_file)) put('a' + ff);  // python-chess Board.san: the file, the rank, or both
                    if (any && same_file) put('1' + fr);
                    if (capture) put('x');
                }
                put('a' + tf);
                put('1' + tr);
                if (promo) { put('='); put(san_letter(promo)); }
            }
        }
        st |= (uint32_t)ply << SAN_ST_PLY_SHIFT;
    }
    if (lane == 0) {
        san[k] = out;
        state[k] = (uint8_t)st;
    }
}

// game g: bad[2g] = the first ply of the game whose status is not ok (-1: none), bad[2g + 1] = that status (BO_PGN_OK if none)
BO_KERNEL void bo_k_san_status(const int *game_off, int n_pos, const uint8_t *state, int *bad) {
    const int g = bo_block(), lane = bo_lane();
    const int a = game_off[g] < 0 ? 0 : game_off[g];
    const int e = game_off[g + 1] < n_pos ? game_off[g + 1] : n_pos;
    int first = -1, st = BO_PGN_OK;
    for (int b0 = a; b0 < e; b0 += 64) {
        const int j = b0 + lane;
        const int s = j < e ? (int)(state[j] >> SAN_ST_PLY_SHIFT) : 0;
        const uint64_t hit = bo_ballot(s != 0);
        if (hit) {
            const int l = bo_lsb64(hit);
            first = b0 + l - a;
            st = bo_shfl(s, l);
            break;
        }
    }
    if (lane == 0) {
        bad[2 * g] = first;
        bad[2 * g + 1] = st;
    }
}

// ---- host: movetext -------------------------------------------------------------------------------------------------------------
// The movetext of one game: n plies with SAN bodies san[i] (8-byte slots), state[0..n] (the suffix of ply i comes from state[i + 1]),
// the root's side to move and fullmove number, per-ply comment flags (bit 0: "{book}" after the move; may be null) and the result
// token.  false when a ply has no SAN (a bad ply: render it first).
static bool pgn_movetext(int n, const uint8_t *san, const uint8_t *state, bool white_first, int fullmove, const uint8_t *comments,
                         const char *result, std::string *out, const char *text = nullptr, const int32_t *text_off = nullptr,
                         const char *final_comment = nullptr) {
    out->clear();
    std::string line;
    auto emit = [&](const char *tok, size_t len) {
        if (!line.empty() && line.size() + 1 + len > 79) {
            out->append(line);
            out->push_back('\n');
            line.clear();
        }
        if (!line.empty()) line.push_back(' ');
        line.append(tok, len);
    };
    char buf[32];
    bool after_comment = false;
    for (int i = 0; i < n; i++) {
        const bool white = (i % 2 == 0) == white_first;
        const int num = fullmove + (i + (white_first ? 0 : 1)) / 2;
        if (white) emit(buf, (size_t)snprintf(buf, sizeof buf, "%d.", num));
        else if (i == 0 || after_comment) emit(buf, (size_t)snprintf(buf, sizeof buf, "%d...", num));  // (a black move after a comment)
        const uint8_t *s = san + (size_t)8 * i;
        int len = 0;
        while (len < 8 && s[len]) { buf[len] = (char)s[len]; len++; }
        if (len == 0) return false;
        const uint8_t nx = state[i + 1];
        if ((nx & SAN_ST_CHECK) && (nx & SAN_ST_NO_MOVE)) buf[len++] = '#';
        else if (nx & SAN_ST_CHECK) buf[len++] = '+';
        emit(buf, (size_t)len);
        after_comment = comments && (comments[i] & 1);
        if (after_comment) emit("{book}", 6);
        if (text && text_off[i + 1] > text_off[i]) {  // (bo_pgn_movetext_text: the ply's comment text)
            std::string c = "{" + std::string(text + text_off[i], (size_t)(text_off[i + 1] - text_off[i])) + "}";
            emit(c.data(), c.size());
            after_comment = true;
        }
    }
    if (final_comment && final_comment[0]) {
        std::string c = "{" + std::string(final_comment) + "}";
        emit(c.data(), c.size());
    }
    emit(result, strlen(result));
    out->append(line);
    out->push_back('\n');
    return true;
}
