// betaone_amd/csrc/bo_pgn.h -- PGN pretraining (the reference's PGNDataset, train.py:81-160, without python-chess): a host tokeniser
// that turns PGN text into packed SAN tokens and eval targets per mainline move, and two device kernels.
//
//   pgn_parse            host.  Headers ([FEN] root, [Variant] filter), movetext (move numbers, NAGs, suffix annotations, ';' and
//                        '%' lines, nested variations and the comments in them skipped), one packed token per mainline move, the
//                        move's comments joined and matched against the eval pattern (pgn_eval_target).  Nothing of the text reaches
//                        the device: a token is the regex's groups, packed in 22 bits.
//   bo_k_pgn_replay      one wave per game: per token, bo_movegen on the current position (move list in LDS), one lane per legal
//                        move tests the token against it, a ballot counts the candidates; exactly one is played with make_move.
//                        Per replayed ply: the position, the action index of the played move, the sample flag and z, written to the
//                        game's slots of the ring (the host placed every game: no atomics).  Zero / several candidates end the
//                        game's replay with BO_PGN_ILLEGAL / BO_PGN_AMBIGUOUS; every loop is bounded by the game's token count.
//   bo_k_pgn_sample      one wave per sample: the planes of the sample's ply with the LIVE tracker of the reference's parse (its
//                        RepetitionTracker holds the game's positions 0..k when ply k is encoded, train.py:96-143), i.e. what
//                        bo_k_encode_positions computes with n_pos = k + 1; pi = one entry (the played move, 1.0); z.
//                        History boards come from replay_planes (bo_replay.h), shared with the self-play sampler.
#pragma once
#include "bo_replay.h"

// ---- packed SAN token -------------------------------------------------------------------------------------------------------------
// bits 0..5 destination square, 6..9 from-file + 1 (0: none), 10..13 from-rank + 1, 14..16 piece letter (0: none, else python-chess
// piece type 2..6), 17..19 promotion (0: none, 2..6), 20..21 kind (0: the SAN regex, 1: O-O, 2: O-O-O)
#define PGN_TOK_TO(t) ((int)((t) & 63u))
#define PGN_TOK_FILE(t) ((int)(((t) >> 6) & 15u) - 1)
#define PGN_TOK_RANK(t) ((int)(((t) >> 10) & 15u) - 1)
#define PGN_TOK_PIECE(t) ((int)(((t) >> 14) & 7u))
#define PGN_TOK_PROMO(t) ((int)(((t) >> 17) & 7u))
#define PGN_TOK_KIND(t) ((int)(((t) >> 20) & 3u))

// does legal move m of P carry out token tk?  (python-chess Board.parse_san's candidate filter)
BO_DEV bool pgn_token_matches(uint32_t tk, const DPos &P, bo_mv m) {
    const int from = MV_FROM(m), to = MV_TO(m), pt = piece_type_at(P, from);
    const int kind = PGN_TOK_KIND(tk);
    if (kind == 1) return pt == 6 && to == from + 2;  // castling moves are generated in e1g1 form
    if (kind == 2) return pt == 6 && to == from - 2;
    const int ff = PGN_TOK_FILE(tk), fr = PGN_TOK_RANK(tk), piece = PGN_TOK_PIECE(tk);
    if (to != PGN_TOK_TO(tk) || MV_PROMO(m) != PGN_TOK_PROMO(tk)) return false;  // (a promotion must match exactly; "=K" never does)
    if ((ff >= 0 && (from & 7) != ff) || (fr >= 0 && (from >> 3) != fr)) return false;
    if (piece) return pt == piece;
    if (ff >= 0 && fr >= 0) return true;                        // fully specified from-square: any piece, e1g1 castling included
    return pt == 1 && (ff >= 0 || (from & 7) == (to & 7));      // pawn moves; without a file the pawn stands on the target's file
}

// game g of a batch: tokens tok[tok_rng[2g] .. tok_rng[2g+1]) from root[g]; its plies go to ring slots slot0[g] + t.
// result[2g] = plies replayed, result[2g + 1] = BO_PGN_OK / BO_PGN_ILLEGAL / BO_PGN_AMBIGUOUS.
BO_KERNEL void bo_k_pgn_replay(const uint32_t *tok, const int *tok_rng, const DPos *root, const int8_t *has_eval, const float *target,
                               const int *slot0, DPos *pos, int *act, float *z, int *smp, int *result) {
    BO_SHARED bo_mv mv[BO_MAX_MOVES];
    const int g = bo_block(), lane = bo_lane();
    const int t0 = tok_rng[2 * g], nt = tok_rng[2 * g + 1] - t0;
    const size_t s0 = (size_t)slot0[g];
    DPos P = root[g];
    finish_key(P);
    int st = BO_PGN_OK, nr = 0;
    for (int t = 0; t < nt; t++) {
        const uint32_t tk = tok[t0 + t];
        bool chk;
        const int n = bo_movegen(P, mv, &chk);
        bo_wave_sync();
        int cnt = 0;
        bo_mv found = 0;
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const uint64_t hit = bo_ballot(j < n && pgn_token_matches(tk, P, mv[j]));
            if (hit && cnt == 0) found = mv[j0 + bo_lsb64(hit)];
            cnt += bo_popc64(hit);
        }
        bo_wave_sync();  // (every lane has read the list before the next ply's movegen rewrites it)
        if (cnt != 1) {
            st = cnt == 0 ? BO_PGN_ILLEGAL : BO_PGN_AMBIGUOUS;
            break;
        }
        if (lane == 0) {
            pos[s0 + t] = P;
            act[s0 + t] = move_to_index(found);
        }
        P = make_move(P, found);
        nr = t + 1;
    }
    // ply t is a sample exactly when move t + 1 was replayed and its comment carries an eval (train.py:104-141)
    for (int t = lane; t < nr; t += 64) {
        const bool s = t + 1 < nr && has_eval[t0 + t + 1] != 0;
        smp[s0 + t] = s ? 1 : 0;
        z[s0 + t] = s ? target[t0 + t + 1] : 0.0f;
    }
    if (lane == 0) {
        result[2 * g] = nr;
        result[2 * g + 1] = st;
    }
}

// sample b = ply s_k[b] of the game whose ply 0 is in ring slot s_g0[b]
BO_KERNEL void bo_k_pgn_sample(const DPos *pos, const int *act, const float *z, const int *s_g0, const int *s_k, float *states,
                               int *out_idx, float *out_val, float *zs) {
    const int b = bo_block(), lane = bo_lane();
    const int g0 = s_g0[b], k = s_k[b], slot = g0 + k;
    const int h0 = k < 7 ? 0 : k - 7;
    // the first ply a history board can repeat: the last irreversible move at or before the oldest history board (no position before
    // it equals one after it)
    int lo = 0;
    for (int base = h0; base > 0; base -= 64) {
        const int j = base - lane;
        const uint64_t irr = bo_ballot(j > 0 && (pos[g0 + j].flags & F_IRREV) != 0);
        if (irr) {
            lo = base - bo_lsb64(irr);
            break;
        }
    }
    replay_planes_rep(states, b, pos, slot, k, [&](int h) {
        const DPos H = pos[h];
        int c = 0;
        for (int j = g0 + lo + lane; j <= slot; j += 64) c += key_equal(pos[j], H) ? 1 : 0;
        c = bo_wave_sum(c);
        return c > 1 ? c - 1 : 0;
    });
    if (lane == 0) {
        out_idx[b] = act[slot];
        out_val[b] = 1.0f;
        zs[b] = z[slot];
    }
}

// ---- host: the tokeniser ------------------------------------------------------------------------------------------------------------
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

struct bo_pgn_s {
    std::vector<int32_t> status, tok_off{0};
    std::vector<DPos> root;
    std::vector<uint32_t> tok;
    std::vector<int8_t> has_eval;
    std::vector<float> target;
    std::vector<int64_t> span;  // per game: [begin, end) of its text in the buffer it was parsed from (bo_pgn_spans)
};

static bool pgn_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f' || (c >= 0x1c && c <= 0x1f); }
static bool pgn_digit(char c) { return c >= '0' && c <= '9'; }

// the eval comment pattern ^([+-])(?:M(\d+)|(\d+)\.(\d+))/\d+ \d+\.\d+s(?:,.*)?$ ('.' does not cross a line end) and train.py's
// parse_pgn_eval + eval_to_value: *target = float32(-value).  false: no eval (no match, or math.exp would overflow: the reference
// skips that sample).
static bool pgn_eval_target(const std::string &c, float *target) {
    const char *s = c.c_str();
    const size_t n = c.size();
    if (n == 0 || c.find_first_of("\n\r") != std::string::npos) return false;
    size_t i = 0;
    auto digits = [&](size_t *b, size_t *e) { *b = i; while (i < n && pgn_digit(s[i])) i++; *e = i; return *e > *b; };
    if (s[0] != '+' && s[0] != '-') return false;
    const bool neg = s[0] == '-';
    i = 1;
    size_t a0, a1, b0 = 0, b1 = 0, x0, x1;
    const bool mate = i < n && s[i] == 'M';
    if (mate) {
        i++;
        if (!digits(&a0, &a1)) return false;
    } else {
        if (!digits(&a0, &a1) || i >= n || s[i] != '.') return false;
        i++;
        if (!digits(&b0, &b1)) return false;
    }
    if (i >= n || s[i++] != '/' || !digits(&x0, &x1) || i >= n || s[i++] != ' ' || !digits(&x0, &x1) || i >= n || s[i++] != '.' ||
        !digits(&x0, &x1) || i >= n || s[i++] != 's')
        return false;
    if (i < n && s[i] != ',') return false;
    double value;
    if (mate) {  // value = 1.0 if sign * int(n) > 0 else -1.0 (so +M0 gives -1.0)
        bool nonzero = false;
        for (size_t k = a0; k < a1; k++) nonzero = nonzero || s[k] != '0';
        value = !neg && nonzero ? 1.0 : -1.0;
    } else {
        const double a = strtod(std::string(s + a0, a1 - a0).c_str(), nullptr);
        const double f = strtod(("0." + std::string(s + b0, b1 - b0)).c_str(), nullptr);
        if (!isfinite(a)) return false;
        double ev = a + f;
        if (neg) ev = -ev;
        const double e = exp(-(ev / 2));
        if (isinf(e)) return false;
        value = 2.0 / (1.0 + e) - 1.0;
        value = value < 1.0 ? value : 1.0;    // Python's min(1.0, value)
        value = value > -1.0 ? value : -1.0;  // max(-1.0, ...)
    }
    *target = (float)(-value);
    return true;
}

// SAN -> packed token: castling, else python-chess's SAN regex ^([NBKRQ])?([a-h])?([1-8])?[-x]?([a-h][1-8])(=?[nbrqkNBRQK])?[+#]?$
// matched with the regex engine's backtracking order (optional groups tried present first), so the groups are the ones it reports.
static int pgn_piece(char c) { return c == 'N' ? 2 : c == 'B' ? 3 : c == 'R' ? 4 : c == 'Q' ? 5 : c == 'K' ? 6 : 0; }
static int pgn_promo(char c) {
    const char l = (char)(c >= 'A' && c <= 'Z' ? c - 'A' + 'a' : c);
    return l == 'n' ? 2 : l == 'b' ? 3 : l == 'r' ? 4 : l == 'q' ? 5 : l == 'k' ? 6 : 0;
}
static bool pgn_pack_san(const std::string &w, uint32_t *out) {
    std::string c = w;
    if (!c.empty() && (c.back() == '+' || c.back() == '#')) c.pop_back();
    if (c == "O-O" || c == "0-0") { *out = 1u << 20; return true; }
    if (c == "O-O-O" || c == "0-0-0") { *out = 2u << 20; return true; }
    const char *s = w.c_str();
    const int L = (int)w.size();
    for (int po = 1; po >= 0; po--) {
        int p0 = 0, pc = 0;
        if (po) { if (L > 0 && pgn_piece(s[0])) { pc = pgn_piece(s[0]); p0 = 1; } else continue; }
        for (int fo = 1; fo >= 0; fo--) {
            int p1 = p0, ff = -1;
            if (fo) { if (p1 < L && s[p1] >= 'a' && s[p1] <= 'h') { ff = s[p1] - 'a'; p1++; } else continue; }
            for (int ro = 1; ro >= 0; ro--) {
                int p2 = p1, fr = -1;
                if (ro) { if (p2 < L && s[p2] >= '1' && s[p2] <= '8') { fr = s[p2] - '1'; p2++; } else continue; }
                for (int so = 1; so >= 0; so--) {
                    int p3 = p2;
                    if (so) { if (p3 < L && (s[p3] == '-' || s[p3] == 'x')) p3++; else continue; }
                    if (!(p3 + 1 < L && s[p3] >= 'a' && s[p3] <= 'h' && s[p3 + 1] >= '1' && s[p3 + 1] <= '8')) continue;
                    const int to = (s[p3 + 1] - '1') * 8 + (s[p3] - 'a');
                    for (int pr = 0; pr < 3; pr++) {  // "=Q", "Q", none
                        int p4 = p3 + 2, promo = 0;
                        if (pr == 0) { if (p4 + 1 < L && s[p4] == '=' && pgn_promo(s[p4 + 1])) { promo = pgn_promo(s[p4 + 1]); p4 += 2; } else continue; }
                        if (pr == 1) { if (p4 < L && pgn_promo(s[p4])) { promo = pgn_promo(s[p4]); p4++; } else continue; }
                        for (int xo = 1; xo >= 0; xo--) {
                            int p5 = p4;
                            if (xo) { if (p5 < L && (s[p5] == '+' || s[p5] == '#')) p5++; else continue; }
                            if (p5 != L) continue;
                            *out = (uint32_t)to | (uint32_t)(ff + 1) << 6 | (uint32_t)(fr + 1) << 10 | (uint32_t)pc << 14 | (uint32_t)promo << 17;
                            return true;
                        }
                    }
                }
            }
        }
    }
    return false;
}

static bool pgn_fen_root(const std::string &fen, DPos *out);  // bo_engine.cpp: parse_fen + one king per side

static std::string pgn_trim(const char *b, const char *e) {
    while (b < e && pgn_ws(*b)) b++;
    while (e > b && pgn_ws(e[-1])) e--;
    return std::string(b, e);
}

// Parses the whole games in text[0, n): appends them to p, returns the bytes consumed.  A game ends at its result token, at the next
// game's first header, or (final) at the end of the text; when !final the text after the last complete game is left for the next call.
// Stops before a game that would exceed max_games games / max_tokens tokens in p (< 0: no limit; at least one game is always taken).
static int64_t pgn_parse(bo_pgn_s *p, const char *t, int64_t n, bool final, int64_t max_games, int64_t max_tokens) {
    int64_t i = 0, consumed = 0;
    auto line_start = [&](int64_t k) { return k == 0 || t[k - 1] == '\n' || t[k - 1] == '\r'; };
    auto skip_line = [&](int64_t k) { while (k < n && t[k] != '\n' && t[k] != '\r') k++; return k; };
    const size_t games0 = p->status.size();
    while (i < n) {
        if (max_games >= 0 && (int64_t)p->status.size() >= max_games && p->status.size() > games0) break;
        std::string fen, variant;
        bool have_fen = false, in_moves = false, any = false, stopped = false, complete = false;
        int status = BO_PGN_OK, depth = 0;
        int64_t first = -1;  // the first byte the game's text proper starts at: its first tag, word or variation (bo_pgn_spans)
        std::vector<uint32_t> toks;
        std::vector<std::string> com;
        int64_t k = i;
        while (k < n) {
            const char c = t[k];
            if (pgn_ws(c)) { k++; continue; }
            if (c == '%' && line_start(k)) { k = skip_line(k); continue; }
            if (c == ';') { k = skip_line(k); continue; }
            if (c == '{') {
                const char *e = (const char *)memchr(t + k + 1, '}', (size_t)(n - k - 1));
                if (!e) { k = n; if (final) complete = true; break; }  // (an unterminated comment runs to the end of the text)
                if (depth == 0 && in_moves && !stopped && !toks.empty()) {
                    const std::string s = pgn_trim(t + k + 1, e);
                    if (!s.empty()) com.back() = com.back().empty() ? s : com.back() + " " + s;
                }
                k = e + 1 - t;
                continue;
            }
            if (c == '(') { if (first < 0) first = k; depth++; k++; any = true; continue; }
            if (c == ')') { if (depth) depth--; k++; continue; }
            if (c == '}') { k++; continue; }  // (a stray closing brace)
            if (c == '[' && depth == 0) {
                if (in_moves) { complete = true; break; }  // the next game's headers: this one ended without a result
                any = true;
                if (first < 0) first = k;
                int64_t q = k + 1;
                while (q < n && pgn_ws(t[q])) q++;
                const int64_t n0 = q;
                while (q < n && !pgn_ws(t[q]) && t[q] != '"' && t[q] != ']') q++;
                const std::string name(t + n0, (size_t)(q - n0));
                while (q < n && pgn_ws(t[q]) && t[q] != '\n') q++;
                if (q < n && t[q] == '"') {
                    std::string v;
                    for (q++; q < n && t[q] != '"'; q++) {
                        if (t[q] == '\\' && q + 1 < n && (t[q + 1] == '"' || t[q + 1] == '\\')) q++;
                        v.push_back(t[q]);
                    }
                    if (q >= n) { k = n; break; }
                    if (name == "FEN") { fen = v; have_fen = true; }
                    if (name == "Variant") variant = v;
                    while (q < n && t[q] != ']' && t[q] != '\n' && t[q] != '\r') q++;
                    k = q < n && t[q] == ']' ? q + 1 : q;
                } else {
                    k = skip_line(q);
                }
                continue;
            }
            if (c == '$') { k++; while (k < n && pgn_digit(t[k])) k++; continue; }
            const int64_t w0 = k;
            while (k < n && !pgn_ws(t[k]) && t[k] != '{' && t[k] != '}' && t[k] != '(' && t[k] != ')' && t[k] != ';' && t[k] != '[') k++;
            if (k == w0) { k++; continue; }  // ('[' inside a variation)
            if (k == n && !final) break;      // the word may go on in the next chunk
            if (first < 0) first = w0;
            any = true;
            in_moves = true;
            if (depth > 0) continue;
            std::string w(t + w0, (size_t)(k - w0));
            if (w == "1-0" || w == "0-1" || w == "1/2-1/2" || w == "*") { complete = true; break; }
            if (stopped) continue;
            if (w == "--" || w == "Z0" || w == "0000" || w == "@@@@") { status = BO_PGN_NULL_MOVE; stopped = true; continue; }
            size_t q = 0;
            while (q < w.size() && pgn_digit(w[q])) q++;
            if (q == w.size() || (q > 0 && w[q] == '.')) w.erase(0, q);  // move number "12." / "12..." (also glued to the move: "12.e4")
            q = 0;
            while (q < w.size() && w[q] == '.') q++;
            w.erase(0, q);
            if (w.empty()) continue;
            for (int r = 0; r < 2 && !w.empty() && (w.back() == '!' || w.back() == '?'); r++) w.pop_back();  // !, ?, !!, ??, !?, ?!
            if (w.empty()) continue;
            if (w == "--" || w == "Z0" || w == "0000" || w == "@@@@") { status = BO_PGN_NULL_MOVE; stopped = true; continue; }
            uint32_t pk;
            if (!pgn_pack_san(w, &pk)) { status = BO_PGN_UNSUPPORTED; stopped = true; continue; }
            toks.push_back(pk);
            com.emplace_back();
        }
        if (k >= n && !complete) {
            if (!final) break;           // an unfinished game: left for the next call
            if (!any) { i = consumed = n; break; }
        }
        if (!any && !complete) { i = consumed = k; continue; }
        // the game is complete
        if (max_tokens >= 0 && p->status.size() > games0 && (int64_t)(p->tok.size() + toks.size()) > max_tokens) break;
        DPos root;
        std::string vl;
        for (char ch : variant) vl.push_back((char)(ch >= 'A' && ch <= 'Z' ? ch - 'A' + 'a' : ch));
        if (!variant.empty() && vl != "standard" && vl != "chess") { status = BO_PGN_VARIANT; toks.clear(); }
        else if (!pgn_fen_root(have_fen ? fen : std::string(), &root)) { status = BO_PGN_BAD_FEN; toks.clear(); }
        if (status == BO_PGN_VARIANT || status == BO_PGN_BAD_FEN) memset(&root, 0, sizeof(root));
        p->status.push_back(status);
        p->root.push_back(root);
        for (size_t j = 0; j < toks.size(); j++) {
            float tg = 0.0f;
            const bool ev = pgn_eval_target(com[j], &tg);
            p->tok.push_back(toks[j]);
            p->has_eval.push_back(ev ? 1 : 0);
            p->target.push_back(ev ? tg : 0.0f);
        }
        p->tok_off.push_back((int32_t)p->tok.size());
        p->span.push_back(first < 0 ? k : first);  // ('%' lines, ';' comments and blanks in front of the game are not part of it)
        p->span.push_back(k);
        i = consumed = k;
    }
    return consumed;
}
