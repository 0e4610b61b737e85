// tests/wave_emulator/walk_driver.cpp -- TEST INFRASTRUCTURE: the host side of the level walk (bo_perft, bo_mate, bo_anchor, bo_anchor_q,
// bo_anchor_eval) under the sanitizers, and a transcript of its outputs to compare two trees by.
// A stand-alone program over the C ABI (include/betaone_engine.h), compiled TOGETHER with bo_engine.cpp -DBO_WAVE_EMU and
// -fsanitize=address,undefined by walk_driver.sh next to it: the device code runs lane by lane on the CPU, "device" pointers are host
// pointers, so a buffer released early, twice or never is the sanitizer's to find (leak detection stays ON: these entry points keep no
// state between calls).  It is run as an executable, never through pytest and never on a GPU.
//
// The inputs are the smallest that reach every branch of the walk: a level that fits, the roots' level split and a level below them
// split (capacity 256; `splits` in the transcript shows it), in bo_perft, bo_mate, bo_anchor and bo_anchor_q each, a bottom
// level at the roots, roots without a move, records that are no positions, the principal variations of bo_mate, quiescence levels, and
// the argument errors.  Every output array is filled with 0xA5 before the call; after it one line is printed: the return code, n_splits,
// a 64-bit FNV-1a digest of every output array (`nodes` is a field of the results) and, for a failed call, bo_last_error().  The
// transcript is a function of the inputs alone: two trees compute the same if and only if their transcripts are equal line for line.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "betaone_engine.h"

static const char *const KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1";
static const char *const START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";
// tests/mate_cases.py
static const char *const KRK = "7k/8/5K2/8/8/8/8/R7 w - - 0 1";                // mate in 2, two key moves
static const char *const EP_MATE = "8/5K1k/8/5Pp1/8/8/8/B1B5 w - g6 0 1";      // mate in 1 by the en-passant capture
static const char *const EP_GONE = "8/5K1k/8/5Pp1/8/8/8/B1B5 w - - 0 1";       // nothing within 2
static const char *const STALE_TRAP = "8/5P1k/5K2/8/8/8/8/8 w - - 0 1";        // mate in 2 by f8=R
static const char *const PROMO_KEYS = "k7/2P5/1K6/8/8/8/8/8 w - - 0 1";        // mate in 1, several keys
static const char *const KQK = "8/8/8/8/8/5K2/Q7/7k w - - 0 1";
static const char *const WIDE = "3q3k/8/8/8/8/8/P7/K7 w - - 0 1";              // 4 moves, 24 replies to each: no mate within 2
static const char *const MATED = "k6R/8/1K6/8/8/8/8/8 b - - 1 1";
static const char *const STALEMATED = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1";
// tests/anchor_cases.py, tests/anchor_q_cases.py
static const char *const MANY_MOVES = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1";
static const char *const MATED_IN_2 = "7k/p4K1p/7P/8/8/8/8/6R1 b - - 0 1";
static const char *const POISONED = "4k3/8/2p5/3p4/8/8/8/3QK3 w - - 0 1";
static const char *const INNER_TERMINALS = "7k/8/6K1/8/8/5Q2/8/8 w - - 0 1";
static const char *const BACK_RANK = "r2r2k1/5ppp/8/8/8/8/3R1PPP/3R2K1 w - - 0 1";
static const char *const EP_BELOW = "4k3/8/8/8/4p3/8/3P4/4K3 w - - 0 1";
static const char *const PROMO_BELOW = "8/2P4k/8/8/8/8/8/K7 b - - 0 1";

static uint64_t fnv(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
    return h;
}
template <class T> static uint64_t fnv(const std::vector<T> &v) { return fnv(v.data(), v.size() * sizeof(T)); }
template <class T> static std::vector<T> poisoned(size_t n) {
    std::vector<T> v(n);
    if (n) memset(v.data(), 0xA5, n * sizeof(T));
    return v;
}

// a FEN as the record bo_mate and bo_anchor take in `positions` (square 0 = a1; ep_key -2: derived)
static bo_position record(const char *fen) {
    bo_position q;
    memset(&q, 0, sizeof(q));
    int sq = 56;
    const char *s = fen;
    for (; *s && *s != ' '; s++) {
        if (*s == '/') sq -= 16;
        else if (*s >= '1' && *s <= '8') sq += *s - '0';
        else {
            const char *kinds = "pnbrqk", *at = strchr(kinds, *s | 0x20);
            q.bb[at - kinds] |= 1ull << sq;
            q.bb[(*s & 0x20) ? 7 : 6] |= 1ull << sq;
            sq++;
        }
    }
    q.turn = s[1] == 'w';
    for (s += 3; *s && *s != ' '; s++) q.castling |= *s == 'K' ? 1u : *s == 'Q' ? 2u : *s == 'k' ? 4u : *s == 'q' ? 8u : 0u;
    q.ep_square = s[1] == '-' ? -1 : (s[1] - 'a') + 8 * (s[2] - '1');
    q.ep_key = -2;
    q.halfmove_clock = 0; q.fullmove_number = 1;
    return q;
}
static std::vector<bo_position> records(const std::vector<const char *> &fens) {
    std::vector<bo_position> v;
    for (const char *f : fens) v.push_back(record(f));
    return v;
}

static void line(const std::string &what, int rc, long long splits, std::initializer_list<uint64_t> digests) {
    std::printf("%-58s rc %2d splits %3lld", what.c_str(), rc, splits);
    for (uint64_t d : digests) std::printf(" %016llx", (unsigned long long)d);
    if (rc) std::printf("  %s", bo_last_error());
    std::printf("\n");
}

static void perft(const char *what, const std::vector<const char *> &fens, int depth, int64_t cap, uint32_t flags) {
    const size_t n = fens.size();
    auto res = poisoned<bo_perft_result>(n);
    auto dm = poisoned<int32_t>(n * BO_MAX_LEGAL);
    auto dn = poisoned<uint64_t>(n * BO_MAX_LEGAL);
    int64_t splits = -7;
    const int rc = bo_perft(0, (int32_t)n, fens.data(), depth, cap, flags, res.data(), dm.data(), dn.data(), &splits, nullptr);
    line(std::string("perft ") + what + " d" + std::to_string(depth) + " cap " + std::to_string(cap) + " flags " + std::to_string(flags), rc, splits,
         {fnv(res), fnv(dm), fnv(dn)});
}

static void mate(const char *what, const std::vector<const char *> &fens, const std::vector<bo_position> &pos, int moves, int64_t cap,
                 uint64_t max_nodes, uint32_t flags) {
    const size_t n = fens.empty() ? pos.size() : fens.size();
    auto res = poisoned<bo_mate_result>(n);
    auto keys = poisoned<int32_t>(n * BO_MAX_LEGAL);
    auto pv = poisoned<int32_t>(n * (size_t)(2 * moves - 1));
    int64_t splits = -7;
    const int rc = bo_mate(0, (int32_t)n, fens.empty() ? nullptr : fens.data(), fens.empty() ? pos.data() : nullptr, moves, cap, max_nodes, flags,
                           res.data(), keys.data(), pv.data(), &splits, nullptr);
    line(std::string("mate ") + what + " n" + std::to_string(moves) + " cap " + std::to_string(cap) + " flags " + std::to_string(flags) +
             (max_nodes ? " budget" : ""), rc, splits, {fnv(res), fnv(keys), fnv(pv)});
}

// quiesce < 0: bo_anchor
static void anchor(const char *what, const std::vector<const char *> &fens, const std::vector<bo_position> &pos, int depth, int quiesce,
                   int64_t cap, uint32_t flags = 0) {
    const size_t n = fens.empty() ? pos.size() : fens.size();
    auto res = poisoned<bo_anchor_result>(n);
    auto words = poisoned<int32_t>(n * BO_MAX_LEGAL);
    auto scores = poisoned<int32_t>(n * BO_MAX_LEGAL);
    int64_t splits = -7;
    const char *const *f = fens.empty() ? nullptr : fens.data();
    const bo_position *p = fens.empty() ? pos.data() : nullptr;
    const int rc = quiesce < 0 ? bo_anchor(0, (int32_t)n, f, p, depth, cap, flags, res.data(), words.data(), scores.data(), &splits, nullptr)
                               : bo_anchor_q(0, (int32_t)n, f, p, depth, quiesce, cap, flags, res.data(), words.data(), scores.data(), &splits, nullptr);
    line(std::string(quiesce < 0 ? "anchor " : "anchor_q ") + what + " d" + std::to_string(depth) + (quiesce < 0 ? "" : " q" + std::to_string(quiesce)) +
             " cap " + std::to_string(cap), rc, splits, {fnv(res), fnv(words), fnv(scores)});
}

int main() {
    if (bo_abi_version() != BO_ABI_VERSION) return 2;
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const int64_t SMALL = 256, DEFAULT = (int64_t)1 << 20;
    const std::vector<const char *> none;
    const std::vector<bo_position> no_records;

    // perft: the sixteen small roots have more than 300 children and split level 0.  Below the roots a split needs a level of more
    // than 256 entries, and under the sanitizer a wave costs tens of milliseconds (Kiwipete at depth 3 is 2088 waves a call), so the
    // walks are kept narrow where the waves are dear: in WIDE the side to move has 4 moves and the other side 24 replies, three such
    // roots have 12 entries on level 1 and 288 on level 2, each with a handful of moves: capacity 256 splits level 1 there, and at
    // depth 4 a chunk of level 2 is split again.
    const uint32_t ALL = BO_PERFT_DIVIDE | BO_PERFT_STATS | BO_PERFT_ORDER;
    const std::vector<const char *> small = {KQK, KRK, KQK, KRK, KQK, KRK, KQK, KRK, KQK, KRK, KQK, KRK, KQK, KRK, KQK, KRK};
    const std::vector<const char *> wide(3, WIDE);
    for (int64_t cap : {SMALL, (int64_t)300, DEFAULT}) perft("small roots", small, 2, cap, ALL);
    for (int64_t cap : {SMALL, DEFAULT}) perft("wide x 3", wide, 3, cap, ALL);
    perft("wide x 3", wide, 4, SMALL, BO_PERFT_ORDER);
    perft("kiwipete+start+mated", {KIWIPETE, START, MATED}, 2, SMALL, ALL);
    perft("kiwipete+mated", {KIWIPETE, MATED}, 1, SMALL, ALL);
    perft("kiwipete+mated", {KIWIPETE, MATED}, 0, SMALL, ALL);
    perft("mated", {MATED}, 3, SMALL, ALL);
    perft("no roots", none, 3, SMALL, 0);
    perft("capacity", {KIWIPETE}, 2, 255, 0);
    perft("bad fen", {KIWIPETE, "8/8/8 w - -", START}, 2, SMALL, 0);
    perft("flag bits", {KIWIPETE}, 2, SMALL, 8);

    // bo_mate: mates in 1 and 2, none within 2, roots without a move; the WIDE roots split level 1 of the second iteration
    const std::vector<const char *> mates = {KRK, EP_MATE, KQK, STALE_TRAP, MATED, EP_GONE, PROMO_KEYS, STALEMATED};
    std::vector<bo_position> mate_records = records(mates);
    mate_records[2].bb[5] |= 1ull << 27;  // a second white king: not a position
    mate_records[2].bb[6] |= 1ull << 27;
    mate_records[5].castling = 0x10u;     // a field out of range
    for (int64_t cap : {SMALL, DEFAULT}) mate("fens", mates, no_records, 2, cap, 0, BO_MATE_PV);
    mate("wide x 3", wide, no_records, 2, SMALL, 0, BO_MATE_PV);
    mate("records", none, mate_records, 2, SMALL, 0, BO_MATE_PV);
    mate("fens", {KRK, KQK, STALE_TRAP}, no_records, 3, SMALL, 0, BO_MATE_PV);
    mate("fens", mates, no_records, 1, SMALL, 0, BO_MATE_PV);
    mate("fens", mates, no_records, 2, SMALL, 1, 0);
    mate("terminal roots", {MATED, STALEMATED}, no_records, 2, SMALL, 0, BO_MATE_PV);
    mate("no position", none, {mate_records[2], mate_records[5]}, 2, SMALL, 0, BO_MATE_PV);
    mate("capacity", mates, no_records, 2, 255, 0, 0);
    mate("bad fen", {KRK, "k7/8/8/8/8/8/8/8 w - - 0 1", KQK}, no_records, 2, SMALL, 0, 0);
    mate("flag bits", mates, no_records, 2, SMALL, 0, 2);

    // the anchor: roots that are leaves (depth 1, the 218-move root among them), inner terminals, quiescence levels that end early
    const std::vector<const char *> big = {KIWIPETE, MANY_MOVES, MATED, START, BACK_RANK};
    const std::vector<const char *> anchors = {STALE_TRAP, MATED_IN_2, MATED, INNER_TERMINALS, STALEMATED};
    const std::vector<const char *> quiets = {POISONED, KRK, MATED, EP_BELOW, PROMO_BELOW, STALEMATED};
    std::vector<bo_position> anchor_records = records(anchors), quiet_records = records(quiets);
    anchor_records[3].bb[7] = 0;          // black men that are not black: not a position
    quiet_records[1].ep_square = 64;      // a field out of range
    anchor("wide x 3", wide, no_records, 3, -1, SMALL);  // level 1 splits: below a fixed-depth walk,
    anchor("wide x 3", wide, no_records, 2, 1, SMALL);   // and with a quiescence level at the bottom
    anchor("big roots", big, no_records, 1, 1, SMALL);   // level 0 splits
    anchor("fens", anchors, no_records, 3, -1, DEFAULT);
    anchor("fens", quiets, no_records, 2, 2, DEFAULT);
    anchor("records", none, quiet_records, 2, 2, DEFAULT);
    anchor("big roots", big, no_records, 1, -1, SMALL);
    anchor("fens", anchors, no_records, 1, -1, SMALL);
    anchor("records", none, anchor_records, 1, -1, SMALL);
    anchor("fens", anchors, no_records, 3, -1, SMALL);
    anchor("fens", quiets, no_records, 2, 0, SMALL);
    anchor("fens", quiets, no_records, 2, 2, SMALL);
    anchor("records", none, anchor_records, 3, -1, SMALL);
    anchor("records", none, quiet_records, 2, 0, SMALL);
    anchor("records", none, quiet_records, 2, 2, SMALL);
    anchor("fens", quiets, no_records, 2, -1, SMALL);
    anchor("terminal roots", {MATED, STALEMATED}, no_records, 2, -1, SMALL);
    anchor("no position", none, {anchor_records[3]}, 2, 1, SMALL);
    anchor("capacity", anchors, no_records, 2, -1, 255);
    anchor("capacity", anchors, no_records, 2, 1, 255);
    anchor("bad fen", {KRK, "4k3/8/8/8/8/8/8/8 w - - 0 1", POISONED}, no_records, 2, -1, SMALL);
    anchor("bad fen", {KRK, "8/8/8 w - -", POISONED}, no_records, 2, 2, SMALL);
    anchor("flag bits", anchors, no_records, 2, -1, SMALL, 1);
    anchor("flag bits", anchors, no_records, 2, 0, SMALL, 1);
    {
        std::vector<bo_position> evs = records(quiets);
        evs.push_back(anchor_records[1]);
        auto out = poisoned<int32_t>(evs.size());
        const int rc = bo_anchor_eval(0, (int32_t)evs.size(), evs.data(), out.data(), nullptr);
        line("anchor_eval", rc, 0, {fnv(out)});
    }
    std::printf("walk driver: done\n");
    return 0;
}
