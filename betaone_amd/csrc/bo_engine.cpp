// betaone_amd/csrc/bo_engine.cpp -- host side of the C ABI (include/betaone_engine.h).
// Compiled by hipcc for gfx950 into libbetaone_hip.so together with the kernels in bo_tree.h.
// No torch types, no chess logic on the host: FEN / UCI text is parsed into plain bitboards and
// everything else (replaying the move stack, keys, legality, draw rules) happens on the device.
#include "../../include/betaone_engine.h"
#include "../../include/betaone_lab.h"  // measurement / introspection entry points: exported by the same library, not part of the boundary

#include "bo_tree.h"
#include "bo_fastw.h"
#include "bo_info.h"
#include "bo_select_wide.h"
#include "bo_replay.h"
#include "bo_train.h"
#include "bo_metrics.h"
#include "bo_pgn.h"
#include "bo_san.h"
#include "bo_analyse.h"
#include "bo_reanalyse.h"
#include "bo_perft.h"
#include "bo_mate.h"
#include "bo_anchor.h"
#include "bo_book.h"
#include "bo_merge.h"
#include "bo_tb.h"
#include "bo_nn_fused.h"
#include "bo_conv.h"
#include "bo_tower.h"
#include "bo_tower_wg.h"
#include "bo_tower_h.h"
#include "bo_tower_s.h"
#include "bo_tower_s16.h"
#include "bo_tower_h16.h"
#include "bo_heads.h"
#include "bo_tower_b1.h"
#include "bo_rt.h"
#include "bo_hostrng.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include <deque>
#include <memory>
#include <type_traits>

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define RT(call)                                                                                     \
    do {                                                                                             \
        int _rc = (call);                                                                            \
        if (_rc != 0) return fail(BO_E_HIP, std::string(#call) + ": " + rt_errstr(_rc));             \
    } while (0)

struct bo_engine {
    Eng d;
    FastW f;
    int fast_reuse = 1;  // keep the played child's subtree for the next search (bo_fast_options)
    // optional timing of the fast mode's select + backup kernel with HIP events on the launch stream (bo_fast_stats)
    int sel_profile = 0, sel_pending = 0;
    long long sel_launches = 0;
    double sel_ms = 0.0;
#if !defined(BO_WAVE_EMU)
    hipEvent_t sel_ev0 = nullptr, sel_ev1 = nullptr;
#endif
    bool fast = false;
    bo_config cfg;
    int device;
    std::vector<void *> allocs;
    int *d_go = nullptr, *d_action = nullptr;
    std::vector<int> h_i32;  // scratch [G]
    std::vector<HostRng> rng;          // one legacy MT19937 stream per game slot (bo_rng_seed)
    // The per-move host exchange goes through two device blocks and their pinned mirrors, one copy each:
    //   res  = [res_n | res_best_idx | res_best_mv | res_total | res_idx[RES_CAP] | res_val[RES_CAP]]  (G rows each)
    //   info = [phase | req_node | root_nlegal | root_term | ply]
    int *d_res_blk = nullptr, *d_info_blk = nullptr;
    int *h_res = nullptr, *h_info = nullptr;  // pinned
    int watch_seen = 0;                        // OR of the watched status word over the fetched result blocks (bo_engine_watch)
    double *h_noise = nullptr;                // pinned [G][256]
    int *h_go = nullptr;                      // pinned [G]
    int *h_action = nullptr;                  // pinned [2][G]: the actions of two consecutive bo_play calls (read by the kernel itself)
    int action_flip = 0;
    rt_event ev_action[2]{};                  // behind the bo_k_play that reads each half: a third bo_play waits for the first one's kernel
    bool ev_action_made[2] = {false, false};
    bool ship = true;                         // the turn's small blocks move by bo_k_ship instead of copy commands (BETAONE_TURN_COPIES=1: copies)
    bool prefetch_valid = false;              // bo_search_result_prefetch has been enqueued behind the searches and nothing was stepped since
    std::vector<int> h_nl, h_term;
    bool nl_valid = false;  // h_nl holds the current roots' legal-move counts (set by bo_selfplay_begin)
    void *setup_dev = nullptr, *setup_host = nullptr;  // staging of bo_games_reset_ex (grow-only)
    size_t setup_cap = 0;
    std::vector<unsigned char> noise_pending;  // roots begun by bo_selfplay_turn(defer_noise) whose Dirichlet draw is still due
    // bo_selfplay_turn(flag 4): searches begun on the device; the roots' state is on its way (ev_begin), bo_selfplay_begun collects it
    std::vector<int> lazy_want;
    bool begin_lazy = false, ev_begin_made = false;
    rt_event ev_begin{};
    // bo_selfplay_autoturn: the turn on the device.  In: the choice() uniforms and per-game flags (pinned, read by the kernel itself), the
    // temperature table; out (behind the five info rows, one bo_k_ship): action | state | compact result [G][8]
    double *h_turn_u = nullptr;
    int *h_turn_flags = nullptr;
    double *d_turn_pw = nullptr;
    std::vector<double> turn_pw_host;
    double turn_pw_tfinal = 0.0;  // the T_final the table was built for (0: none yet)
    int *d_turn_action = nullptr, *d_turn_state = nullptr, *d_turn_cres = nullptr;
    float *d_turn_rv = nullptr;                          // info row 15: v_i (the searched roots' q_value)
    int *d_turn_resigned = nullptr, *d_turn_rnext = nullptr;  // info rows 16, 17 (row 17 stays on the device)
    std::vector<int> resign_en;                          // bo_selfplay_resign: per slot, resignation enabled (flag bit 3)
    float resign_t = 0.0f;
    int resign_k = 1;
    float *d_root_value = nullptr;                       // bo_search_root_value's staging [G]
    TbTable *d_tb_tabs = nullptr;                        // bo_engine_tablebases: room for TB_MAX_TABLES descriptors (Eng.tb_tabs points here)
    std::vector<int> turn_want;
    bool turn_outstanding = false, ev_turn_made = false;
    rt_event ev_turn{};
    template <class T> int alloc(T **p, size_t n) {
        void *v = nullptr;
        int rc = rt_malloc(&v, n * sizeof(T));
        if (rc) return rc;
        allocs.push_back(v);
        *p = (T *)v;
        return 0;
    }
};

extern "C" int bo_abi_version(void) { return BO_ABI_VERSION; }
extern "C" const char *bo_last_error(void) { return g_err.c_str(); }

// ---- text -> plain data (host) ---------------------------------------------------------------------
static const char *START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1";

static bool parse_fen(const char *fen, DPos *out) {
    memset(out, 0, sizeof(*out));
    const char *s = fen;
    while (*s == ' ') s++;
    int r = 7, f = 0;
    for (; *s && *s != ' '; s++) {
        char c = *s;
        if (c == '/') { r--; f = 0; continue; }
        if (c >= '1' && c <= '8') { f += c - '0'; continue; }
        int white = (c >= 'A' && c <= 'Z');
        char l = (char)(white ? c - 'A' + 'a' : c);
        int t = l == 'p' ? 0 : l == 'n' ? 1 : l == 'b' ? 2 : l == 'r' ? 3 : l == 'q' ? 4 : l == 'k' ? 5 : -1;
        if (t < 0 || r < 0 || f > 7) return false;
        out->bb[t] |= BIT(r * 8 + f);
        out->bb[white ? BB_WHITE : BB_BLACK] |= BIT(r * 8 + f);
        f++;
    }
    int turn = 1, ep = -1, half = 0, full = 1;
    uint32_t cr = 0;
    while (*s == ' ') s++;
    if (*s) { if (*s == 'w') turn = 1; else if (*s == 'b') turn = 0; else return false; s++; }
    while (*s == ' ') s++;
    for (; *s && *s != ' '; s++) {
        if (*s == 'K') cr |= 0x02u; else if (*s == 'Q') cr |= 0x04u; else if (*s == 'k') cr |= 0x08u;
        else if (*s == 'q') cr |= 0x10u; else if (*s != '-') return false;
    }
    // python-chess clean_castling_rights(): rook on its corner, king on e1/e8
    const uint64_t wk = out->bb[BB_K] & out->bb[BB_WHITE] & BIT(4), bk = out->bb[BB_K] & out->bb[BB_BLACK] & BIT(60);
    const uint64_t wr = out->bb[BB_R] & out->bb[BB_WHITE], br = out->bb[BB_R] & out->bb[BB_BLACK];
    if (!wk || !(wr & BIT(7))) cr &= ~0x02u;
    if (!wk || !(wr & BIT(0))) cr &= ~0x04u;
    if (!bk || !(br & BIT(63))) cr &= ~0x08u;
    if (!bk || !(br & BIT(56))) cr &= ~0x10u;
    while (*s == ' ') s++;
    if (*s) {
        if (*s != '-') {
            if (s[0] < 'a' || s[0] > 'h' || s[1] < '1' || s[1] > '8') return false;
            ep = (s[1] - '1') * 8 + (s[0] - 'a');
            s += 2;
        } else s++;
    }
    while (*s == ' ') s++;
    if (*s) half = (int)strtol(s, (char **)&s, 10);
    while (*s == ' ') s++;
    if (*s) full = (int)strtol(s, (char **)&s, 10);
    if (full < 1) full = 1;
    out->flags = (turn ? F_TURN : 0u) | cr | ((uint32_t)(ep + 1) << F_EP_SHIFT);
    out->halfmove = half;
    out->fullmove = full;
    return true;
}

// a PGN game's root: its [FEN] (empty: the start position), with exactly one king per side (the move generator needs them)
static bool pgn_fen_root(const std::string &fen, DPos *out) {
    if (!parse_fen(fen.empty() ? START_FEN : fen.c_str(), out)) return false;
    const uint64_t k = out->bb[BB_K];
    return __builtin_popcountll(k & out->bb[BB_WHITE]) == 1 && __builtin_popcountll(k & out->bb[BB_BLACK]) == 1;
}

static bool parse_uci_moves(const char *s, std::vector<bo_mv> *out) {
    out->clear();
    if (!s) return true;
    while (*s) {
        while (*s == ' ') s++;
        if (!*s) break;
        const char *b = s;
        while (*s && *s != ' ') s++;
        size_t n = (size_t)(s - b);
        if (n < 4 || n > 5) return false;
        if (b[0] < 'a' || b[0] > 'h' || b[2] < 'a' || b[2] > 'h' || b[1] < '1' || b[1] > '8' || b[3] < '1' || b[3] > '8') return false;
        int from = (b[1] - '1') * 8 + (b[0] - 'a'), to = (b[3] - '1') * 8 + (b[2] - 'a'), promo = 0;
        if (n == 5) {
            promo = b[4] == 'n' ? 2 : b[4] == 'b' ? 3 : b[4] == 'r' ? 4 : b[4] == 'q' ? 5 : -1;
            if (promo < 0) return false;
        }
        out->push_back(MV(from, to, promo));
    }
    return true;
}

static DPos from_abi(const bo_position &p) { return dpos_from_abi(p); }  // (bo_reanalyse.h: shared with bo_k_records_ring)
static void to_abi(const DPos &d, bo_position *p) {
    for (int i = 0; i < 8; i++) p->bb[i] = d.bb[i];
    p->turn = (int)(d.flags & F_TURN);
    p->castling = (d.flags & F_CASTLE_MASK) >> F_CASTLE_SHIFT;
    p->ep_square = (int)((d.flags & F_EP_MASK) >> F_EP_SHIFT) - 1;
    p->ep_key = (int)((d.flags & F_EPKEY_MASK) >> F_EPKEY_SHIFT) - 1;
    p->halfmove_clock = d.halfmove;
    p->fullmove_number = d.fullmove;
}

// ---- create / destroy -------------------------------------------------------------------------------
extern "C" int bo_engine_create(const bo_config *cfg, int device, bo_engine **out) {
    if (!cfg || !out) return fail(BO_E_ARG, "null argument");
    if (cfg->n_games < 1 || cfg->num_simulations < 0 || cfg->mcts_batch_size < 1 || cfg->max_plies < 2)
        return fail(BO_E_ARG, "n_games/num_simulations/mcts_batch_size/max_plies out of range");
    const bool fast = cfg->mode == 1;
    if (cfg->mode != 0 && cfg->mode != 1) return fail(BO_E_ARG, "mode must be 0 (reference semantics) or 1 (fast)");
    if (fast && (cfg->leaves_per_step < 1 || cfg->leaves_per_step > BO_FW_LMAX)) return fail(BO_E_ARG, "leaves_per_step out of range (1..64)");
    const int root_m = fast ? 1 : (int)(cfg->widen_coeff * sqrt(1.0));
    const int ch_max = fast ? 1 : (int)(cfg->widen_coeff * sqrt((double)cfg->mcts_batch_size));
    if (!fast && (cfg->widen_coeff < 1.0 || ch_max > BO_CH_CAP))
        return fail(BO_E_CONFIG, "WIDEN_COEFF must be >= 1 and int(WIDEN_COEFF*sqrt(MCTS_BATCH_SIZE)) <= 32");
    RT(rt_set_device(device));
    bo_engine *e = new bo_engine();
    e->cfg = *cfg;
    e->device = device;
    EngCfg &c = e->d.c;
    c.G = cfg->n_games; c.S = cfg->num_simulations; c.B = cfg->mcts_batch_size;
    e->fast = fast;
    // Node capacity in reference semantics: a leaf evaluated with k rows of a batch gets int(W*sqrt(k)) children (mcts.py:55-57), and
    // the k over all evaluated leaves of a search sum to at most S, so at most S * max_k int(W*sqrt(k))/k nodes beside the root's
    // (= S for the reference's W = 1.5; a larger WIDEN_COEFF creates more nodes per simulation).
    double per_sim = 1.0;
    for (int k = 1; k <= cfg->mcts_batch_size; k++) {
        const double r = (double)(int)(cfg->widen_coeff * sqrt((double)k)) / (double)k;
        if (r > per_sim) per_sim = r;
    }
    // (fast mode keeps its trees in child-block arenas, bo_fastw.h; the node arrays below then only hold the root's slot)
    c.NCAP = fast ? 2 : (int)ceil(c.S * per_sim) + 2 * root_m + 4;
    c.nstride = c.NCAP;
    c.PLY_CAP = cfg->max_plies; c.TRK_CAP = cfg->max_plies;
    c.UL_MAX = fast ? 1 : c.B; c.CH_MAX = ch_max < 1 ? 1 : ch_max;
    c.cpuct = (float)cfg->cpuct;
    c.keep = (float)(1.0 - cfg->dirichlet_epsilon);
    c.eps = cfg->dirichlet_epsilon;
    c.use_noise = cfg->dirichlet_alpha > 0 ? 1 : 0;
    c.root_m = root_m;
    c.profile = 0;
    { const char *v = getenv("BETAONE_BURST_TWO_PATHS"); c.burst_two = (v && v[0] == '0') ? 0 : 1; }
    c.root_q = 0;
    const size_t G = (size_t)c.G, N = G * (size_t)c.NCAP;
    Eng &d = e->d;
    int rc = 0;
    float *sq = nullptr, *rcp = nullptr; int *wl = nullptr;
    rc |= e->alloc(&sq, (size_t)c.S + 2); rc |= e->alloc(&wl, (size_t)c.B + 1); rc |= e->alloc(&rcp, (size_t)c.S + 3);
    int **iscal[] = {&d.sims_done, &d.n_nodes, &d.rows, &d.n_runs, &d.n_ul, &d.req_nlegal, &d.status,
                     &d.trk_n, &d.n_hist, &d.ctx_mode, &d.root_nch, &d.stat_evals,
                     &d.stat_flushes, &d.stat_term_sims, &d.stat_levels, &d.stat_children_scanned, &e->d_go, &e->d_action};
    for (int **p : iscal) rc |= e->alloc(p, G);
    const size_t res_ints = G * (4 + 2 * (size_t)BO_RES_CAP) + 4, info_ints = G * 18;  // (+ 4: the watched status word, bo_engine_watch; info rows 5..17: bo_selfplay_autoturn's outputs)
    rc |= e->alloc(&e->d_res_blk, res_ints); rc |= e->alloc(&e->d_info_blk, info_ints);
    if (!rc) {
        d.res_n = e->d_res_blk; d.res_best_idx = e->d_res_blk + G; d.res_best_mv = e->d_res_blk + 2 * G; d.res_total = e->d_res_blk + 3 * G;
        d.res_idx = e->d_res_blk + 4 * G; d.res_val = reinterpret_cast<float *>(e->d_res_blk + 4 * G + G * BO_RES_CAP);
        d.res_watch = e->d_res_blk + G * (4 + 2 * (size_t)BO_RES_CAP); d.watch = nullptr; d.watch_n = 1;
        d.phase = e->d_info_blk; d.req_node = e->d_info_blk + G; d.root_nlegal = e->d_info_blk + 2 * G; d.root_term = e->d_info_blk + 3 * G;
        d.ply = e->d_info_blk + 4 * G;
        e->d_turn_action = e->d_info_blk + 5 * G; e->d_turn_state = e->d_info_blk + 6 * G; e->d_turn_cres = e->d_info_blk + 7 * G;
        e->d_turn_rv = reinterpret_cast<float *>(e->d_info_blk + 15 * G); e->d_turn_resigned = e->d_info_blk + 16 * G;
        e->d_turn_rnext = e->d_info_blk + 17 * G;
        rt_memset(e->d_res_blk, 0, res_ints * 4, nullptr); rt_memset(e->d_info_blk, 0, info_ints * 4, nullptr);
    }
    rc |= rt_host_alloc((void **)&e->h_res, res_ints * 4); rc |= rt_host_alloc((void **)&e->h_info, info_ints * 4);
    rc |= rt_host_alloc((void **)&e->h_noise, G * BO_MAX_MOVES * sizeof(double)); rc |= rt_host_alloc((void **)&e->h_go, G * 4);
    rc |= rt_host_alloc((void **)&e->h_action, 2 * G * 4);
    rc |= rt_host_alloc((void **)&e->h_turn_u, G * sizeof(double)); rc |= rt_host_alloc((void **)&e->h_turn_flags, G * 4);
    rc |= e->alloc(&e->d_turn_pw, (size_t)cfg->num_simulations + 1);
    { const char *v = getenv("BETAONE_TURN_COPIES"); e->ship = !(v && v[0] == '1'); }
    rc |= e->alloc(&d.gpos, G * c.PLY_CAP); rc |= e->alloc(&d.trk, G * c.TRK_CAP); rc |= e->alloc(&d.trk_cnt, G * c.TRK_CAP);
    rc |= e->alloc(&d.hist, G * 7);
    rc |= e->alloc(&d.n_visits, N); rc |= e->alloc(&d.parent, N); rc |= e->alloc(&d.first_child, N); rc |= e->alloc(&d.n_children, N);
    rc |= e->alloc(&d.q, N); rc |= e->alloc(&d.prior, N); rc |= e->alloc(&d.move, N); rc |= e->alloc(&d.term, N);
    rc |= e->alloc(&d.eval_slot, N); rc |= e->alloc(&d.npos, N);
    rc |= e->alloc(&d.run_leaf, G * c.B); rc |= e->alloc(&d.run_cnt, G * c.B);
    rc |= e->alloc(&d.ul_node, G * c.UL_MAX); rc |= e->alloc(&d.ul_nlegal, G * c.UL_MAX); rc |= e->alloc(&d.ul_value, G * c.UL_MAX);
    rc |= e->alloc(&d.ul_move, G * c.UL_MAX * BO_CH_CAP); rc |= e->alloc(&d.ul_prior, G * c.UL_MAX * BO_CH_CAP);
    rc |= e->alloc(&d.req_moves, G * BO_MAX_MOVES); rc |= e->alloc(&d.root_moves, G * BO_MAX_MOVES);
    rc |= e->alloc(&d.root_child_rank, G * 2 * BO_CH_CAP); rc |= e->alloc(&d.noise, G * BO_MAX_MOVES);
    rc |= e->alloc(&d.played, G * c.PLY_CAP);
    rc |= e->alloc(&d.prof, G * BO_PROF_SLOTS);
    rc |= e->alloc(&d.resign_cnt, 2 * G); rc |= e->alloc(&e->d_root_value, G);
    if (!rc) rt_memset(d.resign_cnt, 0, 2 * G * 4, nullptr);
    rc |= e->alloc(&e->d_tb_tabs, (size_t)TB_MAX_TABLES); rc |= e->alloc(&d.tb_stat, 3 * G);
    if (!rc) rt_memset(d.tb_stat, 0, 3 * G * 4, nullptr);
    d.tb_tabs = e->d_tb_tabs; d.tb_n = 0; d.tb_flags = 0;
    d.played_now = nullptr;
    if (fast) {
        FastW &f = e->f;
        const size_t L = (size_t)cfg->leaves_per_step;
        f.L = (int)L;
        f.sel_ut = 2; f.sel_flags = FW_SEL_OCT;  // measured fastest on an MI355X (profiles/r03_fast_select_variants.md): eight lanes per game
                                                 // (more than 8 leaves per step: the half-wave forms)
        // Arena capacity per game, in granules of BO_FW_GR records.  A search creates at most S + L + 1 runs (one per expanded
        // node: header + 1..32 record granules, ~6 granules = 768 bytes at chess's ~35 legal moves) on top of the subtree kept
        // from the previous search: room for 24 granules (3 KB) per possible expansion of this and of the previous search.
        // A run that still does not fit is refused (status bit) -- the search goes on with that leaf unexpanded.
        const size_t expansions = (size_t)c.S + L + 2;
        f.NG = cfg->fast_arena_granules > 0 ? cfg->fast_arena_granules : (int)((6 * expansions + 8) * (32 / BO_FW_GR));
        if (f.NG < 64 || f.NG > BO_FW_LINK_MASK) { bo_engine_destroy(e); return fail(BO_E_ARG, "fast_arena_granules out of range (64 .. 2^24 - 1)"); }
        const size_t NR = (size_t)f.NG * BO_FW_GR;
        rc |= e->alloc(&f.arena, G * 2 * NR); rc |= e->alloc(&f.amove, G * 2 * NR);
        f.CS = (FWC_HEAD + FWR_FIELDS * (int)L + 31) / 32 * 32;
        rc |= e->alloc(&f.ctl, G * (size_t)f.CS);
        rc |= e->alloc(&f.played_now, G); rc |= e->alloc(&f.row_pos, G * L);
        rc |= e->alloc(&f.row_moves, G * L * BO_MAX_MOVES);
        rc |= e->alloc(&f.sim_path, G * L * BO_FW_PATH_CAP);
        rc |= e->alloc(&f.row_val, G * L);
        float *st = nullptr, *rt = nullptr;
        rc |= e->alloc(&st, (size_t)BO_FW_SQRT_TAB); rc |= e->alloc(&rt, (size_t)BO_FW_RCP_TAB);
        if (!rc) {
            // RN(sqrt(n)) and RN(1 / k): the double result rounded once more is the correctly rounded binary32 one (53 >= 2 * 24 + 2)
            std::vector<float> hs2(BO_FW_SQRT_TAB), hr2(BO_FW_RCP_TAB, 0.0f);
            for (int n = 0; n < BO_FW_SQRT_TAB; n++) hs2[n] = (float)sqrt((double)n);
            for (int k = 1; k < BO_FW_RCP_TAB; k++) hr2[k] = (float)(1.0 / (double)k);
            rt_h2d(st, hs2.data(), hs2.size() * sizeof(float), nullptr); rt_h2d(rt, hr2.data(), hr2.size() * sizeof(float), nullptr);
            rt_sync(nullptr);
            f.sqrt_tab = st; f.rcp_tab = rt;
            rt_memset(f.ctl, 0, G * (size_t)f.CS * 4, nullptr);
            rt_memset(f.played_now, 0, G * 4, nullptr);
            rt_memset(f.row_val, 0, G * L * 4, nullptr);
            d.played_now = f.played_now;
        }
    }
    if (rc) { bo_engine_destroy(e); return fail(BO_E_HIP, "device allocation failed"); }
    // host-built lookup tables: Python's math.sqrt / int() in double, rounded to binary32 once
    std::vector<float> hs((size_t)c.S + 2);
    for (int n = 0; n < c.S + 2; n++) hs[n] = (float)sqrt((double)n + 1e-8);  // mcts.py:93
    std::vector<int> hw((size_t)c.B + 1);
    for (int k = 0; k <= c.B; k++) hw[k] = (int)(cfg->widen_coeff * sqrt((double)k));  // mcts.py:55-57 with n_visits+1 == k
    std::vector<float> hr((size_t)c.S + 3, 0.0f);
    for (int n = 1; n < c.S + 3; n++) hr[n] = (float)(1.0 / (double)n);  // RN(1/n): rounding the double quotient again is innocuous (53 >= 2*24+2)
    rt_h2d(rcp, hr.data(), hr.size() * sizeof(float), nullptr);
    d.rcp_lut = rcp;
    rt_h2d(sq, hs.data(), hs.size() * sizeof(float), nullptr);
    rt_h2d(wl, hw.data(), hw.size() * sizeof(int), nullptr);
    d.sqrt_lut = sq; d.widen_lut = wl;
    for (int **p : iscal) rt_memset(*p, 0, G * sizeof(int), nullptr);
    rt_memset(d.noise, 0, G * BO_MAX_MOVES * sizeof(double), nullptr);
    rt_sync(nullptr);
    e->h_i32.resize(G);
    e->rng.resize(G);
    for (size_t g = 0; g < G; g++) hr_seed(&e->rng[g], (uint32_t)g);
    memset(e->h_noise, 0, G * BO_MAX_MOVES * sizeof(double));
    e->h_nl.resize(G); e->h_term.resize(G);
    *out = e;
    return BO_OK;
}

extern "C" void bo_engine_destroy(bo_engine *e) {
    if (!e) return;
    rt_set_device(e->device);
    for (void *p : e->allocs) rt_free(p);
    rt_host_free(e->h_res); rt_host_free(e->h_info); rt_host_free(e->h_noise); rt_host_free(e->h_go); rt_host_free(e->h_action);
    rt_host_free(e->h_turn_u); rt_host_free(e->h_turn_flags);
    if (e->ev_turn_made) rt_event_destroy(e->ev_turn);
    for (int i = 0; i < 2; i++) if (e->ev_action_made[i]) rt_event_destroy(e->ev_action[i]);
    if (e->setup_dev) rt_free(e->setup_dev);
    if (e->setup_host) rt_host_free(e->setup_host);
    if (e->ev_begin_made) rt_event_destroy(e->ev_begin);
#if !defined(BO_WAVE_EMU)
    if (e->sel_ev0) { (void)hipEventDestroy(e->sel_ev0); (void)hipEventDestroy(e->sel_ev1); }
#endif
    delete e;
}

// ---- set-up ---------------------------------------------------------------------------------------------
extern "C" int bo_games_reset_ex(bo_engine *e, int n, const int32_t *slots, const char *const *fens, const char *const *moves,
                                 const bo_position *hist, const int32_t *n_hist, const bo_position *trk,
                                 const int32_t *trk_counts, const int32_t *trk_off, void *stream) {
    if (!e || n < 1 || !slots) return fail(BO_E_ARG, "bad arguments");
    const EngCfg &c = e->d.c;
    std::vector<DPos> start((size_t)n);
    std::vector<std::vector<bo_mv>> mv((size_t)n);
    size_t max_moves = 1, max_trk = 1;
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= c.G) return fail(BO_E_ARG, "slot out of range");
        if (!parse_fen(fens && fens[i] ? fens[i] : START_FEN, &start[i])) return fail(BO_E_FEN, "bad FEN");
        if (!parse_uci_moves(moves ? moves[i] : nullptr, &mv[i])) return fail(BO_E_FEN, "bad UCI move list");
        if ((int)mv[i].size() + 2 > c.PLY_CAP) return fail(BO_E_ARG, "move list longer than max_plies");
        if (mv[i].size() > max_moves) max_moves = mv[i].size();
        if (trk_off && (size_t)(trk_off[i + 1] - trk_off[i]) > max_trk) max_trk = (size_t)(trk_off[i + 1] - trk_off[i]);
    }
    if (max_trk > (size_t)c.TRK_CAP) return fail(BO_E_ARG, "tracker larger than max_plies");
    std::vector<bo_mv> flat((size_t)n * max_moves, 0);
    std::vector<int> nm((size_t)n), nh((size_t)n, -1), nt((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        nm[i] = (int)mv[i].size();
        for (size_t k = 0; k < mv[i].size(); k++) flat[(size_t)i * max_moves + k] = mv[i][k];
    }
    std::vector<DPos> hh, tt;
    std::vector<int> tc;
    if (n_hist) {
        hh.resize((size_t)n * 7);
        tt.resize((size_t)n * max_trk);
        tc.resize((size_t)n * max_trk, 0);
        for (int i = 0; i < n; i++) {
            nh[i] = n_hist[i];
            if (nh[i] > 7) return fail(BO_E_ARG, "more than 7 history boards");
            for (int k = 0; k < nh[i]; k++) hh[(size_t)i * 7 + k] = from_abi(hist[(size_t)i * 7 + k]);
            nt[i] = trk_off ? trk_off[i + 1] - trk_off[i] : 0;
            for (int k = 0; k < nt[i]; k++) {
                tt[(size_t)i * max_trk + k] = from_abi(trk[trk_off[i] + k]);
                tc[(size_t)i * max_trk + k] = trk_counts[trk_off[i] + k];
            }
        }
    }
    // One packed upload through the engine's persistent staging buffers (grow-only device + pinned host memory): refilling
    // a finished game's slot happens about once per ply in steady-state self-play, and nine hipMalloc / hipFree pairs per
    // call cost more than the set-up kernel itself.
    std::vector<int> sl(slots, slots + n);
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
    const size_t o_slots = place(sl.size() * 4), o_start = place(start.size() * sizeof(DPos)), o_mv = place(flat.size() * sizeof(bo_mv)),
                 o_nm = place(nm.size() * 4);
    size_t o_nh = 0, o_hh = 0, o_tt = 0, o_tc = 0, o_nt = 0;
    if (n_hist) {
        o_nh = place(nh.size() * 4); o_hh = place(hh.size() * sizeof(DPos)); o_tt = place(tt.size() * sizeof(DPos));
        o_tc = place(tc.size() * 4); o_nt = place(nt.size() * 4);
    }
    int rc = 0;
    if (off > e->setup_cap) {
        if (e->setup_dev) rt_free(e->setup_dev);
        if (e->setup_host) rt_host_free(e->setup_host);
        e->setup_dev = nullptr; e->setup_host = nullptr;
        e->setup_cap = 2 * off + (256u << 10);  // roomy from the start: regrowing means hipFree, i.e. a device synchronisation
        rc = rt_malloc(&e->setup_dev, e->setup_cap) | rt_host_alloc(&e->setup_host, e->setup_cap);
        if (rc) e->setup_cap = 0;
    }
    SetupArgs a;
    memset(&a, 0, sizeof(a));
    if (!rc) {
        char *h = (char *)e->setup_host, *dv = (char *)e->setup_dev;
        memcpy(h + o_slots, sl.data(), sl.size() * 4); memcpy(h + o_start, start.data(), start.size() * sizeof(DPos));
        memcpy(h + o_mv, flat.data(), flat.size() * sizeof(bo_mv)); memcpy(h + o_nm, nm.data(), nm.size() * 4);
        a.slots = (const int *)(dv + o_slots); a.start = (const DPos *)(dv + o_start); a.moves = (const bo_mv *)(dv + o_mv);
        a.n_moves = (const int *)(dv + o_nm); a.max_moves = (int)max_moves; a.max_trk = (int)max_trk;
        if (n_hist) {
            memcpy(h + o_nh, nh.data(), nh.size() * 4); memcpy(h + o_hh, hh.data(), hh.size() * sizeof(DPos));
            memcpy(h + o_tt, tt.data(), tt.size() * sizeof(DPos)); memcpy(h + o_tc, tc.data(), tc.size() * 4);
            memcpy(h + o_nt, nt.data(), nt.size() * 4);
            a.n_hist = (const int *)(dv + o_nh); a.hist = (const DPos *)(dv + o_hh); a.trk = (const DPos *)(dv + o_tt);
            a.trk_cnt = (const int *)(dv + o_tc); a.n_trk = (const int *)(dv + o_nt);
        }
        rc = rt_h2d(dv, h, off, stream);
        if (!rc) rc = RT_LAUNCH(bo_k_setup, n, stream, e->d, a);
        if (!rc && e->fast) rc = RT_LAUNCH(bo_k_fw_reset, n, stream, e->d, e->f, a.slots);
    }
    int rc2 = rt_sync(stream);  // the staging buffers are free again when this returns
    if (rc || rc2) return fail(BO_E_HIP, std::string("bo_games_reset: ") + rt_errstr(rc ? rc : rc2));
    return BO_OK;
}

extern "C" int bo_games_reset(bo_engine *e, int n, const int32_t *slots, const char *const *fens, const char *const *moves,
                              void *stream) {
    return bo_games_reset_ex(e, n, slots, fens, moves, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int bo_root_info(bo_engine *e, int32_t *n_legal, int32_t *terminal, int32_t *ply, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    RT(rt_d2h(e->h_info + 2 * G, e->d_info_blk + 2 * G, 3 * G * 4, stream));  // [root_nlegal | root_term | ply] in one copy
    RT(rt_sync(stream));
    if (n_legal) memcpy(n_legal, e->h_info + 2 * G, G * 4);
    if (terminal) memcpy(terminal, e->h_info + 3 * G, G * 4);
    if (ply) memcpy(ply, e->h_info + 4 * G, G * 4);
    return BO_OK;
}

// ---- search --------------------------------------------------------------------------------------------
static int upload_noise(bo_engine *e, const unsigned char *rows_used, void *stream) {
    const size_t G = (size_t)e->d.c.G;
    size_t cols = 1;  // only the columns some root uses travel (apply_root reads noise[g][j < n_legal(g)])
    for (size_t g = 0; g < G; g++)
        if (rows_used[g] && (size_t)e->h_nl[g] > cols) cols = (size_t)e->h_nl[g];
    if (e->nl_valid && cols < BO_MAX_MOVES)
        RT(rt_h2d_2d(e->d.noise, BO_MAX_MOVES * sizeof(double), e->h_noise, BO_MAX_MOVES * sizeof(double), cols * sizeof(double), G, stream));
    else
        RT(rt_h2d(e->d.noise, e->h_noise, G * BO_MAX_MOVES * sizeof(double), stream));
    return BO_OK;
}

// noise_later: the caller uploads the noise before the first bo_step that applies a root evaluation (bo_selfplay_noise)
static int search_begin_impl(bo_engine *e, const int32_t *go, const double *noise, bool noise_later, float *nn_in_dev, void *stream) {
    if (!e || !go || !nn_in_dev) return fail(BO_E_ARG, "null argument");
    const size_t G = (size_t)e->d.c.G;
    if (e->d.c.use_noise && !noise && !noise_later) return fail(BO_E_ARG, "noise required when dirichlet_alpha > 0");
    if (go != e->h_go) memcpy(e->h_go, go, G * 4);  // pinned staging: one DMA, no pageable bounce buffer
    RT(rt_h2d(e->d_go, e->h_go, G * 4, stream));
    if (noise) {
        if (noise != e->h_noise) memcpy(e->h_noise, noise, G * BO_MAX_MOVES * sizeof(double));
        std::vector<unsigned char> used(G);
        for (size_t g = 0; g < G; g++) used[g] = e->h_go[g] != 0;
        int rc = upload_noise(e, used.data(), stream);
        if (rc) return rc;
    }
    e->nl_valid = false;
    if (e->fast) RT(RT_LAUNCH(bo_k_fw_search_begin, e->d.c.G, stream, e->d, e->f, (const int *)e->d_go, nn_in_dev));
    else RT(RT_LAUNCH(bo_k_search_begin, e->d.c.G, stream, e->d, (const int *)e->d_go, nn_in_dev));
    return BO_OK;
}

extern "C" int bo_search_begin(bo_engine *e, const int32_t *go, const double *noise, float *nn_in_dev, void *stream) {
    return search_begin_impl(e, go, noise, false, nn_in_dev, stream);
}

// bo_k_fw_select comes in one instantiation per (games per half-wave, leaves-per-step capacity, FW_SEL_* flags)
static int launch_fw_select(bo_engine *e, const float *value_dev, int kind, void *stream) {
    const FastW &f = e->f;
    const int G = e->d.c.G, L = f.L;
    if (L == 4 && (f.sel_flags & FW_SEL_LANE)) {  // one lane per game (bo_fastw.h)
        const int blocks = (G + 63) / 64;
        if (f.sel_flags & FW_SEL_NT) return RT_LAUNCH(bo_k_fw_select_lane_nt, blocks, stream, e->d, e->f, value_dev, kind);
        return RT_LAUNCH(bo_k_fw_select_lane, blocks, stream, e->d, e->f, value_dev, kind);
    }
    if (L <= 8 && (f.sel_flags & FW_SEL_QUAD)) {  // four lanes per game, sixteen games per wave
        const int blocks = (G + 15) / 16;
#define SELQ(K) return RT_LAUNCH(K, blocks, stream, e->d, e->f, value_dev, kind)
        if (L > 4) SELQ(bo_k_fw_select_q4l8_0);
        if (f.sel_flags & FW_SEL_DENSE) SELQ(bo_k_fw_select_q4l4_4);
        if (f.sel_flags & FW_SEL_ROOT_IN_REGS) SELQ(bo_k_fw_select_q4l4_2);
        SELQ(bo_k_fw_select_q4l4_0);
#undef SELQ
    }
    if (L <= 8 && (f.sel_flags & FW_SEL_OCT)) {  // eight lanes per game, eight games per wave
        const int blocks = (G + 7) / 8;
        const int fl = f.sel_flags & 3;
#define SELO(K) return RT_LAUNCH(K, blocks, stream, e->d, e->f, value_dev, kind)
        if (L > 4) { if (fl & 2) SELO(bo_k_fw_select_o8l8_2); SELO(bo_k_fw_select_o8l8_0); }
        if (fl == 3) SELO(bo_k_fw_select_o8l4_3);
        if (fl == 2) SELO(bo_k_fw_select_o8l4_2);
        if (fl == 1) SELO(bo_k_fw_select_o8l4_1);
        SELO(bo_k_fw_select_o8l4_0);
#undef SELO
    }
    const int ut = L > 16 ? 1 : (L > 8 && f.sel_ut > 2) ? 2 : L > 4 ? (L > 8 ? 2 : 4) : f.sel_ut;
    const int grid = (G + 2 * ut - 1) / (2 * ut);
#define SEL(K) return RT_LAUNCH(K, grid, stream, e->d, e->f, value_dev, kind)
    const bool fancy = (f.sel_flags & FW_SEL_ROOT_IN_REGS) != 0;  // (L > 4: plain, or non-temporal + root in registers)
    if (L > 16) { if (fancy) SEL(bo_k_fw_select_u1l64_3); SEL(bo_k_fw_select_u1l64_0); }
    if (L > 8) { if (fancy) SEL(bo_k_fw_select_u2l16_3); SEL(bo_k_fw_select_u2l16_0); }
    if (L > 4) { if (fancy) SEL(bo_k_fw_select_u4l8_3); SEL(bo_k_fw_select_u4l8_0); }
#define SEL8(UT)                                                                                  \
    switch (f.sel_flags & 7) {                                                                     \
        case 0: SEL(bo_k_fw_select_u##UT##l4_0); case 1: SEL(bo_k_fw_select_u##UT##l4_1);         \
        case 2: SEL(bo_k_fw_select_u##UT##l4_2); case 3: SEL(bo_k_fw_select_u##UT##l4_3);         \
        case 4: SEL(bo_k_fw_select_u##UT##l4_4); case 5: SEL(bo_k_fw_select_u##UT##l4_5);         \
        case 6: SEL(bo_k_fw_select_u##UT##l4_6); default: SEL(bo_k_fw_select_u##UT##l4_7);        \
    }
    if (ut >= 4) { SEL8(4) }
    SEL8(2)
#undef SEL8
#undef SEL
}

static int step_launch(bo_engine *e, const float *policy_dev, const float *value_dev, int policy_kind, float *nn_in_dev, void *stream, const StepTail &vt) {
    e->prefetch_valid = false;  // (a prefetched result block is older than this step; replays of a captured step are the caller's to track)
    if (e->fast) {  // apply (one wave per row) -> backup + select (half a wave per game) -> leaf positions and planes (one wave per row)
        const int rows = e->d.c.G * e->f.L;
        if (policy_kind != BO_POLICY_NONE) RT(RT_LAUNCH(bo_k_fw_apply, rows, stream, e->d, e->f, policy_dev, value_dev, policy_kind));
#if !defined(BO_WAVE_EMU)
        if (e->sel_profile) {  // eager launches only (events recorded during a graph capture would become graph nodes)
            if (!e->sel_ev0) { RT((int)hipEventCreate(&e->sel_ev0)); RT((int)hipEventCreate(&e->sel_ev1)); }
            if (e->sel_pending) {
                float ms = 0.0f;
                RT((int)hipEventSynchronize(e->sel_ev1));
                RT((int)hipEventElapsedTime(&ms, e->sel_ev0, e->sel_ev1));
                e->sel_ms += ms; e->sel_launches++; e->sel_pending = 0;
            }
            RT((int)hipEventRecord(e->sel_ev0, (hipStream_t)stream));
        }
#endif
        RT(launch_fw_select(e, policy_kind != BO_POLICY_NONE ? e->f.row_val : value_dev, policy_kind, stream));  // (values as bo_k_fw_apply left them: finite)
#if !defined(BO_WAVE_EMU)
        if (e->sel_profile) { RT((int)hipEventRecord(e->sel_ev1, (hipStream_t)stream)); e->sel_pending = 1; }
#endif
        RT(RT_LAUNCH(bo_k_fw_leaf, rows, stream, e->d, e->f, nn_in_dev));
    } else {
        // (the probing instantiation only where the search probes: without it the default kernel runs, the one there was before the tables)
        if (e->d.tb_n > 0 && (e->d.tb_flags & TBF_SEARCH)) RT(RT_LAUNCH(bo_k_step_tb, e->d.c.G, stream, e->d, policy_dev, value_dev, policy_kind, nn_in_dev, vt));
        else RT(RT_LAUNCH(bo_k_step, e->d.c.G, stream, e->d, policy_dev, value_dev, policy_kind, nn_in_dev, vt));
    }
    return BO_OK;
}
extern "C" int bo_step(bo_engine *e, const float *policy_dev, const float *value_dev, int policy_kind, float *nn_in_dev,
                       void *stream) {
    if (!e || !nn_in_dev) return fail(BO_E_ARG, "null argument");
    if (policy_kind != BO_POLICY_NONE && (!policy_dev || !value_dev)) return fail(BO_E_ARG, "policy/value required");
    return step_launch(e, policy_dev, value_dev, policy_kind, nn_in_dev, stream, StepTail{nullptr, nullptr, nullptr, nullptr, 0});
}
extern "C" int bo_step_heads(bo_engine *e, const float *logits_dev, const float *vpart_dev, const float *b1_dev, const float *w2_dev,
                             const float *b2_dev, int rows, float *nn_in_dev, void *stream) {
    if (!e || !nn_in_dev || !logits_dev || !vpart_dev || !b1_dev || !w2_dev || !b2_dev) return fail(BO_E_ARG, "null argument");
    if (e->fast) return fail(BO_E_CONFIG, "bo_step_heads: the reference-semantics search only (fast mode evaluates rows, not games)");
    if (rows < e->d.c.G) return fail(BO_E_ARG, "bo_step_heads: the partial sums must hold a row per game (rows >= G)");
    return step_launch(e, logits_dev, nullptr, BO_POLICY_LOGITS, nn_in_dev, stream, StepTail{vpart_dev, b1_dev, w2_dev, b2_dev, rows});
}

extern "C" int bo_search_poll(bo_engine *e, int32_t *n_running, int32_t *n_requested, int32_t *requested_mask, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    RT(rt_d2h(e->h_info, e->d_info_blk, 2 * G * 4, stream));  // [phase | req_node] in one copy
    const int *ph = e->h_info, *rq = e->h_info + G;
    RT(rt_sync(stream));
    int run = 0, req = 0;
    for (size_t g = 0; g < G; g++) {
        bool r = ph[g] == PH_RUN;
        bool q = r && rq[g] >= 0;
        run += r; req += q;
        if (requested_mask) requested_mask[g] = q ? 1 : 0;
    }
    if (n_running) *n_running = run;
    if (n_requested) *n_requested = req;
    return BO_OK;
}

extern "C" int bo_search_stop(bo_engine *e, const int32_t *stop_mask, int32_t *sims_done, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    const int *d_mask = nullptr;
    if (stop_mask) {
        memcpy(e->h_go, stop_mask, G * 4);
        RT(rt_h2d(e->d_go, e->h_go, G * 4, stream));
        d_mask = e->d_go;
    }
    if (e->fast) {  // the step in flight is dropped (bo_info.h): nothing of it is in the tree
        e->prefetch_valid = false;
        RT(RT_LAUNCH(bo_k_fw_stop, e->d.c.G, stream, e->d, e->f, d_mask));
    } else {
        RT(RT_LAUNCH(bo_k_stop, e->d.c.G, stream, e->d, d_mask));
    }
    if (sims_done) RT(rt_d2h(sims_done, e->d.sims_done, G * 4, stream));
    RT(rt_sync(stream));
    return BO_OK;
}

// One bo_search_info record per slot into out[G] (device memory, or pinned host memory mapped into the device).  Read-only, asynchronous.
extern "C" int bo_search_info(bo_engine *e, int32_t n_lines, bo_search_info_rec *out, void *stream) {
    if (!e || !out) return fail(BO_E_ARG, "bo_search_info: null argument");
    if (!e->fast) return fail(BO_E_CONFIG, "bo_search_info: fast-mode engines only (reference semantics: bo_analysis_result)");
    if (n_lines < 0) return fail(BO_E_ARG, "bo_search_info: n_lines < 0");
    static_assert(sizeof(bo_search_info_rec) == BO_INFO_WORDS * 4, "bo_search_info_rec is the record bo_k_fw_info writes");
    RT(RT_LAUNCH(bo_k_fw_info, e->d.c.G, stream, e->d, e->f, (int)n_lines, (int *)out));
    return BO_OK;
}

extern "C" int bo_search_close(bo_engine *e, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (e->fast) return fail(BO_E_CONFIG, "bo_search_close: reference-semantics engines only");
    if (e->d.c.root_q) return fail(BO_E_STATE, "bo_search_close: root values are on (a closed search's q values lack the last evaluation)");
    e->prefetch_valid = false;  // (as a step: a prefetched result block is older than the closed searches)
    RT(RT_LAUNCH(bo_k_search_close, e->d.c.G, stream, e->d));
    return BO_OK;
}

// the result kernel and the copy of its block, enqueued (no wait)
static int ship(bo_engine *e, int *dst_a, const int *src_a, size_t n_a, int *dst_b, const int *src_b, size_t n_b, void *stream) {
    const size_t n = n_a > n_b ? n_a : n_b;
    const int blocks = (int)((n + 511) / 512 < 1 ? 1 : ((n + 511) / 512 > 128 ? 128 : (n + 511) / 512));  // ~8 words per lane, at most 128 waves
    RT(RT_LAUNCH(bo_k_ship, blocks, stream, dst_a, src_a, (int)n_a, dst_b, src_b, (int)n_b, blocks));
    (void)e;
    return BO_OK;
}

// with_info: [phase | req_node] of every slot comes along (bo_selfplay_turn's "are all searches finished?")
static int result_enqueue(bo_engine *e, void *stream, bool with_info = false) {
    const size_t G = (size_t)e->d.c.G, res_words = G * (4 + 2 * (size_t)BO_RES_CAP) + 4;  // the whole result block (+ the watched word)
    if (with_info && !e->ship) RT(rt_d2h(e->h_info, e->d_info_blk, 2 * G * 4, stream));
    if (e->fast) RT(RT_LAUNCH(bo_k_fw_result, e->d.c.G, stream, e->d, e->f));
    else RT(RT_LAUNCH(bo_k_result, e->d.c.G, stream, e->d));
    if (e->ship) return ship(e, e->h_res, (const int *)e->d_res_blk, res_words, e->h_info, (const int *)e->d_info_blk, with_info ? 2 * G : 0, stream);
    RT(rt_d2h(e->h_res, e->d_res_blk, res_words * 4, stream));
    return BO_OK;
}

static int result_unpack(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *best_move,
                         int32_t *total_visits) {
    const size_t G = (size_t)e->d.c.G;
    const int *h = e->h_res;
    if (res_n) memcpy(res_n, h, G * 4);
    if (best_idx) memcpy(best_idx, h + G, G * 4);
    if (best_move) memcpy(best_move, h + 2 * G, G * 4);
    if (total_visits) memcpy(total_visits, h + 3 * G, G * 4);
    if (res_idx) memcpy(res_idx, h + 4 * G, G * BO_RES_CAP * 4);
    if (res_val) memcpy(res_val, h + 4 * G + G * BO_RES_CAP, G * BO_RES_CAP * 4);
    e->watch_seen |= h[G * (4 + 2 * (size_t)BO_RES_CAP)];
    return BO_OK;
}

// A device status word of the evaluate stage (the split-precision tower's "an activation left the fp16 range", bo_nn_tower_word)
// rides along with every fetched result block: the ply's one host round trip checks it, no copy or wait of its own.
extern "C" int bo_engine_watch(bo_engine *e, int32_t *dev_word) { return bo_engine_watch_words(e, dev_word, 1); }
// n_words = 2: the two words of bo_nn_b1_word ([timeout code | saturation flag]); the copy is word 0 | (word 1 != 0) << 16
extern "C" int bo_engine_watch_words(bo_engine *e, int32_t *dev_words, int32_t n_words) {
    if (!e || n_words < 1 || n_words > 2) return fail(BO_E_ARG, "bad arguments");
    e->d.watch = dev_words;
    e->d.watch_n = n_words;
    return BO_OK;
}
// OR of the watched word over every result block fetched since the last call with clear != 0 (host state; nothing is enqueued)
extern "C" int bo_engine_watch_seen(bo_engine *e, int32_t *seen_out, int32_t clear) {
    if (!e || !seen_out) return fail(BO_E_ARG, "bad arguments");
    *seen_out = e->watch_seen;
    if (clear) e->watch_seen = 0;
    return BO_OK;
}

// The result block and the searches' state enqueued BEHIND the searches' last expected step, without waiting: when the caller later
// finds the stream idle, bo_selfplay_turn(flags 2 | 8) reads both from pinned memory and needs no round trip of its own (if a search
// turns out to need one more evaluation, the caller steps and prefetches again).  Any bo_step after it invalidates it.
extern "C" int bo_search_result_prefetch(bo_engine *e, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    int rc = result_enqueue(e, stream, true);
    if (rc) return rc;
    e->prefetch_valid = true;
    return BO_OK;
}

extern "C" int bo_search_result(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx,
                                int32_t *best_move, int32_t *total_visits, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    int rc = result_enqueue(e, stream);
    if (rc) return rc;
    RT(rt_sync(stream));
    return result_unpack(e, res_n, res_idx, res_val, best_idx, best_move, total_visits);
}

extern "C" int bo_play(bo_engine *e, const int32_t *action, void *stream) {
    if (!e || !action) return fail(BO_E_ARG, "null argument");
    if (e->ship) {  // the kernel reads the actions from pinned host memory itself (two buffers: the previous call's kernel may not have run yet)
        const int half = (e->action_flip ^= 1);
        int *slot = e->h_action + (size_t)half * e->d.c.G;
        if (e->ev_action_made[half]) RT(rt_event_sync(e->ev_action[half]));  // (the kernel that read this half two calls ago has run: normally long since)
        memcpy(slot, action, (size_t)e->d.c.G * 4);
        RT(RT_LAUNCH(bo_k_play, e->d.c.G, stream, e->d, (const int *)slot));
        if (!e->ev_action_made[half]) { RT(rt_event_create(&e->ev_action[half])); e->ev_action_made[half] = true; }
        RT(rt_event_record(e->ev_action[half], stream));
    } else {
        RT(rt_h2d(e->d_action, action, (size_t)e->d.c.G * 4, stream));
        RT(RT_LAUNCH(bo_k_play, e->d.c.G, stream, e->d, (const int *)e->d_action));
    }
    if (e->fast) RT(RT_LAUNCH(bo_k_fw_reroot, e->d.c.G, stream, e->d, e->f, e->fast_reuse));  // tree reuse: the played child becomes the root
    return BO_OK;
}

// ---- native per-move host work (bit-compatible with numpy.random.RandomState; bo_hostrng.h) ----------------------
// The per-game streams are independent, so the G Dirichlet draws / temperature samples of a ply are spread over a few
// persistent worker threads (the GPU idles during this phase: 160 us single-threaded for 256 roots).
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>
namespace {
struct BoPool {
    std::vector<std::thread> workers;
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    const std::function<void(int)> *job = nullptr;
    int n_items = 0, chunk = 1, generation = 0, pending = 0;
    std::atomic<int> next{0};
    bool stop = false;
    pid_t owner = getpid();
    explicit BoPool(int n) {
        for (int i = 0; i < n; i++) workers.emplace_back([this] { loop(); });
    }
    ~BoPool() {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv_go.notify_all();
        for (auto &t : workers) t.join();
    }
    void drain() {
        for (;;) {
            const int b = next.fetch_add(chunk);
            if (b >= n_items) return;
            const int e = b + chunk < n_items ? b + chunk : n_items;
            for (int i = b; i < e; i++) (*job)(i);
        }
    }
    void loop() {
        int seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m);
                cv_go.wait(l, [&] { return stop || generation != seen; });
                if (stop) return;
                seen = generation;
            }
            drain();
            { std::lock_guard<std::mutex> l(m); pending--; }
            cv_done.notify_one();
        }
    }
    // light: microseconds of work in total (sampling one of <= 2 moves per game, flag bookkeeping) -- inline: waking the workers
    // and waiting for every one of them to report back costs a futex round trip (~30-50 us) the device idles through
    void run(int n, const std::function<void(int)> &f, bool light = false) {
        // (a fork()ed child inherits the object but not the threads: it works inline)
        // (fewer than 256 items -- a cohort's 64 roots take ~40 us inline -- are not worth waking the workers for: their wake-up is ~50 us
        //  at best and milliseconds when a worker's core sleeps deeply or is busy: p99 2.9 ms of bo_selfplay_noise, profiles/r05_logs/s16_plyprof.log)
        if (workers.empty() || n < 256 || (light && n <= 2048) || getpid() != owner) { for (int i = 0; i < n; i++) f(i); return; }
        {
            std::lock_guard<std::mutex> l(m);
            job = &f; n_items = n; chunk = 8; next = 0; pending = (int)workers.size(); generation++;
        }
        cv_go.notify_all();
        drain();  // the calling thread works too
        std::unique_lock<std::mutex> l(m);
        cv_done.wait(l, [&] { return pending == 0; });
    }
};
BoPool &host_pool() {
    // never destroyed: the workers end with the process (a destructor would have to join threads that a fork()ed child
    // does not have, or run during interpreter shutdown)
    static BoPool *pool = new BoPool([] {
        const char *v = getenv("BO_HOST_THREADS");
        int n = v ? atoi(v) : 4;
        const int hw = (int)std::thread::hardware_concurrency();
        if (hw > 0 && n > hw / 2) n = hw / 2;  // leave room for the other ranks of a node
        return n < 1 ? 0 : n - 1;
    }());
    return *pool;
}
}  // namespace

extern "C" int bo_rng_seed(bo_engine *e, int slot, uint32_t seed) {
    if (!e || slot < 0 || slot >= e->d.c.G) return fail(BO_E_ARG, "bad slot");
    hr_seed(&e->rng[slot], seed);
    if ((int)e->noise_pending.size() == e->d.c.G) e->noise_pending[slot] = 0;  // a new game: the old root's deferred draw is void
    return BO_OK;
}

extern "C" int bo_rng_state(bo_engine *e, int slot, int set, uint32_t *key624, int32_t *pos, int32_t *has_gauss, double *gauss) {
    if (!e || slot < 0 || slot >= e->d.c.G || !key624 || !pos || !has_gauss || !gauss) return fail(BO_E_ARG, "bad arguments");
    HostRng &r = e->rng[slot];
    if (set) {
        memcpy(r.key, key624, sizeof(r.key));
        r.pos = *pos; r.has_gauss = *has_gauss; r.gauss = *gauss;
    } else {
        memcpy(key624, r.key, sizeof(r.key));
        *pos = r.pos; *has_gauss = r.has_gauss; *gauss = r.gauss;
    }
    return BO_OK;
}

// fetched: the result block is already in e->h_res (bo_selfplay_turn asked for it together with the searches' state)
static int selfplay_sample_impl(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold, double t_initial,
                                double t_final, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx,
                                int32_t *action_out, bool fetched, void *stream) {
    if (!e || !active || !move_number || !res_n || !res_idx || !res_val || !action_out) return fail(BO_E_ARG, "null argument");
    int rc = fetched ? result_unpack(e, res_n, res_idx, res_val, best_idx, nullptr, nullptr)
                     : bo_search_result(e, res_n, res_idx, res_val, best_idx, nullptr, nullptr, stream);
    if (rc) return rc;
    const int G = e->d.c.G;
    host_pool().run(G, [&](int g) {
        if (!active[g]) { action_out[g] = -1; return; }
        const int32_t *ri = res_idx + (size_t)g * BO_RES_CAP;
        const float *rv = res_val + (size_t)g * BO_RES_CAP;
        const int a = e->fast ? hr_select_action_general(&e->rng[g], res_n[g], ri, rv, move_number[g], threshold, t_initial, t_final)
                              : hr_select_action(&e->rng[g], res_n[g], ri, rv, move_number[g], threshold, t_initial, t_final);
        action_out[g] = a >= 0 ? a : -3;  // -3: not sparse enough, the caller samples with the dense NumPy mirror
    }, !e->fast);  // reference semantics: pi has <= 2 entries, a few dozen nanoseconds per game
    return BO_OK;
}

extern "C" int bo_selfplay_sample(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold,
                                  double t_initial, double t_final, int32_t *res_n, int32_t *res_idx, float *res_val,
                                  int32_t *best_idx, int32_t *action_out, void *stream) {
    return selfplay_sample_impl(e, active, move_number, threshold, t_initial, t_final, res_n, res_idx, res_val, best_idx, action_out, false, stream);
}

static int selfplay_begin_impl(bo_engine *e, const int32_t *want, float *nn_in_dev, int32_t *n_legal_out, int32_t *terminal_out,
                               int32_t *go_out, bool defer_noise, void *stream) {
    if (!e || !want || !nn_in_dev) return fail(BO_E_ARG, "null argument");
    const int G = e->d.c.G;
    int rc = bo_root_info(e, e->h_nl.data(), e->h_term.data(), nullptr, stream);
    if (rc) return rc;
    const double alpha = e->cfg.dirichlet_alpha;
    if ((int)e->noise_pending.size() != G) e->noise_pending.assign(G, 0);
    host_pool().run(G, [&](int g) {
        const int go = want[g] && e->h_term[g] == 0;
        e->h_go[g] = go;
        if (want[g]) e->noise_pending[g] = 0;
        if (go && alpha > 0) {
            if (defer_noise) e->noise_pending[g] = 1;
            else hr_dirichlet(&e->rng[g], alpha, e->h_nl[g], &e->h_noise[(size_t)g * BO_MAX_MOVES]);  // mcts.py:192
        }
        if (n_legal_out) n_legal_out[g] = e->h_nl[g];
        if (terminal_out) terminal_out[g] = e->h_term[g];
        if (go_out) go_out[g] = go;
    }, defer_noise || alpha <= 0);  // (without the Dirichlet draws this is flag bookkeeping)
    e->nl_valid = true;
    rc = search_begin_impl(e, e->h_go, (alpha > 0 && !defer_noise) ? e->h_noise : nullptr, defer_noise, nn_in_dev, stream);
    if (rc) return rc;
    return bo_step(e, nullptr, nullptr, BO_POLICY_NONE, nn_in_dev, stream);
}

extern "C" int bo_selfplay_begin(bo_engine *e, const int32_t *want, float *nn_in_dev, int32_t *n_legal_out, int32_t *terminal_out,
                                 int32_t *go_out, void *stream) {
    if (e && e->begin_lazy) return fail(BO_E_STATE, "bo_selfplay_begun has not collected the previous turn's roots yet");
    return selfplay_begin_impl(e, want, nn_in_dev, n_legal_out, terminal_out, go_out, false, stream);
}

// The begin of bo_selfplay_turn(flag 4): nothing here waits for the device.  go is decided by the kernel (wanted and not
// terminal); the roots' state travels behind it and is collected by bo_selfplay_begun once the caller has enqueued the first
// evaluation -- the device goes from the played moves straight into that evaluation instead of idling through a host round trip.
static int selfplay_begin_lazy(bo_engine *e, const int32_t *want, float *nn_in_dev, void *stream) {
    if (e->fast) return fail(BO_E_CONFIG, "bo_selfplay_turn: flag 4 needs a reference-semantics engine");
    const size_t G = (size_t)e->d.c.G;
    e->lazy_want.assign(want, want + G);
    memcpy(e->h_go, want, G * 4);
    if (e->ship) { int rcs = ship(e, e->d_go, e->h_go, G, nullptr, nullptr, 0, stream); if (rcs) return rcs; }  // (h_go is next written by bo_selfplay_begun, behind ev_begin)
    else RT(rt_h2d(e->d_go, e->h_go, G * 4, stream));
    e->nl_valid = false;
    RT(RT_LAUNCH(bo_k_search_begin_want, e->d.c.G, stream, e->d, (const int *)e->d_go, nn_in_dev));
    int rc = bo_step(e, nullptr, nullptr, BO_POLICY_NONE, nn_in_dev, stream);
    if (rc) return rc;
    if (e->ship) { rc = ship(e, e->h_info + 2 * G, (const int *)e->d_info_blk + 2 * G, 3 * G, nullptr, nullptr, 0, stream); if (rc) return rc; }
    else RT(rt_d2h(e->h_info + 2 * G, e->d_info_blk + 2 * G, 3 * G * 4, stream));  // [root_nlegal | root_term | ply]
    if (!e->ev_begin_made) { RT(rt_event_create(&e->ev_begin)); e->ev_begin_made = true; }
    RT(rt_event_record(e->ev_begin, stream));
    e->begin_lazy = true;
    return BO_OK;
}

// Collect what bo_selfplay_turn(flag 4) left on its way: the new roots' legal-move counts, terminal codes and go flags (as
// bo_selfplay_begin reports them), and which roots still need their Dirichlet draw (bo_selfplay_noise).  Waits for the copy
// behind the begin kernels only, not for work enqueued after the turn.
extern "C" int bo_selfplay_begun(bo_engine *e, int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (!e->begin_lazy) return fail(BO_E_STATE, "no bo_selfplay_turn(flag 4) outstanding");
    RT(rt_event_sync(e->ev_begin));
    const int G = e->d.c.G;
    const double alpha = e->cfg.dirichlet_alpha;
    if ((int)e->noise_pending.size() != G) e->noise_pending.assign(G, 0);
    for (int g = 0; g < G; g++) {
        e->h_nl[g] = e->h_info[2 * G + g];
        e->h_term[g] = e->h_info[3 * G + g];
        const int go = e->lazy_want[g] && e->h_term[g] == 0;
        e->h_go[g] = go;
        if (e->lazy_want[g]) e->noise_pending[g] = 0;
        if (go && alpha > 0) e->noise_pending[g] = 1;
        if (n_legal_out) n_legal_out[g] = e->h_nl[g];
        if (terminal_out) terminal_out[g] = e->h_term[g];
        if (go_out) go_out[g] = go;
    }
    e->nl_valid = true;
    e->begin_lazy = false;
    return BO_OK;
}

// The Dirichlet draws bo_selfplay_turn(defer_noise = 1) left out, and their upload: call it after the root evaluation's
// network forward has been enqueued (the host work then overlaps it) and before the bo_step that consumes that evaluation.
extern "C" int bo_selfplay_noise(bo_engine *e, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (e->begin_lazy) return fail(BO_E_STATE, "bo_selfplay_noise: call bo_selfplay_begun first");
    const int G = e->d.c.G;
    const double alpha = e->cfg.dirichlet_alpha;
    if ((int)e->noise_pending.size() != G || alpha <= 0) return BO_OK;
    bool any = false;
    for (int g = 0; g < G; g++) any = any || e->noise_pending[g];
    if (!any) return BO_OK;
    host_pool().run(G, [&](int g) {
        if (e->noise_pending[g]) hr_dirichlet(&e->rng[g], alpha, e->h_nl[g], &e->h_noise[(size_t)g * BO_MAX_MOVES]);
    });
    e->nl_valid = true;
    int rc = upload_noise(e, e->noise_pending.data(), stream);
    e->nl_valid = false;
    std::fill(e->noise_pending.begin(), e->noise_pending.end(), 0);
    return rc;
}

// One host round trip per ply: sample the moves of the finished searches, play them, and begin the next searches
// (self_play.py:121-184 followed by the next iteration's mcts.py:185-203).  Per game the RNG stream order is unchanged:
// the temperature sample, then the Dirichlet draw of the new root.
extern "C" int bo_selfplay_turn(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold, double t_initial,
                                double t_final, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *action_out,
                                const int32_t *want_next, float *nn_in_dev, int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out,
                                int32_t defer_noise, int32_t *completed, void *stream) {
    if (!e || !want_next || !nn_in_dev || !completed) return fail(BO_E_ARG, "null argument");
    *completed = 0;
    const bool poll_first = (defer_noise & 2) != 0, lazy_begin = (defer_noise & 4) != 0, prefetched = (defer_noise & 8) != 0;
    defer_noise &= 1;
    if (prefetched && !poll_first) return fail(BO_E_ARG, "bo_selfplay_turn: flag 8 (result block prefetched) goes with flag 2");
    if (lazy_begin && !defer_noise) return fail(BO_E_ARG, "bo_selfplay_turn: flag 4 (begin without waiting) needs flag 1 (noise later)");
    if (e->begin_lazy) return fail(BO_E_STATE, "bo_selfplay_begun has not collected the previous turn's roots yet");
    if (e->turn_outstanding) return fail(BO_E_STATE, "bo_selfplay_autoturn_collect has not collected the device's turn yet");
    int rc;
    if (poll_first) {
        // "are all searches finished?" and their results in ONE round trip: the result kernel runs behind the last expected
        // step without waiting for the answer (it only reads the trees; if a search needs one more evaluation -- rare -- its
        // block is fetched again by the next call)
        const size_t G = (size_t)e->d.c.G;
        if (!(prefetched && e->prefetch_valid)) {
            rc = result_enqueue(e, stream, true);  // (+ [phase | req_node])
            if (rc) return rc;
        }
        e->prefetch_valid = false;
        RT(rt_sync(stream));
        for (size_t g = 0; g < G; g++)
            if (e->h_info[g] == PH_RUN) { *completed = -1; return BO_OK; }
    }
    rc = selfplay_sample_impl(e, active, move_number, threshold, t_initial, t_final, res_n, res_idx, res_val, best_idx, action_out, poll_first, stream);
    if (rc) return rc;
    for (int g = 0; g < e->d.c.G; g++)
        if (action_out[g] == -3) return BO_OK;  // a pi too dense for the native sampler: the caller samples it, then plays and begins
    rc = bo_play(e, action_out, stream);
    if (rc) return rc;
    rc = lazy_begin ? selfplay_begin_lazy(e, want_next, nn_in_dev, stream)
                    : selfplay_begin_impl(e, want_next, nn_in_dev, n_legal_out, terminal_out, go_out, defer_noise != 0, stream);
    if (rc) return rc;
    *completed = lazy_begin ? 2 : 1;
    return BO_OK;
}

// ---- the turn on the device (ABI 5) ------------------------------------------------------------------------------------------
// bo_selfplay_turn's work without the host in the device's way: the random draw of every move is made AHEAD (per game the stream order
// stays Dirichlet of this search -> choice of this move -> Dirichlet of the next search), the kernels bo_k_turn_sample / bo_k_turn_play are
// enqueued behind the searches' last expected step, and their outputs travel to pinned memory behind them.  Nothing here waits.
extern "C" int bo_selfplay_autoturn(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold, double t_initial,
                                    double t_final, const int32_t *want_next, float *nn_in_dev, int32_t redo, void *stream) {
    if (!e || !active || !move_number || !want_next || !nn_in_dev) return fail(BO_E_ARG, "null argument");
    if (e->fast || e->d.c.root_m != 1 || e->d.c.S < 1)
        return fail(BO_E_CONFIG, "bo_selfplay_autoturn: reference-semantics engines whose root keeps <= 2 children (int(WIDEN_COEFF) == 1, NUM_SIMULATIONS >= 1)");
    if (!(fabs(t_initial - 1.0) < 1e-6) || t_final == 0.0 || !(t_final > 0.0))
        return fail(BO_E_CONFIG, "bo_selfplay_autoturn: TEMPERATURE_INITIAL must be 1 and TEMPERATURE_FINAL > 0 (other settings: bo_selfplay_turn)");
    if (!e->ship) return fail(BO_E_CONFIG, "bo_selfplay_autoturn is not available with BETAONE_TURN_COPIES=1");
    if (e->begin_lazy) return fail(BO_E_STATE, "bo_selfplay_begun has not collected the previous turn's roots yet");
    if (e->turn_outstanding) return fail(BO_E_STATE, "bo_selfplay_autoturn: the previous turn has not been collected");
    const int G = e->d.c.G, S = e->d.c.S;
    if (e->turn_pw_tfinal != t_final) {  // apply_temperature's np.power (self_play.py:37) for every possible pi entry f32(c / S): the host's libm, once
        e->turn_pw_host.resize((size_t)S + 1);
        for (int c = 0; c <= S; c++) {
            const float p = (float)((double)c / (double)S);  // mcts.py:273
            double x = pow((double)p, 1.0 / t_final);
            if (!isfinite(x)) x = 0.0;
            e->turn_pw_host[c] = x;
        }
        RT(rt_h2d(e->d_turn_pw, e->turn_pw_host.data(), ((size_t)S + 1) * sizeof(double), stream));
        RT(rt_sync(stream));  // (once per temperature: the staging vector may be rebuilt by the next change)
        e->turn_pw_tfinal = t_final;
    }
    if (!redo) {
        for (int g = 0; g < G; g++) {
            const double temp = move_number[g] < threshold ? t_initial : t_final;
            int fl = (active[g] ? 1 : 0) | (want_next[g] ? 4 : 0);
            if (active[g] && !(fabs(temp - 1.0) < 1e-6)) fl |= 2;
            if (active[g] && (int)e->resign_en.size() == G && e->resign_en[g]) fl |= 8;
            e->h_turn_flags[g] = fl;
            if (active[g]) e->h_turn_u[g] = hr_double(&e->rng[g]);  // RandomState.choice's random_sample() (self_play.py:73)
        }
        e->turn_want.assign(want_next, want_next + G);
    }
    TurnArgs a;
    a.u = e->h_turn_u; a.flags = e->h_turn_flags; a.pw = e->d_turn_pw;
    a.action = e->d_turn_action; a.state = e->d_turn_state; a.cres = e->d_turn_cres;
    a.root_value = e->d_turn_rv; a.resigned = e->d_turn_resigned; a.resign_next = e->d_turn_rnext;
    a.resign_t = e->resign_t; a.resign_k = e->resign_k;
    e->prefetch_valid = false;
    e->nl_valid = false;
    RT(RT_LAUNCH(bo_k_turn_sample, G, stream, e->d, a));
    RT(RT_LAUNCH(bo_k_turn_play, G, stream, e->d, a, nn_in_dev));
    const size_t Gs = (size_t)G, watch_off = Gs * (4 + 2 * (size_t)BO_RES_CAP);
    int rc = ship(e, e->h_info + 2 * Gs, (const int *)e->d_info_blk + 2 * Gs, 15 * Gs, e->h_res + watch_off, (const int *)e->d_res_blk + watch_off, 4, stream);
    if (rc) return rc;
    if (!e->ev_turn_made) { RT(rt_event_create(&e->ev_turn)); e->ev_turn_made = true; }
    RT(rt_event_record(e->ev_turn, stream));
    rc = bo_step(e, nullptr, nullptr, BO_POLICY_NONE, nn_in_dev, stream);  // the begun searches' first step (a no-op for every game if the turn did not happen)
    if (rc) return rc;
    e->turn_outstanding = true;
    return BO_OK;
}

// 1: the event behind the turn's outputs has been reached (bo_selfplay_autoturn_collect will not wait), 0: not yet
extern "C" int bo_selfplay_autoturn_ready(bo_engine *e, int32_t *ready_out) {
    if (!e || !ready_out) return fail(BO_E_ARG, "null argument");
    if (!e->turn_outstanding) return fail(BO_E_STATE, "no bo_selfplay_autoturn outstanding");
#if defined(BO_WAVE_EMU)
    *ready_out = 1;
#else
    const hipError_t q = hipEventQuery(e->ev_turn);
    if (q != hipSuccess && q != hipErrorNotReady) return fail(BO_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
    *ready_out = q == hipSuccess ? 1 : 0;
#endif
    return BO_OK;
}

extern "C" int bo_selfplay_autoturn_collect_ex(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx,
                                               int32_t *action_out, int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out,
                                               float *root_value_out, int32_t *resigned_out, int32_t *completed) {
    if (!e || !res_n || !res_idx || !res_val || !action_out || !completed) return fail(BO_E_ARG, "null argument");
    if (!e->turn_outstanding) return fail(BO_E_STATE, "no bo_selfplay_autoturn outstanding");
    RT(rt_event_sync(e->ev_turn));
    e->turn_outstanding = false;
    *completed = 0;
    const int G = e->d.c.G;
    const size_t Gs = (size_t)G;
    const int *act = e->h_info + 5 * Gs, *st = e->h_info + 6 * Gs, *cres = e->h_info + 7 * Gs, *rsg = e->h_info + 16 * Gs;
    e->watch_seen |= e->h_res[Gs * (4 + 2 * (size_t)BO_RES_CAP)];
    bool running = false;
    for (int g = 0; g < G; g++) {
        if (st[g] == 2) return fail(BO_E_STATE, "bo_selfplay_autoturn: a search result the device sampler does not cover (slot " + std::to_string(g) + ")");
        running = running || st[g] == 1 || st[g] == 3;  // (3: the watched fault word was set -- bo_engine_watch_seen says so; nothing was played)
    }
    if (running) { *completed = -1; return BO_OK; }  // nothing was played: bo_step once more, then bo_selfplay_autoturn(redo = 1)
    const double alpha = e->cfg.dirichlet_alpha;
    if ((int)e->noise_pending.size() != G) e->noise_pending.assign(G, 0);
    for (int g = 0; g < G; g++) {
        const int *c = cres + (size_t)g * 8;
        action_out[g] = act[g];
        if (e->h_turn_flags[g] & 1) {
            res_n[g] = c[0];
            if (best_idx) best_idx[g] = c[1];
            res_idx[(size_t)g * BO_RES_CAP] = c[4]; res_idx[(size_t)g * BO_RES_CAP + 1] = c[5];
            memcpy(&res_val[(size_t)g * BO_RES_CAP], &c[6], 4); memcpy(&res_val[(size_t)g * BO_RES_CAP + 1], &c[7], 4);
        } else res_n[g] = 0;
        e->h_nl[g] = e->h_info[2 * Gs + g];
        e->h_term[g] = e->h_info[3 * Gs + g];
        const int go = e->turn_want[g] && e->h_term[g] == 0 && !rsg[g];  // (a game that resigned begins no search)
        e->h_go[g] = go;
        if (e->turn_want[g]) e->noise_pending[g] = 0;
        if (go && alpha > 0) e->noise_pending[g] = 1;
        if (n_legal_out) n_legal_out[g] = e->h_nl[g];
        if (terminal_out) terminal_out[g] = e->h_term[g];
        if (go_out) go_out[g] = go;
        if (root_value_out) memcpy(&root_value_out[g], &e->h_info[15 * Gs + g], 4);
        if (resigned_out) resigned_out[g] = rsg[g];
    }
    e->nl_valid = true;
    *completed = 1;
    return BO_OK;
}

extern "C" int bo_selfplay_autoturn_collect(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *action_out,
                                            int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out, int32_t *completed) {
    return bo_selfplay_autoturn_collect_ex(e, res_n, res_idx, res_val, best_idx, action_out, n_legal_out, terminal_out, go_out, nullptr, nullptr,
                                           completed);
}

// The root's q_value kept exact in every backup (ABI 7): v_i of bo_search_root_value / bo_selfplay_autoturn_collect_ex
extern "C" int bo_engine_root_values(bo_engine *e, int32_t on) {
    if (!e) return fail(BO_E_ARG, "null engine");
    e->d.c.root_q = on ? 1 : 0;
    return BO_OK;
}

// Resignation in the device turn (ABI 7): enable[g] != 0 sets flag bit 3 for slot g's next turns (NULL: off for every slot).
extern "C" int bo_selfplay_resign(bo_engine *e, const int32_t *enable, float threshold, int32_t plies) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (plies < 1) return fail(BO_E_ARG, "bo_selfplay_resign: plies must be >= 1");
    if (enable && !(threshold == threshold)) return fail(BO_E_ARG, "bo_selfplay_resign: the threshold is NaN");
    if (enable && e->fast) return fail(BO_E_CONFIG, "bo_selfplay_resign: reference-semantics engines only");
    if (enable && !e->d.c.root_q) return fail(BO_E_STATE, "bo_selfplay_resign: call bo_engine_root_values(e, 1) first");
    const int G = e->d.c.G;
    if (enable) e->resign_en.assign(enable, enable + G);
    else e->resign_en.clear();
    e->resign_t = threshold;
    e->resign_k = plies;
    return BO_OK;
}

// v_i of the host-made turn: the root's q_value of every slot (meaningful for the slots whose search has finished).  Synchronises.
extern "C" int bo_search_root_value(bo_engine *e, float *out, void *stream) {
    if (!e || !out) return fail(BO_E_ARG, "null argument");
    const int G = e->d.c.G;
    RT(RT_LAUNCH(bo_k_root_value, (G + 63) / 64, stream, e->d, e->d_root_value));
    RT(rt_d2h(out, e->d_root_value, (size_t)G * 4, stream));
    RT(rt_sync(stream));
    return BO_OK;
}

// ---- records ------------------------------------------------------------------------------------------------
extern "C" int bo_game_export(bo_engine *e, int slot, bo_position *positions, int32_t *moves, int32_t cap, int32_t *n_plies,
                              void *stream) {
    if (!e || slot < 0 || slot >= e->d.c.G || !n_plies) return fail(BO_E_ARG, "bad arguments");
    const EngCfg &c = e->d.c;
    // ply count and (up to cap) positions / moves in one round trip: the caller's cap is normally exact (it counted the plies)
    const int want = cap < c.PLY_CAP ? (cap > 0 ? cap : 0) : c.PLY_CAP;
    int ply = 0;
    std::vector<DPos> gp((size_t)want);
    std::vector<bo_mv> mv((size_t)want);
    RT(rt_d2h(&ply, e->d.ply + slot, 4, stream));
    if (want > 0 && (positions || moves)) {
        RT(rt_d2h(gp.data(), e->d.gpos + (size_t)slot * c.PLY_CAP, gp.size() * sizeof(DPos), stream));
        RT(rt_d2h(mv.data(), e->d.played + (size_t)slot * c.PLY_CAP, mv.size() * sizeof(bo_mv), stream));
    }
    RT(rt_sync(stream));
    *n_plies = ply;
    if (!positions && !moves) return BO_OK;
    if (ply + 1 > cap) return fail(BO_E_ARG, "export buffer too small");
    for (int i = 0; i <= ply; i++) {
        if (positions) to_abi(gp[i], &positions[i]);
        if (moves && i < ply) moves[i] = mv[i];
    }
    return BO_OK;
}

extern "C" int bo_game_encode(bo_engine *e, int slot, int first, int n, float *out_dev, void *stream) {
    if (!e || slot < 0 || slot >= e->d.c.G || n < 1 || first < 0 || !out_dev) return fail(BO_E_ARG, "bad arguments");
    RT(RT_LAUNCH(bo_k_encode_game, n, stream, e->d, slot, first, out_dev));
    return BO_OK;
}

extern "C" int bo_records_encode(int n_positions, const bo_position *positions, int first, int n, float *out_dev, void *stream) {
    if (n_positions < 1 || !positions || first < 0 || n < 1 || first + n > n_positions || !out_dev)
        return fail(BO_E_ARG, "bad arguments");
    std::vector<DPos> hp((size_t)n_positions);
    for (int i = 0; i < n_positions; i++) hp[i] = from_abi(positions[i]);
    void *dp = nullptr;
    int rc = rt_malloc(&dp, hp.size() * sizeof(DPos));
    if (!rc) rc = rt_h2d(dp, hp.data(), hp.size() * sizeof(DPos), stream);
    if (!rc) rc = RT_LAUNCH(bo_k_encode_positions, n, stream, (const DPos *)dp, n_positions, first, out_dev);
    int rc2 = rt_sync(stream);
    rt_free(dp);
    if (rc || rc2) return fail(BO_E_HIP, std::string("bo_records_encode: ") + rt_errstr(rc ? rc : rc2));
    return BO_OK;
}

// ---- GPU-resident replay buffer (bo_replay.h) ------------------------------------------------------
// Storage is a ring of position slots; a game of n records takes n + 1 consecutive slots (its positions, the final one included: the
// END-of-game tracker counts it), so a sampled ply finds its history blocks next to it.  Games are evicted oldest first when the ring
// comes round.  Host side: the table of resident games; device side: SoA arrays indexed by slot.
struct bo_replay_s {
    int device = 0, W = 2;
    int64_t cap = 0, head = 0, n_records = 0;
    DPos *pos = nullptr;
    int *rep = nullptr, *pi_n = nullptr, *pi_idx = nullptr;
    float *pi_val = nullptr, *z = nullptr, *q = nullptr;   // q: the root value beside z (z itself for a record without one)
    int64_t n_valued = 0;                                 // resident records that carry a root value
    uint64_t epoch = 0;                                   // counts the games added: a bo_replay_merge is good for the epoch it was made in
    struct Game { int64_t start; int32_t n_rec; int32_t game_id; bool valued; };
    std::deque<Game> games;
    std::vector<int64_t> prefix;   // prefix[i] = records of games[0..i) (rebuilt after an add: replay_prefix)
    // a batch's staging block: rows of n ints each -- slot, k and, where the sampler has them, sym and group -- filled on the host and
    // uploaded in one copy
    std::vector<int> h_stage;
    int *stage = nullptr;
    size_t stage_cap = 0;
};

extern "C" int bo_replay_create(int64_t capacity_positions, int pi_width, int device, bo_replay **out) {
    if (!out || capacity_positions < 2 || capacity_positions > (int64_t)0x7fffffff || pi_width < 1 || pi_width > BO_RES_CAP) return fail(BO_E_ARG, "bo_replay_create: bad arguments");
    RT(rt_set_device(device));
    bo_replay *r = new bo_replay();
    r->device = device; r->W = pi_width; r->cap = capacity_positions;
    const size_t n = (size_t)capacity_positions;
    int rc = rt_malloc((void **)&r->pos, n * sizeof(DPos));
    if (!rc) rc = rt_malloc((void **)&r->rep, n * 4);
    if (!rc) rc = rt_malloc((void **)&r->pi_n, n * 4);
    if (!rc) rc = rt_malloc((void **)&r->pi_idx, n * (size_t)pi_width * 4);
    if (!rc) rc = rt_malloc((void **)&r->pi_val, n * (size_t)pi_width * 4);
    if (!rc) rc = rt_malloc((void **)&r->z, n * 4);
    if (!rc) rc = rt_malloc((void **)&r->q, n * 4);
    if (rc) {
        rt_free(r->pos); rt_free(r->rep); rt_free(r->pi_n); rt_free(r->pi_idx); rt_free(r->pi_val); rt_free(r->z); rt_free(r->q);
        delete r;
        return fail(BO_E_HIP, std::string("bo_replay_create: ") + rt_errstr(rc));
    }
    *out = r;
    return BO_OK;
}

extern "C" void bo_replay_destroy(bo_replay *r) {
    if (!r) return;
    rt_free(r->pos); rt_free(r->rep); rt_free(r->pi_n); rt_free(r->pi_idx); rt_free(r->pi_val); rt_free(r->z); rt_free(r->q); rt_free(r->stage);
    delete r;
}

// One finished game: positions[0 .. n_records] (the record wire format's list: position i is the one before move i, the last is the
// final position), pi of record i = entries pi_ptr[i] .. pi_ptr[i + 1] of (pi_idx, pi_val), z[i] as the reference stores it
// (self_play.py:202: the outcome from the point of view of the side to move, sign of zero included).  Evicts the oldest games that
// are in the way; *evicted_records (may be NULL) = how many records that cost.  Synchronises `stream` (host staging is freed).
// root_value[i] (NULL: the game has none): the root's q_value after the search at ply i, from the side to move's point of view like
// z[i]; without it the slot's q is z[i] and the game's records do not count as carrying a value.
static int replay_add_game(const char *who, bo_replay *r, int32_t game_id, const bo_position *positions, int32_t n_records, const int32_t *pi_ptr,
                           const int32_t *pi_idx, const float *pi_val, const float *z, const float *root_value, int64_t *evicted_records,
                           void *stream) {
    if (!r || !positions || n_records < 0 || (n_records && (!pi_ptr || !pi_idx || !pi_val || !z))) return fail(BO_E_ARG, std::string(who) + ": bad arguments");
    if (evicted_records) *evicted_records = 0;
    if (n_records == 0) return BO_OK;  // (a start position that was already over: no examples, self_play.py:101)
    const int64_t need = (int64_t)n_records + 1;
    if (need > r->cap) return fail(BO_E_ARG, std::string(who) + ": the game is longer than the buffer");
    for (int i = 0; i < n_records; i++)
        if (pi_ptr[i + 1] - pi_ptr[i] > r->W || pi_ptr[i + 1] < pi_ptr[i]) return fail(BO_E_ARG, std::string(who) + ": a pi has more entries than the buffer's pi_width");
    r->epoch++;  // (before the first eviction: a merge made earlier is stale from here on, whatever becomes of this call)
    int64_t lost = 0;
    auto evict_front = [&]() {
        const auto &g = r->games.front();
        lost += g.n_rec; r->n_records -= g.n_rec; r->n_valued -= g.valued ? g.n_rec : 0;
        r->games.pop_front();
    };
    if (r->head + need > r->cap) {  // does not fit behind the newest game: the games still living in that tail go, the ring comes round
        while (!r->games.empty() && r->games.front().start >= r->head) evict_front();
        r->head = 0;
    }
    while (!r->games.empty() && r->games.front().start >= r->head && r->games.front().start < r->head + need) evict_front();
    const size_t n = (size_t)need;
    std::vector<DPos> hp(n);
    for (size_t i = 0; i < n; i++) hp[i] = from_abi(positions[i]);
    std::vector<int> hn(n, 0), hi(n * (size_t)r->W, 0);
    std::vector<float> hv(n * (size_t)r->W, 0.0f), hz(n, 0.0f), hq(n, 0.0f);
    for (int i = 0; i < n_records; i++) {
        hn[i] = pi_ptr[i + 1] - pi_ptr[i];
        for (int e = 0; e < hn[i]; e++) { hi[(size_t)i * r->W + e] = pi_idx[pi_ptr[i] + e]; hv[(size_t)i * r->W + e] = pi_val[pi_ptr[i] + e]; }
        hz[i] = z[i];
        hq[i] = root_value ? root_value[i] : z[i];
    }
    const size_t o = (size_t)r->head;
    int rc = rt_h2d(r->pos + o, hp.data(), n * sizeof(DPos), stream);
    if (!rc) rc = rt_h2d(r->pi_n + o, hn.data(), n * 4, stream);
    if (!rc) rc = rt_h2d(r->pi_idx + o * r->W, hi.data(), n * (size_t)r->W * 4, stream);
    if (!rc) rc = rt_h2d(r->pi_val + o * r->W, hv.data(), n * (size_t)r->W * 4, stream);
    if (!rc) rc = rt_h2d(r->z + o, hz.data(), n * 4, stream);
    if (!rc) rc = rt_h2d(r->q + o, hq.data(), n * 4, stream);
    if (!rc) rc = RT_LAUNCH(bo_k_replay_counts, (int)need, stream, (const DPos *)(r->pos + o), (int)need, r->rep + o);
    const int rc2 = rt_sync(stream);
    if (rc || rc2) return fail(BO_E_HIP, std::string(who) + ": " + rt_errstr(rc ? rc : rc2));
    r->games.push_back({r->head, n_records, game_id, root_value != nullptr});
    r->head += need;
    r->n_records += n_records;
    r->n_valued += root_value ? n_records : 0;
    r->prefix.clear();
    if (evicted_records) *evicted_records = lost;
    return BO_OK;
}

extern "C" int bo_replay_add_game(bo_replay *r, int32_t game_id, const bo_position *positions, int32_t n_records, const int32_t *pi_ptr,
                                  const int32_t *pi_idx, const float *pi_val, const float *z, int64_t *evicted_records, void *stream) {
    return replay_add_game("bo_replay_add_game", r, game_id, positions, n_records, pi_ptr, pi_idx, pi_val, z, nullptr, evicted_records, stream);
}

extern "C" int bo_replay_add_game_values(bo_replay *r, int32_t game_id, const bo_position *positions, int32_t n_records, const int32_t *pi_ptr,
                                         const int32_t *pi_idx, const float *pi_val, const float *z, const float *root_value,
                                         int64_t *evicted_records, void *stream) {
    return replay_add_game("bo_replay_add_game_values", r, game_id, positions, n_records, pi_ptr, pi_idx, pi_val, z, root_value, evicted_records,
                           stream);
}

extern "C" int bo_replay_size(bo_replay *r, int64_t *n_records, int64_t *n_games) {
    if (!r) return fail(BO_E_ARG, "null handle");
    if (n_records) *n_records = r->n_records;
    if (n_games) *n_games = (int64_t)r->games.size();
    return BO_OK;
}

extern "C" int bo_replay_values(bo_replay *r, int64_t *n_records_with_value) {
    if (!r || !n_records_with_value) return fail(BO_E_ARG, "bo_replay_values: bad arguments");
    *n_records_with_value = r->n_valued;
    return BO_OK;
}

// record_index q in [0, records) counts the resident records oldest game first (ChessDataset's index space over load_recent_data's
// concatenation, train.py:179-219): its ring slot and its ply in its game.
static void replay_prefix(bo_replay *r) {
    if (!r->prefix.empty()) return;
    r->prefix.reserve(r->games.size() + 1);
    int64_t acc = 0;
    for (const auto &g : r->games) { r->prefix.push_back(acc); acc += g.n_rec; }
    r->prefix.push_back(acc);
}
static void replay_locate(const bo_replay *r, int64_t q, int *slot, int *k) {
    const size_t g = (size_t)(std::upper_bound(r->prefix.begin(), r->prefix.end(), q) - r->prefix.begin()) - 1;
    *k = (int)(q - r->prefix[g]);
    *slot = (int)(r->games[g].start + *k);
}

// ---- merged targets (bo_merge.h; ABI 17) ---------------------------------------------------------------------------------------------
static_assert(BO_MERGE_KEY_INPUT == MERGE_KEY_INPUT && BO_MERGE_KEY_POSITION == MERGE_KEY_POSITION, "merge constants");

struct bo_replay_merge_s {
    bo_replay *r = nullptr;
    uint64_t epoch = 0;
    int key = 0, Wm = 0;
    int64_t n = 0, G = 0, T = 0, largest = 0, in_multi = 0;
    double group_ms = 0.0, merge_ms = 0.0;
    std::vector<int32_t> group_of;   // [records of the buffer] the record's group, -1 = not covered
    std::vector<int64_t> rep_of;     // [n] work-list order: the representative of the item's group
    std::vector<int64_t> reps;       // [G] ascending
    std::vector<int32_t> count;      // [G]
    int *m_idx = nullptr;
    float *m_val = nullptr, *m_z = nullptr, *m_q = nullptr;
};

extern "C" void bo_replay_merge_destroy(bo_replay_merge *m) {
    if (!m) return;
    rt_free(m->m_idx); rt_free(m->m_val); rt_free(m->m_z); rt_free(m->m_q);
    delete m;
}

namespace {
struct MergeScratch {  // device scratch of one bo_replay_merge_create_ex call
    std::vector<void *> p;
    ~MergeScratch() { for (void *q : p) rt_free(q); }
    template <class T> int get(T **out, size_t n) {
        void *q = nullptr;
        const int rc = rt_malloc(&q, n * sizeof(T));
        if (!rc) p.push_back(q);
        *out = (T *)q;
        return rc;
    }
};
#if !defined(BO_WAVE_EMU)
struct MergeClock {  // device events around the kernels (timing events: rt_event has none)
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    MergeClock() { for (auto &x : e) (void)hipEventCreate(&x); }
    ~MergeClock() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
    void mark(int i, void *s) { if (e[i]) (void)hipEventRecord(e[i], (hipStream_t)s); }
    double ms(int i) { float t = 0.0f; return (e[i] && e[i + 1] && hipEventElapsedTime(&t, e[i], e[i + 1]) == hipSuccess) ? (double)t : 0.0; }
};
#else
struct MergeClock { void mark(int, void *) {} double ms(int) { return 0.0; } };
#endif
}  // namespace

extern "C" int bo_replay_merge_create_ex(bo_replay *r, int64_t n, const int64_t *record_index, int32_t key, int64_t table_slots, void *stream,
                                         bo_replay_merge **out) {
    const std::string who = "bo_replay_merge_create";
    if (!r || !out) return fail(BO_E_ARG, who + ": null argument");
    if (key != MERGE_KEY_INPUT && key != MERGE_KEY_POSITION) return fail(BO_E_ARG, who + ": unknown key (0 = input, 1 = position)");
    if (!record_index) n = r->n_records;
    if (n < 1) return fail(BO_E_ARG, who + ": no records");
    if (r->n_records > (int64_t)MERGE_CANON_NONE) return fail(BO_E_ARG, who + ": more than 0x7f7f7f7f resident records");
    int64_t T = table_slots;
    if (n > ((int64_t)1 << 29)) return fail(BO_E_ARG, who + ": more than 2^29 records");
    if (T == 0) for (T = 64; T < 2 * n; T <<= 1) {}
    if (T < 1 || T > ((int64_t)1 << 30) || (T & (T - 1)) != 0) return fail(BO_E_ARG, who + ": table_slots must be 0 or a power of two, 1 .. 2^30");
    replay_prefix(r);
    std::unique_ptr<bo_replay_merge, void (*)(bo_replay_merge *)> m(new bo_replay_merge(), bo_replay_merge_destroy);
    m->r = r; m->epoch = r->epoch; m->key = key; m->n = n; m->T = T;
    m->group_of.assign((size_t)r->n_records, -1);
    std::vector<int> h_slot((size_t)n), h_k((size_t)n), h_rec((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = record_index ? record_index[i] : i;
        if (q < 0 || q >= r->n_records) return fail(BO_E_ARG, who + ": record index out of range");
        if (m->group_of[(size_t)q] != -1) return fail(BO_E_ARG, who + ": record " + std::to_string(q) + " is listed twice");
        m->group_of[(size_t)q] = -2;
        replay_locate(r, q, &h_slot[(size_t)i], &h_k[(size_t)i]);
        h_rec[(size_t)i] = (int)q;
    }
    RT(rt_set_device(r->device));
    MergeScratch sc;
    MergeClock clk;
    MergeGroupArgs ga = {};
    int *d_slot = nullptr, *d_k = nullptr, *d_rec = nullptr;
    int rc = sc.get(&d_slot, (size_t)n);
    if (!rc) rc = sc.get(&d_k, (size_t)n);
    if (!rc) rc = sc.get(&d_rec, (size_t)n);
    if (!rc) rc = sc.get(&ga.owner, (size_t)T);
    if (!rc) rc = sc.get(&ga.canon, (size_t)T);
    if (!rc) rc = sc.get(&ga.gid, (size_t)n);
    if (!rc) rc = sc.get(&ga.status, 1);
    if (!rc) rc = rt_h2d(d_slot, h_slot.data(), (size_t)n * 4, stream);
    if (!rc) rc = rt_h2d(d_k, h_k.data(), (size_t)n * 4, stream);
    if (!rc) rc = rt_h2d(d_rec, h_rec.data(), (size_t)n * 4, stream);
    if (!rc) rc = rt_memset(ga.owner, 0xFF, (size_t)T * 4, stream);
    if (!rc) rc = rt_memset(ga.canon, 0x7F, (size_t)T * 4, stream);
    if (!rc) rc = rt_memset(ga.status, 0, 4, stream);
    ga.pos = r->pos; ga.rep = r->rep; ga.slot = d_slot; ga.k = d_k; ga.rec = d_rec; ga.n = n; ga.T = T; ga.key = key;
    clk.mark(0, stream);
    if (!rc) rc = RT_LAUNCH(bo_k_replay_group, (int)((n + 63) / 64), stream, ga);
    clk.mark(1, stream);
    std::vector<int32_t> gid((size_t)n), canon((size_t)T);
    int32_t over = 0;
    if (!rc) rc = rt_d2h(gid.data(), ga.gid, (size_t)n * 4, stream);
    if (!rc) rc = rt_d2h(canon.data(), ga.canon, (size_t)T * 4, stream);
    if (!rc) rc = rt_d2h(&over, ga.status, 4, stream);
    if (!rc) rc = rt_sync(stream);
    if (rc) return fail(BO_E_HIP, who + ": " + rt_errstr(rc));
    m->group_ms = clk.ms(0);
    if (over)
        return fail(BO_E_STATE, who + ": table overflow: " + std::to_string(over) + " of " + std::to_string(n) + " records found no slot among " +
                                    std::to_string(T));
    // groups in ascending order of their representative, members in ascending record index: a stable counting sort on the host
    m->rep_of.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const int32_t s = gid[(size_t)i];
        if (s < 0 || s >= T || canon[(size_t)s] < 0 || canon[(size_t)s] >= r->n_records || m->group_of[(size_t)canon[(size_t)s]] == -1)
            return fail(BO_E_STATE, who + ": inconsistent table");
        m->rep_of[(size_t)i] = canon[(size_t)s];
    }
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return h_rec[(size_t)x] < h_rec[(size_t)y]; });
    for (int64_t j = 0; j < n; j++) {  // ascending record index: a group's representative comes before its other members
        const int64_t i = order[(size_t)j];
        if (m->rep_of[(size_t)i] == h_rec[(size_t)i]) {
            m->group_of[(size_t)h_rec[(size_t)i]] = (int32_t)m->reps.size();
            m->reps.push_back(h_rec[(size_t)i]);
        }
    }
    const int64_t G = m->G = (int64_t)m->reps.size();
    m->count.assign((size_t)G, 0);
    for (int64_t i = 0; i < n; i++) {
        const int32_t g = m->group_of[(size_t)m->rep_of[(size_t)i]];
        if (g < 0) return fail(BO_E_STATE, who + ": inconsistent table");
        m->group_of[(size_t)h_rec[(size_t)i]] = g;
        m->count[(size_t)g]++;
    }
    std::vector<int> off((size_t)G + 1, 0), fill((size_t)G), mslot((size_t)n);
    for (int64_t g = 0; g < G; g++) {
        off[(size_t)g + 1] = off[(size_t)g] + m->count[(size_t)g];
        fill[(size_t)g] = off[(size_t)g];
        m->largest = std::max<int64_t>(m->largest, m->count[(size_t)g]);
        m->in_multi += m->count[(size_t)g] > 1 ? m->count[(size_t)g] : 0;
    }
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = order[(size_t)j];
        mslot[(size_t)fill[(size_t)m->group_of[(size_t)h_rec[(size_t)i]]]++] = h_slot[(size_t)i];
    }
    MergeArgs ma = {};
    int *d_off = nullptr, *d_mslot = nullptr;
    rc = sc.get(&d_off, (size_t)G + 1);
    if (!rc) rc = sc.get(&d_mslot, (size_t)n);
    if (!rc) rc = sc.get(&ma.usz, (size_t)G);
    if (!rc) rc = rt_h2d(d_off, off.data(), ((size_t)G + 1) * 4, stream);
    if (!rc) rc = rt_h2d(d_mslot, mslot.data(), (size_t)n * 4, stream);
    ma.pi_n = r->pi_n; ma.pi_idx = r->pi_idx; ma.pi_val = r->pi_val; ma.z = r->z; ma.q = r->q; ma.W = r->W; ma.off = d_off; ma.mslot = d_mslot;
    ma.Wm = 0; ma.out_idx = nullptr; ma.out_val = ma.out_z = ma.out_q = nullptr;
    clk.mark(1, stream);
    if (!rc) rc = RT_LAUNCH(bo_k_replay_merge, (int)G, stream, ma);  // the counting pass: the unions' sizes
    std::vector<int32_t> usz((size_t)G);
    if (!rc) rc = rt_d2h(usz.data(), ma.usz, (size_t)G * 4, stream);
    if (!rc) rc = rt_sync(stream);
    if (rc) return fail(BO_E_HIP, who + ": " + rt_errstr(rc));
    m->Wm = r->W;
    for (int64_t g = 0; g < G; g++) {
        if (usz[(size_t)g] > BO_RES_CAP)
            return fail(BO_E_ARG, who + ": the group of record " + std::to_string(m->reps[(size_t)g]) + " (" + std::to_string(m->count[(size_t)g]) +
                                      " records) has more than " + std::to_string(BO_RES_CAP) + " distinct actions in its pis");
        m->Wm = std::max(m->Wm, (int)usz[(size_t)g]);
    }
    const size_t cells = (size_t)G * (size_t)m->Wm;
    rc = rt_malloc((void **)&m->m_idx, cells * 4);
    if (!rc) rc = rt_malloc((void **)&m->m_val, cells * 4);
    if (!rc) rc = rt_malloc((void **)&m->m_z, (size_t)G * 4);
    if (!rc) rc = rt_malloc((void **)&m->m_q, (size_t)G * 4);
    ma.Wm = m->Wm; ma.out_idx = m->m_idx; ma.out_val = m->m_val; ma.out_z = m->m_z; ma.out_q = m->m_q;
    if (!rc) rc = RT_LAUNCH(bo_k_replay_merge, (int)G, stream, ma);
    clk.mark(2, stream);
    if (!rc) rc = rt_sync(stream);
    if (rc) return fail(BO_E_HIP, who + ": " + rt_errstr(rc));
    m->merge_ms = clk.ms(1);
    *out = m.release();
    return BO_OK;
}

extern "C" int bo_replay_merge_create(bo_replay *r, int64_t n, const int64_t *record_index, int32_t key, bo_replay_merge **out) {
    return bo_replay_merge_create_ex(r, n, record_index, key, 0, nullptr, out);
}

extern "C" int bo_replay_merge_info(const bo_replay_merge *m, bo_merge_info *out) {
    if (!m || !out) return fail(BO_E_ARG, "bo_replay_merge_info: null argument");
    out->groups = m->G; out->width = m->Wm; out->records = m->n; out->largest_group = m->largest; out->records_in_groups = m->in_multi;
    out->table_slots = m->T; out->group_ms = m->group_ms; out->merge_ms = m->merge_ms;
    return BO_OK;
}

extern "C" int bo_replay_merge_groups(const bo_replay_merge *m, int64_t *representative, int32_t *count) {
    if (!m || (!representative && !count)) return fail(BO_E_ARG, "bo_replay_merge_groups: null argument");
    if (representative) memcpy(representative, m->rep_of.data(), (size_t)m->n * sizeof(int64_t));
    if (count) memcpy(count, m->count.data(), (size_t)m->G * sizeof(int32_t));
    return BO_OK;
}

// ---- the samplers (bo_replay.h, bo_merge.h; board symmetries: bo_sym.h, ABI 18) -------------------------------------------------------
// A batch of n records, written on `stream` (the kernel is not waited for): states [n,120,8,8] and z [n] always;
//   dense                  pi [n,4672]
//   sparse, sparse_q       pi as the records keep it: pi_idx / pi_val [n, W] (W = the buffer's pi_width; unused places -1 / 0); sparse_q
//                          also the records' root values q [n], from the same launch
//   merged                 sparse_q's batch with the targets of the records' groups: pi_idx / pi_val [n, Wm], z and q the groups' means
// with_sym: sample i under the board symmetry sym[i] (0..3); applied (may be NULL) [n] = the code that was applied.
// A refused call has written nothing and launched nothing: everything is checked on the host first.
enum { REPLAY_DENSE, REPLAY_SPARSE, REPLAY_SPARSE_Q, REPLAY_MERGED };

static int replay_sample(const char *who_c, int kind, bool with_sym, bo_replay *r, bo_replay_merge *m, int32_t n, const int64_t *record_index,
                         const int32_t *sym, ReplayArgs a, void *stream) {
    static void (*const kernels[4][2])(ReplayArgs) = {{bo_k_replay_encode, bo_k_replay_encode_sym},
                                                      {bo_k_replay_encode_sparse, bo_k_replay_encode_sparse_sym},
                                                      {bo_k_replay_encode_sparse_q, bo_k_replay_encode_sparse_q_sym},
                                                      {bo_k_replay_encode_merged, bo_k_replay_encode_merged_sym}};
    const std::string who(who_c);
    const bool merged = kind == REPLAY_MERGED;
    if (!r || (merged && !m) || n < 1 || !record_index || !a.states || !a.zs || (kind == REPLAY_DENSE ? !a.pis : !a.out_idx || !a.out_val) ||
        (kind >= REPLAY_SPARSE_Q && !a.qs) || (with_sym && !sym))
        return fail(BO_E_ARG, who + ": bad arguments");
    for (int i = 0; with_sym && i < n; i++)
        if (sym[i] < 0 || sym[i] > 3) return fail(BO_E_ARG, who + ": symmetry code " + std::to_string(sym[i]) + " of sample " + std::to_string(i) + " is not in 0..3");
    if (merged && m->r != r) return fail(BO_E_ARG, who + ": the merge was made from another buffer");
    if (merged && m->epoch != r->epoch) return fail(BO_E_ARG, who + ": stale merge: games were added to the buffer after it was made");
    // locate: the staging rows slot, k, then sym and group where the sampler has them
    replay_prefix(r);
    const size_t N = (size_t)n, rows = 2 + (with_sym ? 1 : 0) + (merged ? 1 : 0);
    r->h_stage.resize(rows * N);
    int *h_slot = r->h_stage.data(), *h_k = h_slot + N, *h_sym = h_k + N, *h_grp = h_k + (rows - 2) * N;
    for (int i = 0; i < n; i++) {
        const int64_t q = record_index[i];
        if (q < 0 || q >= r->n_records) return fail(BO_E_ARG, who + ": record index out of range");
        replay_locate(r, q, &h_slot[i], &h_k[i]);
        if (with_sym) h_sym[i] = sym[i];
        if (!merged) continue;
        if (m->group_of[(size_t)q] < 0) return fail(BO_E_ARG, who + ": record " + std::to_string(q) + " is not covered by the merge");
        h_grp[i] = m->group_of[(size_t)q];
    }
    // stage: one upload
    if (r->h_stage.size() > r->stage_cap) {
        RT(rt_sync(stream));  // (the previous batch's rows may still be read)
        rt_free(r->stage);
        r->stage = nullptr; r->stage_cap = 0;
        RT(rt_malloc((void **)&r->stage, r->h_stage.size() * 4));
        r->stage_cap = r->h_stage.size();
    }
    RT(rt_h2d(r->stage, r->h_stage.data(), r->h_stage.size() * 4, stream));
    a.pos = r->pos; a.rep = r->rep;
    a.s_slot = r->stage; a.s_k = r->stage + N;
    a.s_sym = with_sym ? r->stage + 2 * N : nullptr;
    a.s_grp = merged ? r->stage + (rows - 1) * N : nullptr;
    if (merged) { a.pi_n = nullptr; a.pi_idx = m->m_idx; a.pi_val = m->m_val; a.z = m->m_z; a.q = m->m_q; a.W = m->Wm; }
    else { a.pi_n = r->pi_n; a.pi_idx = r->pi_idx; a.pi_val = r->pi_val; a.z = r->z; a.q = r->q; a.W = r->W; }
    RT(RT_LAUNCH(kernels[kind][with_sym ? 1 : 0], n, stream, a));
    // the pageable host staging is re-used by the next call: wait for its upload (the encode kernel itself is not waited for)
    RT(rt_sync(stream));
    return BO_OK;
}

static ReplayArgs replay_out(float *states, float *pis, int32_t *out_idx, float *out_val, float *zs, float *qs, int32_t *applied) {
    ReplayArgs a = {};
    a.states = states; a.pis = pis; a.out_idx = (int *)out_idx; a.out_val = out_val; a.zs = zs; a.qs = qs; a.applied = (int *)applied;
    return a;
}

extern "C" int bo_replay_sample(bo_replay *r, int32_t n, const int64_t *record_index, float *states_dev, float *pi_dev, float *z_dev, void *stream) {
    return replay_sample("bo_replay_sample", REPLAY_DENSE, false, r, nullptr, n, record_index, nullptr,
                         replay_out(states_dev, pi_dev, nullptr, nullptr, z_dev, nullptr, nullptr), stream);
}

extern "C" int bo_replay_sample_sparse(bo_replay *r, int32_t n, const int64_t *record_index, float *states_dev, int32_t *pi_idx_dev,
                                       float *pi_val_dev, float *z_dev, void *stream) {
    return replay_sample("bo_replay_sample_sparse", REPLAY_SPARSE, false, r, nullptr, n, record_index, nullptr,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, nullptr, nullptr), stream);
}

extern "C" int bo_replay_sample_sparse_q(bo_replay *r, int32_t n, const int64_t *record_index, float *states_dev, int32_t *pi_idx_dev,
                                         float *pi_val_dev, float *z_dev, float *q_dev, void *stream) {
    return replay_sample("bo_replay_sample_sparse_q", REPLAY_SPARSE_Q, false, r, nullptr, n, record_index, nullptr,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, q_dev, nullptr), stream);
}

extern "C" int bo_replay_sample_merged(bo_replay *r, bo_replay_merge *m, int32_t n, const int64_t *record_index, float *states_dev,
                                       int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev, void *stream) {
    return replay_sample("bo_replay_sample_merged", REPLAY_MERGED, false, r, m, n, record_index, nullptr,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, q_dev, nullptr), stream);
}

extern "C" int bo_replay_sample_sym(bo_replay *r, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev, float *pi_dev,
                                    float *z_dev, int32_t *applied_dev, void *stream) {
    return replay_sample("bo_replay_sample_sym", REPLAY_DENSE, true, r, nullptr, n, record_index, sym,
                         replay_out(states_dev, pi_dev, nullptr, nullptr, z_dev, nullptr, applied_dev), stream);
}

extern "C" int bo_replay_sample_sparse_sym(bo_replay *r, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev,
                                           int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, int32_t *applied_dev, void *stream) {
    return replay_sample("bo_replay_sample_sparse_sym", REPLAY_SPARSE, true, r, nullptr, n, record_index, sym,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, nullptr, applied_dev), stream);
}

extern "C" int bo_replay_sample_sparse_q_sym(bo_replay *r, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev,
                                             int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev, int32_t *applied_dev,
                                             void *stream) {
    return replay_sample("bo_replay_sample_sparse_q_sym", REPLAY_SPARSE_Q, true, r, nullptr, n, record_index, sym,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, q_dev, applied_dev), stream);
}

extern "C" int bo_replay_sample_merged_sym(bo_replay *r, bo_replay_merge *m, int32_t n, const int64_t *record_index, const int32_t *sym,
                                           float *states_dev, int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev,
                                           int32_t *applied_dev, void *stream) {
    return replay_sample("bo_replay_sample_merged_sym", REPLAY_MERGED, true, r, m, n, record_index, sym,
                         replay_out(states_dev, nullptr, pi_idx_dev, pi_val_dev, z_dev, q_dev, applied_dev), stream);
}

// ---- PGN pretraining (bo_pgn.h) --------------------------------------------------------------------------------------------------
static_assert(sizeof(DPos) == BO_PGN_POSITION_BYTES, "ring slot size");

extern "C" int bo_pgn_parse(const char *text, int64_t n_bytes, int32_t final_chunk, int64_t max_games, int64_t max_tokens, int64_t *consumed,
                            bo_pgn **out) {
    if (!out || !consumed || n_bytes < 0 || (n_bytes && !text)) return fail(BO_E_ARG, "bo_pgn_parse: bad arguments");
    bo_pgn *p = new bo_pgn();
    *consumed = pgn_parse(p, text, n_bytes, final_chunk != 0, max_games, max_tokens);
    *out = p;
    return BO_OK;
}

extern "C" int bo_pgn_size(const bo_pgn *p, int64_t *n_games, int64_t *n_tokens, int64_t *scratch_bytes) {
    if (!p) return fail(BO_E_ARG, "null handle");
    const int64_t g = (int64_t)p->status.size(), t = (int64_t)p->tok.size();
    if (n_games) *n_games = g;
    if (n_tokens) *n_tokens = t;
    // tokens, has_eval, target, then per game: token range [2], root, slot0, result[2] -- 16-byte aligned pieces
    auto al = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
    if (scratch_bytes) *scratch_bytes = al(4 * t) + al(t) + al(4 * t) + al(8 * g) + al((int64_t)sizeof(DPos) * g) + al(4 * g) + al(8 * g) + 16;
    return BO_OK;
}

extern "C" int bo_pgn_export(const bo_pgn *p, int32_t *status, int32_t *tok_off, bo_position *roots, uint32_t *tokens, int32_t *has_eval,
                             float *target) {
    if (!p) return fail(BO_E_ARG, "null handle");
    const size_t g = p->status.size(), t = p->tok.size();
    for (size_t i = 0; i < g; i++) {
        if (status) status[i] = p->status[i];
        if (roots) to_abi(p->root[i], &roots[i]);
    }
    if (tok_off) for (size_t i = 0; i <= g; i++) tok_off[i] = p->tok_off[i];
    for (size_t i = 0; i < t; i++) {
        if (tokens) tokens[i] = p->tok[i];
        if (has_eval) has_eval[i] = p->has_eval[i];
        if (target) target[i] = p->target[i];
    }
    return BO_OK;
}

extern "C" int bo_pgn_replay(const bo_pgn *p, const int64_t *slot0, int64_t capacity, void *scratch_dev, int64_t scratch_bytes, void *pos_dev,
                             int32_t *act_dev, float *z_dev, int32_t *smp_dev, int32_t *n_plies_out, int32_t *status_out, void *stream) {
    if (!p || !slot0 || capacity < 1 || capacity > (int64_t)0x7fffffff || !scratch_dev || !pos_dev || !act_dev || !z_dev || !smp_dev)
        return fail(BO_E_ARG, "bo_pgn_replay: bad arguments");
    int64_t need = 0;
    bo_pgn_size(p, nullptr, nullptr, &need);
    if (scratch_bytes < need) return fail(BO_E_ARG, "bo_pgn_replay: scratch smaller than bo_pgn_size's scratch_bytes");
    const int G = (int)p->status.size();
    // the games that go to the device (status ok so far, at least one token), each in its own slots of the ring
    std::vector<int> launch, rng, s0;
    std::vector<DPos> roots;
    for (int g = 0; g < G; g++) {
        const int nt = p->tok_off[g + 1] - p->tok_off[g];
        if (n_plies_out) n_plies_out[g] = 0;
        if (status_out) status_out[g] = p->status[g];
        if (slot0[g] < 0 || nt == 0 || (p->status[g] != BO_PGN_OK && p->status[g] != BO_PGN_NULL_MOVE && p->status[g] != BO_PGN_UNSUPPORTED)) continue;
        if (slot0[g] + nt > capacity) return fail(BO_E_ARG, "bo_pgn_replay: a game's slots run past the ring");
        launch.push_back(g);
        rng.push_back(p->tok_off[g]);
        rng.push_back(p->tok_off[g + 1]);
        s0.push_back((int)slot0[g]);
        roots.push_back(p->root[g]);
    }
    if (launch.empty()) return BO_OK;
    const int64_t t = (int64_t)p->tok.size();
    auto al = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
    char *d = (char *)scratch_dev;
    uint32_t *d_tok = (uint32_t *)d; d += al(4 * t);
    int8_t *d_ev = (int8_t *)d; d += al(t);
    float *d_tg = (float *)d; d += al(4 * t);
    int *d_rng = (int *)d; d += al(8 * G);
    DPos *d_root = (DPos *)d; d += al((int64_t)sizeof(DPos) * G);
    int *d_s0 = (int *)d; d += al(4 * G);
    int *d_res = (int *)d;
    const int n = (int)launch.size();
    std::vector<int> res((size_t)2 * n);
    int rc = t ? rt_h2d(d_tok, p->tok.data(), (size_t)t * 4, stream) : 0;
    if (!rc && t) rc = rt_h2d(d_ev, p->has_eval.data(), (size_t)t, stream);
    if (!rc && t) rc = rt_h2d(d_tg, p->target.data(), (size_t)t * 4, stream);
    if (!rc) rc = rt_h2d(d_rng, rng.data(), rng.size() * 4, stream);
    if (!rc) rc = rt_h2d(d_root, roots.data(), roots.size() * sizeof(DPos), stream);
    if (!rc) rc = rt_h2d(d_s0, s0.data(), s0.size() * 4, stream);
    if (!rc) rc = RT_LAUNCH(bo_k_pgn_replay, n, stream, (const uint32_t *)d_tok, (const int *)d_rng, (const DPos *)d_root, (const int8_t *)d_ev,
                            (const float *)d_tg, (const int *)d_s0, (DPos *)pos_dev, (int *)act_dev, z_dev, (int *)smp_dev, d_res);
    if (!rc) rc = rt_d2h(res.data(), d_res, res.size() * 4, stream);
    const int rc2 = rt_sync(stream);
    if (rc || rc2) return fail(BO_E_HIP, std::string("bo_pgn_replay: ") + rt_errstr(rc ? rc : rc2));
    for (int i = 0; i < n; i++) {
        const int g = launch[i];
        if (n_plies_out) n_plies_out[g] = res[2 * i];
        if (status_out && res[2 * i + 1] != BO_PGN_OK) status_out[g] = res[2 * i + 1];
    }
    return BO_OK;
}

extern "C" int bo_pgn_sample(const void *pos_dev, const int32_t *act_dev, const float *z_dev, int32_t n, const int32_t *game_slot_dev,
                             const int32_t *ply_dev, float *states_dev, int32_t *pi_idx_dev, float *pi_val_dev, float *z_out_dev, void *stream) {
    if (!pos_dev || !act_dev || !z_dev || n < 1 || !game_slot_dev || !ply_dev || !states_dev || !pi_idx_dev || !pi_val_dev || !z_out_dev)
        return fail(BO_E_ARG, "bo_pgn_sample: bad arguments");
    RT(RT_LAUNCH(bo_k_pgn_sample, n, stream, (const DPos *)pos_dev, (const int *)act_dev, z_dev, (const int *)game_slot_dev, (const int *)ply_dev,
                 states_dev, (int *)pi_idx_dev, pi_val_dev, z_out_dev));
    return BO_OK;
}

extern "C" void bo_pgn_destroy(bo_pgn *p) { delete p; }

// ---- analysis of games that are already on the device (bo_analyse.h; ABI 8) ------------------------------------------------------
static_assert(sizeof(bo_analysis) == BO_ANALYSIS_WORDS * 4, "bo_analysis is BO_ANALYSIS_WORDS words");
static_assert(BO_ST_BAD_RANGE == ST_BAD_RANGE, "status bits");

// bo_games_reset for roots that bo_pgn_replay left in HBM.  Asynchronous: every array is read by the kernel when it runs.
extern "C" int bo_games_reset_dev(bo_engine *e, int n, const int32_t *slots_dev, const void *pos_dev, int64_t capacity, const int64_t *first_dev,
                                  const int32_t *ply_dev, void *stream) {
    if (!e || n < 1 || !slots_dev || !pos_dev || !first_dev || !ply_dev) return fail(BO_E_ARG, "bo_games_reset_dev: bad arguments");
    if (e->fast) return fail(BO_E_CONFIG, "bo_games_reset_dev: reference-semantics engines only");
    if (n > e->d.c.G) return fail(BO_E_ARG, "bo_games_reset_dev: more slots than the engine has");
    if (capacity < 1) return fail(BO_E_ARG, "bo_games_reset_dev: the position array is empty");
    SetupDevArgs a;
    a.slots = slots_dev; a.pos = (const DPos *)pos_dev; a.capacity = capacity; a.first = (const long long *)first_dev; a.ply = ply_dev;
    e->nl_valid = false;
    e->prefetch_valid = false;
    RT(RT_LAUNCH(bo_k_setup_dev, n, stream, e->d, a));
    return BO_OK;
}

// The begin of the device turn as an entry point: a wanted slot whose root is not terminal searches (mcts.py:160-162).  No Dirichlet
// noise can be handed in this way: engines created with dirichlet_alpha <= 0 only.  Asynchronous.
extern "C" int bo_search_begin_dev(bo_engine *e, const int32_t *want_dev, float *nn_in_dev, void *stream) {
    if (!e || !want_dev || !nn_in_dev) return fail(BO_E_ARG, "bo_search_begin_dev: null argument");
    if (e->fast) return fail(BO_E_CONFIG, "bo_search_begin_dev: reference-semantics engines only");
    if (e->d.c.use_noise) return fail(BO_E_CONFIG, "bo_search_begin_dev: the roots get no Dirichlet noise (create the engine with dirichlet_alpha <= 0)");
    e->nl_valid = false;
    RT(RT_LAUNCH(bo_k_search_begin_want, e->d.c.G, stream, e->d, (const int *)want_dev, nn_in_dev));
    return BO_OK;
}

// bo_k_result + bo_k_analysis: one bo_analysis record per slot into out[G].  Asynchronous.
extern "C" int bo_analysis_result(bo_engine *e, const int32_t *played_dev, bo_analysis *out, void *stream) {
    if (!e || !out) return fail(BO_E_ARG, "bo_analysis_result: null argument");
    if (e->fast) return fail(BO_E_CONFIG, "bo_analysis_result: reference-semantics engines only");
    if (!e->d.c.root_q) return fail(BO_E_STATE, "bo_analysis_result: call bo_engine_root_values(e, 1) first");
    RT(RT_LAUNCH(bo_k_result, e->d.c.G, stream, e->d));
    RT(RT_LAUNCH(bo_k_analysis, e->d.c.G, stream, e->d, (const int *)played_dev, (int *)out));
    return BO_OK;
}

// ---- reanalysis of self-play records (bo_reanalyse.h; ABI 15) ----------------------------------------------------------------------
static_assert(sizeof(bo_reanalysis) == BO_REANALYSIS_WORDS * 4, "bo_reanalysis is BO_REANALYSIS_WORDS words");
static_assert(BO_ST_PI_OVERFLOW == ST_PI_OVERFLOW, "status bits");
static_assert(sizeof(DPos) == BO_PGN_POSITION_BYTES, "a ring entry");

// n bo_position -> n ring entries, one lane each.  Asynchronous; both arrays are device memory.
extern "C" int bo_records_ring(const bo_position *pos_dev, int64_t n, void *ring_out_dev, void *stream) {
    if (n < 0 || n > ((int64_t)1 << 36)) return fail(BO_E_ARG, "bo_records_ring: n out of range");
    if (n == 0) return BO_OK;
    if (!pos_dev || !ring_out_dev) return fail(BO_E_ARG, "bo_records_ring: null argument");
    RT(RT_LAUNCH(bo_k_records_ring, (int)((n + 63) / 64), stream, pos_dev, (long long)n, (DPos *)ring_out_dev));
    return BO_OK;
}

// bo_k_result + bo_k_reanalysis: one bo_reanalysis record and one pi row of W entries per slot.  Asynchronous.
extern "C" int bo_reanalysis_result(bo_engine *e, const int32_t *played_action_dev, const int64_t *root_dev, const int32_t *old_ptr_dev,
                                    const int32_t *old_idx_dev, const float *old_val_dev, int32_t W, bo_reanalysis *out, int32_t *pi_idx_out,
                                    float *pi_val_out, void *stream) {
    if (!e || !out || !pi_idx_out || !pi_val_out) return fail(BO_E_ARG, "bo_reanalysis_result: null argument");
    if (W < 1 || W > BO_RES_CAP) return fail(BO_E_ARG, "bo_reanalysis_result: W must be 1 .. BO_RES_CAP");
    const int n_old = (root_dev ? 1 : 0) + (old_ptr_dev ? 1 : 0) + (old_idx_dev ? 1 : 0) + (old_val_dev ? 1 : 0);
    if (n_old != 0 && n_old != 4) return fail(BO_E_ARG, "bo_reanalysis_result: root_dev, old_ptr_dev, old_idx_dev and old_val_dev are given together or not at all");
    if (e->fast) return fail(BO_E_CONFIG, "bo_reanalysis_result: reference-semantics engines only");
    if (!e->d.c.root_q) return fail(BO_E_STATE, "bo_reanalysis_result: call bo_engine_root_values(e, 1) first");
    ReanalysisArgs a;
    a.played = played_action_dev; a.root = (const long long *)root_dev; a.old_ptr = old_ptr_dev; a.old_idx = old_idx_dev; a.old_val = old_val_dev;
    a.W = W; a.out = (int *)out; a.pi_idx = pi_idx_out; a.pi_val = pi_val_out;
    RT(RT_LAUNCH(bo_k_result, e->d.c.G, stream, e->d));
    RT(RT_LAUNCH(bo_k_reanalysis, e->d.c.G, stream, e->d, a));
    return BO_OK;
}

// ---- opening books (bo_book.h; ABI 16) ---------------------------------------------------------------------------------------------
static_assert(BO_BOOK_NO_COMBINE == BOOK_NO_COMBINE && BO_BOOK_EVAL_ONE == BOOK_EVAL_ONE, "book constants");

// n work items into a table of T slots, one lane per item.  Asynchronous; every pointer is device memory.
extern "C" int bo_book_insert(const void *pos_dev, int64_t capacity, int64_t n, const int64_t *entry_dev, const int32_t *ply_dev,
                              const int32_t *result_dev, const float *eval_dev, const int32_t *back_dev, int64_t T, int32_t *owner_dev,
                              int64_t *first_dev, int32_t *n_dev, int32_t *w_dev, int32_t *d_dev, int32_t *l_dev, int32_t *n_eval_dev,
                              int32_t *min_ply_dev, int64_t *sum_eval_dev, int32_t *gid_out_dev, int32_t *status_dev, uint32_t flags,
                              void *stream) {
    if (n < 0 || n > (int64_t)0x7fffffff) return fail(BO_E_ARG, "bo_book_insert: n out of range (0 .. 2^31 - 1)");
    if (capacity < 0) return fail(BO_E_ARG, "bo_book_insert: negative capacity");
    if (T < 1 || T > ((int64_t)1 << 30) || (T & (T - 1)) != 0) return fail(BO_E_ARG, "bo_book_insert: T must be a power of two, 1 .. 2^30");
    if (flags & ~(uint32_t)BO_BOOK_NO_COMBINE) return fail(BO_E_ARG, "bo_book_insert: unknown flag bits");
    if (!owner_dev || !first_dev || !n_dev || !w_dev || !d_dev || !l_dev || !n_eval_dev || !min_ply_dev || !sum_eval_dev || !status_dev)
        return fail(BO_E_ARG, "bo_book_insert: null table column or status");
    if (n == 0) return BO_OK;
    if ((capacity > 0 && !pos_dev) || !entry_dev || !ply_dev || !result_dev || !back_dev || !gid_out_dev)
        return fail(BO_E_ARG, "bo_book_insert: null argument");
    BookArgs a;
    a.pos = (const DPos *)pos_dev; a.capacity = capacity; a.n = n; a.T = T; a.entry = entry_dev; a.ply = ply_dev; a.result = result_dev;
    a.back = back_dev; a.eval = eval_dev; a.owner = owner_dev; a.first = first_dev; a.cnt = n_dev; a.w = w_dev; a.d = d_dev; a.l = l_dev;
    a.n_eval = n_eval_dev; a.min_ply = min_ply_dev; a.sum_eval = sum_eval_dev; a.gid = gid_out_dev; a.status = status_dev; a.flags = flags;
    RT(RT_LAUNCH(bo_k_book_insert, (int)((n + 63) / 64), stream, a));
    return BO_OK;
}

extern "C" int bo_pgn_after(const void *pos_dev, const int32_t *act_dev, int64_t capacity, int32_t n, const int64_t *idx_dev, void *pos_out_dev,
                            int32_t *move_out_dev, void *stream) {
    if (!pos_dev || !act_dev || capacity < 1 || n < 1 || !idx_dev || (!pos_out_dev && !move_out_dev)) return fail(BO_E_ARG, "bo_pgn_after: bad arguments");
    RT(RT_LAUNCH(bo_k_pgn_after, (n + 63) / 64, stream, (const DPos *)pos_dev, (const int *)act_dev, (long long)capacity, (int)n, (const long long *)idx_dev,
                 (DPos *)pos_out_dev, (int *)move_out_dev));
    return BO_OK;
}

extern "C" int bo_pgn_spans(const bo_pgn *p, int64_t *begin, int64_t *end) {
    if (!p || !begin || !end) return fail(BO_E_ARG, "bo_pgn_spans: bad arguments");
    for (size_t g = 0; g < p->status.size(); g++) { begin[g] = p->span[2 * g]; end[g] = p->span[2 * g + 1]; }
    return BO_OK;
}

// ---- PGN export (bo_san.h) -----------------------------------------------------------------------------------------------------
extern "C" int bo_san_render(int32_t n_games, int32_t n_positions, const int32_t *game_off_dev, const void *positions_dev,
                             const int32_t *moves_dev, void *san_dev, uint8_t *state_dev, int32_t *bad_dev, void *stream) {
    if (n_games < 1 || n_positions < n_games || !game_off_dev || !positions_dev || !moves_dev || !san_dev || !state_dev || !bad_dev)
        return fail(BO_E_ARG, "bo_san_render: bad arguments");
    RT(RT_LAUNCH(bo_k_san_render, n_positions, stream, (const int *)game_off_dev, (int)n_games, (int)n_positions,
                 (const bo_position *)positions_dev, (const int *)moves_dev, (uint64_t *)san_dev, state_dev));
    RT(RT_LAUNCH(bo_k_san_status, n_games, stream, (const int *)game_off_dev, (int)n_positions, (const uint8_t *)state_dev, (int *)bad_dev));
    return BO_OK;
}

// formatting only: the ep field is the position's ep_key, which the device resolved (python-chess Board.fen()'s "legal" e.p.)
extern "C" int bo_position_fen(const bo_position *p, char *out, int32_t cap) {
    if (!p || !out || cap < 1) return fail(BO_E_ARG, "bo_position_fen: bad arguments");
    if (p->ep_key < -1 || p->ep_key > 63) return fail(BO_E_ARG, "bo_position_fen: ep_key must be resolved (-1 or a square)");
    std::string f;
    for (int r = 7; r >= 0; r--) {
        int empty = 0;
        for (int c = 0; c < 8; c++) {
            const uint64_t b = BIT(r * 8 + c);
            int t = -1;
            for (int i = 0; i < 6; i++) if (p->bb[i] & b) t = i;
            if (t < 0) { empty++; continue; }
            if (empty) { f.push_back((char)('0' + empty)); empty = 0; }
            const char l = "pnbrqk"[t];
            f.push_back((p->bb[BB_WHITE] & b) ? (char)(l - 'a' + 'A') : l);
        }
        if (empty) f.push_back((char)('0' + empty));
        if (r) f.push_back('/');
    }
    f += p->turn ? " w " : " b ";
    const size_t c0 = f.size();
    for (int i = 0; i < 4; i++) if (p->castling & (1u << i)) f.push_back("KQkq"[i]);
    if (f.size() == c0) f.push_back('-');
    f.push_back(' ');
    if (p->ep_key >= 0) { f.push_back((char)('a' + (p->ep_key & 7))); f.push_back((char)('1' + (p->ep_key >> 3))); }
    else f.push_back('-');
    f += " " + std::to_string(p->halfmove_clock) + " " + std::to_string(p->fullmove_number);
    if ((int64_t)f.size() + 1 > cap) return fail(BO_E_ARG, "bo_position_fen: buffer too small");
    memcpy(out, f.c_str(), f.size() + 1);
    return BO_OK;
}

extern "C" int bo_pgn_movetext(int32_t n_plies, const void *san, const uint8_t *state, int32_t root_turn, int32_t root_fullmove,
                               const uint8_t *comments, const char *result, char *out, int64_t cap, int64_t *len_out) {
    if (n_plies < 0 || (n_plies && !san) || !state || !result || !out || !len_out) return fail(BO_E_ARG, "bo_pgn_movetext: bad arguments");
    std::string t;
    if (!pgn_movetext(n_plies, (const uint8_t *)san, state, root_turn != 0, root_fullmove, comments, result, &t))
        return fail(BO_E_ARG, "bo_pgn_movetext: a ply has no SAN");
    *len_out = (int64_t)t.size();
    if ((int64_t)t.size() > cap) return fail(BO_E_ARG, "bo_pgn_movetext: buffer too small");
    memcpy(out, t.data(), t.size());
    return BO_OK;
}

extern "C" int bo_pgn_movetext_text(int32_t n_plies, const void *san, const uint8_t *state, int32_t root_turn, int32_t root_fullmove,
                                    const char *text, const int32_t *text_off, const char *final_comment, const char *result, char *out,
                                    int64_t cap, int64_t *len_out) {
    if (n_plies < 0 || (n_plies && !san) || !state || !result || !out || !len_out || (text && !text_off))
        return fail(BO_E_ARG, "bo_pgn_movetext_text: bad arguments");
    if (text)
        for (int i = 0; i < n_plies; i++)
            if (text_off[i] < 0 || text_off[i + 1] < text_off[i]) return fail(BO_E_ARG, "bo_pgn_movetext_text: text_off is not increasing");
    std::string t;
    if (!pgn_movetext(n_plies, (const uint8_t *)san, state, root_turn != 0, root_fullmove, nullptr, result, &t, text, text_off, final_comment))
        return fail(BO_E_ARG, "bo_pgn_movetext_text: a ply has no SAN");
    *len_out = (int64_t)t.size();
    if ((int64_t)t.size() > cap) return fail(BO_E_ARG, "bo_pgn_movetext_text: buffer too small");
    memcpy(out, t.data(), t.size());
    return BO_OK;
}

// ---- the sparse-target training loss (bo_train.h) and the validation metrics (bo_metrics.h) --------------------------------------
// Calls f with a null pointer of the storage type of a BO_DTYPE_* code; false for an unknown code.
template <class F> static bool train_dtype(int dt, F &&f) {
    switch (dt) {
    case BO_DTYPE_FLOAT32: f((float *)nullptr); return true;
    case BO_DTYPE_BFLOAT16: f((bo_bf16 *)nullptr); return true;
#if !defined(BO_WAVE_EMU)  // (the emulator's host compiler has no _Float16)
    case BO_DTYPE_FLOAT16: f((_Float16 *)nullptr); return true;
#endif
    }
    return false;
}

// The one path of the five entry points below: the arguments they share and the entry point's own (extra_ok), then
// row(TL *, TV *) launches the row kernel of the dtype pair (two null pointers that carry the types), reduce() the kernel behind it.
// A bad argument wins over an unsupported dtype.
template <class Row, class Reduce>
static int train_launch(const char *who, int32_t n, int32_t W, const void *logits, int32_t logits_dtype, const void *value, int32_t value_dtype,
                        const int32_t *pi_idx, const float *pi_val, const float *z, const void *row_out, bool extra_ok, Row &&row,
                        Reduce &&reduce) {
    if (n < 1 || W < 1 || W > BO_RES_CAP || !logits || !value || !pi_idx || !pi_val || !z || !row_out || !extra_ok)
        return fail(BO_E_ARG, std::string(who) + ": bad arguments");
    int rc = 0;
    bool ok = false;
    train_dtype(logits_dtype, [&](auto *tl) { ok = train_dtype(value_dtype, [&](auto *tv) { rc = row(tl, tv); }); });
    if (!ok) return fail(BO_E_CONFIG, std::string(who) + ": unsupported dtype");
    if (!rc) rc = reduce();
    if (rc) return fail(BO_E_HIP, std::string(who) + ": " + rt_errstr(rc));
    return BO_OK;
}
#define BO_TRAIN_TYPES(tl, tv) typedef std::remove_pointer_t<decltype(tl)> TL; typedef std::remove_pointer_t<decltype(tv)> TV

extern "C" int bo_train_loss_forward(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                                     const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, float *row_stats_dev, float *loss3_dev,
                                     void *stream) {
    return train_launch(
        "bo_train_loss_forward", n, W, logits_dev, logits_dtype, value_dev, value_dtype, pi_idx_dev, pi_val_dev, z_dev, row_stats_dev,
        loss3_dev != nullptr,
        [&](auto *tl, auto *tv) {
            BO_TRAIN_TYPES(tl, tv);
            return RT_LAUNCH((bo_k_loss_fwd<TL, TV>), n, stream, (int)W, (const TL *)logits_dev, (const TV *)value_dev, (const int *)pi_idx_dev,
                             pi_val_dev, z_dev, row_stats_dev);
        },
        [&] { return RT_LAUNCH(bo_k_loss_reduce, 1, stream, (int)n, (const float *)row_stats_dev, loss3_dev); });
}

extern "C" int bo_train_loss_backward(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                                      const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *row_stats_dev,
                                      const float *grad_out_dev, void *dlogits_dev, void *dvalue_dev, void *stream) {
    return train_launch(
        "bo_train_loss_backward", n, W, logits_dev, logits_dtype, value_dev, value_dtype, pi_idx_dev, pi_val_dev, z_dev, row_stats_dev,
        grad_out_dev && dlogits_dev && dvalue_dev,
        [&](auto *tl, auto *tv) {
            BO_TRAIN_TYPES(tl, tv);
            return RT_LAUNCH((bo_k_loss_bwd<TL, TV>), n, stream, (int)n, (int)W, (const TL *)logits_dev, (const TV *)value_dev, (const int *)pi_idx_dev,
                             pi_val_dev, z_dev, row_stats_dev, grad_out_dev, (TL *)dlogits_dev, (TV *)dvalue_dev);
        },
        [] { return 0; });
}

// The same with the value target t = (1 - a) z + a q (bo_train.h): q [n] and the mix a (one float32) on the device; row_stats [n,6].
extern "C" int bo_train_loss_forward_mix(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev,
                                         int32_t value_dtype, const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev,
                                         const float *q_dev, const float *mix_dev, float *row_stats_dev, float *loss5_dev, void *stream) {
    return train_launch(
        "bo_train_loss_forward_mix", n, W, logits_dev, logits_dtype, value_dev, value_dtype, pi_idx_dev, pi_val_dev, z_dev, row_stats_dev,
        q_dev && mix_dev && loss5_dev,
        [&](auto *tl, auto *tv) {
            BO_TRAIN_TYPES(tl, tv);
            return RT_LAUNCH((bo_k_loss_fwd_mix<TL, TV>), n, stream, (int)W, (const TL *)logits_dev, (const TV *)value_dev, (const int *)pi_idx_dev,
                             pi_val_dev, z_dev, q_dev, mix_dev, row_stats_dev);
        },
        [&] { return RT_LAUNCH(bo_k_loss_reduce_mix, 1, stream, (int)n, (const float *)row_stats_dev, mix_dev, loss5_dev); });
}

extern "C" int bo_train_loss_backward_mix(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev,
                                          int32_t value_dtype, const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev,
                                          const float *q_dev, const float *mix_dev, const float *row_stats_dev, const float *grad_out_dev,
                                          void *dlogits_dev, void *dvalue_dev, void *stream) {
    return train_launch(
        "bo_train_loss_backward_mix", n, W, logits_dev, logits_dtype, value_dev, value_dtype, pi_idx_dev, pi_val_dev, z_dev, row_stats_dev,
        q_dev && mix_dev && grad_out_dev && dlogits_dev && dvalue_dev,
        [&](auto *tl, auto *tv) {
            BO_TRAIN_TYPES(tl, tv);
            return RT_LAUNCH((bo_k_loss_bwd_mix<TL, TV>), n, stream, (int)n, (int)W, (const TL *)logits_dev, (const TV *)value_dev,
                             (const int *)pi_idx_dev, pi_val_dev, z_dev, q_dev, mix_dev, row_stats_dev, grad_out_dev, (TL *)dlogits_dev,
                             (TV *)dvalue_dev);
        },
        [] { return 0; });
}

// Held-out validation metrics (bo_metrics.h): a record per row, then the rows of every bucket added into accum.
extern "C" int bo_train_metrics(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                                const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *q_dev,
                                const int32_t *bucket_dev, int32_t n_buckets, float *rows_dev, double *accum_dev, void *stream) {
    return train_launch(
        "bo_train_metrics", n, W, logits_dev, logits_dtype, value_dev, value_dtype, pi_idx_dev, pi_val_dev, z_dev, rows_dev,
        n_buckets >= 1 && accum_dev,
        [&](auto *tl, auto *tv) {
            BO_TRAIN_TYPES(tl, tv);
            return RT_LAUNCH((bo_k_metrics_rows<TL, TV>), n, stream, (int)W, (const TL *)logits_dev, (const TV *)value_dev, (const int *)pi_idx_dev,
                             pi_val_dev, z_dev, q_dev, rows_dev);
        },
        [&] { return RT_LAUNCH(bo_k_metrics_reduce, n_buckets, stream, (int)n, (const float *)rows_dev, (const int *)bucket_dev, accum_dev); });
}

// ---- introspection -----------------------------------------------------------------------------------------
extern "C" int bo_debug_search_state(bo_engine *e, int32_t *out, void *stream) {
    if (!e || !out) return fail(BO_E_ARG, "bad arguments");
    if (e->fast) return fail(BO_E_CONFIG, "bo_debug_search_state: reference-semantics engines only");
    const size_t G = (size_t)e->d.c.G;
    const int *src[5] = {e->d.phase, e->d.sims_done, e->d.rows, e->d.req_node, e->d.n_nodes};
    for (int k = 0; k < 5; k++) RT(rt_d2h(out + k * G, src[k], G * 4, stream));
    RT(rt_sync(stream));
    return BO_OK;
}

extern "C" int bo_debug_tree(bo_engine *e, int slot, bo_node *out, int32_t cap, int32_t *n_nodes, void *stream) {
    if (!e || slot < 0 || slot >= e->d.c.G || !n_nodes) return fail(BO_E_ARG, "bad arguments");
    const EngCfg &c = e->d.c;
    int nn = 0;
    RT(rt_d2h(&nn, e->d.n_nodes + slot, 4, stream));
    RT(rt_sync(stream));
    if (e->fast) {  // child-block arena (bo_fastw.h): nodes in breadth-first order, children in record order
        const FastW &f = e->f;
        int head[FWC_HEAD];
        RT(rt_d2h(head, f.ctl + (size_t)slot * f.CS, sizeof(head), stream));
        RT(rt_sync(stream));
        const int cur = head[FWC_CUR], top = head[FWC_TOP];
        std::vector<WRec> A((size_t)top * BO_FW_GR);
        std::vector<bo_mv> M((size_t)top * BO_FW_GR);
        const size_t aoff = ((size_t)slot * 2 + (size_t)cur) * (size_t)f.NG * BO_FW_GR;
        RT(rt_d2h(A.data(), f.arena + aoff, A.size() * sizeof(WRec), stream));
        RT(rt_d2h(M.data(), f.amove + aoff, M.size() * sizeof(bo_mv), stream));
        RT(rt_sync(stream));
        std::vector<bo_node> nodes;
        std::vector<int> rec;  // record id of each node
        auto push = [&](int r, int parent) {
            bo_node nd;
            nd.parent = parent; nd.n_visits = A[r].n; nd.first_child = 0; nd.n_children = 0; nd.q_value = A[r].w; nd.prior = A[r].prior;
            nd.move = r == 0 ? 0 : M[r];
            nd.terminal = A[r].link == FW_MATE ? 1 : A[r].link == FW_DRAW ? 2 : A[r].link >= 0 ? 0 : -1;
            nodes.push_back(nd); rec.push_back(r);
        };
        push(0, -1);
        for (size_t i = 0; i < nodes.size(); i++) {
            const int link = A[rec[i]].link;
            if (link < 0) continue;
            const int first = link & BO_FW_LINK_MASK, ng = ((link >> 24) & 127) + 1;
            if (first < 1 + BO_FW_HG || (size_t)(first + ng) * BO_FW_GR > A.size()) return fail(BO_E_HIP, "corrupt child-run link");
            nodes[i].first_child = (int)nodes.size();
            for (int k = 0; k < ng * BO_FW_GR; k++)
                if (A[(size_t)first * BO_FW_GR + k].n >= 0) { push(first * BO_FW_GR + k, (int)i); nodes[i].n_children++; }
        }
        *n_nodes = (int)nodes.size();
        if (!out) return BO_OK;
        if ((int)nodes.size() > cap) return fail(BO_E_ARG, "tree buffer too small");
        memcpy(out, nodes.data(), nodes.size() * sizeof(bo_node));
        return BO_OK;
    }
    *n_nodes = nn;
    if (!out) return BO_OK;
    if (nn > cap) return fail(BO_E_ARG, "tree buffer too small");
    const size_t off = (size_t)slot * c.NCAP, N = (size_t)nn;
    std::vector<int> nv(N), pa(N), fc(N), nc(N);
    std::vector<float> q(N), pr(N);
    std::vector<bo_mv> mv(N);
    std::vector<signed char> tm(N);
    RT(rt_d2h(nv.data(), e->d.n_visits + off, N * 4, stream)); RT(rt_d2h(pa.data(), e->d.parent + off, N * 4, stream));
    RT(rt_d2h(fc.data(), e->d.first_child + off, N * 4, stream)); RT(rt_d2h(nc.data(), e->d.n_children + off, N * 4, stream));
    RT(rt_d2h(q.data(), e->d.q + off, N * 4, stream)); RT(rt_d2h(pr.data(), e->d.prior + off, N * 4, stream));
    RT(rt_d2h(mv.data(), e->d.move + off, N * sizeof(bo_mv), stream)); RT(rt_d2h(tm.data(), e->d.term + off, N, stream));
    RT(rt_sync(stream));
    for (size_t i = 0; i < N; i++) {
        out[i].parent = pa[i]; out[i].n_visits = nv[i]; out[i].first_child = fc[i]; out[i].n_children = nc[i];
        out[i].q_value = q[i]; out[i].prior = pr[i]; out[i].move = mv[i]; out[i].terminal = tm[i];
    }
    return BO_OK;
}

extern "C" int bo_debug_fast(bo_engine *e, int slot, int32_t *ctl_out, int32_t ctl_cap, int32_t *paths_out, void *stream) {
    if (!e || slot < 0 || slot >= e->d.c.G) return fail(BO_E_ARG, "bad arguments");
    if (!e->fast) return fail(BO_E_CONFIG, "bo_debug_fast: fast-mode engines only");
    const FastW &f = e->f;
    if (ctl_out) {
        if (ctl_cap < f.CS) return fail(BO_E_ARG, "control block buffer too small");
        RT(rt_d2h(ctl_out, f.ctl + (size_t)slot * f.CS, (size_t)f.CS * 4, stream));
    }
    std::vector<int32_t> dm;  // the device keeps the path rows depth-major (FW_PIDX); this call hands them out simulation-major [L][PATH_CAP] as it always has
    if (paths_out) {
        dm.resize((size_t)f.L * BO_FW_PATH_CAP);
        RT(rt_d2h(dm.data(), f.sim_path + (size_t)slot * f.L * BO_FW_PATH_CAP, dm.size() * 4, stream));
    }
    RT(rt_sync(stream));
    if (paths_out)
        for (int s = 0; s < f.L; s++)
            for (int d = 0; d < BO_FW_PATH_CAP; d++) paths_out[(size_t)s * BO_FW_PATH_CAP + d] = dm[FW_PIDX(f.L, s, d)];
    return BO_OK;
}

extern "C" int bo_fast_options(bo_engine *e, int32_t tree_reuse, int32_t games_per_halfwave, int32_t select_flags) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (!e->fast) return fail(BO_E_CONFIG, "bo_fast_options: fast-mode engines only");
    if (games_per_halfwave >= 0 && games_per_halfwave != 1 && games_per_halfwave != 2 && games_per_halfwave != 4)
        return fail(BO_E_ARG, "bo_fast_options: games_per_halfwave must be 1, 2 or 4");
    if (tree_reuse >= 0) e->fast_reuse = tree_reuse ? 1 : 0;
    if (games_per_halfwave >= 0) e->f.sel_ut = games_per_halfwave == 1 ? 2 : games_per_halfwave;  // (one game per half-wave is the form for more than 16 leaves per step)
    if (select_flags >= 0) e->f.sel_flags = select_flags & (FW_SEL_NT | FW_SEL_ROOT_IN_REGS | FW_SEL_DENSE | FW_SEL_LANE | FW_SEL_OCT | FW_SEL_QUAD);
    return BO_OK;
}

#if !defined(BO_WAVE_EMU)
__global__ void bo_k_nothing() {}
#endif
extern "C" int bo_event_pair_overhead(double *ms_out, int32_t samples, void *stream) {
    if (!ms_out || samples < 1 || samples > 256) return fail(BO_E_ARG, "bad arguments");
#if defined(BO_WAVE_EMU)
    (void)stream;
    *ms_out = 0.0;
    return BO_OK;
#else
    hipEvent_t e0, e1;
    RT((int)hipEventCreate(&e0));
    RT((int)hipEventCreate(&e1));
    // pair around ONE empty kernel = overhead + one empty kernel; around TWO = overhead + two: overhead = 2 * p1 - p2
    std::vector<float> v[2];
    int rc = 0;
    for (int i = 0; i < samples + 4 && !rc; i++) {  // (the first few launches load the code object and warm the queue)
        for (int k = 0; k < 2 && !rc; k++) {
            rc = (int)hipEventRecord(e0, (hipStream_t)stream);
            for (int j = 0; j <= k; j++) hipLaunchKernelGGL(bo_k_nothing, dim3(1), dim3(64), 0, (hipStream_t)stream);
            if (!rc) rc = (int)hipEventRecord(e1, (hipStream_t)stream);
            if (!rc) rc = (int)hipEventSynchronize(e1);
            float ms = 0.0f;
            if (!rc) rc = (int)hipEventElapsedTime(&ms, e0, e1);
            if (!rc && i >= 4) v[k].push_back(ms);
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    RT(rc);
    std::sort(v[0].begin(), v[0].end());
    std::sort(v[1].begin(), v[1].end());
    const double p1 = v[0][v[0].size() / 2], p2 = v[1][v[1].size() / 2], ov = 2.0 * p1 - p2;
    *ms_out = ov > 0.0 ? ov : 0.0;
    return BO_OK;
#endif
}

extern "C" int bo_fast_stats(bo_engine *e, uint64_t *granules_read, uint64_t *path_nodes, int32_t *arena_granules, int32_t time_select, double *select_ms,
                             int64_t *select_launches, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    if (!e->fast) return fail(BO_E_CONFIG, "bo_fast_stats: fast-mode engines only");
    const size_t G = (size_t)e->d.c.G;
    std::vector<int32_t> tmp(2 * G);
    const size_t pitch = (size_t)e->f.CS * 4;
    if (granules_read) RT(rt_d2h_2d(tmp.data(), 4, e->f.ctl + FWC_GRAN, pitch, 4, G, stream));
    if (path_nodes) RT(rt_d2h_2d(tmp.data() + G, 4, e->f.ctl + FWC_PNODES, pitch, 4, G, stream));
    if (arena_granules) RT(rt_d2h_2d(arena_granules, 4, e->f.ctl + FWC_TOP, pitch, 4, G, stream));
    RT(rt_sync(stream));
    for (size_t g = 0; g < G; g++) {  // (32-bit counters per game on the device: 2^31 granules are 256 GB through one game's select path)
        if (granules_read) granules_read[g] = (uint64_t)(uint32_t)tmp[g];
        if (path_nodes) path_nodes[g] = (uint64_t)(uint32_t)tmp[G + g];
    }
    RT(rt_sync(stream));
#if !defined(BO_WAVE_EMU)
    if (e->sel_pending) {
        float ms = 0.0f;
        RT((int)hipEventSynchronize(e->sel_ev1));
        RT((int)hipEventElapsedTime(&ms, e->sel_ev0, e->sel_ev1));
        e->sel_ms += ms; e->sel_launches++; e->sel_pending = 0;
    }
#endif
    if (select_ms) *select_ms = e->sel_ms;
    if (select_launches) *select_launches = e->sel_launches;
    if (time_select >= 0) {
        if (time_select && !e->sel_profile) { e->sel_ms = 0.0; e->sel_launches = 0; }
        e->sel_profile = time_select ? 1 : 0;
    }
    return BO_OK;
}

extern "C" int bo_engine_status(bo_engine *e, int32_t *status, int32_t *evals, int32_t *flushes, int32_t *term_sims,
                                int32_t *levels, int32_t *children_scanned, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    if (status) RT(rt_d2h(status, e->d.status, G * 4, stream));
    if (evals) RT(rt_d2h(evals, e->d.stat_evals, G * 4, stream));
    if (flushes) RT(rt_d2h(flushes, e->d.stat_flushes, G * 4, stream));
    if (e->fast) {  // the fast mode keeps these counters in the games' control blocks (bo_fastw.h)
        const size_t pitch = (size_t)e->f.CS * 4;
        if (term_sims) RT(rt_d2h_2d(term_sims, 4, e->f.ctl + FWC_TERM, pitch, 4, G, stream));
        if (levels) RT(rt_d2h_2d(levels, 4, e->f.ctl + FWC_LEVELS, pitch, 4, G, stream));
        if (children_scanned) RT(rt_d2h_2d(children_scanned, 4, e->f.ctl + FWC_KIDS, pitch, 4, G, stream));
    } else {
        if (term_sims) RT(rt_d2h(term_sims, e->d.stat_term_sims, G * 4, stream));
        if (levels) RT(rt_d2h(levels, e->d.stat_levels, G * 4, stream));
        if (children_scanned) RT(rt_d2h(children_scanned, e->d.stat_children_scanned, G * 4, stream));
    }
    RT(rt_sync(stream));
    return BO_OK;
}

extern "C" int bo_debug_profile(bo_engine *e, int enable, uint64_t *cycles_out, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    if (cycles_out) {
        RT(rt_d2h(cycles_out, e->d.prof, G * BO_PROF_SLOTS * sizeof(uint64_t), stream));
        RT(rt_sync(stream));
    }
    if (enable >= 0) {
        if (enable && !e->d.c.profile) RT(rt_memset(e->d.prof, 0, G * BO_PROF_SLOTS * sizeof(uint64_t), stream));
        e->d.c.profile = enable;  // 1: every game-step; N > 1: only game-steps longer than N cycles
    }
    return BO_OK;
}

extern "C" int bo_movegen_batch(bo_engine *e, int n, const bo_position *pos, int32_t *moves_out, int32_t *n_out,
                                int32_t *check_out, void *stream) {
    if (!e || n < 1 || !pos || !moves_out || !n_out) return fail(BO_E_ARG, "bad arguments");
    std::vector<DPos> hp((size_t)n);
    for (int i = 0; i < n; i++) hp[i] = from_abi(pos[i]);
    void *dp = nullptr, *dm = nullptr, *dn = nullptr, *dc = nullptr;
    int rc = rt_malloc(&dp, hp.size() * sizeof(DPos)) | rt_malloc(&dm, (size_t)n * BO_MAX_MOVES * sizeof(bo_mv)) |
             rt_malloc(&dn, (size_t)n * 4) | rt_malloc(&dc, (size_t)n * 4);
    std::vector<bo_mv> hm((size_t)n * BO_MAX_MOVES);
    std::vector<int> hc((size_t)n);
    if (!rc) rc = rt_h2d(dp, hp.data(), hp.size() * sizeof(DPos), stream);
    if (!rc) rc = RT_LAUNCH(bo_k_movegen, n, stream, (const DPos *)dp, (bo_mv *)dm, (int *)dn, (int *)dc);
    if (!rc) rc = rt_d2h(hm.data(), dm, hm.size() * sizeof(bo_mv), stream) | rt_d2h(n_out, dn, (size_t)n * 4, stream) |
                  rt_d2h(hc.data(), dc, (size_t)n * 4, stream);
    int rc2 = rt_sync(stream);
    rt_free(dp); rt_free(dm); rt_free(dn); rt_free(dc);
    if (rc || rc2) return fail(BO_E_HIP, std::string("bo_movegen_batch: ") + rt_errstr(rc ? rc : rc2));
    for (size_t i = 0; i < hm.size(); i++) moves_out[i] = hm[i];
    if (check_out) for (int i = 0; i < n; i++) check_out[i] = hc[i];
    return BO_OK;
}

// ---- wide PUCT select (roofline workload; independent of an engine instance) ----------------------------------
extern "C" int bo_select_wide(const void *blocks_dev, const int32_t *root_block_dev, const int32_t *root_n_dev,
                              const float *sqrt_lut_dev, int n_trees, int max_depth, float cpuct, int grid_blocks,
                              int32_t *out_leaf_dev, int32_t *out_levels_dev, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)blocks_dev; (void)root_block_dev; (void)root_n_dev; (void)sqrt_lut_dev; (void)n_trees; (void)max_depth;
    (void)cpuct; (void)grid_blocks; (void)out_leaf_dev; (void)out_levels_dev; (void)stream;
    return fail(BO_E_CONFIG, "bo_select_wide is a gfx950-only kernel");
#else
    if (!blocks_dev || !root_block_dev || !root_n_dev || !sqrt_lut_dev || !out_leaf_dev || !out_levels_dev || n_trees < 1)
        return fail(BO_E_ARG, "bad arguments");
    const int U = 4;  // trees in flight per half-wave (bo_select_wide.h)
    if (grid_blocks < 1) {
        // one workgroup per 8*U trees and no grid-stride tail; measured on MI355X at 262 144 trees: 4096 (strided) 85.9 us,
        // 8192 (exact) 83.1 us, 16384 (half of the workgroups exit at once) 81.3 us -- launch twice the exact grid.
        grid_blocks = 2 * ((n_trees + 8 * U - 1) / (8 * U));
    }
    if (grid_blocks > 65536) grid_blocks = 65536;
    hipLaunchKernelGGL(bo_k_select_wide, dim3((unsigned)grid_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const WideBlock *)blocks_dev, (const int *)root_block_dev, (const int *)root_n_dev, sqrt_lut_dev,
                       n_trees, max_depth, cpuct, (int *)out_leaf_dev, (int *)out_levels_dev);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// ---- fused epilogues of the evaluate stage (bo_nn_fused.h); independent of an engine instance -----------------------
extern "C" int bo_nn_bias_act(float *x_dev, const float *bias_dev, const float *residual_dev, int batch, int channels,
                              void *stream) {
#if defined(BO_WAVE_EMU)
    (void)x_dev; (void)bias_dev; (void)residual_dev; (void)batch; (void)channels; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_bias_act is a gfx950-only kernel");
#else
    if (!x_dev || !bias_dev || batch < 1 || channels < 1) return fail(BO_E_ARG, "bad arguments");
    const long n4 = (long)batch * channels * 16;
    long blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(bo_k_bias_act, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x_dev, bias_dev, residual_dev, n4,
                       channels);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

extern "C" int bo_nn_se_residual(float *x_dev, const float *bias_dev, const float *w1_dev, const float *w2_dev,
                                 const float *residual_dev, int batch, int channels, int hidden, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)x_dev; (void)bias_dev; (void)w1_dev; (void)w2_dev; (void)residual_dev; (void)batch; (void)channels; (void)hidden; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_se_residual is a gfx950-only kernel");
#else
    if (!x_dev || !bias_dev || !w1_dev || !w2_dev || !residual_dev || batch < 1) return fail(BO_E_ARG, "bad arguments");
    if (channels < 1 || channels > BO_SE_MAX_C || hidden < 1 || hidden > BO_SE_MAX_H) return fail(BO_E_CONFIG, "SE block: channels <= 256, hidden <= 32");
    const size_t lds = (size_t)channels * 65 * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void *)bo_k_se_residual, hipFuncAttributeMaxDynamicSharedMemorySize, 256 * 65 * 4);
        attr_set = true;
    }
    hipLaunchKernelGGL(bo_k_se_residual, dim3((unsigned)batch), dim3(256), lds, (hipStream_t)stream, x_dev, bias_dev, w1_dev, w2_dev,
                       residual_dev, channels, hidden);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// small-batch form: the result replaces `residual_inout_dev`, x is only read (bo_nn_fused.h: bo_k_se_residual_small)
extern "C" int bo_nn_se_residual_small(const float *x_dev, const float *bias_dev, const float *w1_dev, const float *w2_dev,
                                       float *residual_inout_dev, int batch, int channels, int hidden, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)x_dev; (void)bias_dev; (void)w1_dev; (void)w2_dev; (void)residual_inout_dev; (void)batch; (void)channels; (void)hidden; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_se_residual_small is a gfx950-only kernel");
#else
    if (!x_dev || !bias_dev || !w1_dev || !w2_dev || !residual_inout_dev || batch < 1 || batch > 65535) return fail(BO_E_ARG, "bad arguments");
    if (channels < 16 || channels > BO_SE_MAX_C || (channels & 15) || hidden < 1 || hidden > 16)
        return fail(BO_E_CONFIG, "small SE block: channels a multiple of 16 <= 256, hidden <= 16");
    hipLaunchKernelGGL(bo_k_se_residual_small, dim3((unsigned)(channels / 16), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, x_dev, bias_dev,
                       w1_dev, w2_dev, residual_inout_dev, channels, hidden);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// ---- direct 3x3 convolution on the fp32 matrix cores (bo_conv.h); independent of an engine instance ---------------
extern "C" int bo_nn_conv3x3(const float *x_dev, const float *wpacked_dev, const float *bias_dev, const float *residual_dev,
                             float *y_dev, int batch, int c_in, int c_out, int mode, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)x_dev; (void)wpacked_dev; (void)bias_dev; (void)residual_dev; (void)y_dev; (void)batch; (void)c_in; (void)c_out; (void)mode; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_conv3x3 is a gfx950-only kernel");
#else
    if (!x_dev || !wpacked_dev || !bias_dev || !y_dev || batch < 1) return fail(BO_E_ARG, "bad arguments");
    if (mode < 0 || mode > 2 || (mode == 2 && !residual_dev)) return fail(BO_E_ARG, "bad epilogue mode");
    const bo_f32x4 *wp = reinterpret_cast<const bo_f32x4 *>(wpacked_dev);
    hipStream_t st = (hipStream_t)stream;
#define BO_CONV_CASE(CI, CO)                                                                                              \
    if (c_in == CI && c_out == CO) {                                                                                      \
        hipLaunchKernelGGL((bo_k_conv3x3<CI, CO>), dim3((unsigned)batch), dim3(CO * 2), 0, st, x_dev, wp, bias_dev, residual_dev, \
                           y_dev, mode);                                                                                  \
        RT((int)hipGetLastError());                                                                                       \
        return BO_OK;                                                                                                     \
    }
    BO_CONV_CASE(120, 64) BO_CONV_CASE(64, 64) BO_CONV_CASE(120, 128) BO_CONV_CASE(128, 128) BO_CONV_CASE(120, 256) BO_CONV_CASE(256, 256)
#undef BO_CONV_CASE
    return fail(BO_E_CONFIG, "bo_nn_conv3x3: supported (c_in, c_out): (120|C, C) for C in {64, 128, 256}");
#endif
}

// ---- the whole residual tower as one persistent kernel (bo_tower.h) ------------------------------------------------
#if !defined(BO_WAVE_EMU)
struct bo_tower_s {
    int channels = 0, n_layers = 0, n_cu = 0, device = 0, algo = 0;
    int head_channels = 0, head_split = 0, head_w_off = 0, head_b_off = 0;
    bo_f32x4 *wts = nullptr;
    float *params = nullptr;
    bo_tower_layer *layers = nullptr;
    int *overflow = nullptr;  // BO_TOWER_SPLIT_F16: an activation left the fp16 range
    int64_t n_weights = 0, n_params = 0;
    std::vector<bo_tower_layer_desc> host_layers;  // (bo_nn_tower_pair_check compares two towers' descriptors)
};
#else
struct bo_tower_s { int unused; };
#endif

extern "C" int bo_nn_tower_create(const bo_tower_layer_desc *layers, int n_layers, const float *weights, int64_t n_weights,
                                  const float *params, int64_t n_params, int channels, int algo, const bo_tower_head_desc *head, int device,
                                  bo_tower **out) {
#if defined(BO_WAVE_EMU)
    (void)head; (void)algo; (void)layers; (void)n_layers; (void)weights; (void)n_weights; (void)params; (void)n_params; (void)channels; (void)device; (void)out;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    static_assert(sizeof(bo_tower_layer_desc) == sizeof(bo_tower_layer), "descriptor layouts must agree");
    if (!layers || !weights || !params || !out || n_layers < 1 || n_layers > 4096) return fail(BO_E_ARG, "bad arguments");
    const bool split_w = algo == BO_TOWER_SPLIT_F16 || algo == BO_TOWER_SPLIT_F16_T16;
    const bool f16_w = algo == BO_TOWER_DIRECT_F16 || algo == BO_TOWER_DIRECT_F16_T16;
    const bool half_w = f16_w || split_w;  // fp16 weight fragments, 16-byte offsets
    if (half_w ? (channels != 128 && channels != 256) : (channels != 64 && channels != 128))
        return fail(BO_E_CONFIG, "bo_nn_tower: channels must be 64 or 128 (fp32: two padded images per board in LDS) or 128 / 256 (BO_TOWER_DIRECT_F16, BO_TOWER_SPLIT_F16)");
    if (n_weights % 4) return fail(BO_E_ARG, "n_weights must be a multiple of 4");
    if (algo != BO_TOWER_DIRECT && algo != BO_TOWER_WINOGRAD && !half_w) return fail(BO_E_ARG, "unknown algo");
    if (algo == BO_TOWER_SPLIT_F16_T16 && channels != 128) return fail(BO_E_CONFIG, "BO_TOWER_SPLIT_F16_T16: 128 filters (other widths: BO_TOWER_SPLIT_F16)");
    if (f16_w && !head) return fail(BO_E_ARG, "BO_TOWER_DIRECT_F16 needs the fused head (it has no tower output buffer)");
    const int C = channels;
    const int split = split_w ? 2 : 1;  // (hi, lo) fragment pairs; one more float (the inverse weight scale) behind every bias
    for (int l = 0; l < n_layers; l++) {  // every offset the kernel will form stays inside the two buffers
        const bo_tower_layer_desc &L = layers[l];
        // K steps per layer: direct = groups of 8 input channels, Winograd = groups of 4; the input conv is padded to 128
        const int cin = L.kind == 0 ? 128 : C;
        const int want_t4 = algo == BO_TOWER_DIRECT ? cin / 8 : algo == BO_TOWER_WINOGRAD ? cin / 4 : 9 * cin / 16;
        const int64_t w4 = algo == BO_TOWER_DIRECT ? (int64_t)9 * want_t4 * C * 2
                           : algo == BO_TOWER_WINOGRAD ? (int64_t)want_t4 * (C / 16) * 4 * 64 : (int64_t)want_t4 * (C / 32) * 64 * split;
        if (L.kind < 0 || L.kind > 3 || (l == 0) != (L.kind == 0)) return fail(BO_E_ARG, "layer " + std::to_string(l) + ": bad kind");
        if (L.kind == 1 && (l + 1 >= n_layers || layers[l + 1].kind < 2)) return fail(BO_E_ARG, "a first conv must be followed by a second conv");
        if (L.kind >= 2 && layers[l - 1].kind != 1) return fail(BO_E_ARG, "a second conv must follow a first conv");
        if (L.t4 != want_t4) return fail(BO_E_ARG, "layer " + std::to_string(l) + ": t4 must be " + std::to_string(want_t4));
        if (L.w_off4 < 0 || ((int64_t)L.w_off4 + w4) * 4 > n_weights) return fail(BO_E_ARG, "weights offset out of range");
        if (L.bias_off < 0 || (int64_t)L.bias_off + C + (split - 1) > n_params) return fail(BO_E_ARG, "bias offset out of range");
        if ((algo == BO_TOWER_WINOGRAD || split_w) && (L.bias_off & 3)) return fail(BO_E_ARG, "BO_TOWER_WINOGRAD / BO_TOWER_SPLIT_F16: bias_off must be a multiple of 4 floats");
        if (L.kind == 3) {
            if (L.hidden < 1 || L.hidden > 16) return fail(BO_E_CONFIG, "SE hidden width must be 1..16");
            if (half_w && L.hidden > C / 16) return fail(BO_E_CONFIG, "fp16-pipe towers: SE hidden width must be <= channels/16");
            if (L.se_w1_off < 0 || (int64_t)L.se_w1_off + (int64_t)L.hidden * C > n_params || L.se_w2_off < 0 ||
                (int64_t)L.se_w2_off + (int64_t)L.hidden * C > n_params)
                return fail(BO_E_ARG, "SE weight offset out of range");
        }
        if ((L.last != 0) != (l == n_layers - 1)) return fail(BO_E_ARG, "exactly the final layer stores the output");
    }
    if (layers[n_layers - 1].kind < 2) return fail(BO_E_ARG, "the tower must end with a second conv");
    if (head) {
        if (algo == BO_TOWER_DIRECT) return fail(BO_E_CONFIG, "fused head convolutions need BO_TOWER_WINOGRAD, BO_TOWER_DIRECT_F16 or BO_TOWER_SPLIT_F16");
        if (head->channels < 1 || head->channels > 256 || head->split < 0 || head->split > head->channels) return fail(BO_E_ARG, "bad head channels/split");
        if (head->b_off < 0 || (int64_t)head->b_off + head->channels + (split - 1) > n_params) return fail(BO_E_ARG, "head bias offset out of range");
        if (algo == BO_TOWER_WINOGRAD) {
            if (head->w_off < 0 || (head->w_off & 3) || (int64_t)head->w_off + (int64_t)((head->channels + 15) / 16) * 16 * C > n_params)
                return fail(BO_E_ARG, "head weight offset out of range");
        } else if (head->w_off < 0 || ((int64_t)head->w_off + (int64_t)((head->channels + 31) / 32) * (C / 16) * 64 * split) * 4 > n_weights) {
            return fail(BO_E_ARG, "head weight offset out of range");
        }
    }
    RT(rt_set_device(device));
    hipDeviceProp_t prop;
    RT((int)hipGetDeviceProperties(&prop, device));
    bo_tower_s *t = new bo_tower_s();
    t->channels = C; t->n_layers = n_layers; t->n_cu = prop.multiProcessorCount; t->device = device; t->algo = algo;
    if (head) { t->head_channels = head->channels; t->head_split = head->split; t->head_w_off = head->w_off; t->head_b_off = head->b_off; }
    t->n_weights = n_weights; t->n_params = n_params;
    t->host_layers.assign(layers, layers + n_layers);
    int rc = (int)hipMalloc((void **)&t->wts, (size_t)n_weights * 4);
    if (!rc) rc = (int)hipMalloc((void **)&t->params, (size_t)n_params * 4);
    if (!rc) rc = (int)hipMalloc((void **)&t->layers, (size_t)n_layers * sizeof(bo_tower_layer));
    if (!rc) rc = (int)hipMalloc((void **)&t->overflow, 8);  // [status word | scratch of bo_nn_tower_status's exchange]
    if (!rc) rc = (int)hipMemset(t->overflow, 0, 8);
    if (!rc) rc = (int)hipMemcpy(t->wts, weights, (size_t)n_weights * 4, hipMemcpyHostToDevice);
    if (!rc) rc = (int)hipMemcpy(t->params, params, (size_t)n_params * 4, hipMemcpyHostToDevice);
    if (!rc) rc = (int)hipMemcpy(t->layers, layers, (size_t)n_layers * sizeof(bo_tower_layer), hipMemcpyHostToDevice);
    if (rc) {
        (void)hipFree(t->wts); (void)hipFree(t->params); (void)hipFree(t->layers); (void)hipFree(t->overflow);
        delete t;
        return fail(BO_E_HIP, std::string("bo_nn_tower_create: ") + rt_errstr(rc));
    }
    *out = t;
    return BO_OK;
#endif
}

// Rate (kHz) of the constant-rate clock the in-kernel timings are taken with (wall_clock64: hipDeviceAttributeWallClockRate).
extern "C" int bo_device_wall_clock_khz(int device, int32_t *khz_out) {
#if defined(BO_WAVE_EMU)
    (void)device; (void)khz_out;
    return fail(BO_E_CONFIG, "gfx950 only");
#else
    if (!khz_out) return fail(BO_E_ARG, "null argument");
    int v = 0;
    RT((int)hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, device));
    *khz_out = v;
    return BO_OK;
#endif
}

static int tower_forward_impl(bo_tower *t, const float *x_dev, float *y_dev, void *head_a_dev, void *head_b_dev, int batch, void *timing_dev, void *stream);
extern "C" int bo_nn_tower_forward(bo_tower *t, const float *x_dev, float *y_dev, void *head_a_dev, void *head_b_dev, int batch,
                                   void *stream) {
    return tower_forward_impl(t, x_dev, y_dev, head_a_dev, head_b_dev, batch, nullptr, stream);
}
// The same launch with its duration noted by the kernel itself in `timing_dev` (BO_TOWER_SPLIT_F16 only): uint64 [seq | arrivals |
// start[4096] | end[4096]], zeroed by the caller; launch k made with this buffer leaves its first workgroup's start and its last
// workgroup's end in slot k % 4096 (units: the device's constant-rate clock, hipDeviceAttributeWallClockRate kHz).  One launch per
// buffer at a time (launches of one stream).  For measurements inside captured graphs, where no event pair fits between two nodes.
extern "C" int bo_nn_tower_forward_timed(bo_tower *t, const float *x_dev, float *y_dev, void *head_a_dev, void *head_b_dev, int batch,
                                         void *timing_dev, void *stream) {
    return tower_forward_impl(t, x_dev, y_dev, head_a_dev, head_b_dev, batch, timing_dev, stream);
}
static int tower_forward_impl(bo_tower *t, const float *x_dev, float *y_dev, void *head_a_dev, void *head_b_dev, int batch, void *timing_dev, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)x_dev; (void)y_dev; (void)head_a_dev; (void)head_b_dev; (void)batch; (void)stream; (void)timing_dev;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    if (!t || !x_dev || batch < 1) return fail(BO_E_ARG, "bad arguments");
    bo_tower_head hd;
    if (t->head_channels > 0) {
        if ((t->head_split > 0 && !head_a_dev) || (t->head_split < t->head_channels && !head_b_dev)) return fail(BO_E_ARG, "head output buffers missing");
        hd.channels = t->head_channels; hd.split = t->head_split; hd.w_off = t->head_w_off; hd.b_off = t->head_b_off;
        hd.out_a = (float *)head_a_dev; hd.out_b = (float *)head_b_dev;
    } else if (!y_dev) {
        return fail(BO_E_ARG, "y_dev is required for a tower without fused heads");
    }
    const int slots = t->n_cu * (t->channels == 64 && t->algo == BO_TOWER_DIRECT ? 2 : 1);  // direct, 64 filters: two 2-wave workgroups share a CU
    const unsigned grid = (unsigned)(batch < slots ? batch : slots);
    hipStream_t st = (hipStream_t)stream;
    if (t->algo == BO_TOWER_DIRECT_F16 || t->algo == BO_TOWER_DIRECT_F16_T16) {  // two boards per workgroup
        bo_tower_head_h hh;
        hh.channels = t->head_channels; hh.split = t->head_split; hh.w_off8 = t->head_w_off; hh.b_off = t->head_b_off;
        hh.out_a = (_Float16 *)head_a_dev; hh.out_b = (_Float16 *)head_b_dev;
        const int pairs = (batch + 1) / 2;
        const unsigned g2 = (unsigned)(pairs < t->n_cu ? pairs : t->n_cu);
        const bo_h8 *w8 = reinterpret_cast<const bo_h8 *>(t->wts);
        static const int ar_h16 = [] { const char *v = getenv("BETAONE_TOWER_H16_AR"); return (v && atoi(v) == 6) ? 6 : 3; }();  // (LAB: ring depth of the 256-filter instance)
        if (t->algo == BO_TOWER_DIRECT_F16_T16 && t->channels == 256 && ar_h16 == 6) hipLaunchKernelGGL((bo_k_tower_h16<256, 2, 6>), dim3(g2), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, batch, hh);
        else if (t->algo == BO_TOWER_DIRECT_F16_T16 && t->channels == 256) hipLaunchKernelGGL((bo_k_tower_h16<256, 2, 3>), dim3(g2), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, batch, hh);
        else if (t->algo == BO_TOWER_DIRECT_F16_T16) hipLaunchKernelGGL((bo_k_tower_h16<128, 1>), dim3(g2), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, batch, hh);
        else if (t->channels == 256) hipLaunchKernelGGL((bo_k_tower_h<256, 2>), dim3(g2), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, batch, hh);
        else hipLaunchKernelGGL((bo_k_tower_h<128, 1>), dim3(g2), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, batch, hh);
        RT((int)hipGetLastError());
        return BO_OK;
    }
    if (t->algo == BO_TOWER_SPLIT_F16 || t->algo == BO_TOWER_SPLIT_F16_T16) {  // float32 in and out, fp16 (hi, lo) pairs on the matrix pipe; one board per workgroup
        bo_tower_head_s hs;
        hs.channels = t->head_channels; hs.split = t->head_split; hs.w_off8 = t->head_w_off; hs.b_off = t->head_b_off;
        hs.out_a = (float *)head_a_dev; hs.out_b = (float *)head_b_dev; hs.overflow = t->overflow;
        hs.timing = (unsigned long long *)timing_dev;
        const bo_h8 *w8 = reinterpret_cast<const bo_h8 *>(t->wts);
        // 256 filters: two tiles per wave double every register set.  Weight fragments 8 K-steps ahead: 41 spilled registers (160 B of
        // scratch); 4 ahead: none, and as fast (1 667-1 672 us against 1 678-1 679 per 256 boards, same box: profiles/r04_tower256_ring.md).
        // BETAONE_TOWER256_AR=8 keeps the old instance selectable for A/B runs.
        static const int ar256 = [] { const char *v = getenv("BETAONE_TOWER256_AR"); return (v && v[0] == '8') ? 8 : 4; }();
        if (t->algo == BO_TOWER_SPLIT_F16_T16)  // the same products as 16x16x32 tiles (bo_tower_s16.h: the chip holds a higher clock under them)
            // (weight fragments 6 K-steps = 24 KiB per wave ahead; 12 ahead needs all 512 registers + 12 spilled and measured 185 us
            // against 179 for a lone 64-board launch: profiles/r05_device_turn_and_tiles.md)
            hipLaunchKernelGGL((bo_k_tower_s16<6>), dim3(grid), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, y_dev, batch, hs, bo_tower_pair{});
        else if (t->channels == 256 && ar256 == 8) hipLaunchKernelGGL((bo_k_tower_s<256, 2, 1, 8>), dim3(grid), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, y_dev, batch, hs, bo_tower_pair{});
        else if (t->channels == 256) hipLaunchKernelGGL((bo_k_tower_s<256, 2, 1, 4>), dim3(grid), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, y_dev, batch, hs, bo_tower_pair{});
        else  // (B operands read two K-steps ahead, weight fragments requested twelve ahead: profiles/r03_split_tower.md)
            hipLaunchKernelGGL((bo_k_tower_s<128, 1, 2, 12>), dim3(grid), dim3(256), 0, st, x_dev, w8, t->params, t->layers, t->n_layers, y_dev, batch, hs, bo_tower_pair{});
        RT((int)hipGetLastError());
        return BO_OK;
    }
    if (t->algo == BO_TOWER_WINOGRAD && t->channels == 128)
        hipLaunchKernelGGL((bo_k_tower_wg<128>), dim3(grid), dim3(512), 0, st, x_dev, t->wts, t->params, t->layers, t->n_layers, y_dev, batch, hd);
    else if (t->algo == BO_TOWER_WINOGRAD)
        hipLaunchKernelGGL((bo_k_tower_wg<64>), dim3(grid), dim3(256), 0, st, x_dev, t->wts, t->params, t->layers, t->n_layers, y_dev, batch, hd);
    else if (t->channels == 128)
        hipLaunchKernelGGL((bo_k_tower<128>), dim3(grid), dim3(256), 0, st, x_dev, t->wts, t->params, t->layers, t->n_layers, y_dev, batch);
    else
        hipLaunchKernelGGL((bo_k_tower<64>), dim3(grid), dim3(128), 0, st, x_dev, t->wts, t->params, t->layers, t->n_layers, y_dev, batch);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// ---- two nets in one launch of the split-precision tower (a match: row b evaluated by the net of its game's side to move) --------
extern "C" int bo_nn_tower_pair_check(bo_tower *t0, bo_tower *t1) {
#if defined(BO_WAVE_EMU)
    (void)t0; (void)t1;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    if (!t0 || !t1) return fail(BO_E_ARG, "null tower");
    if (t0->algo != t1->algo || (t0->algo != BO_TOWER_SPLIT_F16 && t0->algo != BO_TOWER_SPLIT_F16_T16))
        return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: both towers must be BO_TOWER_SPLIT_F16 or both BO_TOWER_SPLIT_F16_T16");
    if (t0->device != t1->device) return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: the two towers live on different devices");
    if (t0->channels != t1->channels || t0->n_layers != t1->n_layers || t0->n_weights != t1->n_weights || t0->n_params != t1->n_params)
        return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: the two towers differ in channels, layers or buffer sizes");
    if (t0->head_channels != t1->head_channels || t0->head_split != t1->head_split || t0->head_w_off != t1->head_w_off || t0->head_b_off != t1->head_b_off)
        return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: the two towers' head descriptors differ");
    if (t0->head_channels == 0) return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: the towers need their fused head convolutions");
    if (memcmp(t0->host_layers.data(), t1->host_layers.data(), t0->host_layers.size() * sizeof(bo_tower_layer_desc)) != 0)
        return fail(BO_E_CONFIG, "bo_nn_tower_forward_pair: the two towers' layer descriptors differ");
    return BO_OK;
#endif
}

extern "C" int bo_nn_tower_forward_pair(bo_tower *t0, bo_tower *t1, const int32_t *sel_dev, const float *x_dev, void *head_a_dev,
                                        void *head_b_dev, int batch, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)t0; (void)t1; (void)sel_dev; (void)x_dev; (void)head_a_dev; (void)head_b_dev; (void)batch; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    if (int rc = bo_nn_tower_pair_check(t0, t1)) return rc;
    if (!sel_dev || !x_dev || batch < 1) return fail(BO_E_ARG, "bad arguments");
    if ((t0->head_split > 0 && !head_a_dev) || (t0->head_split < t0->head_channels && !head_b_dev)) return fail(BO_E_ARG, "head output buffers missing");
    bo_tower_head_s hs;
    hs.channels = t0->head_channels; hs.split = t0->head_split; hs.w_off8 = t0->head_w_off; hs.b_off = t0->head_b_off;
    hs.out_a = (float *)head_a_dev; hs.out_b = (float *)head_b_dev; hs.overflow = t0->overflow;
    bo_tower_pair pr;
    pr.sel = sel_dev; pr.wts1 = reinterpret_cast<const bo_h8 *>(t1->wts); pr.params1 = t1->params; pr.overflow1 = t1->overflow;
    const unsigned grid = (unsigned)(batch < t0->n_cu ? batch : t0->n_cu);
    hipStream_t st = (hipStream_t)stream;
    const bo_h8 *w8 = reinterpret_cast<const bo_h8 *>(t0->wts);
    // the single-net launch's instances with PAIR = true (bo_nn_tower_forward: why these ring depths)
    if (t0->algo == BO_TOWER_SPLIT_F16_T16)
        hipLaunchKernelGGL((bo_k_tower_s16<6, true>), dim3(grid), dim3(256), 0, st, x_dev, w8, t0->params, t0->layers, t0->n_layers, nullptr, batch, hs, pr);
    else if (t0->channels == 256)
        hipLaunchKernelGGL((bo_k_tower_s<256, 2, 1, 4, true>), dim3(grid), dim3(256), 0, st, x_dev, w8, t0->params, t0->layers, t0->n_layers, nullptr, batch, hs, pr);
    else
        hipLaunchKernelGGL((bo_k_tower_s<128, 1, 2, 12, true>), dim3(grid), dim3(256), 0, st, x_dev, w8, t0->params, t0->layers, t0->n_layers, nullptr, batch, hs, pr);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

extern "C" void bo_nn_tower_destroy(bo_tower *t) {
#if !defined(BO_WAVE_EMU)
    if (!t) return;
    (void)hipFree(t->wts); (void)hipFree(t->params); (void)hipFree(t->layers); (void)hipFree(t->overflow);
#endif
    delete t;
}

#if !defined(BO_WAVE_EMU)
__global__ void bo_k_word_exchange(int *word, int *out) { *out = atomicExch(word, 0); }
#endif

// Read AND clear the tower's status word in one atomic exchange on `stream` -- the stream the tower is launched on: ordered behind
// the forwards it reports on, and a forward that sets the word while it is being read is not lost between a copy and a memset.
extern "C" int bo_nn_tower_status(bo_tower *t, int32_t *overflow_out, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)overflow_out; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    if (!t || !overflow_out) return fail(BO_E_ARG, "bad arguments");
    hipLaunchKernelGGL(bo_k_word_exchange, dim3(1), dim3(1), 0, (hipStream_t)stream, t->overflow, t->overflow + 1);
    RT((int)hipGetLastError());
    RT(rt_d2h(overflow_out, t->overflow + 1, 4, stream));
    RT(rt_sync(stream));
    return BO_OK;
#endif
}

// Device address of the tower's status word (non-zero: an activation left the fp16 range), for bo_engine_watch.
extern "C" int bo_nn_tower_word(bo_tower *t, void **dev_word_out) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)dev_word_out;
    return fail(BO_E_CONFIG, "bo_nn_tower is a gfx950-only kernel");
#else
    if (!t || !dev_word_out) return fail(BO_E_ARG, "bad arguments");
    *dev_word_out = t->overflow;
    return BO_OK;
#endif
}

// ---- the tower of one board (a few boards) as ONE launch spread over the chip (bo_tower_b1.h): uci.py's batch-1 evaluations ------
struct bo_b1_s {
#if !defined(BO_WAVE_EMU)
    int device = 0, C = 0, n_layers = 0, max_batch = 0;
    bool split = false;             // every layer came with (hi, lo) fp16 weights: the tiles multiply on the fp16 matrix pipe
    bo_b1_layer *layers = nullptr;  // device table
    float *bufs = nullptr, *pool = nullptr;
    unsigned *sync = nullptr;       // [max_batch counters | status word | padding], a block of its own (zeroed before every launch)
    size_t sync_bytes = 0;
    unsigned long long *prof = nullptr;  // bo_nn_b1_profile: per-wave phase clocks of the next launches (NULL: off)
#endif
};

extern "C" int bo_nn_b1_create(const bo_b1_layer_desc *layers, int n_layers, int channels, int max_batch, int device, bo_b1 **out) {
#if defined(BO_WAVE_EMU)
    (void)layers; (void)n_layers; (void)channels; (void)max_batch; (void)device; (void)out;
    return fail(BO_E_CONFIG, "bo_nn_b1 is a gfx950-only kernel");
#else
    if (!layers || !out || n_layers < 1 || n_layers > BO_B1_MAX_LAYERS || (n_layers & 1) == 0) return fail(BO_E_ARG, "bo_nn_b1_create: 1 + 2 x blocks layers");
    if (channels != 64 && channels != 128 && channels != 256) return fail(BO_E_CONFIG, "bo_nn_b1: 64, 128 or 256 filters");
    const int tiles = (channels / 16) * 4;
    if (max_batch < 1 || max_batch * tiles > 256) return fail(BO_E_CONFIG, "bo_nn_b1: (filters / 16) x 4 x batch workgroups must be resident at once (<= 256)");
    std::vector<bo_b1_layer> tab((size_t)n_layers);
    int n_split = 0;
    for (int l = 0; l < n_layers; l++) {
        const bo_b1_layer_desc &d = layers[l];
        if (!d.weights_dev || !d.bias_dev) return fail(BO_E_ARG, "bo_nn_b1_create: null weights");
        const int want_cin = l == 0 ? 128 : channels, want_mode_lo = (l == 0 || (l & 1)) ? 0 : 1;
        if (d.c_in != want_cin || d.c_in_x < 1 || d.c_in_x > d.c_in || (l > 0 && d.c_in_x != channels)) return fail(BO_E_ARG, "bo_nn_b1_create: layer channel counts");
        if ((l == 0 || (l & 1)) ? d.mode != 0 : (d.mode != 1 && d.mode != 2)) return fail(BO_E_ARG, "bo_nn_b1_create: layer modes must be 0, then (0, 1 | 2) per block");
        (void)want_mode_lo;
        if (d.mode == 2 && (!d.se_w1_dev || !d.se_w2_dev || d.se_hidden < 1 || d.se_hidden > 16)) return fail(BO_E_CONFIG, "bo_nn_b1: SE hidden width 1..16");
        tab[l].w = (const bo_f32x4 *)d.weights_dev; tab[l].bias = d.bias_dev; tab[l].se_w1 = d.se_w1_dev; tab[l].se_w2 = d.se_w2_dev;
        tab[l].cin = d.c_in; tab[l].cin_x = d.c_in_x; tab[l].mode = d.mode; tab[l].se_h = d.se_hidden;
        tab[l].w_split = (const bo_f32x4 *)d.weights_split_dev; tab[l].inv_scale = d.inv_scale; tab[l].pad = 0;
        if (d.weights_split_dev && !(d.inv_scale > 0.0f)) return fail(BO_E_ARG, "bo_nn_b1_create: split weights need inv_scale > 0");
        n_split += d.weights_split_dev ? 1 : 0;
    }
    if (n_split != 0 && n_split != n_layers) return fail(BO_E_ARG, "bo_nn_b1_create: split weights for every layer or for none");
    RT((int)hipSetDevice(device));
    bo_b1 *t = new bo_b1();
    t->device = device; t->C = channels; t->n_layers = n_layers; t->max_batch = max_batch; t->split = n_split == n_layers;
    t->sync_bytes = (((size_t)2 * max_batch + 2) * 4 + 63) / 64 * 64;
    int rc = (int)hipMalloc((void **)&t->layers, tab.size() * sizeof(bo_b1_layer));
    if (!rc) rc = (int)hipMemcpy(t->layers, tab.data(), tab.size() * sizeof(bo_b1_layer), hipMemcpyHostToDevice);
    if (!rc) rc = (int)hipMalloc((void **)&t->bufs, (size_t)3 * max_batch * channels * 64 * 4);
    if (!rc) rc = (int)hipMalloc((void **)&t->pool, (size_t)max_batch * 4 * channels * 4);
    if (!rc) rc = (int)hipMalloc((void **)&t->sync, t->sync_bytes);
    if (!rc) rc = (int)hipMemset(t->sync, 0, t->sync_bytes);
    if (rc) {
        (void)hipFree(t->layers); (void)hipFree(t->bufs); (void)hipFree(t->pool); (void)hipFree(t->sync);
        delete t;
        return fail(BO_E_HIP, std::string("bo_nn_b1_create: ") + hipGetErrorString((hipError_t)rc));
    }
    *out = t;
    return BO_OK;
#endif
}

// One evaluation's tower: x [batch,120,8,8] -> y [batch,C,8,8] on `stream`.  The handle's buffers are used by the launch: one launch
// of a handle at a time (launches on ONE stream are in order; two streams need two handles).  Capturable (memset node + kernel node).
extern "C" int bo_nn_b1_forward(bo_b1 *t, const float *x_dev, float *y_dev, int batch, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)x_dev; (void)y_dev; (void)batch; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_b1 is a gfx950-only kernel");
#else
    if (!t || !x_dev || !y_dev) return fail(BO_E_ARG, "null argument");
    if (batch < 1 || batch > t->max_batch) return fail(BO_E_ARG, "bo_nn_b1_forward: batch beyond the handle's max_batch");
    hipStream_t st = (hipStream_t)stream;
    // No memset in front of the launch: the arrival counters run on from launch to launch (bo_b1_args::sync).
    bo_b1_args a;
    a.x = x_dev; a.y = y_dev; a.bufs = t->bufs; a.pool = t->pool; a.sync = t->sync; a.layers = t->layers; a.n_layers = t->n_layers; a.B = batch;
    a.prof = t->prof; a.MB = t->max_batch;
    const dim3 grid((unsigned)((t->C / 16) * 4), (unsigned)batch);
    static const int mode = [] { const char *v = getenv("BETAONE_B1_MODE"); return (v && v[0] >= '0' && v[0] <= '2') ? v[0] - '0' : (int)BO_B1_SC1; }();
#define BO_B1_LAUNCH_P(CC, PP)                                                                                       \
    do {                                                                                                             \
        if (mode == BO_B1_ACQ) hipLaunchKernelGGL((bo_k_tower_b1<CC, BO_B1_ACQ, PP>), grid, dim3(256), 0, st, a);    \
        else if (mode == BO_B1_NT) hipLaunchKernelGGL((bo_k_tower_b1<CC, BO_B1_NT, PP>), grid, dim3(256), 0, st, a); \
        else hipLaunchKernelGGL((bo_k_tower_b1<CC, BO_B1_SC1, PP>), grid, dim3(256), 0, st, a);                      \
    } while (0)
#define BO_B1_LAUNCH(CC) do { if (t->split) BO_B1_LAUNCH_P(CC, BO_B1_SPLIT); else BO_B1_LAUNCH_P(CC, BO_B1_F32); } while (0)
    if (t->C == 256) BO_B1_LAUNCH(256);
    else if (t->C == 128) BO_B1_LAUNCH(128);
    else BO_B1_LAUNCH(64);
#undef BO_B1_LAUNCH_P
#undef BO_B1_LAUNCH
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// *code_out = 0, or 1 + the phase of a hand-off wait that gave up in the LAST launch (the evaluation's output is then invalid).
// Synchronises `stream` (the stream the launches went to).
extern "C" int bo_nn_b1_status(bo_b1 *t, int32_t *code_out, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)code_out; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_b1 is a gfx950-only kernel");
#else
    if (!t || !code_out) return fail(BO_E_ARG, "bad arguments");
    int32_t two[2] = {0, 0};
    RT(rt_d2h(two, t->sync + 2 * t->max_batch, 8, stream));
    RT(rt_sync(stream));
    *code_out = two[0] ? two[0] : (two[1] ? -1 : 0);
    if (two[0] || two[1]) {  // a fault leaves the counters anywhere: start over from zero (the stream is idle here)
        RT((int)hipMemsetAsync(t->sync, 0, t->sync_bytes, (hipStream_t)stream));
        RT(rt_sync(stream));
    }
    return BO_OK;
#endif
}

// Device address of the handle's two status words [timeout code | saturation flag], for bo_engine_watch_words(.., 2): a search or
// a self-play ply then learns of a hand-off that gave up (or a saturated activation) with the result block it fetches anyway.
extern "C" int bo_nn_b1_word(bo_b1 *t, void **dev_words_out) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)dev_words_out;
    return fail(BO_E_CONFIG, "bo_nn_b1 is a gfx950-only kernel");
#else
    if (!t || !dev_words_out) return fail(BO_E_ARG, "bad arguments");
    *dev_words_out = t->sync + 2 * t->max_batch;
    return BO_OK;
#endif
}

// LAB: shader-clock sums per wave of the phases of a layer {wait for the hand-off, slab loads + staging, matrix pipe, reduction,
// epilogue + signal, layers} over the launches since enable = 1; enable = 0 copies them out ([batch * tiles * 4 waves][8], `cap`
// entries of 8) and switches the stamps off.  Synchronises the device.
extern "C" int bo_nn_b1_profile(bo_b1 *t, int enable, uint64_t *out, int cap) {
#if defined(BO_WAVE_EMU)
    (void)t; (void)enable; (void)out; (void)cap;
    return fail(BO_E_CONFIG, "bo_nn_b1 is a gfx950-only kernel");
#else
    if (!t) return fail(BO_E_ARG, "null handle");
    const size_t n = (size_t)t->max_batch * (size_t)(t->C / 16) * 4 * 4 * 8;
    RT((int)hipDeviceSynchronize());
    if (enable) {
        if (!t->prof) RT((int)hipMalloc((void **)&t->prof, n * 8));
        RT((int)hipMemset(t->prof, 0, n * 8));
        return BO_OK;
    }
    if (!t->prof) return fail(BO_E_STATE, "bo_nn_b1_profile: not enabled");
    if (out) RT((int)hipMemcpy(out, t->prof, std::min(n, (size_t)cap * 8) * 8, hipMemcpyDeviceToHost));
    (void)hipFree(t->prof);
    t->prof = nullptr;
    return BO_OK;
#endif
}

extern "C" void bo_nn_b1_destroy(bo_b1 *t) {
#if !defined(BO_WAVE_EMU)
    if (!t) return;
    (void)hipFree(t->prof);
    (void)hipFree(t->layers); (void)hipFree(t->bufs); (void)hipFree(t->pool); (void)hipFree(t->sync);
#endif
    delete t;
}

// LAB: a one-thread kernel that notes the device's constant-rate clock: ring[0] = entries written (atomic), entry k = ring[1 + 2k] =
// tag, ring[2 + 2k] = wall_clock64() -- enqueued between the launches of a stream (also inside captured graphs) it gives the timeline of
// that stream's phases as the device ran them (rocprofv3 changes how streams overlap; event pairs cannot sit between graph nodes).
#if !defined(BO_WAVE_EMU)
__global__ void bo_k_stamp(unsigned long long *ring, unsigned long long tag, unsigned long long cap) {
    const unsigned long long k = __hip_atomic_fetch_add(ring, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k < cap) { ring[1 + 2 * k] = tag; ring[2 + 2 * k] = wall_clock64(); }
}
#endif
extern "C" int bo_debug_stamp(void *ring_dev, uint64_t tag, uint64_t capacity, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)ring_dev; (void)tag; (void)capacity; (void)stream;
    return fail(BO_E_CONFIG, "gfx950 only");
#else
    if (!ring_dev) return fail(BO_E_ARG, "null ring");
    hipLaunchKernelGGL(bo_k_stamp, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long *)ring_dev, (unsigned long long)tag, (unsigned long long)capacity);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// A stream whose kernels run on the compute units named by the mask only (bit i = CU i) -- and which has a hardware queue of its own, which
// is what K > 2 cohorts need first (pool streams share queues; profiles/r04_cohort_cu_masks.md: full masks 3.03 ms, pool streams 4.1 ms per ply).
extern "C" int bo_stream_create_cu_mask(int device, const uint32_t *mask_words, int n_words, void **stream_out) {
#if defined(BO_WAVE_EMU)
    (void)device; (void)mask_words; (void)n_words; (void)stream_out;
    return fail(BO_E_CONFIG, "gfx950 only");
#else
    if (!mask_words || n_words < 1 || !stream_out) return fail(BO_E_ARG, "bad arguments");
    bool any = false;
    for (int i = 0; i < n_words; i++) any = any || mask_words[i] != 0;
    if (!any) return fail(BO_E_ARG, "an empty CU mask would never run a kernel");
    RT((int)hipSetDevice(device));
    hipStream_t st = nullptr;
    RT((int)hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, mask_words));
    *stream_out = (void *)st;
    return BO_OK;
#endif
}
extern "C" int bo_stream_destroy(void *stream) {
#if defined(BO_WAVE_EMU)
    (void)stream;
    return fail(BO_E_CONFIG, "gfx950 only");
#else
    if (!stream) return BO_OK;
    RT((int)hipStreamDestroy((hipStream_t)stream));
    return BO_OK;
#endif
}

// ---- policy FC + softmax + value head behind the tower: two launches (bo_heads.h) ------------------------------------
extern "C" int bo_nn_heads(const void *p_dev, const void *v_dev, const float *wp_dev, const float *bp_dev, const float *w1_dev,
                           const float *b1_dev, const float *w2_dev, const float *b2_dev, float *policy_out_dev, float *value_out_dev,
                           float *scratch_dev, int batch, int flags, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)p_dev; (void)v_dev; (void)wp_dev; (void)bp_dev; (void)w1_dev; (void)b1_dev; (void)w2_dev; (void)b2_dev; (void)policy_out_dev;
    (void)value_out_dev; (void)scratch_dev; (void)batch; (void)flags; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_heads is a gfx950-only kernel");
#else
    if (!p_dev || !v_dev || !wp_dev || !bp_dev || !w1_dev || !b1_dev || !w2_dev || !b2_dev || !policy_out_dev || (!value_out_dev && !(flags & 4)) || !scratch_dev)
        return fail(BO_E_ARG, "null argument");
    if ((flags & 4) && (flags & 1)) return fail(BO_E_ARG, "bo_nn_heads: flags 4 (no rows kernel) leaves LOGITS: it excludes flags 1 (softmax)");
    if (batch < 1 || batch > 65536) return fail(BO_E_ARG, "bo_nn_heads: 1 <= batch <= 65536");
    bo_heads_args a;
    a.p = p_dev; a.v = v_dev; a.wp = wp_dev; a.bp = bp_dev; a.w1 = w1_dev; a.b1 = b1_dev; a.w2 = w2_dev; a.b2 = b2_dev;
    a.policy_out = policy_out_dev; a.value_out = value_out_dev;
    a.vpart = scratch_dev;  // [16 K chunks][batch][256]
    a.B = batch; a.softmax = flags & 1; a.pb = bo_heads_policy_boards(batch);
    const int otw = 4 / (a.pb >> 5);
    const unsigned tiles = (unsigned)(((batch + a.pb - 1) / a.pb) * ((BO_HEADS_NA / 32 + otw - 1) / otw) + ((batch + 63) / 64) * 4 * BO_HEADS_KS);
    if (flags & 2) hipLaunchKernelGGL(bo_k_heads_tiles<true>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, bo_heads_pair{});   // fp16 head planes
    else hipLaunchKernelGGL(bo_k_heads_tiles<false>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, bo_heads_pair{});
    if (!(flags & 4)) hipLaunchKernelGGL(bo_k_heads_rows, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);  // (4: bo_step_heads is the rows' consumer)
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// the same with two nets' float32 head weights, row b on the net sel_dev[b] names (bo_heads.h: bo_heads_pair)
extern "C" int bo_nn_heads_pair(const void *p_dev, const void *v_dev, const bo_head_weights *net0, const bo_head_weights *net1,
                                const int32_t *sel_dev, float *policy_out_dev, float *value_out_dev, float *scratch_dev, int batch, int flags,
                                void *stream) {
#if defined(BO_WAVE_EMU)
    (void)p_dev; (void)v_dev; (void)net0; (void)net1; (void)sel_dev; (void)policy_out_dev; (void)value_out_dev; (void)scratch_dev; (void)batch;
    (void)flags; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_heads_pair is a gfx950-only kernel");
#else
    if (!p_dev || !v_dev || !net0 || !net1 || !sel_dev || !policy_out_dev || !value_out_dev || !scratch_dev) return fail(BO_E_ARG, "null argument");
    for (const bo_head_weights *w : {net0, net1})
        if (!w->wp || !w->bp || !w->w1 || !w->b1 || !w->w2 || !w->b2) return fail(BO_E_ARG, "null head weight");
    if (flags & ~3) return fail(BO_E_ARG, "bo_nn_heads_pair: flags 1 (softmax) and 2 (fp16 planes) only");
    if (batch < 1 || batch > 65536) return fail(BO_E_ARG, "bo_nn_heads_pair: 1 <= batch <= 65536");
    bo_heads_args a;
    a.p = p_dev; a.v = v_dev; a.wp = net0->wp; a.bp = net0->bp; a.w1 = net0->w1; a.b1 = net0->b1; a.w2 = net0->w2; a.b2 = net0->b2;
    a.policy_out = policy_out_dev; a.value_out = value_out_dev;
    a.vpart = scratch_dev;
    a.B = batch; a.softmax = flags & 1; a.pb = bo_heads_policy_boards(batch);
    bo_heads_pair q;
    q.sel = sel_dev; q.wp = net1->wp; q.bp = net1->bp; q.w1 = net1->w1; q.b1 = net1->b1; q.w2 = net1->w2; q.b2 = net1->b2;
    const int otw = 4 / (a.pb >> 5);
    const unsigned tiles = (unsigned)(((batch + a.pb - 1) / a.pb) * ((BO_HEADS_NA / 32 + otw - 1) / otw) + ((batch + 63) / 64) * 4 * BO_HEADS_KS);
    if (flags & 2) hipLaunchKernelGGL((bo_k_heads_tiles<true, true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, q);
    else hipLaunchKernelGGL((bo_k_heads_tiles<false, true>), dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, q);
    hipLaunchKernelGGL(bo_k_heads_rows_pair, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a, q);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

#if !defined(BO_WAVE_EMU)
// out[b] = sel[b] ? (logits1, value1)[b] : (logits0, value0)[b]; one workgroup per row
__global__ void __launch_bounds__(256)
bo_k_merge_rows(const int32_t *__restrict__ sel, const float *__restrict__ l0, const float *__restrict__ v0, const float *__restrict__ l1,
                const float *__restrict__ v1, float *__restrict__ lo, float *__restrict__ vo, int width) {
    const int b = (int)blockIdx.x;
    const bool one = __builtin_amdgcn_readfirstlane(sel[b]) != 0;
    const float *src = (one ? l1 : l0) + (size_t)b * width;
    float *dst = lo + (size_t)b * width;
    for (int i = threadIdx.x; i < width; i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x == 0) vo[b] = (one ? v1 : v0)[b];
}

// sel[g] = net_of_white[g] ^ (the root of slot g has black to move); slots past the root stack's capacity keep net_of_white
__global__ void bo_k_match_select(Eng e, const int32_t *__restrict__ net_of_white, int32_t *__restrict__ sel) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= e.c.G) return;
    const int ply = e.ply[g];
    const bool black = ply >= 0 && ply < e.c.PLY_CAP && !(e.gpos[(size_t)g * e.c.PLY_CAP + ply].flags & F_TURN);
    sel[g] = (net_of_white[g] != 0) ^ (black ? 1 : 0);
}
#endif

extern "C" int bo_nn_merge_rows(const int32_t *sel_dev, const float *logits0_dev, const float *value0_dev, const float *logits1_dev,
                                const float *value1_dev, float *logits_out_dev, float *value_out_dev, int batch, int width, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)sel_dev; (void)logits0_dev; (void)value0_dev; (void)logits1_dev; (void)value1_dev; (void)logits_out_dev; (void)value_out_dev;
    (void)batch; (void)width; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_merge_rows is a gfx950-only kernel");
#else
    if (!sel_dev || !logits0_dev || !value0_dev || !logits1_dev || !value1_dev || !logits_out_dev || !value_out_dev) return fail(BO_E_ARG, "null argument");
    if (batch < 1 || batch > (1 << 22) || width < 1 || width > (1 << 16)) return fail(BO_E_ARG, "bo_nn_merge_rows: 1 <= batch <= 2^22, 1 <= width <= 65536");
    hipLaunchKernelGGL(bo_k_merge_rows, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, sel_dev, logits0_dev, value0_dev, logits1_dev,
                       value1_dev, logits_out_dev, value_out_dev, width);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

extern "C" int bo_match_select(bo_engine *e, const int32_t *net_of_white_dev, int32_t *sel_dev, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)e; (void)net_of_white_dev; (void)sel_dev; (void)stream;
    return fail(BO_E_CONFIG, "bo_match_select is a gfx950-only kernel");
#else
    if (!e || !net_of_white_dev || !sel_dev) return fail(BO_E_ARG, "null argument");
    if (e->fast) return fail(BO_E_CONFIG, "bo_match_select: reference-semantics engines only (fast mode has L rows per game)");
    const int G = e->d.c.G;
    hipLaunchKernelGGL(bo_k_match_select, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->d, net_of_white_dev, sel_dev);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// fp16 head planes and fp16 Linear weights, any number of rows: policy FC + softmax in one kernel, the whole value head in another
extern "C" int bo_nn_heads_f16(const void *p_dev, const void *v_dev, const void *wp_f16_dev, const float *bp_dev, const void *w1_f16_dev,
                               const float *b1_dev, const float *w2_dev, const float *b2_dev, float *policy_out_dev, float *value_out_dev,
                               float *scratch_dev, int batch, int flags, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)p_dev; (void)v_dev; (void)wp_f16_dev; (void)bp_dev; (void)w1_f16_dev; (void)b1_dev; (void)w2_dev; (void)b2_dev; (void)policy_out_dev;
    (void)value_out_dev; (void)scratch_dev; (void)batch; (void)flags; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_heads_f16 is a gfx950-only kernel");
#else
    if (!p_dev || !v_dev || !wp_f16_dev || !bp_dev || !w1_f16_dev || !b1_dev || !w2_dev || !b2_dev || !policy_out_dev || !value_out_dev)
        return fail(BO_E_ARG, "null argument");
    if (batch < 1 || batch > (1 << 22)) return fail(BO_E_ARG, "bo_nn_heads_f16: 1 <= batch <= 4194304");
    bo_heads_h_args a;
    a.p = (const _Float16 *)p_dev; a.v = (const _Float16 *)v_dev; a.wp = (const _Float16 *)wp_f16_dev; a.w1 = (const _Float16 *)w1_f16_dev;
    a.bp = bp_dev; a.b1 = b1_dev; a.w2 = w2_dev; a.b2 = b2_dev; a.policy_out = policy_out_dev; a.value_out = value_out_dev;
    a.B = batch; a.softmax = flags & 1; a.stats = scratch_dev;
    if (a.softmax && !scratch_dev) return fail(BO_E_ARG, "bo_nn_heads_f16: the softmax needs scratch_dev (20 * batch floats)");
    const dim3 pgrid((unsigned)((batch + 255) / 256), BO_HEADS_PS);
    if (a.softmax) {
        hipLaunchKernelGGL(bo_k_heads_policy_h<0>, pgrid, dim3(256), 0, (hipStream_t)stream, a);
        hipLaunchKernelGGL(bo_k_heads_policy_h<1>, pgrid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(bo_k_heads_policy_h<2>, pgrid, dim3(256), 0, (hipStream_t)stream, a);
    }
    hipLaunchKernelGGL(bo_k_heads_value_h, dim3((unsigned)((batch + 63) / 64)), dim3(256), 0, (hipStream_t)stream, a);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

extern "C" int bo_nn_value_tail(const float *h_dev, const float *w_dev, const float *bias_dev, float *out_dev, int batch, int hidden, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)h_dev; (void)w_dev; (void)bias_dev; (void)out_dev; (void)batch; (void)hidden; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_value_tail is a gfx950-only kernel");
#else
    if (!h_dev || !w_dev || !bias_dev || !out_dev || batch < 1 || hidden < 1) return fail(BO_E_ARG, "bad arguments");
    hipLaunchKernelGGL(bo_k_value_tail, dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, (hipStream_t)stream, h_dev, w_dev, bias_dev, out_dev, batch, hidden);
    RT((int)hipGetLastError());
    return BO_OK;
#endif
}

// small-batch form of bo_nn_conv3x3 (bo_conv.h: bo_k_conv3x3_small): (c_out/16) x 4 workgroups per board
extern "C" int bo_nn_conv3x3_small(const float *x_dev, const float *wpacked_dev, const float *bias_dev, const float *residual_dev, float *y_dev,
                                   int batch, int c_in, int c_in_x, int c_out, int mode, void *stream) {
#if defined(BO_WAVE_EMU)
    (void)x_dev; (void)wpacked_dev; (void)bias_dev; (void)residual_dev; (void)y_dev; (void)batch; (void)c_in; (void)c_in_x; (void)c_out; (void)mode; (void)stream;
    return fail(BO_E_CONFIG, "bo_nn_conv3x3_small is a gfx950-only kernel");
#else
    if (!x_dev || !wpacked_dev || !bias_dev || !y_dev || batch < 1 || batch > 65535) return fail(BO_E_ARG, "bad arguments");
    if (mode < 0 || mode > 2 || (mode == 2 && !residual_dev)) return fail(BO_E_ARG, "bad epilogue mode");
    if (c_in_x < 1 || c_in_x > c_in) return fail(BO_E_ARG, "c_in_x must be in 1..c_in");
    const bo_f32x4 *wp = reinterpret_cast<const bo_f32x4 *>(wpacked_dev);
    hipStream_t st = (hipStream_t)stream;
#define BO_SMALL_CASE(CI, CO)                                                                                                             \
    if (c_in == CI && c_out == CO) {                                                                                                      \
        hipLaunchKernelGGL((bo_k_conv3x3_small<CI, CO>), dim3(CO / 16, 4, (unsigned)batch), dim3(256), 0, st, x_dev, wp, bias_dev, residual_dev, \
                           y_dev, c_in_x, mode);                                                                                          \
        RT((int)hipGetLastError());                                                                                                       \
        return BO_OK;                                                                                                                     \
    }
    BO_SMALL_CASE(128, 64) BO_SMALL_CASE(64, 64) BO_SMALL_CASE(128, 128) BO_SMALL_CASE(128, 256) BO_SMALL_CASE(256, 256)
#undef BO_SMALL_CASE
    return fail(BO_E_CONFIG, "bo_nn_conv3x3_small: supported (c_in, c_out): (128 | C, C) for C in {64, 128, 256}");
#endif
}

// ---- perft on the device (bo_perft.h), and the level walk it shares with forced mates and the anchor opponent ------------------------
// Level l of the walk is a frontier (positions and tags) in HBM; level 0 holds the roots.  Every level but the last one generated also
// keeps its move counts and their scan, because a level whose children do not fit the next buffer is expanded chunk by chunk.  One run
// object (Walk) owns every device buffer of a call, one function (walk_level) is the recursion; bo_perft, bo_mate and bo_anchor differ in
// the kernels their hooks launch.
namespace {
// Device memory that frees itself: the pointer and its element count, move-only.  Releasing waits for nothing: the owner of a DevBuf
// synchronises the stream before the buffer goes (Walk's destructor; the one sync of bo_anchor_eval).
template <class T> struct DevBuf {
    T *p = nullptr;
    int64_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    ~DevBuf() { rt_free(p); }
    int alloc(int64_t m) {  // exactly m entries (the old contents are dead)
        rt_free(p);
        p = nullptr; n = 0;
        const int rc = rt_malloc((void **)&p, (size_t)m * sizeof(T));
        if (rc) p = nullptr; else n = m;
        return rc;
    }
    // grow-only, doubling up to `limit` entries (the old contents are dead: a buffer is refilled before it is read); no limit: exactly `need`
    int room(int64_t need, int64_t limit = 0) { return n >= need ? 0 : alloc(std::max(need, std::min(limit, 2 * n))); }
};
template <class T> struct HostBuf {  // its pinned-host twin
    T *p = nullptr;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    ~HostBuf() { if (p) rt_host_free(p); }
    int alloc(int64_t m) {  // exactly m entries (the old contents are dead)
        if (p) rt_host_free(p);
        p = nullptr;
        const int rc = rt_host_alloc((void **)&p, (size_t)m * sizeof(T));
        if (rc) p = nullptr;
        return rc;
    }
};

struct WalkLevel {
    DevBuf<DPos> pos;          // the frontier [have]: have = pos.n
    DevBuf<int32_t> tag, cnt;  // [have]; the move counts [have_scan]: have_scan = cnt.n
    DevBuf<uint64_t> off;      // their scan [have_scan + 1]
    DevBuf<uint8_t> mate_val;  // bo_mate: one value byte per entry [have]
    DevBuf<uint64_t> live;     // bo_mate, attacker levels (even): the live masks [have][4]
    DevBuf<int16_t> val;       // bo_anchor: one value per entry [have]
};
// Everything one call of bo_perft, bo_mate or bo_anchor holds on the device.  The destructor's body runs before the members go, so the
// stream is synchronised before any buffer of the run is released, on every return path.  (A run whose call has failed is not used again.)
struct Walk {
    const char *name;  // the caller's, for messages
    void *stream;
    int64_t cap, splits = 0;
    int depth = 0, quiesce = 0;  // levels 0 .. depth - 1 full width, then `quiesce` levels over the tactical moves (bo_anchor_q only)
    uint32_t flags = 0;          // bo_perft's
    uint64_t visited = 0;        // bo_mate, bo_anchor: frontier entries of every level of every walk (include/betaone_engine.h: nodes)
    std::vector<WalkLevel> lv;
    DevBuf<int32_t> tsum;
    DevBuf<uint64_t> tbase;
    DevBuf<int64_t> d_word;
    HostBuf<int64_t> h_word;
    // per root: the roots kernel's in-place buffer, move words [256], counts, check bits, active -> root
    DevBuf<DPos> d_roots;
    DevBuf<int32_t> root_moves, root_n, root_chk, act;
    DevBuf<uint64_t> nodes, sums, stats;               // bo_perft: per root move, per root, per root [PF_NSTATS]
    DevBuf<int32_t> n_keys, key;                       // bo_mate, per root: keys, lowest key
    DevBuf<uint64_t> keymask;                          // bo_mate, per root: key mask [4]
    DevBuf<int32_t> scores, score, n_best, best, n_act;  // bo_anchor, per root: score row [256], score, best moves, lowest best, moves
    Walk(const char *name_, void *stream_, int64_t cap_) : name(name_), stream(stream_), cap(cap_) {}
    ~Walk() { (void)rt_sync(stream); }  // nothing of ours is in flight when its memory goes
    int levels() const { return depth + quiesce; }
    int words() {
        RT(d_word.alloc(2));
        RT(h_word.alloc(2));
        return BO_OK;
    }
    int room(int l, int64_t n) {
        RT(lv[l].pos.room(n, cap));
        RT(lv[l].tag.room(n, cap));
        return BO_OK;
    }
    int room_scan(int l, int64_t n) {
        WalkLevel &L = lv[l];
        if (L.cnt.n >= n) return BO_OK;
        RT(L.cnt.room(n, std::max(cap, n)));
        const int64_t m = L.cnt.n, nt = (m + BO_PERFT_TILE - 1) / BO_PERFT_TILE;
        RT(L.off.alloc(m + 1));
        RT(tsum.room(nt));
        RT(tbase.room(nt));
        return BO_OK;
    }
    int room_roots(int64_t n) {
        RT(d_roots.room(n));
        RT(root_moves.room(n * BO_MAX_MOVES));
        RT(root_n.room(n));
        RT(root_chk.room(n));
        RT(act.room(n));
        return BO_OK;
    }
    int scan(int l, int64_t n) {  // cnt -> off of level l, the total into h_word[0]: the one word the host reads between levels
        WalkLevel &L = lv[l];
        const int nt = (int)((n + BO_PERFT_TILE - 1) / BO_PERFT_TILE);
        RT(RT_LAUNCH(bo_k_perft_tile_sums, nt, stream, (const int32_t *)L.cnt.p, n, tsum.p));
        RT(RT_LAUNCH(bo_k_perft_tile_scan, 1, stream, (const int32_t *)tsum.p, nt, tbase.p, L.off.p, n));
        RT(RT_LAUNCH(bo_k_perft_offsets, nt, stream, (const int32_t *)L.cnt.p, n, (const uint64_t *)tbase.p, L.off.p));
        RT(rt_d2h(h_word.p, L.off.p + n, 8, stream));
        RT(rt_sync(stream));
        return BO_OK;
    }
};

// The subtree below entries [0, n) of level l, whose frontier is in place.  The hooks H of a walk:
//   enter(l, n, &bottom)  launches what fills cnt (and the values) of level l; bottom: the level has no children to walk
//   room(l, n)            room for n entries of level l
//   expand(l, a, e)       the children of entries [a, e) of level l into level l + 1
//   backup(l, a, e)       the values of those children, taken to the bottom, into their parents
//   after(a, n)           level 0 only: the roots [a, n) behind the last child
template <class H> int walk_level(Walk &R, H &h, int l, int64_t n) {
    WalkLevel &L = R.lv[l];
    bool bottom = false;
    int rc = h.enter(l, n, &bottom);
    if (rc) return rc;
    int64_t a = 0;
    if (!bottom) {
        rc = R.scan(l, n);
        if (rc) return rc;
        int64_t left = R.h_word.p[0];
        while (a < n && left > 0) {
            int64_t e = n, c = left;
            if (left > R.cap) {  // the rest of the level does not fit: the longest run of entries from a that does
                RT(RT_LAUNCH(bo_k_perft_split, 1, R.stream, (const uint64_t *)L.off.p, a, n, R.cap, R.d_word.p));
                RT(rt_d2h(R.h_word.p, R.d_word.p, 16, R.stream));
                RT(rt_sync(R.stream));
                e = R.h_word.p[0];
                c = R.h_word.p[1];
                if (e <= a || e > n || c < 1 || c > R.cap) return fail(BO_E_STATE, std::string(R.name) + ": the level split is inconsistent");
                if (c < left) R.splits++;
            }
            rc = h.room(l + 1, c);
            if (!rc) rc = h.expand(l, a, e);
            if (!rc) rc = walk_level(R, h, l + 1, c);
            if (!rc) rc = h.backup(l, a, e);
            if (rc) return rc;
            left -= c;
            a = e;
        }
    }
    return l == 0 && a < n ? h.after(a, n) : BO_OK;
}

// what the generator's 256-move lists and its king lookups need of a position (include/betaone_engine.h: "not a position")
bool position_ok(const DPos &p) {
    uint64_t all = 0;
    for (int i = 0; i < 6; i++) {
        if (all & p.bb[i]) return false;
        all |= p.bb[i];
    }
    if ((p.bb[BB_WHITE] & p.bb[BB_BLACK]) || (p.bb[BB_WHITE] | p.bb[BB_BLACK]) != all) return false;
    if (p.bb[BB_P] & (RANK_1 | RANK_8)) return false;
    for (int c = 0; c < 2; c++) {
        const uint64_t own = p.bb[c ? BB_BLACK : BB_WHITE];
        auto cnt = [&](int t) { return __builtin_popcountll(p.bb[t] & own); };
        if (cnt(BB_K) != 1 || __builtin_popcountll(own) > 16 || cnt(BB_P) > 8) return false;
        const int extra = std::max(0, cnt(BB_N) - 2) + std::max(0, cnt(BB_B) - 2) + std::max(0, cnt(BB_R) - 2) + std::max(0, cnt(BB_Q) - 1);
        if (extra > 8 - cnt(BB_P)) return false;
    }
    return true;
}
bool record_ok(const bo_position &q, DPos *p) {
    const bool fields = (q.turn == 0 || q.turn == 1) && q.castling <= 0xFu && q.ep_square >= -1 && q.ep_square <= 63 && q.ep_key >= -2 && q.ep_key <= 63;
    if (fields) *p = from_abi(q);
    return fields && position_ok(*p);
}
int capacity_ok(const std::string &who, int64_t capacity) {
    if (capacity < BO_MAX_MOVES || capacity > ((int64_t)1 << 26))
        return fail(BO_E_CONFIG, who + ": capacity must be 256 (the children of one position) .. 2^26 positions per level");
    return BO_OK;
}

// The roots of bo_mate and bo_anchor that are positions, and their rows in the caller's arrays.  Every result is zeroed, then init(result)
// row by row; a FEN that is no position fails the call there, a record that is none gets the status `not_a_position` and is left out.
template <class Res, class Init>
int collect_roots(const std::string &who, size_t N, const char *const *fens, const bo_position *positions, Res *results, Init init,
                  int32_t not_a_position, std::vector<DPos> &roots, std::vector<int32_t> &index) {
    roots.reserve(N); index.reserve(N);
    memset(results, 0, N * sizeof(Res));
    for (size_t i = 0; i < N; i++) {
        DPos p;
        init(results[i]);
        if (fens) {
            if (!pgn_fen_root(fens[i] ? fens[i] : "", &p) || !position_ok(p)) return fail(BO_E_FEN, who + ": bad FEN (root " + std::to_string(i) + ")");
        } else if (!record_ok(positions[i], &p)) { results[i].status = not_a_position; continue; }
        roots.push_back(p);
        index.push_back((int32_t)i);
    }
    return BO_OK;
}

// The roots on the device: finished in place (key fields as bo_k_perft_roots leaves them), their move lists moves [n][256], counts and
// check bits; active = the roots that are searched: a position with a move.
int prepare_roots(Walk &R, std::vector<DPos> &roots, std::vector<int32_t> &moves, std::vector<int32_t> &rn, std::vector<int32_t> &chk,
                  std::vector<int32_t> &active) {
    const size_t n = roots.size();
    moves.assign(n * BO_MAX_MOVES, -1); rn.assign(n, 0); chk.assign(n, 0); active.clear();
    if (!n) return BO_OK;
    int rc = R.room_roots((int64_t)n);
    if (rc) return rc;
    RT(rt_h2d(R.d_roots.p, roots.data(), n * sizeof(DPos), R.stream));
    RT(RT_LAUNCH(bo_k_mate_roots, n, R.stream, R.d_roots.p, R.root_moves.p, R.root_n.p, R.root_chk.p));
    RT(rt_d2h(roots.data(), R.d_roots.p, n * sizeof(DPos), R.stream));
    RT(rt_d2h(moves.data(), R.root_moves.p, moves.size() * 4, R.stream));
    RT(rt_d2h(rn.data(), R.root_n.p, n * 4, R.stream));
    RT(rt_d2h(chk.data(), R.root_chk.p, n * 4, R.stream));
    RT(rt_sync(R.stream));
    for (size_t r = 0; r < n; r++)
        if (!(chk[r] & 2) && rn[r] > 0) active.push_back((int32_t)r);
    return BO_OK;
}

struct PerftWalk {
    Walk &R;
    uint32_t mode(int l) const { return ((R.flags & BO_PERFT_ORDER) ? PF_ORDER : 0u) | (l == 0 ? PF_ROOT_LEVEL : 0u); }
    int enter(int l, int64_t n, bool *bottom) {
        WalkLevel &L = R.lv[l];
        *bottom = l == R.depth - 1;
        if (*bottom && (R.flags & BO_PERFT_STATS))
            RT(RT_LAUNCH(bo_k_perft_count_stats, n, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (int64_t)0, R.nodes.p, R.sums.p,
                         R.stats.p, mode(l)));
        else if (*bottom)
            RT(RT_LAUNCH(bo_k_perft_count, n, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (int64_t)0, (int32_t *)nullptr, R.nodes.p,
                         R.sums.p, mode(l) | PF_LEAF));
        else {
            const int rc = R.room_scan(l, n);
            if (rc) return rc;
            RT(RT_LAUNCH(bo_k_perft_count, n, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (int64_t)0, L.cnt.p, R.nodes.p, R.sums.p,
                         mode(l)));
        }
        return BO_OK;
    }
    int room(int l, int64_t n) { return R.room(l, n); }
    int expand(int l, int64_t a, int64_t e) {
        WalkLevel &L = R.lv[l], &C = R.lv[l + 1];
        RT(RT_LAUNCH(bo_k_perft_expand, e - a, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (const uint64_t *)L.off.p, a, C.pos.p,
                     C.tag.p, C.pos.n, mode(l)));
        return BO_OK;
    }
    int backup(int, int64_t, int64_t) { return BO_OK; }
    int after(int64_t, int64_t) { return BO_OK; }
};
}  // namespace

extern "C" int bo_perft(int device, int32_t n_roots, const char *const *fens, int32_t depth, int64_t capacity, uint32_t flags,
                        bo_perft_result *results, int32_t *divide_moves, uint64_t *divide_nodes, int64_t *n_splits, void *stream) {
    if (n_splits) *n_splits = 0;
    if (n_roots < 0 || n_roots > (1 << 20) || depth < 0 || depth > 64 || (flags & ~7u) || (n_roots && !results))
        return fail(BO_E_ARG, "bo_perft: bad arguments (n_roots <= 2^20, 0 <= depth <= 64)");
    const bool divide = (flags & BO_PERFT_DIVIDE) != 0;
    if (divide && n_roots && (!divide_moves || !divide_nodes)) return fail(BO_E_ARG, "bo_perft: BO_PERFT_DIVIDE needs divide_moves and divide_nodes");
    int rc = capacity_ok("bo_perft", capacity);
    if (rc) return rc;
    if (n_roots == 0) return BO_OK;
    std::vector<DPos> roots((size_t)n_roots);
    for (int i = 0; i < n_roots; i++) {
        if (!pgn_fen_root(fens && fens[i] ? fens[i] : "", &roots[i])) return fail(BO_E_FEN, "bo_perft: bad FEN (root " + std::to_string(i) + ")");
    }
    const size_t N = (size_t)n_roots;
    memset(results, 0, N * sizeof(bo_perft_result));
    if (divide) {
        for (size_t i = 0; i < N * BO_MAX_MOVES; i++) { divide_moves[i] = -1; divide_nodes[i] = 0; }
    }
    if (depth == 0) {
        for (size_t i = 0; i < N; i++) results[i].nodes = 1;
        return BO_OK;
    }
    RT(rt_set_device(device));
    Walk R("bo_perft", stream, capacity);
    R.depth = depth; R.flags = flags;
    R.lv.resize((size_t)depth);
    WalkLevel &L0 = R.lv[0];  // level 0: the roots (outside `capacity`: the caller chose their number)
    RT(L0.pos.alloc(n_roots));
    RT(L0.tag.alloc(n_roots));
    RT(R.root_moves.alloc(n_roots * (int64_t)BO_MAX_MOVES));
    RT(R.root_n.alloc(n_roots));
    RT(R.nodes.alloc(n_roots * (int64_t)BO_MAX_MOVES));
    RT(R.sums.alloc(n_roots));
    RT(R.stats.alloc(n_roots * (int64_t)PF_NSTATS));
    rc = R.words();
    if (rc) return rc;
    std::vector<int32_t> tags(N);
    for (size_t i = 0; i < N; i++) tags[i] = (int32_t)(i * BO_MAX_MOVES);
    RT(rt_h2d(L0.pos.p, roots.data(), N * sizeof(DPos), stream));
    RT(rt_h2d(L0.tag.p, tags.data(), N * 4, stream));
    RT(rt_memset(R.nodes.p, 0, N * BO_MAX_MOVES * 8, stream));
    RT(rt_memset(R.sums.p, 0, N * 8, stream));
    RT(rt_memset(R.stats.p, 0, N * PF_NSTATS * 8, stream));
    RT(RT_LAUNCH(bo_k_perft_roots, n_roots, stream, L0.pos.p, R.root_moves.p, R.root_n.p));
    RT(rt_sync(stream));  // (roots and tags are host vectors of this frame)
    PerftWalk P{R};
    rc = walk_level(R, P, 0, n_roots);
    if (rc) return rc;
    std::vector<uint64_t> nodes(N * BO_MAX_MOVES), sums(N), stats(N * PF_NSTATS);
    std::vector<int32_t> rmoves(N * BO_MAX_MOVES), rn(N);
    RT(rt_d2h(nodes.data(), R.nodes.p, nodes.size() * 8, stream));
    RT(rt_d2h(sums.data(), R.sums.p, sums.size() * 8, stream));
    RT(rt_d2h(stats.data(), R.stats.p, stats.size() * 8, stream));
    RT(rt_d2h(rmoves.data(), R.root_moves.p, rmoves.size() * 4, stream));
    RT(rt_d2h(rn.data(), R.root_n.p, rn.size() * 4, stream));
    RT(rt_sync(stream));
    for (size_t r = 0; r < N; r++) {
        bo_perft_result &o = results[r];
        o.n_moves = rn[r];
        for (int i = 0; i < BO_MAX_MOVES; i++) o.nodes += nodes[r * BO_MAX_MOVES + i];
        if (flags & BO_PERFT_ORDER) o.checksum = sums[r];
        if (flags & BO_PERFT_STATS) {
            const uint64_t *s = &stats[r * PF_NSTATS];
            o.stats.captures = s[PF_CAPTURES]; o.stats.en_passant = s[PF_EP]; o.stats.castles = s[PF_CASTLES];
            o.stats.promotions = s[PF_PROMOTIONS]; o.stats.checks = s[PF_CHECKS]; o.stats.checkmates = s[PF_CHECKMATES];
            o.stats.stalemates = s[PF_STALEMATES];
        }
        if (divide) {
            for (int i = 0; i < BO_MAX_MOVES; i++) {
                divide_moves[r * BO_MAX_MOVES + i] = rmoves[r * BO_MAX_MOVES + i];
                divide_nodes[r * BO_MAX_MOVES + i] = nodes[r * BO_MAX_MOVES + i];
            }
        }
    }
    if (n_splits) *n_splits = R.splits;
    return BO_OK;
}

// ---- forced mates on the device (bo_mate.h) ----------------------------------------------------------------------------------------
// The walk is perft's.  Each level also keeps one value byte per entry, an attacker level (even) the live masks of its entries; after a
// chunk of level l + 1 has been taken to the bottom, its values are backed up into the parents of level l that the chunk was expanded from.
namespace {
struct MateRoot {
    int32_t dtm = 0, searched = 0, n_moves = 0, n_keys = 0, key = -1, chk = 0;
    uint64_t mask[4] = {0, 0, 0, 0};
};
struct MateWalk {
    Walk &R;
    int enter(int l, int64_t n, bool *bottom) {
        WalkLevel &L = R.lv[l];
        const bool last = l == R.depth - 1;
        R.visited += (uint64_t)n;
        if (!(l & 1))
            RT(RT_LAUNCH(bo_k_mate_attack, n, R.stream, (const DPos *)L.pos.p, L.cnt.p, L.mate_val.p, L.live.p,
                         l == 0 ? R.keymask.p : (uint64_t *)nullptr, (last ? MT_LAST : 0u) | (l == 0 ? MT_ROOT : 0u)));
        else
            RT(RT_LAUNCH(bo_k_perft_count, n, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (int64_t)0, L.cnt.p, (uint64_t *)nullptr,
                         (uint64_t *)nullptr, 0u));
        *bottom = last;  // (every count is 0: no offsets are read)
        return BO_OK;
    }
    int room(int l, int64_t n) {
        int rc = R.room(l, n);
        if (!rc) rc = R.room_scan(l, n);
        WalkLevel &L = R.lv[l];
        const int64_t m = L.pos.n;
        if (rc || L.mate_val.n >= m) return rc;
        RT(L.mate_val.alloc(m));
        if (!(l & 1)) RT(L.live.alloc(4 * m));
        return BO_OK;
    }
    int room_keys(int64_t n) {
        RT(R.n_keys.room(n));
        RT(R.key.room(n));
        RT(R.keymask.room(4 * n));
        return BO_OK;
    }
    int expand(int l, int64_t a, int64_t e) {
        WalkLevel &L = R.lv[l], &C = R.lv[l + 1];
        if (!(l & 1))
            RT(RT_LAUNCH(bo_k_mate_expand, e - a, R.stream, (const DPos *)L.pos.p, (const uint64_t *)L.off.p, (const uint64_t *)L.live.p, a, C.pos.p,
                         C.tag.p, C.pos.n));
        else
            RT(RT_LAUNCH(bo_k_perft_expand, e - a, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (const uint64_t *)L.off.p, a, C.pos.p,
                         C.tag.p, C.pos.n, 0u));
        return BO_OK;
    }
    int backup(int l, int64_t a, int64_t e) {
        WalkLevel &L = R.lv[l];
        const uint8_t *below = l + 1 < (int)R.lv.size() ? R.lv[l + 1].mate_val.p : nullptr;  // (read only by parents that have children)
        if (l == 0)
            RT(RT_LAUNCH(bo_k_mate_backup_root, e - a, R.stream, (const int32_t *)L.cnt.p, (const uint64_t *)L.off.p, a, below, L.mate_val.p,
                         (const uint64_t *)L.live.p, R.keymask.p, (const int32_t *)R.act.p, (const int32_t *)R.root_moves.p, R.n_keys.p, R.key.p));
        else
            RT(RT_LAUNCH(bo_k_mate_backup, e - a, R.stream, (const int32_t *)L.cnt.p, (const uint64_t *)L.off.p, a, below, L.mate_val.p,
                         (uint32_t)!(l & 1)));
        return BO_OK;
    }
    int after(int64_t a, int64_t n) { return backup(0, a, n); }  // mates in 1 and roots without a live move
};

// Iterative deepening over `roots` (finished in place): n = 1 .. N over the roots still unresolved.  moves [n][256] = the roots' move lists.
int mate_solve(MateWalk &M, std::vector<DPos> &roots, int N, uint64_t max_nodes, std::vector<MateRoot> &out, std::vector<int32_t> &moves) {
    Walk &R = M.R;
    const size_t n = roots.size();
    out.assign(n, MateRoot());
    std::vector<int32_t> rn, chk, active;
    int rc = n ? M.room_keys((int64_t)n) : BO_OK;
    if (!rc) rc = prepare_roots(R, roots, moves, rn, chk, active);
    if (rc) return rc;
    for (size_t r = 0; r < n; r++) {
        out[r].n_moves = rn[r];
        out[r].chk = chk[r];
    }
    std::vector<DPos> sub;
    std::vector<uint8_t> v;
    std::vector<int32_t> nk, ky;
    std::vector<uint64_t> km;
    for (int it = 1; it <= N && !active.empty(); it++) {
        if (max_nodes && R.visited > max_nodes) break;
        const size_t na = active.size();
        R.depth = 2 * it - 1;
        if (R.lv.size() < (size_t)R.depth) R.lv.resize((size_t)R.depth);
        rc = M.room(0, (int64_t)na);
        if (rc) return rc;
        sub.resize(na);
        for (size_t i = 0; i < na; i++) sub[i] = roots[(size_t)active[i]];
        RT(rt_h2d(R.lv[0].pos.p, sub.data(), na * sizeof(DPos), R.stream));
        RT(rt_h2d(R.act.p, active.data(), na * 4, R.stream));
        RT(rt_sync(R.stream));
        rc = walk_level(R, M, 0, (int64_t)na);
        if (rc) return rc;
        v.resize(na); nk.resize(na); ky.resize(na); km.resize(na * 4);
        RT(rt_d2h(v.data(), R.lv[0].mate_val.p, na, R.stream));
        RT(rt_d2h(nk.data(), R.n_keys.p, na * 4, R.stream));
        RT(rt_d2h(ky.data(), R.key.p, na * 4, R.stream));
        RT(rt_d2h(km.data(), R.keymask.p, na * 32, R.stream));
        RT(rt_sync(R.stream));
        std::vector<int32_t> next;
        for (size_t i = 0; i < na; i++) {
            MateRoot &o = out[(size_t)active[i]];
            o.searched = it;
            if (!v[i]) { next.push_back(active[i]); continue; }
            if (v[i] != 2 * it - 1) return fail(BO_E_STATE, "bo_mate: a root resolved at another depth than the iteration's");
            o.dtm = v[i]; o.n_keys = nk[i]; o.key = ky[i];
            for (int w = 0; w < 4; w++) o.mask[w] = km[i * 4 + w];
        }
        active.swap(next);
    }
    return BO_OK;
}

// The principal variation of every solved root: pv [n][W].  Along the line the attacker's move is known (the lowest-index key); the
// defender's replies of all unfinished lines become one batch of roots, solved at the remaining distance.
int mate_pv(MateWalk &M, const std::vector<DPos> &roots, const std::vector<MateRoot> &out, const std::vector<int32_t> &index, int W, int32_t *pv) {
    Walk &R = M.R;
    struct Line { size_t row; DPos A; int32_t key; int d, ply; };
    std::vector<Line> lines;
    for (size_t r = 0; r < roots.size(); r++)
        if (out[r].dtm > 0) {
            lines.push_back(Line{(size_t)index[r], roots[r], out[r].key, out[r].dtm, 0});
            pv[(size_t)index[r] * W] = out[r].key;
        }
    for (;;) {
        std::vector<size_t> S;
        for (size_t i = 0; i < lines.size(); i++)
            if (lines[i].d > 1) S.push_back(i);
        if (S.empty()) return BO_OK;
        const size_t ns = S.size();
        std::vector<DPos> A(ns);
        std::vector<int32_t> keys(ns);
        int nsub = 1;
        for (size_t j = 0; j < ns; j++) { A[j] = lines[S[j]].A; keys[j] = lines[S[j]].key; nsub = std::max(nsub, (lines[S[j]].d - 1) / 2); }
        if (R.lv.size() < 2) R.lv.resize(2);
        int rc = R.room_roots((int64_t)ns);
        if (!rc) rc = M.room_keys((int64_t)ns);
        if (!rc) rc = M.room(0, (int64_t)ns);
        if (rc) return rc;
        WalkLevel &L = R.lv[0];
        RT(rt_h2d(L.pos.p, A.data(), ns * sizeof(DPos), R.stream));
        RT(rt_h2d(R.key.p, keys.data(), ns * 4, R.stream));
        RT(RT_LAUNCH(bo_k_mate_play, (ns + 63) / 64, R.stream, (const DPos *)L.pos.p, (const int32_t *)R.key.p, (int64_t)ns, L.pos.p, L.tag.p));
        RT(RT_LAUNCH(bo_k_mate_roots, ns, R.stream, L.pos.p, R.root_moves.p, R.root_n.p, R.root_chk.p));  // the replies' words
        RT(RT_LAUNCH(bo_k_perft_count, ns, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (int64_t)0, L.cnt.p, (uint64_t *)nullptr,
                     (uint64_t *)nullptr, 0u));
        rc = R.scan(0, (int64_t)ns);
        if (rc) return rc;
        const int64_t T = R.h_word.p[0];
        if (T < (int64_t)ns) return fail(BO_E_STATE, "bo_mate: a defender on a mating line has no reply");
        rc = R.room(1, T);
        if (rc) return rc;
        RT(RT_LAUNCH(bo_k_perft_expand, ns, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (const uint64_t *)L.off.p, (int64_t)0,
                     R.lv[1].pos.p, R.lv[1].tag.p, R.lv[1].pos.n, 0u));
        std::vector<DPos> B((size_t)T);
        std::vector<uint64_t> off(ns + 1);
        std::vector<int32_t> words(ns * BO_MAX_MOVES);
        RT(rt_d2h(B.data(), R.lv[1].pos.p, (size_t)T * sizeof(DPos), R.stream));
        RT(rt_d2h(off.data(), L.off.p, (ns + 1) * 8, R.stream));
        RT(rt_d2h(words.data(), R.root_moves.p, words.size() * 4, R.stream));
        RT(rt_sync(R.stream));
        std::vector<MateRoot> ob;
        std::vector<int32_t> mb;
        rc = mate_solve(M, B, nsub, 0, ob, mb);
        if (rc) return rc;
        for (size_t j = 0; j < ns; j++) {
            Line &ln = lines[S[j]];
            int64_t best = -1;
            bool open = false;  // a reply that is not mated within the distance
            for (int64_t k = (int64_t)off[j]; k < (int64_t)off[j + 1]; k++) {
                open = open || ob[(size_t)k].dtm == 0;
                if (best < 0 || ob[(size_t)k].dtm > ob[(size_t)best].dtm) best = k;
            }
            if (best < 0 || open || ob[(size_t)best].dtm != ln.d - 2) return fail(BO_E_STATE, "bo_mate: the line's replies do not add up to the root's distance");
            int32_t *row = pv + ln.row * (size_t)W + ln.ply;
            row[1] = words[j * BO_MAX_MOVES + (size_t)(best - (int64_t)off[j])];
            row[2] = ob[(size_t)best].key;
            ln.A = B[(size_t)best]; ln.key = ob[(size_t)best].key; ln.d -= 2; ln.ply += 2;
        }
    }
}
}  // namespace

extern "C" int bo_mate(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t max_moves, int64_t capacity,
                       uint64_t max_nodes, uint32_t flags, bo_mate_result *results, int32_t *key_moves, int32_t *pv, int64_t *n_splits, void *stream) {
    if (n_splits) *n_splits = 0;
    if (n_roots < 0 || n_roots > (1 << 20) || (fens != nullptr) == (positions != nullptr))
        return fail(BO_E_ARG, "bo_mate: exactly one of fens and positions, n_roots <= 2^20");
    if (max_moves < 1 || max_moves > BO_MATE_MAX_MOVES) return fail(BO_E_ARG, "bo_mate: max_moves must be 1 .. 16");
    int rc = capacity_ok("bo_mate", capacity);
    if (rc) return rc;
    if (flags & ~(uint32_t)BO_MATE_PV) return fail(BO_E_ARG, "bo_mate: unknown flag bits");
    if (n_roots && (!results || ((flags & BO_MATE_PV) && !pv))) return fail(BO_E_ARG, "bo_mate: results (and pv with BO_MATE_PV) must be given");
    if (n_roots == 0) return BO_OK;
    const size_t N = (size_t)n_roots;
    const int W = 2 * max_moves - 1;
    std::vector<DPos> roots;     // the roots that are positions
    std::vector<int32_t> index;  // their rows in the caller's arrays
    rc = collect_roots("bo_mate", N, fens, positions, results, [](bo_mate_result &o) { o.key = -1; }, BO_MATE_NOT_A_POSITION, roots, index);
    if (rc) return rc;
    if (key_moves)
        for (size_t i = 0; i < N * BO_MAX_MOVES; i++) key_moves[i] = -1;
    if (flags & BO_MATE_PV)
        for (size_t i = 0; i < N * (size_t)W; i++) pv[i] = -1;
    if (roots.empty()) return BO_OK;
    RT(rt_set_device(device));
    Walk R("bo_mate", stream, capacity);
    MateWalk M{R};
    rc = R.words();
    if (rc) return rc;
    std::vector<MateRoot> out;
    std::vector<int32_t> moves;
    rc = mate_solve(M, roots, max_moves, max_nodes, out, moves);
    if (!rc && (flags & BO_MATE_PV)) rc = mate_pv(M, roots, out, index, W, pv);
    if (rc) return rc;
    for (size_t r = 0; r < roots.size(); r++) {
        const size_t i = (size_t)index[r];
        bo_mate_result &o = results[i];
        const MateRoot &m = out[r];
        o.n_moves = m.n_moves;
        if (m.chk & 2) { o.status = BO_MATE_NOT_A_POSITION; o.n_moves = 0; continue; }
        if (m.n_moves == 0) { o.status = (m.chk & 1) ? BO_MATE_CHECKMATED : BO_MATE_STALEMATED; continue; }
        o.dtm = m.dtm; o.searched = m.searched; o.n_keys = m.n_keys; o.key = m.key;
        if (key_moves && m.dtm) {
            int k = 0;
            for (int j = 0; j < BO_MAX_MOVES; j++)
                if (m.mask[j >> 6] >> (j & 63) & 1) key_moves[i * BO_MAX_MOVES + (size_t)k++] = moves[r * BO_MAX_MOVES + (size_t)j];
        }
    }
    for (size_t i = 0; i < N; i++) results[i].nodes = R.visited;
    if (n_splits) *n_splits = R.splits;
    return BO_OK;
}

// ---- the anchor opponent on the device (bo_anchor.h) ---------------------------------------------------------------------------------
// The walk is perft's again, with mate's order of work: a level's chunk is expanded, the chunk below is taken to the bottom, then its
// values are backed up into the parents it came from.  Every level keeps one int16 per entry; level 0 holds the roots that have a move.
// With quiescence Q > 0 (bo_anchor_q) the walk has D + Q levels: 0 .. D - 1 full width, D .. D + Q - 1 over the tactical moves only.
namespace {
struct AnchorWalk {
    Walk &R;
    int enter(int l, int64_t n, bool *bottom) {
        WalkLevel &L = R.lv[l];
        R.visited += (uint64_t)n;
        const bool quiet = l >= R.depth;  // a quiescence level (Q > 0 only): its children are the tactical moves
        *bottom = l == R.levels() - 1;
        if (*bottom && quiet) RT(RT_LAUNCH(bo_k_anchor_qleaf, n, R.stream, (const DPos *)L.pos.p, L.cnt.p, L.val.p, (int32_t)l));
        else if (*bottom)
            RT(RT_LAUNCH(bo_k_anchor_leaf, n, R.stream, (const DPos *)L.pos.p, L.cnt.p, L.val.p, l == 0 ? R.scores.p : (int32_t *)nullptr, (int32_t)l,
                         l == 0 ? AN_ROOT : 0u));
        else if (quiet) RT(RT_LAUNCH(bo_k_anchor_qcount, n, R.stream, (const DPos *)L.pos.p, L.cnt.p, L.val.p, (int32_t)l));
        else RT(RT_LAUNCH(bo_k_anchor_count, n, R.stream, (const DPos *)L.pos.p, L.cnt.p, L.val.p, (int32_t)l));
        return BO_OK;
    }
    int room(int l, int64_t n) {
        int rc = R.room(l, n);
        if (!rc) rc = R.room_scan(l, n);
        if (rc) return rc;
        RT(R.lv[l].val.room(R.lv[l].pos.n));
        return BO_OK;
    }
    int expand(int l, int64_t a, int64_t e) {
        WalkLevel &L = R.lv[l], &C = R.lv[l + 1];
        if (l >= R.depth)
            RT(RT_LAUNCH(bo_k_anchor_qexpand, e - a, R.stream, (const DPos *)L.pos.p, (const uint64_t *)L.off.p, a, C.pos.p, C.tag.p, C.pos.n));
        else
            RT(RT_LAUNCH(bo_k_perft_expand, e - a, R.stream, (const DPos *)L.pos.p, (const int32_t *)L.tag.p, (const uint64_t *)L.off.p, a, C.pos.p,
                         C.tag.p, C.pos.n, 0u));
        return BO_OK;
    }
    int backup(int l, int64_t a, int64_t e) {
        WalkLevel &L = R.lv[l];
        const int16_t *below = l + 1 < R.levels() ? R.lv[l + 1].val.p : nullptr;
        if (l == 0)
            RT(RT_LAUNCH(bo_k_anchor_backup_root, e - a, R.stream, (const int32_t *)R.n_act.p, (const uint64_t *)L.off.p, a, below, R.scores.p,
                         R.score.p, R.n_best.p, R.best.p, (const int32_t *)R.act.p, (const int32_t *)R.root_moves.p));
        else if (l >= R.depth)  // a quiescence level: the entry's own value (the floor) stands unless a tactical move beats it
            RT(RT_LAUNCH(bo_k_anchor_backup_q, e - a, R.stream, (const int32_t *)L.cnt.p, (const uint64_t *)L.off.p, a, below, L.val.p));
        else
            RT(RT_LAUNCH(bo_k_anchor_backup, e - a, R.stream, (const int32_t *)L.cnt.p, (const uint64_t *)L.off.p, a, below, L.val.p));
        return BO_OK;
    }
    // (below level 0, entries behind the last child have no move, or no tactical one: they keep the count kernel's value)
    int after(int64_t a, int64_t n) {
        if (R.levels() == 1) return backup(0, a, n);  // the roots are the leaves: their scores are the leaf kernel's
        return fail(BO_E_STATE, "bo_anchor: a root with moves has no children");
    }
};

// bo_anchor (quiesce 0, who "bo_anchor") and bo_anchor_q: one body; at quiesce 0 the kernels and the bytes are bo_anchor's
int anchor_search(const std::string &who, int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t depth,
                  int32_t quiesce, int64_t capacity, uint32_t flags, bo_anchor_result *results, int32_t *root_moves, int32_t *move_scores,
                  int64_t *n_splits, void *stream) {
    if (n_splits) *n_splits = 0;
    if (n_roots < 0 || n_roots > (1 << 20) || (fens != nullptr) == (positions != nullptr))
        return fail(BO_E_ARG, who + ": exactly one of fens and positions, n_roots <= 2^20");
    if (depth < 1 || depth > BO_ANCHOR_MAX_DEPTH) return fail(BO_E_ARG, who + ": depth must be 1 .. 8");
    if (quiesce < 0 || quiesce > BO_ANCHOR_MAX_QUIESCE) return fail(BO_E_ARG, who + ": quiesce must be 0 .. 8");
    int rc = capacity_ok(who, capacity);
    if (rc) return rc;
    if (flags) return fail(BO_E_ARG, who + ": unknown flag bits");
    if (n_roots && !results) return fail(BO_E_ARG, who + ": results must be given");
    if (n_roots == 0) return BO_OK;
    const size_t N = (size_t)n_roots;
    std::vector<DPos> roots;     // the roots that are positions
    std::vector<int32_t> index;  // their rows in the caller's arrays
    rc = collect_roots(who, N, fens, positions, results, [](bo_anchor_result &o) { o.best = -1; }, BO_ANCHOR_NOT_A_POSITION, roots, index);
    if (rc) return rc;
    for (size_t i = 0; i < N * BO_MAX_MOVES; i++) {
        if (root_moves) root_moves[i] = -1;
        if (move_scores) move_scores[i] = INT32_MIN;
    }
    if (roots.empty()) return BO_OK;
    RT(rt_set_device(device));
    Walk R("bo_anchor", stream, capacity);
    AnchorWalk A{R};
    R.depth = depth; R.quiesce = quiesce;
    R.lv.resize((size_t)R.levels());
    rc = R.words();
    if (rc) return rc;
    const int64_t n = (int64_t)roots.size();
    RT(R.n_act.alloc(n));
    RT(R.scores.alloc(n * BO_MAX_MOVES));
    RT(R.score.alloc(n));
    RT(R.n_best.alloc(n));
    RT(R.best.alloc(n));
    std::vector<int32_t> moves, rn, chk, active, nact;
    rc = prepare_roots(R, roots, moves, rn, chk, active);
    if (rc) return rc;
    std::vector<DPos> sub;
    for (int32_t r : active) { nact.push_back(rn[(size_t)r]); sub.push_back(roots[(size_t)r]); }
    const size_t na = active.size();
    std::vector<int32_t> sc(na * BO_MAX_MOVES), s1(na), nb(na), bm(na);
    if (na) {
        rc = A.room(0, (int64_t)na);
        if (rc) return rc;
        std::vector<int32_t> tags(na, 0);
        RT(rt_h2d(R.lv[0].pos.p, sub.data(), na * sizeof(DPos), stream));
        RT(rt_h2d(R.lv[0].tag.p, tags.data(), na * 4, stream));
        RT(rt_h2d(R.act.p, active.data(), na * 4, stream));
        RT(rt_h2d(R.n_act.p, nact.data(), na * 4, stream));
        RT(rt_sync(stream));  // (host vectors of this frame)
        rc = walk_level(R, A, 0, (int64_t)na);
        if (rc) return rc;
        RT(rt_d2h(sc.data(), R.scores.p, sc.size() * 4, stream));
        RT(rt_d2h(s1.data(), R.score.p, na * 4, stream));
        RT(rt_d2h(nb.data(), R.n_best.p, na * 4, stream));
        RT(rt_d2h(bm.data(), R.best.p, na * 4, stream));
        RT(rt_sync(stream));
    }
    for (size_t r = 0; r < (size_t)n; r++) {
        bo_anchor_result &o = results[(size_t)index[r]];
        if (chk[r] & 2) o.status = BO_ANCHOR_NOT_A_POSITION;
        else if (rn[r] == 0) o.status = (chk[r] & 1) ? BO_ANCHOR_CHECKMATED : BO_ANCHOR_STALEMATED;
        else o.n_moves = rn[r];
    }
    for (size_t k = 0; k < na; k++) {
        const size_t r = (size_t)active[k], i = (size_t)index[r];
        results[i].score = s1[k]; results[i].n_best = nb[k]; results[i].best = bm[k];
        for (int j = 0; j < rn[r]; j++) {
            if (root_moves) root_moves[i * BO_MAX_MOVES + (size_t)j] = moves[r * BO_MAX_MOVES + (size_t)j];
            if (move_scores) move_scores[i * BO_MAX_MOVES + (size_t)j] = sc[k * BO_MAX_MOVES + (size_t)j];
        }
    }
    for (size_t i = 0; i < N; i++) results[i].nodes = R.visited;
    if (n_splits) *n_splits = R.splits;
    return BO_OK;
}
}  // namespace

extern "C" int bo_anchor(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t depth, int64_t capacity,
                         uint32_t flags, bo_anchor_result *results, int32_t *root_moves, int32_t *move_scores, int64_t *n_splits, void *stream) {
    return anchor_search("bo_anchor", device, n_roots, fens, positions, depth, 0, capacity, flags, results, root_moves, move_scores, n_splits, stream);
}

extern "C" int bo_anchor_q(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t depth, int32_t quiesce,
                           int64_t capacity, uint32_t flags, bo_anchor_result *results, int32_t *root_moves, int32_t *move_scores,
                           int64_t *n_splits, void *stream) {
    return anchor_search("bo_anchor_q", device, n_roots, fens, positions, depth, quiesce, capacity, flags, results, root_moves, move_scores,
                         n_splits, stream);
}

extern "C" int bo_anchor_eval(int device, int32_t n, const bo_position *positions, int32_t *ev_out, void *stream) {
    if (n < 0 || n > (1 << 24) || (n && (!positions || !ev_out))) return fail(BO_E_ARG, "bo_anchor_eval: positions and ev_out must be given, n <= 2^24");
    if (n == 0) return BO_OK;
    std::vector<DPos> pos;
    std::vector<int32_t> index;
    for (int32_t i = 0; i < n; i++) {
        DPos p;
        ev_out[i] = INT32_MIN;
        if (!record_ok(positions[i], &p)) continue;
        pos.push_back(p);
        index.push_back(i);
    }
    if (pos.empty()) return BO_OK;
    RT(rt_set_device(device));
    const size_t m = pos.size();
    DevBuf<DPos> d_pos;
    DevBuf<int32_t> d_out;
    std::vector<int32_t> out(m);
    int rc = d_pos.alloc((int64_t)m);
    if (!rc) rc = d_out.alloc((int64_t)m);
    if (!rc) rc = rt_h2d(d_pos.p, pos.data(), m * sizeof(DPos), stream);
    if (!rc) rc = RT_LAUNCH(bo_k_anchor_eval, m, stream, (const DPos *)d_pos.p, d_out.p);
    if (!rc) rc = rt_d2h(out.data(), d_out.p, m * 4, stream);
    const int rs = rt_sync(stream);  // nothing returns between the allocations and here: the stream is idle when the two buffers go
    RT(rc);
    RT(rs);
    for (size_t k = 0; k < m; k++) ev_out[index[k]] = out[k];
    return BO_OK;
}

// ---- endgame tablebases on the device (bo_tb.h) ------------------------------------------------------------------------------------
struct bo_tb {
    int device = 0;
    std::string name;               // "KQK": each side's pieces in the order Q R B N P
    TbTable self{};                 // (codes: device memory)
    int64_t n = 0;                  // entries
    std::vector<bo_tb *> subs;      // the sub-tables the passes read (a subset of what bo_tb_create was given)
    TbTable *d_tabs = nullptr;      // [1 + subs]: this table, then its sub-tables
    uint64_t *d_counter = nullptr;  // [2]
    uint64_t *h_counter = nullptr;  // pinned [2]
    bool complete = false;
    int passes = 0;
    bo_tb_info info{};              // of the complete table
};
namespace {
const char TB_ORDER[] = "QRBNP";
int tb_piece_type(char c) { return c == 'P' ? 1 : c == 'N' ? 2 : c == 'B' ? 3 : c == 'R' ? 4 : c == 'Q' ? 5 : 0; }
// "KQKR" -> the two sides' pieces, each sorted Q R B N P.  false: not a material name
bool tb_parse(const char *m, std::string side[2]) {
    if (!m || m[0] != 'K') return false;
    int k = 0;
    for (const char *c = m + 1; *c; c++) {
        if (*c == 'K') { if (++k > 1) return false; }
        else if (!tb_piece_type(*c)) return false;
        else side[k].push_back(*c);
    }
    if (k != 1) return false;
    for (int i = 0; i < 2; i++) std::sort(side[i].begin(), side[i].end(), [](char a, char b) { return strchr(TB_ORDER, a) < strchr(TB_ORDER, b); });
    return true;
}
uint32_t tb_sig_host(const std::string &strong, const std::string &weak) {
    uint32_t s = 0;
    for (char c : strong) s += 1u << (3 * (tb_piece_type(c) - 1));
    for (char c : weak) s += 1u << (16 + 3 * (tb_piece_type(c) - 1));
    return s;
}
// the name with the stronger side first: more men, then the better first piece in the order Q R B N P
std::string tb_canonical(std::string a, std::string b) {
    auto key = [](const std::string &x) {
        std::string k;
        for (char c : x) k.push_back((char)('0' + (strchr(TB_ORDER, c) - TB_ORDER)));
        return k;
    };
    const bool swap = b.size() > a.size() || (b.size() == a.size() && key(b) < key(a));
    return swap ? "K" + b + "K" + a : "K" + a + "K" + b;
}
bool tb_draw_material(const std::string &a, const std::string &b) {
    const std::string all = a + b;
    return all.empty() || (all.size() == 1 && (all[0] == 'B' || all[0] == 'N'));
}
// the materials one move away from (a, b): a capture, a promotion, a capture with promotion
void tb_children(const std::string &a, const std::string &b, std::vector<std::pair<std::string, std::string>> *out) {
    auto sorted = [](std::string x) {
        std::sort(x.begin(), x.end(), [](char p, char q) { return strchr(TB_ORDER, p) < strchr(TB_ORDER, q); });
        return x;
    };
    for (int side = 0; side < 2; side++) {
        const std::string &own = side ? b : a, &opp = side ? a : b;
        std::vector<std::string> opps{opp};  // the opponent's men after this side's move: as they are, or one taken
        for (size_t i = 0; i < opp.size(); i++) { std::string o = opp; o.erase(i, 1); opps.push_back(o); }
        std::vector<std::string> owns{own};
        if (own.find('P') != std::string::npos) {
            for (const char *q = "QRBN"; *q; q++) { std::string o = own; o[o.find('P')] = *q; owns.push_back(sorted(o)); }
        }
        for (const std::string &o : owns)
            for (const std::string &p : opps) {
                if (o == own && p == opp) continue;
                out->push_back(side ? std::make_pair(p, o) : std::make_pair(o, p));
            }
    }
}
void tb_stats_host(bo_tb *tb, const uint16_t *codes) {
    bo_tb_info &I = tb->info;
    memset(&I, 0, sizeof(I));
    I.n_entries = tb->n;
    I.n_men = tb->self.n_men;
    I.passes = tb->passes;
    I.complete = tb->complete ? 1 : 0;
    snprintf(I.material, sizeof(I.material), "%s", tb->name.c_str());
    uint64_t h = BO_PERFT_FNV_BASIS;
    for (int s = 0; s < 2; s++) {
        bo_tb_side_stats &S = I.side[s];
        S.max_win_ply = S.max_loss_ply = -1;
        for (int64_t i = s * (tb->n / 2); i < (s + 1) * (tb->n / 2); i++) {
            const uint16_t c = codes[i];
            h = (h ^ (uint64_t)(c & 0xFF)) * BO_PERFT_FNV_PRIME;
            h = (h ^ (uint64_t)(c >> 8)) * BO_PERFT_FNV_PRIME;
            if (!c) continue;
            S.legal++;
            if (c == 1) { S.draws++; continue; }
            const int k = c - 2;
            if (k & 1) { S.wins++; S.max_win_ply = std::max(S.max_win_ply, k); }
            else { S.losses++; S.max_loss_ply = std::max(S.max_loss_ply, k); }
        }
    }
    I.fnv1a = h;
}
int tb_refresh_stats(bo_tb *tb, void *stream) {
    std::vector<uint16_t> host((size_t)tb->n);
    RT(rt_d2h(host.data(), tb->self.codes, (size_t)tb->n * 2, stream));
    RT(rt_sync(stream));
    tb_stats_host(tb, host.data());
    return BO_OK;
}
}  // namespace

extern "C" void bo_tb_destroy(bo_tb *tb) {
    if (!tb) return;
    (void)rt_set_device(tb->device);
    rt_free(tb->self.codes);
    rt_free(tb->d_tabs);
    rt_free(tb->d_counter);
    if (tb->h_counter) rt_host_free(tb->h_counter);
    delete tb;
}

extern "C" int bo_tb_create(int device, const char *material, bo_tb *const *sub_tables, int32_t n_sub, bo_tb **out) {
    if (!out || n_sub < 0 || (n_sub && !sub_tables)) return fail(BO_E_ARG, "bo_tb_create: bad arguments");
    *out = nullptr;
    std::string side[2];
    if (!tb_parse(material, side)) return fail(BO_E_ARG, "bo_tb_create: a material is K, the strong side's pieces, K, the weak side's pieces (QRBNP)");
    const int men = 2 + (int)side[0].size() + (int)side[1].size();
    if (men > TB_MAX_MEN) return fail(BO_E_ARG, "bo_tb_create: " + std::string(material) + " has " + std::to_string(men) + " men; tables have 2 to 4");
    if (side[0].find('P') != std::string::npos && side[1].find('P') != std::string::npos)
        return fail(BO_E_CONFIG, "bo_tb_create: " + std::string(material) + " has pawns on both sides: en passant is not handled (a follow-up)");
    for (int i = 0; i < n_sub; i++) {
        if (!sub_tables[i]) return fail(BO_E_ARG, "bo_tb_create: null sub-table");
        if (sub_tables[i]->device != device) return fail(BO_E_ARG, "bo_tb_create: a sub-table lives on another device");
    }
    if (tb_canonical(side[0], side[1]) != "K" + side[0] + "K" + side[1])
        return fail(BO_E_ARG, "bo_tb_create: the strong side comes first: write " + tb_canonical(side[0], side[1]));
    bo_tb *tb = new bo_tb();
    tb->device = device;
    tb->name = "K" + side[0] + "K" + side[1];
    TbTable &T = tb->self;
    T.n_men = men;
    T.sig = tb_sig_host(side[0], side[1]);
    int s = 0;
    T.pt[s] = 6; T.strong[s++] = 1;
    for (char c : side[0]) { T.pt[s] = (uint8_t)tb_piece_type(c); T.strong[s++] = 1; }
    T.pt[s] = 6; T.strong[s++] = 0;
    for (char c : side[1]) { T.pt[s] = (uint8_t)tb_piece_type(c); T.strong[s++] = 0; }
    tb->n = (int64_t)2 << (6 * men);
    // the sub-tables the material needs
    std::vector<std::pair<std::string, std::string>> kids;
    tb_children(side[0], side[1], &kids);
    for (const auto &k : kids) {
        if (tb_draw_material(k.first, k.second)) continue;
        const uint32_t sig = tb_sig_host(k.first, k.second), sig_m = tb_sig_host(k.second, k.first);
        if (sig == T.sig || sig_m == T.sig) continue;
        bo_tb *found = nullptr;
        for (int i = 0; i < n_sub && !found; i++)
            if (sub_tables[i]->self.sig == sig || sub_tables[i]->self.sig == sig_m) found = sub_tables[i];
        const std::string want = tb_canonical(k.first, k.second);
        if (!found) {
            const std::string msg = "bo_tb_create: " + tb->name + " needs the sub-table " + want + ", which was not given";
            delete tb;
            return fail(BO_E_STATE, msg);
        }
        if (!found->complete) { delete tb; return fail(BO_E_STATE, "bo_tb_create: the sub-table " + want + " is not complete (build or upload it first)"); }
        if (std::find(tb->subs.begin(), tb->subs.end(), found) == tb->subs.end()) tb->subs.push_back(found);
    }
    std::vector<TbTable> tabs{T};
    int rc = rt_set_device(device);
    if (!rc) rc = rt_malloc((void **)&T.codes, (size_t)tb->n * 2);
    tabs[0].codes = T.codes;
    for (bo_tb *sub : tb->subs) tabs.push_back(sub->self);
    if (!rc) rc = rt_malloc((void **)&tb->d_tabs, tabs.size() * sizeof(TbTable));
    if (!rc) rc = rt_malloc((void **)&tb->d_counter, 16);
    if (!rc) rc = rt_host_alloc((void **)&tb->h_counter, 16);
    if (!rc) rc = rt_h2d(tb->d_tabs, tabs.data(), tabs.size() * sizeof(TbTable), nullptr);
    if (!rc) rc = rt_memset(T.codes, 0, (size_t)tb->n * 2, nullptr);
    if (!rc) rc = rt_sync(nullptr);  // (tabs is a vector of this frame)
    if (rc) { bo_tb_destroy(tb); return fail(BO_E_HIP, std::string("bo_tb_create: ") + rt_errstr(rc)); }
    *out = tb;
    return BO_OK;
}

extern "C" int bo_tb_build(bo_tb *tb, int32_t max_passes, int32_t *passes, void *stream) {
    if (passes) *passes = 0;
    if (!tb) return fail(BO_E_ARG, "bo_tb_build: null table");
    RT(rt_set_device(tb->device));
    int max_sub = -1;  // the largest value in any sub-table
    for (bo_tb *s : tb->subs)
        for (int k = 0; k < 2; k++) max_sub = std::max(max_sub, std::max(s->info.side[k].max_win_ply, s->info.side[k].max_loss_ply));
    const int grid = (int)(tb->n / TB_RUN), n_tabs = 1 + (int)tb->subs.size();
    tb->complete = false;
    tb->passes = 0;
    RT(RT_LAUNCH(bo_k_tb_init, grid, stream, (const TbTable *)tb->d_tabs));
    bool done = false;
    for (int i = 1; !done && (max_passes < 0 || i <= max_passes); i++) {
        if (i > 0x7ff0) return fail(BO_E_STATE, "bo_tb_build: the passes do not end");
        RT(rt_memset(tb->d_counter, 0, 16, stream));
        RT(RT_LAUNCH(bo_k_tb_pass, grid, stream, (const TbTable *)tb->d_tabs, n_tabs, i, tb->d_counter));
        RT(rt_d2h(tb->h_counter, tb->d_counter, 16, stream));  // the one counter the host reads between passes
        RT(rt_sync(stream));
        tb->passes = i;
        if (tb->h_counter[1]) return fail(BO_E_STATE, "bo_tb_build: " + tb->name + ": a child position has no code (a sub-table is wrong)");
        done = tb->h_counter[0] == 0 && i - 1 > max_sub;
    }
    tb->complete = done;
    if (passes) *passes = tb->passes;
    return tb_refresh_stats(tb, stream);
}

extern "C" int bo_tb_verify(bo_tb *tb, uint64_t *mismatches, void *stream) {
    if (!tb || !mismatches) return fail(BO_E_ARG, "bo_tb_verify: bad arguments");
    RT(rt_set_device(tb->device));
    RT(rt_memset(tb->d_counter, 0, 16, stream));
    RT(RT_LAUNCH(bo_k_tb_verify, (int)(tb->n / TB_RUN), stream, (const TbTable *)tb->d_tabs, 1 + (int)tb->subs.size(), tb->d_counter));
    RT(rt_d2h(tb->h_counter, tb->d_counter, 16, stream));
    RT(rt_sync(stream));
    *mismatches = tb->h_counter[0];
    return BO_OK;
}

extern "C" int bo_tb_stats(bo_tb *tb, bo_tb_info *out) {
    if (!tb || !out) return fail(BO_E_ARG, "bo_tb_stats: bad arguments");
    if (!tb->info.n_entries) {  // neither built nor uploaded yet
        RT(rt_set_device(tb->device));
        const int rc = tb_refresh_stats(tb, nullptr);
        if (rc) return rc;
    }
    *out = tb->info;
    return BO_OK;
}

extern "C" int bo_tb_download(bo_tb *tb, uint16_t *codes, int64_t n_entries) {
    if (!tb || !codes) return fail(BO_E_ARG, "bo_tb_download: bad arguments");
    if (n_entries != tb->n) return fail(BO_E_ARG, "bo_tb_download: " + tb->name + " has " + std::to_string(tb->n) + " entries");
    RT(rt_set_device(tb->device));
    RT(rt_d2h(codes, tb->self.codes, (size_t)tb->n * 2, nullptr));
    RT(rt_sync(nullptr));
    return BO_OK;
}

extern "C" int bo_tb_upload(bo_tb *tb, const uint16_t *codes, int64_t n_entries, int32_t passes) {
    if (!tb || !codes) return fail(BO_E_ARG, "bo_tb_upload: bad arguments");
    if (n_entries != tb->n) return fail(BO_E_ARG, "bo_tb_upload: " + tb->name + " has " + std::to_string(tb->n) + " entries");
    RT(rt_set_device(tb->device));
    RT(rt_h2d(tb->self.codes, codes, (size_t)tb->n * 2, nullptr));
    RT(rt_sync(nullptr));
    tb->complete = true;
    tb->passes = passes;
    tb_stats_host(tb, codes);
    return BO_OK;
}

extern "C" int bo_tb_probe(bo_tb *const *tbs, int32_t n_tb, const bo_position *positions, int32_t n, uint16_t *codes, int32_t *status, void *stream) {
    if (n_tb < 0 || n_tb > TB_MAX_TABLES || (n_tb && !tbs) || n < 0 || (n && (!positions || !codes || !status)))
        return fail(BO_E_ARG, "bo_tb_probe: bad arguments (at most 64 tables)");
    std::vector<TbTable> tabs;
    for (int i = 0; i < n_tb; i++) {
        if (!tbs[i]) return fail(BO_E_ARG, "bo_tb_probe: null table");
        if (tbs[i]->device != tbs[0]->device) return fail(BO_E_ARG, "bo_tb_probe: the tables live on different devices");
        if (!tbs[i]->complete) return fail(BO_E_STATE, "bo_tb_probe: the table " + tbs[i]->name + " is not complete");
        tabs.push_back(tbs[i]->self);
    }
    if (n == 0) return BO_OK;
    if (n_tb) RT(rt_set_device(tbs[0]->device));
    TbTable *d_tabs = nullptr;
    bo_position *d_pos = nullptr;
    uint16_t *d_codes = nullptr;
    int32_t *d_status = nullptr;
    int rc = rt_malloc((void **)&d_tabs, std::max<size_t>(1, tabs.size()) * sizeof(TbTable));
    if (!rc) rc = rt_malloc((void **)&d_pos, (size_t)n * sizeof(bo_position));
    if (!rc) rc = rt_malloc((void **)&d_codes, (size_t)n * 2);
    if (!rc) rc = rt_malloc((void **)&d_status, (size_t)n * 4);
    if (!rc && n_tb) rc = rt_h2d(d_tabs, tabs.data(), tabs.size() * sizeof(TbTable), stream);
    if (!rc) rc = rt_h2d(d_pos, positions, (size_t)n * sizeof(bo_position), stream);
    if (!rc) rc = RT_LAUNCH(bo_k_tb_probe, (n + 63) / 64, stream, (const TbTable *)d_tabs, n_tb, (const bo_position *)d_pos, n, d_codes, d_status);
    if (!rc) rc = rt_d2h(codes, d_codes, (size_t)n * 2, stream);
    if (!rc) rc = rt_d2h(status, d_status, (size_t)n * 4, stream);
    const int rc2 = rt_sync(stream);
    rt_free(d_tabs); rt_free(d_pos); rt_free(d_codes); rt_free(d_status);
    if (rc || rc2) return fail(BO_E_HIP, std::string("bo_tb_probe: ") + rt_errstr(rc ? rc : rc2));
    return BO_OK;
}

// ---- tablebases in the search (bo_tree.h: step_body<true>, root_prepare) -------------------------------------------------------------
extern "C" int bo_engine_tablebases(bo_engine *e, bo_tb *const *tbs, int32_t n_tb, int32_t flags) {
    if (!e || n_tb < 0 || (n_tb && !tbs)) return fail(BO_E_ARG, "bo_engine_tablebases: bad arguments");
    if (n_tb > TB_MAX_TABLES) return fail(BO_E_ARG, "bo_engine_tablebases: at most " + std::to_string(TB_MAX_TABLES) + " tables");
    if (flags & ~(TBF_SEARCH | TBF_ADJUDICATE)) return fail(BO_E_ARG, "bo_engine_tablebases: unknown flag bits (1 probe in the search, 2 adjudicate at the root)");
    if (e->fast) return fail(BO_E_CONFIG, "bo_engine_tablebases: reference-semantics engines only");
    std::vector<TbTable> tabs;
    for (int i = 0; i < n_tb; i++) {
        if (!tbs[i]) return fail(BO_E_ARG, "bo_engine_tablebases: null table");
        if (tbs[i]->device != e->device) return fail(BO_E_ARG, "bo_engine_tablebases: the table " + tbs[i]->name + " lives on another device than the engine");
        if (!tbs[i]->complete) return fail(BO_E_STATE, "bo_engine_tablebases: the table " + tbs[i]->name + " is not complete");
        tabs.push_back(tbs[i]->self);
    }
    RT(rt_set_device(e->device));
    if (n_tb) {
        RT(rt_h2d(e->d_tb_tabs, tabs.data(), tabs.size() * sizeof(TbTable), nullptr));
        RT(rt_sync(nullptr));  // (tabs is a vector of this frame)
    }
    e->d.tb_n = n_tb;
    e->d.tb_flags = n_tb ? flags : 0;
    return BO_OK;
}

extern "C" int bo_engine_tb_stats(bo_engine *e, int32_t *tb_nodes, int32_t *tb_sims, int32_t *adjudicated, void *stream) {
    if (!e) return fail(BO_E_ARG, "null engine");
    const size_t G = (size_t)e->d.c.G;
    std::vector<int> h(3 * G);
    RT(rt_d2h(h.data(), e->d.tb_stat, 3 * G * 4, stream));
    RT(rt_sync(stream));
    for (size_t g = 0; g < G; g++) {
        if (tb_nodes) tb_nodes[g] = h[3 * g];
        if (tb_sims) tb_sims[g] = h[3 * g + 1];
        if (adjudicated) adjudicated[g] = h[3 * g + 2];
    }
    return BO_OK;
}
