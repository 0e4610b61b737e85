// tests/wave_emulator/poison_driver.cpp -- TEST INFRASTRUCTURE: memory-safety evidence for the tree step on NON-FINITE evaluation rows.
// A stand-alone program over the C ABI (include/betaone_engine.h), compiled TOGETHER with bo_engine.cpp -DBO_WAVE_EMU and
// -fsanitize=address,undefined by poison_driver.sh next to it: the device code runs lane by lane on the CPU, "device" pointers are
// host pointers.  It is run as an executable, never through pytest and never on a GPU.
//
// Per case a 2-slot engine (60 simulations, batch 8) searches; slot 0's rows are poisoned at its root evaluation or from its 4th
// evaluation on, slot 1 gets a clean net.  The driver knows no move lists, so "one NaN at a legal index" is played as NaN at every
// second action and "+inf at a legal index" as +inf at every third: some legal entries of every row are hit and some are not.
// Reference-semantics engines with widen 1.5 and 4.0, and the fast mode with 4 leaves per step.  Checked per case: slot 0 carries
// BO_ST_NAN_SCORE and slot 1 no bit, both searches ran all their simulations, and slot 0's tree (bo_debug_tree) has finite priors and
// q, parents and child blocks inside the tree, no move 0 below the root and no two siblings with the same move.  The sanitizers check
// the rest.  Exit status 0 and a last line "poison driver: clean" mean exactly that.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "betaone_engine.h"
#include "betaone_lab.h"

#define CHECK(x) do { int rc_ = (x); if (rc_) { std::fprintf(stderr, "%s -> %d: %s\n", #x, rc_, bo_last_error()); return 1; } } while (0)

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();
enum Poison { ROW_NAN, HALF_NAN, THIRD_INF, VALUE_NAN, VALUE_INF, LOGIT_NAN, LOGIT_INF, LOGITS_ALL_NINF, N_POISON };
static const char *const NAMES[N_POISON] = {"probs: row all NaN", "probs: NaN at every 2nd action", "probs: +inf at every 3rd action", "probs: value NaN",
                                            "probs: value +inf", "logits: one NaN", "logits: one +inf", "logits: row all -inf"};

static uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// a clean evaluation of one input row: a function of the position only
static void evaluate(const float *planes, bool logits, float *pol, float *val) {
    uint64_t h = 0;
    for (int i = 98 * 64; i < BO_ROW_FLOATS; i++) h = mix(h ^ (uint64_t)(int64_t)planes[i] ^ ((uint64_t)i << 20));
    double sum = 0.0;
    for (int a = 0; a < BO_NUM_ACTIONS; a++) {
        const double u = (double)(mix(h + (uint64_t)a) >> 40) / 16777216.0;
        pol[a] = logits ? (float)((u - 0.5) * 6.0) : (float)std::exp((u - 0.5) * 6.0);
        sum += pol[a];
    }
    if (!logits) for (int a = 0; a < BO_NUM_ACTIONS; a++) pol[a] = (float)(pol[a] / sum);
    *val = (float)(((double)(mix(h ^ 0xABCDEFull) >> 40) / 16777216.0 * 2.0 - 1.0) * 0.9);
}
// (fast: that mode's softmax runs over the legal moves only -- a single logit would not be read, so the NaN / +inf logits are spread like the
//  probabilities; the reference-semantics step takes the maximum and the sum over the whole row: one logit anywhere spoils it)
static void poison_row(int p, bool fast, float *pol, float *val) {
    if (fast && p == LOGIT_NAN) p = HALF_NAN;
    if (fast && p == LOGIT_INF) p = THIRD_INF;
    switch (p) {
        case ROW_NAN: for (int a = 0; a < BO_NUM_ACTIONS; a++) pol[a] = NaN; break;
        case HALF_NAN: for (int a = 0; a < BO_NUM_ACTIONS; a += 2) pol[a] = NaN; break;
        case THIRD_INF: for (int a = 0; a < BO_NUM_ACTIONS; a += 3) pol[a] = Inf; break;
        case VALUE_NAN: *val = NaN; break;
        case VALUE_INF: *val = Inf; break;
        case LOGIT_NAN: pol[1234] = NaN; break;
        case LOGIT_INF: pol[1234] = Inf; break;
        case LOGITS_ALL_NINF: for (int a = 0; a < BO_NUM_ACTIONS; a++) pol[a] = -Inf; break;
    }
}

static int check_tree(bo_engine *e, const char *what) {
    int32_t n = 0;
    CHECK(bo_debug_tree(e, 0, nullptr, 0, &n, nullptr));
    std::vector<bo_node> t((size_t)(n > 0 ? n : 1));
    CHECK(bo_debug_tree(e, 0, t.data(), n, &n, nullptr));
    int bad = 0;
    for (int i = 0; i < n; i++) {
        const bo_node &x = t[(size_t)i];
        if (!std::isfinite(x.prior) || !std::isfinite(x.q_value)) bad++;
        if (i > 0 && (x.parent < 0 || x.parent >= n || x.move == 0)) bad++;
        if (x.n_children < 0 || (x.n_children > 0 && (x.first_child <= 0 || x.first_child + x.n_children > n))) { bad++; continue; }
        for (int a = 0; a < x.n_children; a++)
            for (int b = a + 1; b < x.n_children; b++)
                if (t[(size_t)(x.first_child + a)].move == t[(size_t)(x.first_child + b)].move) bad++;
    }
    if (bad) std::fprintf(stderr, "%s: %d defects in slot 0's tree of %d nodes\n", what, bad, n);
    return bad;
}

static int run_case(int fast_L, double widen, int p, bool at_root, int *failures) {
    const int G = 2, L = fast_L ? fast_L : 1, S = 60, R = G * L;
    const bool logits = p >= LOGIT_NAN;
    bo_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.n_games = G; cfg.num_simulations = S; cfg.mcts_batch_size = 8; cfg.max_plies = 64;
    cfg.cpuct = 1.0; cfg.widen_coeff = widen; cfg.dirichlet_alpha = 0.0; cfg.dirichlet_epsilon = 0.25;
    cfg.mode = fast_L ? 1 : 0; cfg.leaves_per_step = L;
    bo_engine *e = nullptr;
    CHECK(bo_engine_create(&cfg, 0, &e));
    const int32_t slots[2] = {0, 1};
    const char *fens[2] = {nullptr, "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"};
    const char *moves[2] = {nullptr, nullptr};
    CHECK(bo_games_reset(e, G, slots, fens, moves, nullptr));
    std::vector<float> nn_in((size_t)R * BO_ROW_FLOATS, 0.0f), pol((size_t)R * BO_NUM_ACTIONS, 0.0f), val((size_t)R, 0.0f);
    const int32_t go[2] = {1, 1};
    CHECK(bo_search_begin(e, go, nullptr, nn_in.data(), nullptr));
    CHECK(bo_step(e, nullptr, nullptr, BO_POLICY_NONE, nn_in.data(), nullptr));
    int steps = 0, evals0 = 0;
    char what[160];
    std::snprintf(what, sizeof(what), "%s widen %.1f, %s, %s", fast_L ? "fast L=4" : "reference", widen, NAMES[p], at_root ? "root evaluation" : "from the 4th evaluation");
    for (;;) {
        int32_t running = 0, requested = 0, mask[2] = {0, 0};
        CHECK(bo_search_poll(e, &running, &requested, mask, nullptr));
        if (!running) break;
        for (int r = 0; r < R; r++) evaluate(&nn_in[(size_t)r * BO_ROW_FLOATS], logits, &pol[(size_t)r * BO_NUM_ACTIONS], &val[(size_t)r]);
        if (fast_L || mask[0]) {
            evals0++;
            if (at_root ? evals0 == 1 : evals0 >= 4)
                for (int r = 0; r < L; r++) poison_row(p, fast_L != 0, &pol[(size_t)r * BO_NUM_ACTIONS], &val[(size_t)r]);
        }
        CHECK(bo_step(e, pol.data(), val.data(), logits ? BO_POLICY_LOGITS : BO_POLICY_PROBS, nn_in.data(), nullptr));
        if (++steps > 2 * S + 4) { std::fprintf(stderr, "%s: the search does not end\n", what); *failures += 1; break; }
    }
    int32_t st[2] = {0, 0};
    CHECK(bo_engine_status(e, st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    static int32_t res_n[2], res_idx[2 * BO_RES_CAP], best_idx[2], best_mv[2], total[2];
    static float res_val[2 * BO_RES_CAP];
    CHECK(bo_search_result(e, res_n, res_idx, res_val, best_idx, best_mv, total, nullptr));
    int bad = 0;
    if (!(st[0] & BO_ST_NAN_SCORE) || st[1] != 0) { std::fprintf(stderr, "%s: status %d %d (wanted bit %d in slot 0 only)\n", what, st[0], st[1], BO_ST_NAN_SCORE); bad++; }
    if (total[0] != S || total[1] != S) { std::fprintf(stderr, "%s: visits %d %d of %d\n", what, total[0], total[1], S); bad++; }
    bad += check_tree(e, what);
    std::printf("%-96s status %3d %d  steps %3d  %s\n", what, st[0], st[1], steps, bad ? "DEFECTS" : "ok");
    *failures += bad ? 1 : 0;
    bo_engine_destroy(e);
    return 0;
}

int main() {
    if (bo_abi_version() != BO_ABI_VERSION) return 2;
    int failures = 0, cases = 0;
    const struct { int fast_L; double widen; } modes[3] = {{0, 1.5}, {0, 4.0}, {4, 1.5}};
    for (const auto &m : modes)
        for (int p = 0; p < N_POISON; p++)
            for (int at_root = 1; at_root >= 0; at_root--) {
                if ((p == VALUE_NAN || p == VALUE_INF) && at_root) continue;  // the root's evaluation gives priors only: its value is not backed up
                if (run_case(m.fast_L, m.widen, p, at_root != 0, &failures)) return 1;
                cases++;
            }
    std::printf("poison driver: %s (%d cases, %d with defects)\n", failures ? "DEFECTS" : "clean", cases, failures);
    return failures ? 1 : 0;
}
