/*
 * include/betaone_engine.h -- C ABI of the MI355X self-play rollout engine (libbetaone_hip.so).
 *
 * The reference (kevinh-e/BetaOne) has no FFI layer: its hot path is plain Python
 *   run_mcts(root_board, model, history, tracker)      /root/reference/mcts.py:155-280
 *   _evaluate_batch(nodes, paths, model)               /root/reference/mcts.py:283-295
 *   run_self_play_game(model, game_id)                 /root/reference/self_play.py:84-216
 *   utils.encode_board / move_to_index / index_to_move /root/reference/utils.py:111-365
 * called by main.py:56 and uci.py:63,84.  This header is what a ctypes binding of that path
 * binds instead; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * BO_E_* code and never throws; bo_last_error() gives the text.  "dev" pointers are raw device
 * addresses (tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All kernels are enqueued on `stream`; functions documented as "synchronises" wait for it.
 * One engine = one GPU = G game slots; NN input row g / policy row g / value g belong to slot g.
 */
#ifndef BETAONE_ENGINE_H
#define BETAONE_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an output size, a struct, or the layout a caller has to produce changes (2: bo_debug_profile (betaone_lab.h) returns
 * [G][BO_PROF_SLOTS = 16] counters, the BO_TOWER_WINOGRAD packed-weight K order for 128 filters is winograd_k_order's;
 * 3: fast-mode arenas are allocated in 128-byte granules of 8 records, bo_fast_stats counts granules; 7: resignation and root values,
 * additions only; 8: analysis of games that are on the device -- bo_games_reset_dev, bo_search_begin_dev, bo_analysis_result,
 * bo_pgn_after, bo_pgn_spans, status bit BO_ST_BAD_RANGE -- additions only; 9: the value target as a mix of the game's outcome and
 * the search's root value -- bo_replay_add_game_values, bo_replay_values, bo_replay_sample_sparse_q, bo_train_loss_forward_mix,
 * bo_train_loss_backward_mix -- additions only; 10: perft on the device -- bo_perft, bo_perft_result -- additions only; 11: endgame
 * tablebases on the device -- bo_tb_create, bo_tb_build, bo_tb_verify, bo_tb_stats, bo_tb_download, bo_tb_upload, bo_tb_probe,
 * bo_tb_destroy -- additions only; 12: held-out validation metrics on the device -- bo_train_metrics and the BO_METRIC_* columns --
 * additions only; 13: a search that waits for its last leaf evaluation is finished without it -- bo_search_close -- addition only;
 * 14: endgame tablebases inside the search and at the root -- bo_engine_tablebases, bo_engine_tb_stats, bo_debug_tree's terminal codes
 * 3 / 4 / 5, bo_root_info's terminal code 3 -- additions only; 15: reanalysis of self-play records -- bo_records_ring,
 * bo_reanalysis_result, status bit BO_ST_PI_OVERFLOW -- additions only; 16: opening books -- bo_book_insert -- addition only;
 * 18: board symmetries in the replay samplers -- bo_replay_sample_sym, _sparse_sym, _sparse_q_sym, _merged_sym -- additions only;
 * 19: forced mates on the device -- bo_mate, bo_mate_result -- additions only; 20: the anchor opponent -- bo_anchor, bo_anchor_eval,
 * bo_anchor_result -- additions only; 21: an interactive front end on the fast mode -- bo_search_stop accepts fast-mode engines,
 * bo_search_info -- additions only; 22: quiescence behind the anchor's fixed-depth walk -- bo_anchor_q, BO_ANCHOR_MAX_QUIESCE --
 * additions only).
 * A caller checks
 * bo_abi_version() == BO_ABI_VERSION before anything else (tests/c_abi_smoke.c). */
#define BO_ABI_VERSION 22
#define BO_NUM_ACTIONS 4672          /* config.NUM_ACTIONS, config.py:29 */
#define BO_INPUT_CHANNELS 120        /* config.INPUT_CHANNELS, config.py:28 */
#define BO_ROW_FLOATS (120 * 64)
#define BO_MAX_LEGAL 256
#define BO_RES_CAP 256

enum {
    BO_OK = 0,
    BO_E_ARG = -1,        /* bad argument */
    BO_E_HIP = -2,        /* HIP runtime error */
    BO_E_CONFIG = -3,     /* unsupported configuration (see bo_engine_create) */
    BO_E_FEN = -4,        /* unparsable FEN / UCI move */
    BO_E_STATE = -5       /* call out of order */
};

/* per-game status bits reported by bo_engine_status() */
enum {
    BO_ST_NODE_OVERFLOW = 1, BO_ST_DEPTH_OVERFLOW = 2, BO_ST_NAN_SCORE = 4, BO_ST_PLY_OVERFLOW = 8,
    /* BO_ST_NAN_SCORE -- non-finite evaluations.  A game is flagged when a prior the engine would store, or a value it would back up, is
     * NaN or +-inf: a probability at a legal move of the row (BO_POLICY_PROBS; entries at other actions of a leaf's row are never
     * read), a softmax term whose row maximum or sum is not finite (BO_POLICY_LOGITS: one NaN or +inf logit, a row of -inf only; single
     * -inf logits are legitimate and give probability 0), a root prior after the noise renormalisation, a leaf's value.  The bit is set
     * by the bo_step / bo_step_heads call that consumes the row, not by a later selection.  The offender counts as 0.0f (fast mode: a
     * legal mass that is not finite gives uniform priors, like a mass of 0), so every stored prior is finite, every node's move comes
     * from its own parent's legal moves without duplicates among siblings, the search runs to its end, and other slots are untouched.
     * Finite rows are never flagged.  (A selection that meets NaN scores all the same still sets the bit, as before.) */
    /* BO_ST_DEPTH_OVERFLOW in FAST mode -- the path cap.  A descent's path holds at most 64 nodes, the root included.  A descent whose
     * path already holds 64 nodes ends at the child it chose last, even though that child is expanded: the visit is backed up as a
     * draw (0.0) over those 64 nodes, with the step's other simulations and in their order, and is counted among the terminal
     * simulations; the child's state does not change, so later descents may go on ending there.  The search delivers all its
     * simulations and pi is a distribution over the legal moves.  The bit is set in the step that cut the descent short and stays set
     * until the slot is reset.  Callers that check the status words (Engine.check_status) treat it as a fault today -- unlike a
     * full arena (BO_ST_NODE_OVERFLOW), which they count as a condition of one search. */
    BO_ST_ILLEGAL_ACTION = 16, BO_ST_UL_OVERFLOW = 32, BO_ST_TRK_OVERFLOW = 64,
    BO_ST_BAD_RANGE = 128,  /* (ABI 8) bo_games_reset_dev: the slot's positions are not inside the array */
    BO_ST_PI_OVERFLOW = 256 /* (ABI 15) bo_reanalysis_result: the search's pi has more entries than the rows hold.  A condition of one
                             * record: set in bo_reanalysis.status only, never in the slot's own status word */
};

enum { BO_POLICY_NONE = 0, BO_POLICY_LOGITS = 1, BO_POLICY_PROBS = 2 };

/* The constants of config.py that the path reads at call time (config.py:32-41,59). */
typedef struct {
    int32_t n_games;            /* G: game slots resident on this GPU */
    int32_t num_simulations;    /* config.NUM_SIMULATIONS */
    int32_t mcts_batch_size;    /* config.MCTS_BATCH_SIZE */
    int32_t max_plies;          /* capacity of one game's position stack (>= plies + 2) */
    double cpuct;               /* config.CPUCT */
    double widen_coeff;         /* config.WIDEN_COEFF (>= 1.0, int(w*sqrt(batch)) <= 32) */
    double dirichlet_alpha;     /* config.DIRICHLET_ALPHA (only its sign is used on the device) */
    double dirichlet_epsilon;   /* config.DIRICHLET_EPSILON */
    int32_t mode;               /* 0 = the reference's search semantics (bit-exact); 1 = FAST mode (csrc/bo_fastw.h):
                                 * virtual loss, leaves_per_step distinct leaves per game per step, full-width
                                 * expansion -- NOT the reference's semantics */
    int32_t leaves_per_step;    /* FAST mode: L (1..64); NN tensors then have n_games*L rows, row = g*L + r */
    int32_t fast_arena_granules;/* FAST mode: 128-byte granules per game arena (there are two per game); 0 = default, 24 per possible
                                 * expansion of this and the previous search (3 KB; a chess node's run takes ~6).  A run that does
                                 * not fit is refused (BO_ST_NODE_OVERFLOW) and the search goes on with that leaf unexpanded. */
} bo_config;

/* A position as plain data.  bb: pawns, knights, bishops, rooks, queens, kings, white, black. */
typedef struct {
    uint64_t bb[8];
    int32_t turn;             /* 1 white, 0 black */
    uint32_t castling;        /* bit0 K, bit1 Q, bit2 k, bit3 q */
    int32_t ep_square;        /* python-chess Board.ep_square, -1 = None */
    int32_t ep_key;           /* -2: derive (ep square iff an ep capture is legal); else the key's ep (-1 none) */
    int32_t halfmove_clock;
    int32_t fullmove_number;
} bo_position;

typedef struct bo_engine bo_engine;

int bo_abi_version(void);
const char *bo_last_error(void);

int bo_engine_create(const bo_config *cfg, int device, bo_engine **out);
void bo_engine_destroy(bo_engine *e);

/* ---- game set-up ---------------------------------------------------------------------------
 * (Re)start the games in `slots[0..n)`: position `fens[i]` (NULL = standard start, self_play.py:91)
 * followed by the space-separated UCI moves `moves[i]` (NULL = none) -- i.e. a python-chess Board
 * with its move stack, which the draw rules need (mcts.py:36,152).  The repetition tracker holds
 * every position of that stack and the history planes use the <=7 positions before the current
 * one (self_play.py:93-109,182-184).  Also prepares the first search root.  Synchronises. */
int bo_games_reset(bo_engine *e, int n, const int32_t *slots, const char *const *fens, const char *const *moves,
                   void *stream);

/* Same, but with the caller's own history boards and tracker contents (uci.py:62-63 passes
 * whatever it accumulated): hist[i*7 .. i*7+n_hist[i]) boards BEFORE the root (oldest first),
 * tracker keys trk[trk_off[i] .. trk_off[i+1]) with their counts.  Synchronises. */
int bo_games_reset_ex(bo_engine *e, int n, const int32_t *slots, const char *const *fens, const char *const *moves,
                      const bo_position *hist, const int32_t *n_hist, const bo_position *trk,
                      const int32_t *trk_counts, const int32_t *trk_off, void *stream);

/* Root facts the host needs before a search: number of legal moves (np.random.dirichlet needs it,
 * mcts.py:191-192) and is_game_over(claim_draw=True) of the current position (0 no, 1 side to move
 * is checkmated, 2 draw; self_play.py:101-102; with bo_engine_tablebases' adjudication also 3: the tables give the root as lost for
 * the side to move -- the game ends as if that side had resigned -- and 2 for a root they give as drawn).  Synchronises.  Arrays are [G]. */
int bo_root_info(bo_engine *e, int32_t *n_legal, int32_t *terminal, int32_t *ply, void *stream);

/* ---- one search per game, all games in lock step ------------------------------------------------
 * bo_search_begin: start run_mcts for every slot with go[g] != 0.  noise[g*256 + i] is the
 * Dirichlet sample of the i-th legal move of game g in python-chess order (mcts.py:192-198);
 * may be NULL when dirichlet_alpha <= 0.  Writes planes 0..97 of NN input row g (nn_in_dev,
 * float32 [G,120,8,8], NCHW contiguous). */
int bo_search_begin(bo_engine *e, const int32_t *go, const double *noise, float *nn_in_dev, void *stream);

/* bo_step: consume the net's output for the rows requested by the previous step (policy_dev
 * float32 [G,4672] logits or softmax probabilities per `policy_kind`, value_dev float32 [G]),
 * run select / terminal backups / expand+backup flushes until each game needs its next
 * evaluation, and write that leaf's planes into nn_in_dev row g.  First call of a search:
 * policy_kind = BO_POLICY_NONE.  Asynchronous on `stream`. */
int bo_step(bo_engine *e, const float *policy_dev, const float *value_dev, int policy_kind, float *nn_in_dev,
            void *stream);
/* (ABI 6) bo_step with the TAIL of the evaluate stage inside the step kernel: behind bo_nn_heads(flags & 4) -- which stops after the
 * logits and the partial sums of value_fc1 -- the wave that consumes a game's row does what the stage's rows kernel would have done
 * with it: the softmax of mcts.py:185,287 (at the indices it needs) and value = tanh(value_fc2(relu(value_fc1 + bias)))
 * (network.py:195-197).  Same float32 operations in the same order as bo_nn_heads' own second launch: the search sees the same
 * bits either way (tests/test_baseline_configs_gpu.py), one launch and one pass over the rows less per evaluation.
 * logits_dev [G,4672]; vpart_dev = bo_nn_heads' scratch_dev [16][rows][256] (rows = that call's batch >= G, row g <-> game g);
 * b1_dev [256], w2_dev [256], b2_dev [1] = value_fc1.bias, value_fc2.weight, value_fc2.bias.  Reference-semantics engines only. */
int bo_step_heads(bo_engine *e, const float *logits_dev, const float *vpart_dev, const float *b1_dev, const float *w2_dev,
                  const float *b2_dev, int rows, float *nn_in_dev, void *stream);

/* How many searches are still running / how many rows were requested by the last step.
 * requested_mask (optional, [G] int32) marks the rows the net must evaluate.  Synchronises. */
int bo_search_poll(bo_engine *e, int32_t *n_running, int32_t *n_requested, int32_t *requested_mask, void *stream);

/* Interrupt running searches between two steps (the reference can only stop between whole
 * searches, uci.py:73): for every game with stop_mask[g] != 0 (NULL = all) whose search is running, the pending rows are
 * flushed exactly like the tail batch of mcts.py:256-257, an evaluation still outstanding is dropped, and the search is
 * marked finished -- bo_search_result then returns what the reference returns for NUM_SIMULATIONS = sims_done[g]
 * (optional out, [G] int32: simulations completed per game).  Synchronises.
 * (ABI 21) FAST-mode engines: the step in flight -- the rows the last bo_step selected, which wait for their evaluation -- is
 * ABANDONED: its simulations are not counted and nothing of them is in the tree (the virtual loss is never written, a step is backed
 * up by the NEXT step, and materialising a row writes no tree record), the control block's rows and simulations go to 0, no evaluation
 * is requested any more and the search is marked finished.  sims_done[g] -- a multiple of leaves_per_step unless the search was about
 * to end -- and the tree are those after the last completed backup: a stopped fast search equals a search created with
 * num_simulations = sims_done[g], and bo_search_result answers from that tree.  One exception: a search stopped before the step
 * that consumes its ROOT's evaluation has an unexpanded root, sims_done 0 and a uniform pi (a search with num_simulations = 0 would
 * still have expanded the root).  The per-slot evaluation counter of bo_engine_status includes the dropped rows.  A later
 * bo_search_begin on the slot continues in the same tree.  Slots that are idle, finished or not in the mask are untouched. */
int bo_search_stop(bo_engine *e, const int32_t *stop_mask, int32_t *sims_done, void *stream);

/* (ABI 13) Finish, WITHOUT its evaluation, every running search that waits for its last leaf evaluation: a leaf is requested, no rows
 * are pending and NUM_SIMULATIONS - sims_done <= MCTS_BATCH_SIZE.  The step behind that evaluation would re-select the leaf for the
 * remaining simulations, expand it and back its value up (mcts.py:247-257, 291-295): every node from the leaf up to the root gains that
 * many visits.  Here the visits are added and the search is marked finished; the leaf is not expanded and no q_value moves.
 * bo_search_result, both turns and the records -- which read the visit counts of the root's children (mcts.py:259-280) -- give what
 * they give behind the evaluated step; root values and the tree below the root do not (BO_E_STATE with bo_engine_root_values on).
 * Every other search -- finished, idle, waiting for its root's evaluation, in the middle of a run of terminal simulations, or with more
 * than one batch to go -- is left untouched: the caller goes on with bo_step as before.  Reference-semantics engines only.
 * Asynchronous on `stream`; capturable. */
int bo_search_close(bo_engine *e, void *stream);

/* Result of the finished searches (mcts.py:259-280): sparse pi (res_n[g] entries of
 * (action index, probability) at [g*BO_RES_CAP ..]), best move as action index (-1: no legal
 * move, the reference raises ValueError) and as from|to<<6|promo<<12, total root-child visits.
 * Synchronises. */
int bo_search_result(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx,
                     int32_t *best_move, int32_t *total_visits, void *stream);

/* self_play.py:125-184: play action[g] (an index into the 4672 actions; -2 = play the search's
 * best move; -1 = leave the game alone) with the reference's decode-error / illegal-move
 * fallbacks, push it on the game's stack and tracker, prepare the next root.  Asynchronous: the kernel reads the actions from a
 * two-deep pinned ring of the engine's when it runs; a call whose half of the ring is still unread (two calls back-to-back without
 * the device catching up) waits for that kernel first, so any number of calls may be enqueued. */
int bo_play(bo_engine *e, const int32_t *action, void *stream);

/* ---- per-move host work, natively -----------------------------------------------------------------
 * The reference draws np.random.dirichlet (mcts.py:192) and np.random.choice (self_play.py:73) once per move.
 * With one legacy MT19937 stream per game slot kept inside the engine (bit-compatible with
 * numpy.random.RandomState(seed): same seeding, same legacy gamma/dirichlet algorithm, same draws), the per-move
 * host work of thousands of games is two calls:
 *   bo_selfplay_sample : bo_search_result + select_move_with_temperature (self_play.py:59-80) for every active
 *                        game; action_out[g] = sampled action index, -1 inactive, -3 "pi has more than two
 *                        non-zero entries (or temperature 0): sample with the dense NumPy mirror" (the caller
 *                        may move the stream out and back with bo_rng_state).  Synchronises.
 *   bo_selfplay_begin  : bo_root_info + Dirichlet noise for every game with want[g] != 0 whose root is not
 *                        terminal + bo_search_begin + the first bo_step.  Synchronises (root info). */
int bo_rng_seed(bo_engine *e, int slot, uint32_t seed);
int bo_rng_state(bo_engine *e, int slot, int set, uint32_t *key624, int32_t *pos, int32_t *has_gauss, double *gauss);
int bo_selfplay_sample(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold,
                       double t_initial, double t_final, int32_t *res_n, int32_t *res_idx, float *res_val,
                       int32_t *best_idx, int32_t *action_out, void *stream);
int bo_selfplay_begin(bo_engine *e, const int32_t *want, float *nn_in_dev, int32_t *n_legal_out, int32_t *terminal_out,
                      int32_t *go_out, void *stream);

/* bo_selfplay_sample + bo_play + bo_selfplay_begin(want_next) in one call (one host round trip per ply).  *completed = 0
 * if some game's pi was too dense for the native sampler (action -3): nothing was played, the caller samples that game
 * with the dense NumPy mirror, then calls bo_play and bo_selfplay_begin itself. */
int bo_selfplay_turn(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold, double t_initial,
                     double t_final, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *action_out,
                     const int32_t *want_next, float *nn_in_dev, int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out,
                     int32_t defer_noise, int32_t *completed, void *stream);
/* defer_noise is a bit set.  Bit 1 (value 2): first ask whether every search has finished (bo_search_poll); if one is still
 * running nothing is done and *completed = -1 -- the caller issues another evaluate + step and calls again.
 * Bit 0, defer_noise = 1: the Dirichlet draws of the new roots (mcts.py:190-201) and their upload are left to bo_selfplay_noise,
 * to be called after the root evaluations' network forward has been enqueued on `stream` (the host work overlaps it) and
 * before the bo_step that consumes those evaluations.  Per game the RNG stream order is the same either way.
 * Bit 2 (value 4, with bit 0): the begin does not wait for the device either -- the kernel itself starts the search of every
 * wanted game whose new root is not terminal (mcts.py:160-162), *completed = 2, and n_legal_out / terminal_out / go_out are
 * NOT written: bo_selfplay_begun returns them (as bo_selfplay_begin would have) once the caller has enqueued the first
 * evaluation; it waits for the copy behind the begin kernels only.  Order: bo_selfplay_turn(4) -> enqueue the network
 * forward -> bo_selfplay_begun -> bo_selfplay_noise -> bo_step.  (Reference-semantics engines.)
 * Bit 3 (value 8, with bit 1): the result block and the searches' state have been enqueued behind the searches already
 * (bo_search_result_prefetch) and no step has been issued since: the call then only waits for `stream` and reads both from pinned
 * memory -- a cohort whose stream is idle is turned without a device round trip. */
int bo_selfplay_begun(bo_engine *e, int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out);
/* (ABI 4) Enqueue the result kernel and the copy of [result block | searches' state] to pinned host memory on `stream`, behind the
 * searches' last expected step, and return without waiting (see bo_selfplay_turn, bit 3).  Replaying a CAPTURED step afterwards makes the
 * block stale without the library knowing: the caller prefetches again (bo_step itself invalidates it). */
int bo_search_result_prefetch(bo_engine *e, void *stream);
int bo_selfplay_noise(bo_engine *e, void *stream);

/* (ABI 5) The turn of a ply ON THE DEVICE: bo_selfplay_turn's work -- result, select_move_with_temperature (self_play.py:59-80), the
 * played move (self_play.py:125-184) and the begin of the next searches (mcts.py:160-162) -- enqueued on `stream` BEHIND the searches'
 * last expected bo_step, so that the device goes from a ply's last tree step straight into the next ply's root evaluation; the host
 * is not waited for.  What stays on the host is every random draw and every libm call: per game with active[g] != 0 this call draws the
 * uniform np.random.choice would draw for the move (self_play.py:73) from the slot's stream NOW (the stream order per game is unchanged:
 * Dirichlet of this search, choice of this move, Dirichlet of the next search) and hands it to the kernel; apply_temperature's
 * p ** (1 / T) comes from a table built here with the host's pow for every visit count 0..NUM_SIMULATIONS.  The rest of the sampling is
 * IEEE arithmetic restated on the device for a pi of <= 2 non-zero entries (the reference's root keeps <= 2 children).
 * Needs a reference-semantics engine with int(WIDEN_COEFF) == 1, t_initial == 1, t_final > 0 (BO_E_CONFIG otherwise: use
 * bo_selfplay_turn).  redo != 0: enqueue the same turn again with the draws already made (after *completed == -1 below).
 * Order per ply: [bo_selfplay_noise -> bo_step x n] -> bo_selfplay_autoturn -> enqueue the next root evaluation's network forward ->
 * bo_selfplay_autoturn_collect -> bo_selfplay_noise -> bo_step ...  Asynchronous. */
int bo_selfplay_autoturn(bo_engine *e, const int32_t *active, const int32_t *move_number, int32_t threshold, double t_initial,
                         double t_final, const int32_t *want_next, float *nn_in_dev, int32_t redo, void *stream);
/* *ready_out = 1 once the device has passed the turn's outputs (bo_selfplay_autoturn_collect will not wait), else 0.  Never blocks. */
int bo_selfplay_autoturn_ready(bo_engine *e, int32_t *ready_out);
/* Wait for the turn's outputs (not for work enqueued behind them) and return them: the sparse pi of every game that searched (res_n,
 * res_idx / res_val rows of BO_RES_CAP like bo_search_result; <= 2 entries), best_idx (may be NULL), the action played (-1: none), and --
 * as bo_selfplay_begin reports them -- the new roots' legal-move counts, terminal codes and go flags (any may be NULL).
 * *completed = 1: done; -1: some search was still running when the turn came up -- NOTHING was played or begun: issue one more
 * evaluation + bo_step, then bo_selfplay_autoturn(redo = 1).  A result the device sampler does not cover is BO_E_STATE. */
int bo_selfplay_autoturn_collect(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *action_out,
                                 int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out, int32_t *completed);

/* ---- (ABI 7, additions) root values and resignation ----------------------------------------------------------------------------
 * v_i = the root's q_value after the search at ply i (float32 as the tree holds it; mcts.py:120-144 update_recursive, the value from the
 * perspective of the side to move at the root).  Both turns report the same bits.
 * bo_engine_root_values(e, 1): keep the root's q_value exact in every backup (the step kernel's run of terminal simulations otherwise
 * updates the root's visit count only: selection never reads the root's q).  Off by default; v_i below is meaningful only with it on.
 * Call it before the first bo_step a graph captures (a captured launch keeps the engine state it was captured with).
 * bo_selfplay_autoturn_collect_ex: bo_selfplay_autoturn_collect plus, per slot, root_value_out[g] = v_i (0 where the game did not search)
 * and resigned_out[g] (1: the game resigned at this ply; action -1, no move played, no next search begun, go_out 0).  Either may be NULL.
 * bo_selfplay_resign: resignation in the device turn from the next bo_selfplay_autoturn on.  enable [G] (NULL: off for every slot):
 * per slot, resignation enabled.  An enabled game resigns at ply i, before it plays, when v_i < threshold (float32 compare) at that ply
 * and at its side's previous plies - 1 searches (i - 2, i - 4, ...): a counter per slot and ply parity, reset by bo_games_reset*,
 * decided by the turn's first kernel from the committed value and committed by the second one only when the turn happens (a redo
 * after *completed == -1 counts nothing twice).  plies >= 1.  Reference-semantics engines with root values on (BO_E_STATE otherwise).
 * bo_search_root_value: out [G] = the root's q_value of every slot (v_i for a finished search) -- the host-made turn's v_i.
 * Synchronises. */
int bo_selfplay_autoturn_collect_ex(bo_engine *e, int32_t *res_n, int32_t *res_idx, float *res_val, int32_t *best_idx, int32_t *action_out,
                                    int32_t *n_legal_out, int32_t *terminal_out, int32_t *go_out, float *root_value_out,
                                    int32_t *resigned_out, int32_t *completed);
int bo_engine_root_values(bo_engine *e, int32_t on);
int bo_selfplay_resign(bo_engine *e, const int32_t *enable, float threshold, int32_t plies);
int bo_search_root_value(bo_engine *e, float *out, void *stream);

/* ---- records ------------------------------------------------------------------------------------
 * The game in `slot` as plain data: its positions[0..n_plies] and moves[0..n_plies). */
int bo_game_export(bo_engine *e, int slot, bo_position *positions, int32_t *moves, int32_t cap, int32_t *n_plies,
                   void *stream);
/* Training encodings of plies [first, first+n) of the game in `slot` with the CURRENT (end of
 * game) tracker, float32 [n,120,8,8] into out_dev (self_play.py:200-208).  Asynchronous. */
int bo_game_encode(bo_engine *e, int slot, int first, int n, float *out_dev, void *stream);

/* The same encodings from a compact record on any rank (betaone_amd/records.py wire format): positions[0..n_positions)
 * as returned by bo_game_export (ep_key filled), plies [first, first+n) into out_dev.  Needs no engine.  Synchronises. */
int bo_records_encode(int n_positions, const bo_position *positions, int first, int n, float *out_dev, void *stream);

/* ---- FAST mode options ---------------------------------------------------------------------------- */
/* FAST mode (cfg.mode = 1; NOT the reference's semantics).  Every argument: -1 leaves the
 * setting as it is.  tree_reuse != 0 (default) keeps the played child's subtree as the next search's tree -- the reference
 * rebuilds the tree every move (mcts.py:176).  games_per_halfwave (2 or 4, default 2): games the select + backup kernel
 * interleaves per half-wavefront in the half-wave forms (leaves_per_step > 8 caps it at 2, > 16 at 1).  select_flags (default 16):
 * bit 0 non-temporal loads of the child runs, bit 1 the root's run stays in registers for all descents of a step, bit 2 the
 * half-wave kernel is built for one more wavefront per SIMD (register spills), bit 3 (leaves_per_step == 4 only) the
 * one-lane-per-game form, bit 4 (leaves_per_step <= 8) eight lanes per game = eight games per wave-instruction.
 * All variants compute the same trees (tests/test_engine_gpu.py); the defaults are the fastest measured on an MI355X. */
int bo_fast_options(bo_engine *e, int32_t tree_reuse, int32_t games_per_halfwave, int32_t select_flags);
#define BO_FAST_GRANULE_BYTES 128    /* a fast-mode arena is allocated in granules of 8 16-byte records */
/* per game [G]: status bits, NN evaluations, flushes, terminal simulations, tree levels descended,
 * children scanned by the PUCT select (the last two give the select kernel's algorithmic bytes). */
int bo_engine_status(bo_engine *e, int32_t *status, int32_t *evals, int32_t *flushes, int32_t *term_sims,
                     int32_t *levels, int32_t *children_scanned, void *stream);


/* ---- stand-alone kernels -------------------------------------------------------------------------
 * Legal moves (python-chess order) of n raw positions: moves_out [n,256] int32, n_out [n], check_out [n]. */
int bo_movegen_batch(bo_engine *e, int n, const bo_position *pos, int32_t *moves_out, int32_t *n_out,
                     int32_t *check_out, void *stream);


/* ---- fused epilogues of the evaluate stage (network.py:64-118 with BatchNorm folded), NCHW float32, 8x8 ----------
 * x = relu(x + bias[c] (+ residual)) in place; residual_dev may be NULL.  Asynchronous on `stream`. */
int bo_nn_bias_act(float *x_dev, const float *bias_dev, const float *residual_dev, int batch, int channels, void *stream);
/* x = relu((x + bias[c]) * sigmoid(W2 relu(W1 mean_hw(x + bias))) + residual) in place: the SE residual block's tail
 * (network.py:33-45,100-118).  w1 [hidden][channels], w2 [channels][hidden].  Asynchronous on `stream`. */
int bo_nn_se_residual(float *x_dev, const float *bias_dev, const float *w1_dev, const float *w2_dev,
                      const float *residual_dev, int batch, int channels, int hidden, void *stream);

/* 3x3 convolution (padding 1) over 8x8 boards on the fp32 matrix cores with the epilogue fused, NCHW float32:
 *   mode 0: y = conv(x) + bias      1: y = relu(conv(x) + bias)      2: y = relu(conv(x) + bias + residual)
 * wpacked_dev: the [c_out][c_in][3][3] weights re-ordered as [tap 9][c_in/8][c_out][2][4] with element
 * (tap, t4, oc, k, e) = W[oc][8*t4 + 2*e + k][tap] (betaone_amd/fused_net.py:pack_conv_weight).
 * Supported (c_in, c_out): (120 | C, C) for C in {64, 128, 256}.  Asynchronous on `stream`. */
/* Small-batch form of bo_nn_se_residual (uci.py's single-position searches): a board's layer in channels/16 workgroups;
 * x_dev is only read, the result replaces residual_inout_dev: r = relu((x + bias[c]) * gate[b,c] + r).  channels a multiple
 * of 16 (<= 256), hidden <= 16. */
int bo_nn_se_residual_small(const float *x_dev, const float *bias_dev, const float *w1_dev, const float *w2_dev,
                            float *residual_inout_dev, int batch, int channels, int hidden, void *stream);
/* Everything behind the tower's head convolutions in two launches (csrc/bo_heads.h; network.py:186-197 + the softmax of
 * mcts.py:185,287): policy_out = softmax(policy_fc(p)) (flags bit 0 clear: the logits), value_out = tanh(value_fc2(relu(value_fc1(v)))).
 * p [batch,128], v [batch,2048], policy_fc weight [4672,128] + bias, value_fc1 weight [256,2048] + bias, value_fc2 weight
 * [256] + bias [1], all float32 row-major on the device; policy_out [batch,4672], value_out [batch].  scratch_dev:
 * 4096 * batch floats (value_fc1's partial sums, no initial contents needed).  Any batch up to 65536.
 * flags: bit 0 = softmax; bit 1 (value 2) = p and v are float16 (the head planes of the BO_TOWER_DIRECT_F16 tower): they are
 * widened on load, weights, accumulation and outputs stay float32; bit 2 (value 4, ABI 6; excludes bit 0) = stop after the first
 * launch: policy_out holds the logits, scratch_dev the partial sums, value_out_dev is not written (may be NULL) -- bo_step_heads
 * finishes both where they are consumed. */
int bo_nn_heads(const void *p_dev, const void *v_dev, const float *wp_dev, const float *bp_dev, const float *w1_dev,
                const float *b1_dev, const float *w2_dev, const float *b2_dev, float *policy_out_dev, float *value_out_dev,
                float *scratch_dev, int batch, int flags, void *stream);
/* (ABI 4) The same behind the fp16 tower at any number of rows (fast mode: 4 096 .. 131 072 rows per evaluation; network.py:186-197 under
 * torch.autocast, softmax of mcts.py:287 in float32): p [batch,128], v [batch,2048], policy_fc weight [4672,128] and value_fc1 weight
 * [256,2048] float16 row-major; biases, value_fc2 weight [256] + bias float32; products on the fp16 matrix pipe with float32
 * accumulation, logits never rounded to float16.  The probabilities are written once: a first launch leaves every board's (max, sum of
 * exp) per output range in scratch_dev (20 * batch floats, no initial contents needed; may be NULL without softmax), a second
 * computes every logits tile again and stores exp(x - max) / sum; a third launch is the whole value head.  flags bit 0 = softmax.
 * 1 <= batch <= 4194304. */
int bo_nn_heads_f16(const void *p_dev, const void *v_dev, const void *wp_f16_dev, const float *bp_dev, const void *w1_f16_dev,
                    const float *b1_dev, const float *w2_dev, const float *b2_dev, float *policy_out_dev, float *value_out_dev,
                    float *scratch_dev, int batch, int flags, void *stream);
int bo_nn_conv3x3(const float *x_dev, const float *wpacked_dev, const float *bias_dev, const float *residual_dev,
                  float *y_dev, int batch, int c_in, int c_out, int mode, void *stream);

/* Small-batch form of bo_nn_conv3x3 (uci.py's single-position analysis): (c_out/16) x 4 workgroups per board, K split
 * over the four waves of a workgroup.  wpacked_dev: [c_out/16][tap 9][c_in/16][64][4] with element (ot, tap, g, lane, e) =
 * W[16*ot + (lane & 15)][16*g + 4*e + (lane >> 4)][tap]; c_in in {64, 128, 256} is the (zero-padded) channel count of
 * the weights, c_in_x <= c_in the channel count of x (120 for the input conv with c_in = 128).  Same modes. */
int bo_nn_conv3x3_small(const float *x_dev, const float *wpacked_dev, const float *bias_dev, const float *residual_dev, float *y_dev,
                        int batch, int c_in, int c_in_x, int c_out, int mode, void *stream);

/* The whole residual tower (input conv + N residual blocks, /root/reference/network.py:48-118,167-190, BatchNorm
 * folded) as ONE persistent kernel that keeps each board's activations in LDS.  channels in {64, 128}.
 * Layer l: kind 0 = input conv 120 -> C with ReLU (first layer only; weights zero-padded to 128 input channels),
 * 1 = first conv of a block with ReLU, 2 = second conv + skip + ReLU, 3 = second conv + SE gate + skip + ReLU
 * (W1 [hidden][C], W2 [C][hidden], no biases, hidden <= 16); `last` = 1 on the final layer only.
 * algo BO_TOWER_DIRECT (csrc/bo_tower.h): implicit GEMM; t4 = c_in/8; weights per layer [tap 9][t4][C][2][4] as for
 *   bo_nn_conv3x3.
 * algo BO_TOWER_WINOGRAD (csrc/bo_tower_wg.h): F(2x2,3x3); t4 = c_in/4 K-steps; weights per layer
 *   [t4][C/16][4][64][4] with element (step, ob, pq, lane, e) = (G g G^T)[4*pq + e] of filter
 *   g = W[16*ob + (lane & 15)][channel(step, lane >> 4)], G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], position = 4*row + col;
 *   channel(step, k) = 4*step + k for C = 64 and, for C = 128 (every layer has 128 input channels, the first one padded),
 *   with step = 4*c + sl: 16*(4*(c & 1) + sl) + 4*(c >> 1) + k -- the K order in which a wave of the kernel only ever
 *   transforms input channels that it produced itself (csrc/bo_tower_wg.h: OWN).  bias_off must be a multiple of 4.
 * algo BO_TOWER_DIRECT_F16 (csrc/bo_tower_h.h): fp16 weights and activations, fp32 accumulation, two boards per
 *   workgroup; channels in {128, 256}; t4 = 9*c_in/16 K-steps; `weights` holds fp16 data (n_weights still counts
 *   4-byte units): per layer [t4][C/32][64][8] with element (step, mt, lane, i) = W[32*mt + (lane & 31)]
 *   [16*(step % (c_in/16)) + 8*(lane >> 5) + i][tap = step / (c_in/16)] at 16-byte offset w_off4.  Needs `head`: its
 *   weights [ceil(channels/32)][C/16][64][8] fp16 with element (mt, st, lane, i) = Wh[32*mt + (lane & 31)][16*st +
 *   8*(lane >> 5) + i] at 16-byte offset w_off in `weights`; head outputs are fp16; y_dev is unused.
 * algo BO_TOWER_SPLIT_F16 (csrc/bo_tower_s.h): float32 in and out, computed on the fp16 matrix pipe -- every float32 weight
 *   and activation is a (hi, lo) pair of fp16 values (hi = RN16(v), lo = RN16(v - hi)), every product three fp16 MFMAs with
 *   float32 accumulation (relative product error 2^-22); one board per workgroup; channels in {128, 256}; layout as
 *   BO_TOWER_DIRECT_F16 with every fragment doubled: per layer [t4][C/32][2 = hi, lo][64][8] fp16 of s*W, s a power of two
 *   chosen by the caller (largest |s*W| below 2^15), and 1/s as ONE MORE float behind the layer's bias (params[bias_off + C];
 *   bias_off a multiple of 4).
 *   `head` is optional: weights [ceil(channels/32)][C/16][2][64][8] at 16-byte offset w_off in `weights`, bias [channels]
 *   followed by the inverse scale in params; head outputs are float32.  y_dev (optional) receives the tower output.
 * algo BO_TOWER_SPLIT_F16_T16 (ABI 5, csrc/bo_tower_s16.h; 128 filters): BO_TOWER_SPLIT_F16 with the products issued as 16x16x32 tiles (the chip
 *   holds a higher clock under them: profiles/r05_tower_bound.md); everything as for BO_TOWER_SPLIT_F16 except the per-layer fragment order
 *   [tap 9][c_in/32][C/16][2 = hi, lo][64][8]: element (tap, g, ot, hl, lane, i) = s*W[16*ot + (lane & 15)][32*g + 8*(lane >> 4) + i][tap]
 *   (t4 still counts K-steps of 16 channels: 9*c_in/16).
 * algo BO_TOWER_DIRECT_F16_T16 (ABI 5, csrc/bo_tower_h16.h; 128 or 256 filters): BO_TOWER_DIRECT_F16 as 16x16x32 tiles; per-layer fragment order
 *   [tap 9][c_in/32][C/16][64][8]: element (tap, g, ot, lane, i) = W[16*ot + (lane & 15)][32*g + 8*(lane >> 4) + i][tap]; head weights unchanged.
 * weights: float32 at float4 offset w_off4; params: float32 biases and SE matrices at float offsets.
 * head (optional, BO_TOWER_WINOGRAD only): the policy and value 1x1 convolutions + ReLU (network.py:101-113,191-195)
 *   fused behind the tower: bias [channels] and weights in params, the weights packed [ceil(channels/16)][C/16][64][4]
 *   with element (mb, g, lane, e) = Wh[16*mb + (lane & 15)][16*g + 4*e + (lane >> 4)] (0 beyond the last channel) at
 *   a float offset w_off that is a multiple of 4; output channels [0, split) go to
 *   head_a_dev [batch][split][64], the rest to head_b_dev [batch][channels - split][64]; y_dev may then be NULL.
 * bo_nn_tower_create validates every offset and copies the three HOST arrays to `device`;
 * bo_nn_tower_forward(x_dev [batch,120,8,8] -> y_dev [batch,C,8,8], NCHW float32) is asynchronous on `stream`.
 * bo_nn_value_tail: out[b] = tanh(w . h[b] + bias[0]) (value_fc2 + tanh, network.py:116-118,197). */
enum { BO_TOWER_DIRECT = 0, BO_TOWER_WINOGRAD = 1, BO_TOWER_DIRECT_F16 = 2, BO_TOWER_SPLIT_F16 = 3, BO_TOWER_SPLIT_F16_T16 = 4, BO_TOWER_DIRECT_F16_T16 = 5 };
typedef struct bo_tower_layer_desc {
    int32_t w_off4, t4, bias_off, kind, se_w1_off, se_w2_off, hidden, last;
} bo_tower_layer_desc;
typedef struct bo_tower_head_desc {
    int32_t channels, split, w_off, b_off;
} bo_tower_head_desc;
typedef struct bo_tower_s bo_tower;
int bo_nn_tower_create(const bo_tower_layer_desc *layers, int n_layers, const float *weights, int64_t n_weights,
                       const float *params, int64_t n_params, int channels, int algo, const bo_tower_head_desc *head, int device,
                       bo_tower **out);
int bo_nn_tower_forward(bo_tower *tower, const float *x_dev, float *y_dev, void *head_a_dev, void *head_b_dev, int batch, void *stream);
int bo_device_wall_clock_khz(int device, int32_t *khz_out);   /* rate of that clock (hipDeviceAttributeWallClockRate) */
/* (ABI 4) A HIP stream confined to a set of compute units (hipExtStreamCreateWithCUMask): bit i of mask_words = CU i of `device`.
 * CohortRollout gives every cohort such a stream with a disjoint set: the stream has a hardware queue of its own (pool streams share
 * queues: four cohorts then wait for each other's launches) and its kernels stay off the other cohorts' CUs (the reference's counterpart
 * is one OS process per game batch, main.py:160-175).  The handle is a
 * hipStream_t for every `stream` argument of this header and for torch.cuda.ExternalStream. */
int bo_stream_create_cu_mask(int device, const uint32_t *mask_words, int n_words, void **stream_out);
int bo_stream_destroy(void *stream);
int bo_nn_value_tail(const float *h_dev, const float *w_dev, const float *bias_dev, float *out_dev, int batch, int hidden, void *stream);
void bo_nn_tower_destroy(bo_tower *tower);
/* BO_TOWER_SPLIT_F16 carries every activation as a pair of fp16 numbers: a value beyond +-65504 is saturated and the forward's result
 * is wrong.  *overflow_out = 1 if that happened in any forward since the last call (the flag is cleared), 0 otherwise (always 0 for
 * the other algorithms).  Synchronises `stream`.  A net that trips it needs the fp32-pipe tower (BETAONE_F32_TOWER=fp32). */
int bo_nn_tower_status(bo_tower *tower, int32_t *overflow_out, void *stream);
/* (ABI 4) Device address of that status word, for bo_engine_watch: the self-play loop then checks it with every ply's result block
 * instead of only when finished games are handed over (the reference has no counterpart: its float32 net cannot saturate). */
int bo_nn_tower_word(bo_tower *tower, void **dev_word_out);
/* (ABI 4) Let the engine's result kernels copy `*dev_word` (any int32 device word, NULL: none) behind the result block, so that
 * bo_search_result / bo_selfplay_turn bring it to the host in the round trip they make anyway; bo_engine_watch_seen returns the OR
 * of the values seen since the last call with clear != 0.  Nothing is enqueued and nothing waits in either call. */
int bo_engine_watch(bo_engine *engine, int32_t *dev_word);
/* (ABI 5) The same for n_words (1 or 2) consecutive words: the copy is word 0 | (word 1 != 0 ? 0x10000 : 0).  Two words are what
 * bo_nn_b1_word returns -- the one-launch tower's [hand-off timeout code | saturation flag] -- so uci.py's searches and small self-play
 * batches, which that tower evaluates, stop on an invalid evaluation instead of using it. */
int bo_engine_watch_words(bo_engine *engine, int32_t *dev_words, int32_t n_words);
int bo_engine_watch_seen(bo_engine *engine, int32_t *seen_out, int32_t clear);


/* ---- (ABI 4) GPU-resident replay buffer: csrc/bo_replay.h ----------------------------------------------------------------------
 * Replaces, on the training side of the path's hand-over, train.load_recent_data + ChessDataset (/root/reference/train.py:179-219): the
 * finished games stay in HBM as compact records (position 80 B, end-of-game repetition count, sparse pi, z: ~110 B per ply) and a
 * batch of the triples ChessDataset.__getitem__ yields -- state float32 [120,8,8], dense pi [4672], z -- is expanded on the device for
 * the loop that consumes it (train_network, train.py:252-262).  capacity in POSITION slots (a game of n records takes n + 1); the
 * oldest games are evicted when the ring comes round (the reference keeps the most recent iterations, train.py:190-193). */
typedef struct bo_replay_s bo_replay;
int bo_replay_create(int64_t capacity_positions, int pi_width, int device, bo_replay **out);
/* positions[0 .. n_records] (position i before move i; the last one final), pi of record i = entries pi_ptr[i] .. pi_ptr[i+1] (at most
 * pi_width), z[i] as self_play.py:202 stores it.  *evicted_records (may be NULL): records of the games that had to go. */
int bo_replay_add_game(bo_replay *rb, int32_t game_id, const bo_position *positions, int32_t n_records, const int32_t *pi_ptr,
                       const int32_t *pi_idx, const float *pi_val, const float *z, int64_t *evicted_records, void *stream);
int bo_replay_size(bo_replay *rb, int64_t *n_records, int64_t *n_games);
/* record_index[i] in [0, records): resident records, oldest game first.  states [n,120,8,8], pi [n,4672], z [n] (device, float32). */
int bo_replay_sample(bo_replay *rb, int32_t n, const int64_t *record_index, float *states_dev, float *pi_dev, float *z_dev, void *stream);
/* (ABI 6, addition) The same batch with pi as the records keep it, for the sparse-target loss below: states [n,120,8,8] bit-identical
 * to bo_replay_sample's, pi_idx [n,W] int32 (unused slots -1), pi_val [n,W] float32 (unused slots 0), z [n]; W = the pi_width the
 * buffer was created with.  Same checks as bo_replay_sample. */
int bo_replay_sample_sparse(bo_replay *rb, int32_t n, const int64_t *record_index, float *states_dev, int32_t *pi_idx_dev, float *pi_val_dev,
                            float *z_dev, void *stream);
/* (ABI 9, additions) Root values in the buffer.  A slot keeps one float32 q beside its z: root_value[i], the root's q_value after the
 * search at ply i from the side to move's point of view (what a BOG2 record carries) -- the same point of view as z[i], no sign flip.
 * root_value may be NULL: the call is then bo_replay_add_game, the slots keep q = z and the game's records do not count as carrying a
 * value.  bo_replay_values: how many resident records carry one (eviction takes a game's count with it).
 * bo_replay_sample_sparse_q: bo_replay_sample_sparse plus q [n] float32; states, pi_idx, pi_val and z are bit-identical to that call's
 * for the same indices, q comes from the same launch.  Same checks. */
int bo_replay_add_game_values(bo_replay *rb, int32_t game_id, const bo_position *positions, int32_t n_records, const int32_t *pi_ptr,
                              const int32_t *pi_idx, const float *pi_val, const float *z, const float *root_value,
                              int64_t *evicted_records, void *stream);
int bo_replay_values(bo_replay *rb, int64_t *n_records_with_value);
int bo_replay_sample_sparse_q(bo_replay *rb, int32_t n, const int64_t *record_index, float *states_dev, int32_t *pi_idx_dev,
                              float *pi_val_dev, float *z_dev, float *q_dev, void *stream);
void bo_replay_destroy(bo_replay *rb);

/* ---- (ABI 17, addition) merged targets: csrc/bo_merge.h, records.GpuReplayBuffer.merge_duplicates ----------------------------------
 * The records of a training window whose inputs coincide (every game's ply 0, the shared opening plies) are grouped on the device and
 * each group gets ONE target: the mean of its members' sparse pi (the union of their actions in ascending order), z and q -- summed in
 * float64 over the members in ascending record index, divided by the count and rounded once to float32.  A group of one keeps its
 * record's entries in the record's order and z, q bit for bit.
 *   key BO_MERGE_KEY_INPUT: two records are equal iff bo_replay_sample writes the same 120 planes for them (up to 8 boards with their
 *     repetition planes, turn, castling, both counters, the en-passant square).  BO_MERGE_KEY_POSITION: the transposition key of the
 *     current board alone (histories and counters are ignored; the legal moves are the same).
 *   bo_replay_merge_create: record_index [n] distinct resident records in any order (n <= 2^29), or NULL: every resident record (n is
 *     ignored).
 *     The result does not depend on the order of the list.  Synchronous (null stream).  _ex: table_slots = the grouping table's size, a
 *     power of two up to 2^30 (0: the smallest one >= 2 n, at least 64); a table with fewer slots than there are groups is BO_E_STATE ("table
 *     overflow").  A group whose pis hold more than 256 distinct actions (impossible for legal pis) is BO_E_ARG, naming the group's
 *     representative record.
 *   bo_replay_merge_info: groups; width Wm = max(pi_width, largest union); records covered; largest group; records in groups of more
 *     than one; the table's size; device-event times of the grouping kernel and of the two merge launches (0 where there are none).
 *   bo_replay_merge_groups: representative [records] = per covered record, in the order of the list the merge was made from, the LOWEST
 *     record index of its group; count [groups] in ascending order of the groups' representatives.  Either may be NULL.
 *   bo_replay_sample_merged: bo_replay_sample_sparse_q's batch -- states bit-identical for the same indices -- with the targets of the
 *     records' groups: pi_idx / pi_val [n, Wm] (unused slots -1 / 0), z [n], q [n].  One launch.  BO_E_ARG: a merge of another buffer;
 *     a record the merge does not cover; a "stale merge" -- any bo_replay_add_game* on the buffer after the merge was made (records
 *     move and leave: make a new one). */
typedef struct bo_replay_merge_s bo_replay_merge;
#define BO_MERGE_KEY_INPUT 0
#define BO_MERGE_KEY_POSITION 1
typedef struct bo_merge_info {
    int64_t groups, width, records, largest_group, records_in_groups, table_slots;
    double group_ms, merge_ms;
} bo_merge_info;
int bo_replay_merge_create(bo_replay *rb, int64_t n, const int64_t *record_index, int32_t key, bo_replay_merge **out);
int bo_replay_merge_create_ex(bo_replay *rb, int64_t n, const int64_t *record_index, int32_t key, int64_t table_slots, void *stream,
                              bo_replay_merge **out);
int bo_replay_merge_info(const bo_replay_merge *m, bo_merge_info *out);
int bo_replay_merge_groups(const bo_replay_merge *m, int64_t *representative, int32_t *count);
int bo_replay_sample_merged(bo_replay *rb, bo_replay_merge *m, int32_t n, const int64_t *record_index, float *states_dev,
                            int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev, void *stream);
void bo_replay_merge_destroy(bo_replay_merge *m);

/* ---- (ABI 18, additions) board symmetries in the samplers: csrc/bo_sym.h ------------------------------------------------------------
 * The four samplers with one transform code per sample: sym [n] on the HOST, bit 0 = colour flip (colours swapped, ranks mirrored, turn
 * toggled, castling K<->k Q<->q, en-passant square ^ 56), bit 1 = file mirror (a <-> h, en-passant square ^ 7).  The mirror bit is
 * dropped for a sample whose CURRENT position has any castling right; applied [n] int32 on the DEVICE (may be NULL) receives the code
 * that was applied.  All eight history boards of a sample get that code; both move counters are kept.  The pi indices are those of the
 * transformed moves (utils.move_to_index of the mirrored move); entry order, values, z and q do not change.  Code 0 for every sample
 * writes, bit for bit, what the call without _sym writes.  Same checks as those calls; a code outside 0..3 is BO_E_ARG and nothing is
 * launched. */
int bo_replay_sample_sym(bo_replay *rb, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev, float *pi_dev,
                         float *z_dev, int32_t *applied_dev, void *stream);
int bo_replay_sample_sparse_sym(bo_replay *rb, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev,
                                int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, int32_t *applied_dev, void *stream);
int bo_replay_sample_sparse_q_sym(bo_replay *rb, int32_t n, const int64_t *record_index, const int32_t *sym, float *states_dev,
                                  int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev, int32_t *applied_dev, void *stream);
int bo_replay_sample_merged_sym(bo_replay *rb, bo_replay_merge *m, int32_t n, const int64_t *record_index, const int32_t *sym,
                                float *states_dev, int32_t *pi_idx_dev, float *pi_val_dev, float *z_dev, float *q_dev, int32_t *applied_dev,
                                void *stream);

/* ---- (ABI 4) the residual tower of ONE board (a few boards) as ONE launch spread over the chip: csrc/bo_tower_b1.h ----------------
 * Replaces, for uci.py's single-position searches (/root/reference/uci.py:60-93 -> mcts.py:183-185: PolicyValueNet.forward at
 * batch 1, /root/reference/network.py:167-185), the per-layer launches of bo_nn_conv3x3_small / bo_nn_se_residual_small.
 * Layer l = 0 is the input convolution (weights packed for 128 input channels, c_in_x = 120 present), then (conv1, conv2) per
 * residual block: mode 0 = relu(conv + bias), 1 = relu(conv + bias + block input), 2 = relu((conv + bias) * SE gate + block input)
 * with se_w1 [hidden][C], se_w2 [C][hidden] (network.py:33-45), hidden <= 16.  Weights: the layout of bo_nn_conv3x3_small.
 * All pointers are device addresses that must stay valid for the handle's life.  (filters / 16) * 4 * batch <= 256. */
typedef struct bo_b1_layer_desc {
    const void *weights_dev;
    const float *bias_dev;
    const float *se_w1_dev, *se_w2_dev;
    int32_t c_in, c_in_x, mode, se_hidden;
    const void *weights_split_dev;   /* NULL, or (hi, lo) fp16 pairs of inv_scale^-1 * W: the tiles then multiply on the fp16 matrix pipe
                                        (three MFMAs per product, float32 accumulation: the precision of BO_TOWER_SPLIT_F16); for every
                                        layer or for none.  Layout [C/16][tap 9][c_in/16][64 lanes][hi x4 | lo x4]. */
    float inv_scale;                 /* 1 / (the power of two the split weights were scaled by) */
    int32_t reserved;
} bo_b1_layer_desc;
typedef struct bo_b1_s bo_b1;
int bo_nn_b1_create(const bo_b1_layer_desc *layers, int n_layers, int channels, int max_batch, int device, bo_b1 **out);
/* x [batch,120,8,8] -> y [batch,channels,8,8] float32 on `stream`; capturable; one launch of a handle in flight at a time. */
int bo_nn_b1_forward(bo_b1 *tower, const float *x_dev, float *y_dev, int batch, void *stream);
/* *code_out = 0; 1 + the phase of a hand-off wait that gave up in the last launch (bounded spins: the kernel always ends; its output
 * is invalid then); or -1: an activation left the fp16 range with split weights (saturated: the output is wrong, use a handle without
 * split weights).  Synchronises `stream`. */
int bo_nn_b1_status(bo_b1 *tower, int32_t *code_out, void *stream);
/* (ABI 5) Device address of the two status words bo_nn_b1_status reads ([timeout code | saturation flag]; sticky until that call). */
int bo_nn_b1_word(bo_b1 *tower, void **dev_words_out);
void bo_nn_b1_destroy(bo_b1 *tower);

/* ---- (ABI 6, additions) two nets in one evaluate stage: head-to-head matches (betaone_amd/match.py) -------------------------------
 * In a match the net that evaluates row g is the net of the side to move at game g's root; it changes every ply and differs between
 * games.  sel_dev (int32 [batch], device): 0 = the first net, non-zero = the second.
 * bo_nn_tower_pair_check: BO_OK if the two towers can share one launch -- both BO_TOWER_SPLIT_F16 or both BO_TOWER_SPLIT_F16_T16, same
 * device, channels, fused head and identical layer descriptors and buffer sizes (every offset the kernel forms is then valid in both),
 * BO_E_CONFIG otherwise.
 * bo_nn_tower_forward_pair: bo_nn_tower_forward with the fused heads, board b on the weights of the tower sel_dev[b] names -- ONE launch,
 * each workgroup streams the weights of its own board's net (csrc/bo_tower_s.h, bo_tower_s16.h: PAIR).  Results are bit-identical to
 * each net's own launch.  A saturated activation sets BOTH towers' status words (bo_nn_tower_word).  Asynchronous on `stream`. */
int bo_nn_tower_pair_check(bo_tower *tower0, bo_tower *tower1);
int bo_nn_tower_forward_pair(bo_tower *tower0, bo_tower *tower1, const int32_t *sel_dev, const float *x_dev, void *head_a_dev,
                             void *head_b_dev, int batch, void *stream);
/* bo_nn_heads (flags 0 / 1 / 2; the rows are not left to bo_step_heads) with two nets' float32 head weights, row b on the set sel_dev[b]
 * names.  A tile of boards that all use one net runs once; a tile that mixes the two runs once per net and stores only that net's rows
 * (the cost stays in mixed tiles: keep each net's rows in contiguous runs).  Bit-identical to each net's own bo_nn_heads. */
typedef struct bo_head_weights {
    const float *wp, *bp;   /* policy_fc weight [4672,128] + bias [4672] */
    const float *w1, *b1;   /* value_fc1 weight [256,2048] + bias [256] */
    const float *w2, *b2;   /* value_fc2 weight [256] + bias [1] */
} bo_head_weights;
int bo_nn_heads_pair(const void *p_dev, const void *v_dev, const bo_head_weights *net0, const bo_head_weights *net1, const int32_t *sel_dev,
                     float *policy_out_dev, float *value_out_dev, float *scratch_dev, int batch, int flags, void *stream);
/* Every other pair of evaluate stages runs both nets over the whole batch; the rows are then merged: logits_out[b] / value_out[b] =
 * those of net sel_dev[b].  logits [batch,width], value [batch], float32, device.  Asynchronous on `stream`. */
int bo_nn_merge_rows(const int32_t *sel_dev, const float *logits0_dev, const float *value0_dev, const float *logits1_dev,
                     const float *value1_dev, float *logits_out_dev, float *value_out_dev, int batch, int width, void *stream);
/* sel_dev[g] = net_of_white_dev[g] ^ (the root of slot g has black to move), read from the engine's device state on `stream`: enqueue it
 * behind the turn that moves the roots and ahead of the evaluation (a reference-semantics engine: NN row g = slot g).  Inactive slots
 * get some value. */
int bo_match_select(bo_engine *engine, const int32_t *net_of_white_dev, int32_t *sel_dev, void *stream);

/* ---- (ABI 6, additions) the training loss of train.calculate_loss with a sparse target: csrc/bo_train.h ---------------------------
 * Replaces F.cross_entropy(logits, dense_pi) + F.mse_loss(value, z) (/root/reference/train.py:222-249) for targets of at most W entries
 * per row: pi_idx [n,W] int32 (an entry is valid when 0 <= idx < 4672; the valid entries of a row are distinct), pi_val [n,W] float32,
 * z [n] float32.  logits [n,4672] and value [n] in logits_dtype / value_dtype (BO_DTYPE_*); arithmetic is float32.
 * row_stats [n,4] float32 (device): per row max, log sum exp(x - max), the policy and the value term -- written by the forward, read by
 * the backward.  loss3 float32 [3] (device) = [policy + value, policy, value], each a mean over the rows, summed in a fixed order
 * (bit-reproducible).  grad_out float32 [3] (device): the gradient of loss3 (e.g. [scale, 0, 0] for a backward from the total).
 * dlogits / dvalue: the gradients in the inputs' dtypes.  Asynchronous on `stream`; capturable. */
enum { BO_DTYPE_FLOAT32 = 0, BO_DTYPE_FLOAT16 = 1, BO_DTYPE_BFLOAT16 = 2 };
int bo_train_loss_forward(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                          const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, float *row_stats_dev, float *loss3_dev,
                          void *stream);
int bo_train_loss_backward(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                           const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *row_stats_dev,
                           const float *grad_out_dev, void *dlogits_dev, void *dvalue_dev, void *stream);
/* (ABI 9, additions) The value head regressed on t[b] = (1 - a) z[b] + a q[b]: q [n] float32 (bo_replay_sample_sparse_q), and the mix a
 * as ONE float32 on the device (mix_dev), read by the kernels like grad_out -- a schedule changes it under a captured step.
 * row_stats [n,6] float32: max, log sum exp, the policy term, (v - t)^2, (v - z)^2, (v - q)^2.
 * loss5 float32 [5] = [policy + value_mix, policy, value_mix, value_vs_z, value_vs_q]: value_mix the mean of (v - t)^2, the last two the
 * means against z and q alone -- diagnostics without a gradient: grad_out stays [3], the gradient of loss5[0..2].
 * a == 0 selects t = z: loss5[0..2], dlogits and dvalue are then bit for bit those of the two calls above, whatever q holds (NaN
 * included).  a outside [0, 1] or NaN is not clamped: all of loss5 and dvalue are NaN.  Otherwise as the two calls above. */
int bo_train_loss_forward_mix(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                              const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *q_dev,
                              const float *mix_dev, float *row_stats_dev, float *loss5_dev, void *stream);
int bo_train_loss_backward_mix(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                               const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *q_dev,
                               const float *mix_dev, const float *row_stats_dev, const float *grad_out_dev, void *dlogits_dev,
                               void *dvalue_dev, void *stream);

/* ---- (ABI 12, additions) held-out validation metrics: csrc/bo_metrics.h ---------------------------------------------------------------
 * What a net's logits [n,4672] and value [n] say about records it was not trained on, with the inputs of bo_train_loss_forward (the
 * same dtypes, float32 arithmetic) plus q [n] float32 (NULL: no root values, se_q is 0) and bucket [n] int32 (NULL: every row is
 * bucket 0; a row whose id is outside [0, n_buckets) is counted nowhere).
 * rows [n][BO_METRIC_ROW_COLS] float32 (device, written): one record per row, columns BO_METRIC_ROW_*.  With the row's valid entries e
 * (0 <= pi_idx < 4672), p = softmax(logits row) and i* the valid entry with the largest pi_val (ties: the lowest action):
 *   BAD                a logit is NaN, +inf or -inf, or the value is NaN: every other column of the record is then 0
 *   HAS_POLICY         the row has a valid entry (and is not bad); without one the policy columns RANK .. P_SUPPORT are 0
 *   DECISIVE           z != 0
 *   RANK               actions a with logit[a] > logit[i*], or equal and a < i* (stored values compared: exact in every dtype)
 *   TOP1, TOP3, TOP5   RANK < 1, 3, 5
 *   ARGMAX_IN_SUPPORT  the net's argmax (the lowest action among equal maxima) is a valid entry of the row
 *   CE                 -sum_e pi_val[e] log p[pi_idx[e]]: the bits of bo_train_loss_forward's row_stats[b][2] on the same inputs
 *   TARGET_ENTROPY     -sum_e pi_val[e] log pi_val[e] over pi_val[e] > 0;   NET_ENTROPY  -sum_a p[a] log p[a]
 *   P_TOP, P_SUPPORT   p[i*], sum_e p[pi_idx[e]]
 *   SE_Z, SE_Q, ABS_V  (v - z)^2, (v - q)^2, |v|;   SIGN_OK  z != 0 and v z > 0;   Z, V  the outcome and the value themselves
 * accum [n_buckets][BO_METRIC_COLS] float64 (device, ADDED TO -- zero it before a pass): column N_ROWS counts the bucket's rows that are
 * not bad, every later column c is the sum of row column c - 1 over the bucket's rows, in a fixed order (bit-reproducible).  The
 * counts are sums of small integers in float64: exact, whatever the split into batches.  Nothing is read back: a validation pass needs
 * no host synchronisation before its end.  Asynchronous on `stream`; capturable. */
enum {
    BO_METRIC_ROW_BAD = 0, BO_METRIC_ROW_HAS_POLICY, BO_METRIC_ROW_DECISIVE, BO_METRIC_ROW_RANK, BO_METRIC_ROW_TOP1, BO_METRIC_ROW_TOP3,
    BO_METRIC_ROW_TOP5, BO_METRIC_ROW_ARGMAX_IN_SUPPORT, BO_METRIC_ROW_CE, BO_METRIC_ROW_TARGET_ENTROPY, BO_METRIC_ROW_NET_ENTROPY,
    BO_METRIC_ROW_P_TOP, BO_METRIC_ROW_P_SUPPORT, BO_METRIC_ROW_SE_Z, BO_METRIC_ROW_SE_Q, BO_METRIC_ROW_ABS_V, BO_METRIC_ROW_SIGN_OK,
    BO_METRIC_ROW_Z, BO_METRIC_ROW_V, BO_METRIC_ROW_COLS
};
enum {
    BO_METRIC_N_ROWS = 0, BO_METRIC_N_BAD, BO_METRIC_N_POLICY_ROWS, BO_METRIC_N_DECISIVE, BO_METRIC_SUM_RANK, BO_METRIC_SUM_TOP1,
    BO_METRIC_SUM_TOP3, BO_METRIC_SUM_TOP5, BO_METRIC_SUM_ARGMAX_IN_SUPPORT, BO_METRIC_SUM_CE, BO_METRIC_SUM_TARGET_ENTROPY,
    BO_METRIC_SUM_NET_ENTROPY, BO_METRIC_SUM_P_TOP, BO_METRIC_SUM_P_SUPPORT, BO_METRIC_SUM_SE_Z, BO_METRIC_SUM_SE_Q, BO_METRIC_SUM_ABS_V,
    BO_METRIC_SUM_SIGN_OK, BO_METRIC_SUM_Z, BO_METRIC_SUM_V, BO_METRIC_COLS
};
int bo_train_metrics(int32_t n, int32_t W, const void *logits_dev, int32_t logits_dtype, const void *value_dev, int32_t value_dtype,
                     const int32_t *pi_idx_dev, const float *pi_val_dev, const float *z_dev, const float *q_dev /* may be NULL */,
                     const int32_t *bucket_dev /* may be NULL */, int32_t n_buckets, float *rows_dev /* [n][BO_METRIC_ROW_COLS] */,
                     double *accum_dev /* [n_buckets][BO_METRIC_COLS], added to */, void *stream);

/* ---- (ABI 6, additions) PGN pretraining: csrc/bo_pgn.h --------------------------------------------------------------------------
 * Replaces the reference's PGNDataset (train.py:81-160: python-chess reads the games, parses SAN and encodes 120 planes per position in
 * DataLoader workers).  Host: bo_pgn_parse tokenises PGN text -- per game the root ([FEN] if present, else the start position), one
 * packed SAN token per mainline move, per move "has eval" and the float32 target -value of its eval comment, and a status.  Device:
 * bo_pgn_replay replays the tokens (one wave per game; legal moves on the device, the token resolved by a ballot) into a ring of
 * position slots that the caller owns; bo_pgn_sample encodes samples from it with the LIVE repetition tracker of the reference's parse.
 * text: PGN bytes.  final_chunk = 0: the text after the last complete game is not consumed (*consumed says how far the games went; pass
 * the rest again with the next chunk); 1: the text ends there.  max_games / max_tokens (< 0: no limit) stop before the game that would
 * exceed them (one game is always taken).  The handle is host memory. */
enum {
    BO_PGN_OK = 0,           /* every token replayed */
    BO_PGN_VARIANT = 1,      /* [Variant] other than standard / chess: skipped, no tokens */
    BO_PGN_BAD_FEN = 2,      /* unparsable [FEN], or not one king per side: skipped, no tokens */
    BO_PGN_UNSUPPORTED = 3,  /* a movetext word that is neither SAN nor castling: the tokens before it are kept */
    BO_PGN_NULL_MOVE = 4,    /* a null move (--, Z0, 0000, @@@@): the tokens before it are kept */
    BO_PGN_ILLEGAL = 5,      /* (bo_pgn_replay) a token no legal move matches: the plies before it are kept */
    BO_PGN_AMBIGUOUS = 6,    /* (bo_pgn_replay) a token several legal moves match: the plies before it are kept */
    BO_PGN_MISMATCH = 7      /* (bo_san_render) a legal move whose position after it is not the game's next position */
};
#define BO_PGN_POSITION_BYTES 80   /* one ring slot of pos_dev */
typedef struct bo_pgn_s bo_pgn;
int bo_pgn_parse(const char *text, int64_t n_bytes, int32_t final_chunk, int64_t max_games, int64_t max_tokens, int64_t *consumed,
                 bo_pgn **out);
/* games, tokens, and the device scratch bo_pgn_replay needs for this handle (any pointer may be NULL) */
int bo_pgn_size(const bo_pgn *p, int64_t *n_games, int64_t *n_tokens, int64_t *scratch_bytes);
/* host copies (any pointer may be NULL): status [games], tok_off [games + 1] (game g's tokens are tok_off[g] .. tok_off[g+1]), roots
 * [games], tokens / has_eval / target [tokens].  A token: bits 0-5 destination square, 6-9 from-file + 1, 10-13 from-rank + 1, 14-16
 * piece (0 none, 2..6 = N B R Q K), 17-19 promotion (0 none, 2..6), 20-21 kind (0 SAN, 1 O-O, 2 O-O-O). */
int bo_pgn_export(const bo_pgn *p, int32_t *status, int32_t *tok_off, bo_position *roots, uint32_t *tokens, int32_t *has_eval, float *target);
/* Replays game g into ring slots slot0[g] .. slot0[g] + its tokens - 1 (slot0 host int64 [games]; < 0: skip the game; every range
 * inside [0, capacity); games must not share slots).  Per replayed ply t in slot s = slot0[g] + t: pos_dev[s] (the position before the
 * move, BO_PGN_POSITION_BYTES), act_dev[s] (the move's action index), smp_dev[s] (1: ply t is a sample -- move t + 1 was replayed and
 * has an eval), z_dev[s] (the sample's target, move t + 1's).  n_plies_out / status_out (host int32 [games], may be NULL): the plies
 * replayed and the final status.  scratch_dev: >= bo_pgn_size's scratch_bytes of device memory.  Synchronises `stream`. */
int bo_pgn_replay(const bo_pgn *p, const int64_t *slot0, int64_t capacity, void *scratch_dev, int64_t scratch_bytes, void *pos_dev,
                  int32_t *act_dev, float *z_dev, int32_t *smp_dev, int32_t *n_plies_out, int32_t *status_out, void *stream);
/* Sample i = ply ply_dev[i] of the game whose ply 0 is in slot game_slot_dev[i] (device int32 [n]): states [n,120,8,8] with the
 * repetition counts of the game's plies 0 .. ply (the reference's live tracker), pi_idx [n] = act, pi_val [n] = 1, z [n].
 * Asynchronous on `stream`. */
int bo_pgn_sample(const void *pos_dev, const int32_t *act_dev, const float *z_dev, int32_t n, const int32_t *game_slot_dev, const int32_t *ply_dev,
                  float *states_dev, int32_t *pi_idx_dev, float *pi_val_dev, float *z_out_dev, void *stream);
void bo_pgn_destroy(bo_pgn *p);

/* ---- (ABI 6, additions) PGN export: csrc/bo_san.h ----------------------------------------------------------------------------
 * The inverse of the replay above: games held as positions P_0..P_n and moves m_0..m_{n-1} (P_{i+1} the position after m_i -- what
 * FinishedGame and the compact records hold) rendered as PGN movetext.  The SAN is rendered on the device, one wave per position.
 *
 * bo_san_render: positions_dev (bo_position [n_positions], device) hold the games back to back, game g in positions
 * game_off_dev[g] .. game_off_dev[g + 1] - 1 (device int32 [n_games + 1], increasing, game_off[0] = 0, game_off[n_games] =
 * n_positions; every game has at least its root).  moves_dev (device int32 [n_positions]): moves_dev[k] = the move played from
 * position k (from | to << 6 | promo << 12), ignored for a game's last position.  Positions need resolved ep_key fields or -2.
 * Per position k: san_dev[k] (8 bytes) = the SAN of the move played from it, without the check suffix, NUL-padded (at most 6
 * characters; all zero for a game's last position and a bad ply); state_dev[k] = bit 0 the side to move is in check, bit 1 it has
 * no legal move, bits 4-7 the status of the move played from it (BO_PGN_OK, BO_PGN_ILLEGAL: not a legal move, BO_PGN_MISMATCH:
 * legal, but the position after it differs from position k + 1 in its key or counters).  The suffix of move i is '#' if state of
 * position i + 1 has bits 0 and 1, '+' if bit 0 only.  bad_dev (device int32 [2 * n_games]): per game the first bad ply (-1 none)
 * and its status.  Asynchronous on `stream`. */
int bo_san_render(int32_t n_games, int32_t n_positions, const int32_t *game_off_dev, const void *positions_dev, const int32_t *moves_dev,
                  void *san_dev, uint8_t *state_dev, int32_t *bad_dev, void *stream);
/* FEN of a position, as python-chess Board.fen() writes it: the en-passant field is ep_key (an ep square only when an ep capture
 * is legal; -2 is refused: resolve it first).  Writes a NUL-terminated string of at most cap bytes.  Host only. */
int bo_position_fen(const bo_position *p, char *out, int32_t cap);
/* Movetext of one game from bo_san_render's output (host copies): san [n_plies * 8], state [n_plies + 1], the root's side to move
 * (1 white) and fullmove number, comments [n_plies] (bit 0: "{book}" after the move; NULL: none) and the result token.  Move numbers
 * "N." before white's moves and "N..." before a black move that opens the game or follows a comment; lines of at most 79
 * characters, no token split; ends with the result token and '\n'.  *len_out = the text's length; BO_E_ARG if it does not fit
 * in cap bytes (nothing is written then) or a ply has no SAN.  Host only. */
int bo_pgn_movetext(int32_t n_plies, const void *san, const uint8_t *state, int32_t root_turn, int32_t root_fullmove, const uint8_t *comments,
                    const char *result, char *out, int64_t cap, int64_t *len_out);
/* (ABI 7) The same with a comment TEXT per ply: comment i is text[text_off[i] .. text_off[i + 1]) (text_off [n_plies + 1]; an empty
 * range: none), written as "{...}" after move i -- e.g. the eval comments "+0.12/100 0.00s" of self-play records.  final_comment (may
 * be NULL or empty) is written as one more "{...}" after the last move (e.g. "White resigns").  Same layout rules. */
int bo_pgn_movetext_text(int32_t n_plies, const void *san, const uint8_t *state, int32_t root_turn, int32_t root_fullmove, const char *text,
                         const int32_t *text_off, const char *final_comment, const char *result, char *out, int64_t cap, int64_t *len_out);

/* ---- (ABI 8, additions) analysis of games that are already on the device: csrc/bo_analyse.h, betaone_amd/analyse.py ----------------
 * "Here is a file of games, what does the net think of them": one search per position of every game bo_pgn_replay left in HBM.  The
 * reference has no counterpart (uci.py searches one position a GUI hands it); bo_games_reset sets a slot up from a FEN and UCI move
 * strings -- text parsing on the host, a serial make_move loop on one lane and a synchronise -- which is the wrong tool for tens of
 * thousands of roots that are device memory already.  Reference-semantics engines only (BO_E_CONFIG in fast mode).
 *
 * bo_games_reset_dev: bo_games_reset (self-play context) for n slots from positions in the ring's format (BO_PGN_POSITION_BYTES each,
 * what bo_pgn_replay writes): slot slots_dev[i] becomes the game whose ply 0 is entry first_dev[i], at ply ply_dev[i] -- positions
 * first .. first + ply are copied (64 per pass), the tracker holds each once (the live tracker bo_pgn_sample encodes with), the moves
 * are recovered from consecutive positions, counters and status are reset, the root is prepared.  ASYNCHRONOUS, and every pointer is
 * device memory read when the kernel runs: a batch can be set up behind the previous batch's bo_analysis_result with no host wait.
 * What the host cannot check the kernel does: a range that leaves [0, capacity) gives BO_ST_BAD_RANGE, ply + 1 > max_plies
 * BO_ST_PLY_OVERFLOW (BO_ST_TRK_OVERFLOW) in the slot's status; such a slot holds an empty game, terminal code -1, and is not searched;
 * a slot number outside the engine is ignored.  Nothing outside [0, capacity) is read.
 * bo_search_begin_dev: bo_search_begin decided on the device -- slot g searches when want_dev[g] != 0 and its root is not terminal
 * (mcts.py:160-162).  No Dirichlet noise: engines with dirichlet_alpha <= 0 only (BO_E_CONFIG otherwise).  Then bo_step as usual.
 * bo_analysis_result: the result kernel of bo_search_result, then one bo_analysis record per slot into out[G] (device memory, or pinned
 * device-mapped host memory; each word is stored once).  played_dev [G] (may be NULL): the move the game played from the slot's root
 * (from | to << 6 | promo << 12, -1 none).  Needs bo_engine_root_values(e, 1) (BO_E_STATE otherwise).  Asynchronous.
 *   terminal: the root's is_game_over(claim_draw=True) code (0, 1 side to move is mated, 2 draw -- a game that played on past a
 *     claimable draw has such roots; -1 refused slot); n_legal; phase: 0 idle (the root was not searched), 1 the search is still
 *     running (step once more), 2 finished -- the fields below are filled only then; status: the slot's BO_ST_* bits; ply; sims_done;
 *     watch: the word(s) named to bo_engine_watch as the result kernel saw them (non-zero: the evaluations are invalid).
 *   total_visits, best_move: bo_search_result's.  root_value: the root's q_value (side to move).  played_*: whether played_dev[g] is a
 *     child of the root, its visit count and q_value as the tree holds it (the child's own side's view); 0 when it is no child.
 *   pv: the principal variation, at most BO_PV_CAP moves: from the root, at each node the child with the most visits, the first
 *     maximum in child order (at the root in legal-move order, so pv[0] == best_move); it ends at a node without children or whose
 *     best child has no visit.  total_visits == 0 gives pv_len 0.
 * bo_pgn_after: for n entries idx_dev[i] (device int64) of a ring: move_out_dev[i] = the move act_dev names at that position (-1: not
 * decodable, or the entry is outside [0, capacity)), pos_out_dev[i] (BO_PGN_POSITION_BYTES each) = the position after it; either
 * output may be NULL.  The position after a game's last move is not in the ring.  Asynchronous.
 * bo_pgn_spans: host.  begin / end [games]: the bytes [begin, end) of each parsed game in the text given to bo_pgn_parse (tag section
 * and movetext, from its first tag or word: '%' lines and ';' comments in front of it are outside), so that a writer can keep the
 * game's tags.  The offsets count from the `text` of that one call: a caller that parses a file in chunks adds its own offset. */
#define BO_PV_CAP 16
typedef struct bo_analysis {
    int32_t terminal, n_legal, total_visits, best_move;
    float root_value;
    int32_t played_is_child, played_visits;
    float played_q;
    int32_t pv_len, pv[BO_PV_CAP];
    int32_t phase, status, ply, sims_done, watch, reserved[2];
} bo_analysis;
int bo_games_reset_dev(bo_engine *e, int n, const int32_t *slots_dev, const void *pos_dev, int64_t capacity, const int64_t *first_dev,
                       const int32_t *ply_dev, void *stream);
int bo_search_begin_dev(bo_engine *e, const int32_t *want_dev, float *nn_in_dev, void *stream);
int bo_analysis_result(bo_engine *e, const int32_t *played_dev, bo_analysis *out, void *stream);
int bo_pgn_after(const void *pos_dev, const int32_t *act_dev, int64_t capacity, int32_t n, const int64_t *idx_dev, void *pos_out_dev,
                 int32_t *move_out_dev, void *stream);
int bo_pgn_spans(const bo_pgn *p, int64_t *begin, int64_t *end);

/* ---- (ABI 15, additions) reanalysis of self-play records: csrc/bo_reanalyse.h, betaone_amd/reanalyse.py ---------------------------
 * The positions a .bog record stores are searched again with a newer net; the record gets that search's pi and root value.  The search
 * is the analysis path above (bo_games_reset_dev, bo_search_begin_dev, bo_step); these two calls are its ends.
 *
 * bo_records_ring: n bo_position in DEVICE memory -- the concatenated positions of a file's games, n_plies + 1 per game, as they sit in
 * the record bodies -- become n ring entries (BO_PGN_POSITION_BYTES each) in ring_out_dev: what bo_pgn_replay writes for the same
 * positions, byte for byte (flag word, resolved e.p. key, key hash, and the "reached by an irreversible move" bit, which entry i takes
 * from entry i - 1 when it is that position's child).  One lane per position.  n == 0 does nothing.  Asynchronous.
 * bo_reanalysis_result: the result kernel of bo_search_result, then per slot one bo_reanalysis record into out[G] and one pi row into
 * pi_idx_out / pi_val_out [G][W] (device memory, or pinned device-mapped host memory; each word is stored once).  1 <= W <= BO_RES_CAP
 * (BO_E_ARG).  Needs bo_engine_root_values(e, 1) (BO_E_STATE) and a reference-semantics engine (BO_E_CONFIG).  Asynchronous.
 *   played_action_dev [G] (may be NULL): the ACTION INDEX the game played from the slot's root (-1 none).
 *   root_dev [G] int64: the root's index r into old_ptr_dev (-1: the root has no old pi); its old entries are old_idx_dev / old_val_dev
 *     [old_ptr_dev[r] .. old_ptr_dev[r + 1]).  The four old-pi pointers are given together or are all NULL (no root has an old pi).
 *   terminal, n_legal, phase, status, ply, sims_done, watch: as in bo_analysis; the fields below and the rows are written only for
 *     phase 2 with terminal 0 -- the rows of every other slot are not touched.
 *   The rows: the first min(pi_n, W) entries of bo_search_result's row, in its order and with its bits, then (-1, 0).  pi_n: the
 *     entries the search produced; pi_n > W sets BO_ST_PI_OVERFLOW in the record's status.
 *   total_visits, best_idx: bo_search_result's.  root_value: the root's q_value (side to move).  played_prob: the row's value at
 *     played_action_dev[g] (the whole row, not only its first W entries), 0 when it is absent.
 *   has_old: root_dev[g] >= 0.  tv: 0.5 * (sum over the new entries in row order of |new - old(a)| + sum over the old entries whose
 *     action the new row does not have, in stored order, of old), old(a) the first old entry with action a or 0; accumulated in float64
 *     in exactly that order, rounded once to float32.  agree: the old pi's first maximum in stored order names the same action as the
 *     new row's first maximum in row order (0 for an empty old pi).  The new row's first maximum is best_idx unless visit counts tie:
 *     best_idx breaks ties in legal-move order, the row is in child order.  has_old 0 gives tv 0 and agree 0. */
#define BO_REANALYSIS_WORDS 16
typedef struct bo_reanalysis {
    int32_t terminal, n_legal, total_visits, best_idx;
    float root_value;
    int32_t pi_n;
    float played_prob;
    int32_t has_old, agree;
    float tv;
    int32_t phase, status, ply, sims_done, watch, reserved;
} bo_reanalysis;
int bo_records_ring(const bo_position *pos_dev, int64_t n, void *ring_out_dev, void *stream);
int bo_reanalysis_result(bo_engine *e, const int32_t *played_action_dev, const int64_t *root_dev, const int32_t *old_ptr_dev,
                         const int32_t *old_idx_dev, const float *old_val_dev, int32_t W, bo_reanalysis *out, int32_t *pi_idx_out,
                         float *pi_val_out, void *stream);

/* ---- (ABI 16, addition) opening books from games: csrc/bo_book.h, betaone_amd/book.py -----------------------------------------------
 * Every position of every game inside a ply window, grouped by its exact transposition key, with integer aggregates per group.  The
 * positions are ring entries (BO_PGN_POSITION_BYTES each) that bo_pgn_replay / bo_records_ring left in pos_dev[capacity]; the entry's own
 * khash word is the probe start and a filter (read, never recomputed), equality is the exact key: the eight bitboards, the side to
 * move, the castling rights and the en-passant square where a capture is legal.  Entries with an equal key and different khash words
 * (a caller's error) are never merged.  Engine-less; one lane per item; asynchronous on `stream`; every pointer is device memory the
 * caller owns.
 *   Work item i (n items, 0 <= n < 2^31): entry_dev[i] (int64 index into the ring), ply_dev[i], result_dev[i] (0 unknown, 1 white won,
 *     2 draw, 3 black won), eval_dev[i] (float32 seen by the side to move at the entry; NaN: none; eval_dev may be NULL: no item has
 *     one), back_dev[i]: how many entries directly in front of entry_dev[i] belong to the same game and the window.  An item with an
 *     equal key among those entries is SKIPPED: a game counts once per position, at the lowest ply it reaches it.
 *   The table: T slots, T a power of two <= 2^30, as columns the caller prepares: owner int32 [T] = -1, first int64 [T] = INT64_MAX,
 *     min_ply int32 [T] = INT32_MAX, and n, w, d, l, n_eval int32 [T] = 0, sum_eval int64 [T] = 0.  After the call a slot with
 *     owner >= 0 is one group: owner = the index of the item that claimed the slot, first = the smallest entry index in the group,
 *     n = items (games) counted, w / d / l = those with result 1 / 2 / 3, n_eval = those with an eval, sum_eval = the sum of
 *     lrintf(clamp(eval, -1, 1) * BO_BOOK_EVAL_ONE) in WHITE's view (negated where black is to move), min_ply = the lowest ply.
 *     Integers only: the columns of a group do not depend on the order of the items (its slot and its owner can; compare by first).
 *     One call fills one table: owner holds indices into THIS call's item arrays.
 *   gid_out_dev [n] int32: the item's slot; -1 skipped (counted already, or a bad entry); -2 overflow: T probes found neither an empty
 *     slot nor the item's group -- nothing of it is counted; run again with a larger T.
 *   status_dev int32 [2], ADDED TO: [0] overflow items, [1] bad entries -- an entry outside [0, capacity) contributes nothing, and
 *     nothing outside the ring is ever read (back_dev is cut at entry 0).
 *   flags: BO_BOOK_NO_COMBINE -- every lane issues its own atomics; without it the lanes of a wave that found the same slot combine
 *     first (same columns either way).
 * BO_E_ARG: n or capacity negative, T no power of two or out of range, unknown flag bits, a NULL column or status, and with n > 0 any
 * other NULL pointer but eval_dev.  n == 0 does nothing.  Probing is linear, one relaxed agent-scope compare-and-swap on owner per
 * probed slot; no workgroup waits for another. */
#define BO_BOOK_NO_COMBINE 1u
#define BO_BOOK_EVAL_ONE (1 << 20)
int bo_book_insert(const void *pos_dev, int64_t capacity, int64_t n, const int64_t *entry_dev, const int32_t *ply_dev,
                   const int32_t *result_dev, const float *eval_dev /* may be NULL */, const int32_t *back_dev, int64_t T,
                   int32_t *owner_dev, int64_t *first_dev, int32_t *n_dev, int32_t *w_dev, int32_t *d_dev, int32_t *l_dev,
                   int32_t *n_eval_dev, int32_t *min_ply_dev, int64_t *sum_eval_dev, int32_t *gid_out_dev, int32_t *status_dev,
                   uint32_t flags, void *stream);

/* ---- (ABI 10, additions) perft on the device: csrc/bo_perft.h, betaone_amd/perft.py ------------------------------------------------
 * perft(depth) = the number of move sequences of length `depth` from a root, as python-chess's Board perft counts them: draw rules are
 * ignored, only a position without legal moves ends a line.  The tree is walked level by level on a frontier in device memory, one
 * wavefront per position, with the move generator and make_move of the searches (csrc/bo_chess.h).  Engine-less; SYNCHRONISES `stream`
 * (the level sizes are read back) and allocates and frees its own device memory.
 *
 * fens [n_roots]: FEN strings, NULL = the start position (fens itself may be NULL: all start positions); a root needs one king per
 * side (BO_E_FEN otherwise, as for an unparsable FEN).  The roots' en-passant key is resolved as bo_games_reset resolves it.
 * depth >= 0.  capacity: positions per level buffer, 256 <= capacity <= 2^26 (BO_E_CONFIG otherwise); there is one buffer per level
 * below the root, allocated as far as it is used.  When the children of a level do not fit, the level is split into chunks of
 * consecutive entries whose children do fit and each chunk is taken to the bottom before the next starts: *n_splits (may be NULL)
 * counts the extra chunks.  The results do not depend on capacity.  n_roots <= 2^20; n_roots == 0 does nothing.
 * flags: BO_PERFT_DIVIDE fills divide_moves / divide_nodes ([n_roots][BO_MAX_LEGAL], both needed then, else ignored): the root's moves
 * in generated order (from | to << 6 | promo << 12; -1 beyond n_moves) and the node count below each (depth 0: all zero);
 * BO_PERFT_STATS fills results[r].stats (slower: every leaf is made and its own moves generated instead of counting the last level
 * in bulk); BO_PERFT_ORDER fills results[r].checksum.  Fields that were not asked for are zero.
 * A root without legal moves has 0 nodes for depth >= 1; depth 0 gives 1 node, zero stats and checksum 0. */
enum { BO_PERFT_DIVIDE = 1, BO_PERFT_STATS = 2, BO_PERFT_ORDER = 4 };
typedef struct bo_perft_stats {   /* over the leaves (the positions at `depth`), the published perft breakdown */
    uint64_t captures;            /* the last move took a piece, en passant included */
    uint64_t en_passant;          /* the last move was an en-passant capture */
    uint64_t castles;             /* ... a castling move */
    uint64_t promotions;          /* ... a promotion */
    uint64_t checks;              /* the leaf's side to move is in check (checkmates included) */
    uint64_t checkmates;          /* in check and no legal move */
    uint64_t stalemates;          /* not in check and no legal move */
} bo_perft_stats;
typedef struct bo_perft_result {
    uint64_t nodes;               /* perft(depth) of this root */
    uint64_t checksum;            /* BO_PERFT_ORDER: sum mod 2^64, over every node at depth 0 .. depth - 1, of the FNV-1a hash of its move
                                   * list in generated order: h = 0xcbf29ce484222325, per move word m: h = (h ^ m) * 0x100000001b3 */
    bo_perft_stats stats;         /* BO_PERFT_STATS */
    int32_t n_moves;              /* legal moves of the root (depth 0: not generated, 0) */
    int32_t reserved;
} bo_perft_result;
int bo_perft(int device, int32_t n_roots, const char *const *fens, int32_t depth, int64_t capacity, uint32_t flags, bo_perft_result *results,
             int32_t *divide_moves, uint64_t *divide_nodes, int64_t *n_splits, void *stream);

/* ---- (ABI 11, additions) endgame tablebases on the device: csrc/bo_tb.h, betaone_amd/tablebase.py ----------------------------------
 * Distance to mate in plies, 50-move rule ignored, no castling rights, 2 to 4 men, pawns on one side only (so no en passant).
 * material: the strong side first, "KQK", "KPK", "KBNK", "KQKR" ...; each side's pieces are kept in the order Q R B N P.  The strong
 * side is white in the table's frame; the colour-swapped material is served by the mirror (ranks flipped, colours and the side to move
 * swapped).  5 or more men, a malformed name, the weaker side first ("KKQ", "KPKR": the message names "KQK", "KRKP"): BO_E_ARG; pawns on both sides ("KPKP"): BO_E_CONFIG (a follow-up: it needs en passant).
 * Index: idx = ((stm * 64 + sq[0]) * 64 + sq[1]) ... over the piece list K, strong pieces, k, weak pieces; stm 0 = the strong side
 * moves; 2 * 64^men entries.  Payload: one uint16 per entry -- 0 not a position, 1 draw, 2 + k mate in k plies (k even: the side to
 * move is mated in k, k = 0 checkmate; k odd: the side to move mates in k).
 * bo_tb_create: sub_tables [n] are the complete tables a capture or a promotion of `material` leads to (KK, KBK and KNK need none:
 * insufficient material, a draw); one that is needed and not given, or not complete: BO_E_STATE with its name in bo_last_error().
 * The table keeps the pointers: destroy it before its sub-tables.
 * bo_tb_build: the classification of every index, then passes 1, 2, ... (pass i assigns exactly the entries whose value is i), until a
 * pass assigns nothing and i - 1 exceeds the largest value in any sub-table.  max_passes < 0: to the end; otherwise at most that many
 * passes (0: the classification only) and the table stays incomplete when they do not reach the end.  *passes (may be NULL) = passes
 * run.  SYNCHRONISES `stream` (one counter is read after each pass).  Two builds give the same bytes.
 * bo_tb_verify: every entry recomputed from its children's codes (and every index's legality); *mismatches must be 0.
 * bo_tb_stats: per side to move (0 strong, 1 weak) over the payload; complete tables only fill `complete` = 1.
 * bo_tb_download / bo_tb_upload: the payload as a host array of n_entries uint16 (BO_E_ARG when n_entries is not the table's); an
 * uploaded table counts as complete.
 * bo_tb_probe: positions [n] (HOST memory) against the set tbs [n_tb <= 64, complete tables on one device]: codes [n] (uint16) and
 * status [n] (BO_TB_*) to host memory; SYNCHRONISES `stream`.  Clocks and the e.p. square are ignored. */
enum {
    BO_TB_COVERED = 0,         /* codes[i] is the position's code (insufficient material: 1, no table needed) */
    BO_TB_NO_TABLE = 1,        /* its material's table is not in the set */
    BO_TB_TOO_MANY_MEN = 2,    /* more than 4 men */
    BO_TB_CASTLING = 3,        /* castling rights */
    BO_TB_PAWNS_BOTH = 4,      /* pawns of both colours */
    BO_TB_NOT_A_POSITION = 5   /* the table holds code 0 for it (the side not to move is in check, ...) or a king is missing */
};
typedef struct bo_tb bo_tb;
typedef struct bo_tb_side_stats {
    uint64_t legal, wins, draws, losses;   /* entries with this side to move: code != 0, odd k, code 1, even k */
    int32_t max_win_ply, max_loss_ply;     /* the largest k of a win / of a loss, -1 when there is none */
} bo_tb_side_stats;
typedef struct bo_tb_info {
    int64_t n_entries;
    int32_t n_men, passes, complete, reserved;
    uint64_t fnv1a;                        /* FNV-1a (64 bit) over the payload's little-endian bytes */
    bo_tb_side_stats side[2];              /* 0: the strong side to move, 1: the weak side */
    char material[16];                     /* the name as the table keeps it */
} bo_tb_info;
int bo_tb_create(int device, const char *material, bo_tb *const *sub_tables, int32_t n_sub, bo_tb **out);
int bo_tb_build(bo_tb *tb, int32_t max_passes, int32_t *passes, void *stream);
int bo_tb_verify(bo_tb *tb, uint64_t *mismatches, void *stream);
int bo_tb_stats(bo_tb *tb, bo_tb_info *out);
int bo_tb_download(bo_tb *tb, uint16_t *codes, int64_t n_entries);
int bo_tb_upload(bo_tb *tb, const uint16_t *codes, int64_t n_entries, int32_t passes);
int bo_tb_probe(bo_tb *const *tbs, int32_t n_tb, const bo_position *positions, int32_t n, uint16_t *codes, int32_t *status, void *stream);
void bo_tb_destroy(bo_tb *tb);

/* ---- (ABI 14, additions) the tables inside the search and at the root: csrc/bo_tree.h, DESIGN "Tablebases in the search" -------------
 * bo_engine_tablebases: the engine's searches read the set tbs [n_tb <= 64, complete tables on the engine's device] from now on.
 *   flags bit 0: probe in the search -- a leaf the rules leave ongoing, with <= 4 men and no castling rights, that the set gives as a
 *     draw or as a mate in k with halfmove clock + k <= 100 becomes a terminal leaf of value 0 / +-(1 - min(k, 512) / 1024) (the sign as
 *     for the rule mate: seen by the side that just moved).  The root is never probed in the search.  bo_debug_tree reports such leaves
 *     with terminal 3 (the side to move wins), 4 (it loses), 5 (draw).  The step then launches the kernel's probing instantiation.
 *   flags bit 1: adjudicate -- every new root (bo_games_reset*, bo_play, the device turn) the rules leave ongoing and the set covers as
 *     drawn gets terminal code 2, as lost for the side to move code 3; no search begins there.  No clock condition (tablebase.rescore's rule).
 *   n_tb = 0 (or flags 0): off -- every path is bit for bit what it is without the call.
 *   The descriptors are copied; the TABLES are not: they must outlive the engine's use of them (destroy the engine, or turn the set
 *   off, before bo_tb_destroy).  Call it before a step or a turn is captured into a graph: the kernel arguments are baked into the
 *   capture.  Synchronises the device's null stream.  BO_E_ARG: more than 64 tables, unknown flag bits, a table on another device;
 *   BO_E_STATE: an incomplete table (its name in bo_last_error()); BO_E_CONFIG: a fast-mode engine.
 * bo_engine_tb_stats: per game [G] (any may be NULL): table leaves created and simulations absorbed by table leaves since the game's
 *   set-up, and 1 where the game's CURRENT root was adjudicated (terminal 2 or 3 from the tables, not from the rules).  Synchronises. */
int bo_engine_tablebases(bo_engine *e, bo_tb *const *tbs, int32_t n_tb, int32_t flags);
int bo_engine_tb_stats(bo_engine *e, int32_t *tb_nodes, int32_t *tb_sims, int32_t *adjudicated, void *stream);

/* ---- (ABI 19, additions) forced mates on the device: csrc/bo_mate.h, betaone_amd/mate.py ---------------------------------------------
 * Is there a forced mate in at most max_moves moves for the root's side to move (the attacker), in how many plies, and by which first
 * moves?  dtm = plies to mate with best play by both sides (odd for the attacker; mate in m moves = dtm 2 m - 1), 0 = none within the
 * budget.  Draw rules are IGNORED, as in perft and the tablebases: only a position without legal moves ends a line.  A search for mate
 * in at most n moves is a full-width walk to depth 2 n - 1 over perft's frontier with an AND/OR backup.  Engine-less; SYNCHRONISES
 * `stream` and allocates and frees its own device memory, as bo_perft does.
 *
 * Roots: EITHER fens [n_roots] (NULL entries = the start position; a FEN that does not parse or is not a position: BO_E_FEN, as for
 * bo_perft) OR positions [n_roots] (HOST memory, as bo_tb_probe takes them; a record that is not a position gets status
 * BO_MATE_NOT_A_POSITION and is not searched).  Not a position: not exactly one king per side, overlapping or inconsistent bitboards,
 * pawns on the first or last rank, more than 16 men or more promoted pieces than missing pawns on a side (the move list has room for
 * 256 moves), and -- seen by the device -- the side NOT to move in check.  n_roots <= 2^20; n_roots == 0 does nothing.
 * max_moves N: 1 .. 16.  capacity: as for bo_perft (256 .. 2^26 positions per level buffer, BO_E_CONFIG otherwise; the results do not
 * depend on it, *n_splits counts the extra chunks).
 * The driver deepens iteratively: n = 1, 2, ..., N over the roots still unresolved; a root resolved at iteration n has dtm = 2 n - 1
 * exactly and drops out.  max_nodes (0 = unlimited): before an iteration starts, if the nodes counted so far exceed it, the call stops;
 * results[r].searched = the largest n completed for that root.
 * nodes: the positions the walks of this call visited -- the frontier entries of every level of every iteration, the roots included,
 * each of which had its move list generated by the level's count kernel; the passes of BO_MATE_PV count too (and are not bounded by
 * max_nodes).  It is the number of the WHOLE call, the same in every result.  (Not counted: the child lists an attacker entry generates
 * to classify its moves, and the regeneration in the expand kernels.)
 * key_moves (may be NULL) [n_roots][BO_MAX_LEGAL]: the root moves that begin a shortest mate, in generated order, -1 beyond n_keys.
 * flags: BO_MATE_PV fills pv [n_roots][2 N - 1] (needed then), -1 beyond dtm: the attacker plays the lowest-index key move, the
 * defender the reply of longest resistance (lowest index on ties).  It is computed by solving again along the line -- the defender's
 * replies of all solved roots become one batch of roots at n - 1, N - 1 further passes -- and MAY COST AS MUCH AS THE SOLVE.
 * Arguments are checked in this order, before any device call: n_roots out of range or both / neither of fens and positions
 * (BO_E_ARG); max_moves out of range (BO_E_ARG); capacity (BO_E_CONFIG); unknown flag bits (BO_E_ARG); results NULL with n_roots > 0,
 * or BO_MATE_PV without pv (BO_E_ARG). */
enum { BO_MATE_PV = 1 };
enum { BO_MATE_OK = 0, BO_MATE_CHECKMATED = 1, BO_MATE_STALEMATED = 2, BO_MATE_NOT_A_POSITION = 3 };
#define BO_MATE_MAX_MOVES 16
typedef struct bo_mate_result {
    int32_t status;               /* BO_MATE_*: ok; the root's side to move is checkmated / stalemated; not a position */
    int32_t dtm;                  /* plies to mate, 0 = none found within `searched` moves */
    int32_t searched;             /* the largest n completed for this root (a resolved root: its mate distance in moves) */
    int32_t n_moves;              /* legal moves of the root */
    int32_t n_keys;               /* root moves that begin a shortest mate */
    int32_t key;                  /* the lowest-index one (from | to << 6 | promo << 12), -1 none */
    uint64_t nodes;               /* of the whole call, see above */
} bo_mate_result;
int bo_mate(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t max_moves, int64_t capacity,
            uint64_t max_nodes, uint32_t flags, bo_mate_result *results, int32_t *key_moves, int32_t *pv, int64_t *n_splits, void *stream);

/* ---- (ABI 20, additions) the anchor opponent on the device: csrc/bo_anchor.h, betaone_amd/anchor.py ----------------------------------
 * A deterministic classical player: a fixed-depth FULL-WIDTH negamax with a small integer static evaluation (DESIGN.md "Anchor
 * opponent"), for whole batches of roots.  Draw rules are IGNORED inside the tree, as in perft and bo_mate: only a position without
 * legal moves ends a line.  With p the plies below the root and D = depth:
 *   val(P, p) = -(BO_ANCHOR_MATE - p) if P has no legal move and is in check, 0 if it has none and is not;
 *               ev(P) if p == D;  the maximum over the moves m of -val(P.m, p + 1) otherwise.
 * ev(P), centipawns from the side to move's view = the terms of its men minus the terms of the other side's.  For a man on file index
 * f and rank index r counted from its owner's back rank, e = min(f, 7 - f), d = e + min(r, 7 - r): pawn 100 + 2 (r - 1)^2 + 3 e;
 * knight 300 + 8 d; bishop 320 + 4 d; rook 500, + 20 if r == 6; queen 900 + 2 d; king 8 d if no queen of either colour is on the
 * board, else -6 r.  |ev| < 15000; every value fits an int16.
 * Per root: move_scores[i] = -val(root.m_i, 1) in the generator's order; score = their maximum (a mate in 1 scores
 * BO_ANCHOR_MATE - 1); best = the lowest-index move that reaches it; n_best = how many do.  Engine-less; SYNCHRONISES `stream` and
 * allocates and frees its own device memory, as bo_mate does.
 *
 * Roots, "not a position", n_roots and capacity: exactly as for bo_mate.  depth: 1 .. BO_ANCHOR_MAX_DEPTH.  flags: none defined (0).
 * nodes: the frontier entries of levels 0 .. depth - 1 of the whole call (the positions whose move lists a level's kernel generated;
 * the children the last level makes and evaluates are not entries), the same in every result and at every capacity.
 * root_moves, move_scores (each may be NULL) [n_roots][BO_MAX_LEGAL]: entries beyond n_moves are -1 and INT32_MIN.
 * Arguments are checked in this order, before any device call: n_roots out of range or both / neither of fens and positions
 * (BO_E_ARG); depth out of range (BO_E_ARG); capacity (BO_E_CONFIG); flag bits (BO_E_ARG); results NULL with n_roots > 0 (BO_E_ARG).
 *
 * bo_anchor_eval: ev_out[i] = ev(positions[i]) (HOST memory both), one wave per position; INT32_MIN for a record that is not a
 * position by the host-side rules above.  n <= 2^24; n == 0 does nothing.  Synchronises. */
enum { BO_ANCHOR_OK = 0, BO_ANCHOR_CHECKMATED = 1, BO_ANCHOR_STALEMATED = 2, BO_ANCHOR_NOT_A_POSITION = 3 };
#define BO_ANCHOR_MAX_DEPTH 8
#define BO_ANCHOR_MATE 30000
typedef struct bo_anchor_result {
    int32_t status;               /* BO_ANCHOR_*: ok; the root's side to move is checkmated / stalemated; not a position */
    int32_t score;                /* the maximum of the move scores (0 unless status is ok) */
    int32_t best;                 /* the lowest-index move that reaches it (from | to << 6 | promo << 12), -1 none */
    int32_t n_best;               /* moves that reach it */
    int32_t n_moves;              /* legal moves of the root */
    int32_t reserved;             /* 0 */
    uint64_t nodes;               /* of the whole call, see above */
} bo_anchor_result;
int bo_anchor(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t depth, int64_t capacity,
              uint32_t flags, bo_anchor_result *results, int32_t *root_moves, int32_t *move_scores, int64_t *n_splits, void *stream);
int bo_anchor_eval(int device, int32_t n, const bo_position *positions, int32_t *ev_out, void *stream);

/* ---- (ABI 22, additions) quiescence behind the anchor's fixed-depth walk ----------------------------------------------------------
 * bo_anchor_q is bo_anchor with `quiesce` = Q, 0 .. BO_ANCHOR_MAX_QUIESCE, after `depth`: the same results, arrays and status rules.
 * At p == D a position with a legal move gets qs(P, D, Q) in place of ev(P):
 *   The TACTICAL moves of P: all its legal moves if its side to move is in check; otherwise the legal moves that capture (the
 *   destination holds an enemy man, or an en passant capture) or promote (to any piece); in the generator's order.
 *   qs(P, p, q) = -(BO_ANCHOR_MATE - p) if P has no legal move and is in check, 0 if it has none and is not;  ev(P) if q == 0;
 *                 otherwise the maximum of the FLOOR -- ev(P) if P is not in check, -BO_ANCHOR_MATE if it is (no standing pat in
 *                 check) -- and of -qs(P.m, p + 1, q - 1) over the tactical moves m.
 * Draw rules are ignored, as above.  p <= D + Q <= 16 and -BO_ANCHOR_MATE itself are representable: every value still fits an int16.
 * A mate score out of the quiescence plies is a FORCED mate: the mated side stood in check at each of its nodes, so every one of its
 * replies was searched.  A found mate is therefore a score >= BO_ANCHOR_MATE - (D + Q).
 * nodes: the frontier entries of levels 0 .. D + Q - 1 -- levels 0 .. D - 1 are full width, an entry of level D .. D + Q - 1 has its
 * tactical moves as children; the children the last level makes are not entries.  The same at every capacity.
 * quiesce == 0 takes bo_anchor's path: the same kernels, byte-identical output.
 * Arguments are checked in this order, before any device call: n_roots / fens / positions (BO_E_ARG); depth (BO_E_ARG); quiesce
 * (BO_E_ARG); capacity (BO_E_CONFIG); flag bits (BO_E_ARG); results NULL with n_roots > 0 (BO_E_ARG). */
#define BO_ANCHOR_MAX_QUIESCE 8
int bo_anchor_q(int device, int32_t n_roots, const char *const *fens, const bo_position *positions, int32_t depth, int32_t quiesce,
                int64_t capacity, uint32_t flags, bo_anchor_result *results, int32_t *root_moves, int32_t *move_scores, int64_t *n_splits,
                void *stream);

/* ---- (ABI 21, additions) a look at a running FAST-mode search: csrc/bo_info.h, betaone_amd/uci.py -----------------------------------
 * bo_search_info: one bo_search_info_rec per slot into out[G] (device memory, or pinned device-mapped host memory; every word is stored
 * exactly once).  Read-only and asynchronous; to be enqueued between two bo_step calls (or before the first / after the last), whatever
 * the slots' phases.  Fast-mode engines only (BO_E_CONFIG: reference-semantics engines have bo_analysis_result).
 *   phase (0 idle, 1 running, 2 finished), status (BO_ST_* bits), terminal (bo_root_info's code), n_legal, sims_done (of this search:
 *   completed backups only); root_visits: the root record's count (visits kept from earlier searches included); arena_top /
 *   arena_granules: granules in use / per arena; watch: the word(s) named to bo_engine_watch as the last result kernel left them.
 *   n_lines = min(n_lines asked for, BO_INFO_LINES, root children with a visit); 0 for a terminal or unexpanded root.
 *   line[i]: the root child with the i-th most visits; among equal counts the earlier child in record (= legal-move) order first, so
 *     line[0].move is bo_search_result's best move on the same tree.  visits; w: the child's raw float32 value sum, seen by the side
 *     to move at the root (csrc/bo_fastw.h: W of a node is seen by the player who moved into it) -- the host divides; prior.
 *     pv[0 .. pv_len): pv[0] == move, then at each node the child with the most visits, the first maximum in record order; the
 *     variation ends at a node without children (unvisited, known mate, known draw), at a node whose best child has no visit, and
 *     at BO_INFO_PV moves.  Words beyond n_lines / pv_len are 0. */
#define BO_INFO_LINES 8
#define BO_INFO_PV 24
typedef struct bo_info_line {
    int32_t move, visits;
    float w, prior;
    int32_t pv_len, pv[BO_INFO_PV], reserved[3];
} bo_info_line;
typedef struct bo_search_info_rec {
    int32_t phase, status, terminal, n_legal, sims_done, root_visits, arena_top, arena_granules, watch, n_lines, reserved[6];
    bo_info_line line[BO_INFO_LINES];
} bo_search_info_rec;
int bo_search_info(bo_engine *e, int32_t n_lines, bo_search_info_rec *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
