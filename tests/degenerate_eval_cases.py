"""tests/degenerate_eval_cases.py -- backend-independent bodies of the tests of the tree step on DEGENERATE evaluation rows (emu on
CPU, hip on GPU): the rows a trained net produces and the hash net of the other suites never does.

Part A, finite rows (fake_model.FAMILIES): priors of exactly 0 and denormal priors (stable_rank's ties among zeros, select_leaf's
argmax over scores of exactly 0, denormals kept by the GPU build), no legal mass at all (the root's `sum + 1e-12f`), values of exactly
+-1 and +-0.  The engine must give the oracle's bits.

Part B, non-finite rows: the contract at BO_ST_NAN_SCORE (include/betaone_engine.h).  The step that consumes a row with a NaN or an
infinity where the engine would store a prior or back up a value flags the game, stores finite priors only, builds every node from
its own parent's legal moves, and the search runs to its end without touching the other slots."""
from __future__ import annotations

import functools

import numpy as np

import engine_cases as EC
import golden_util as G
from betaone_amd import engine as E
from engine_harness import Buf, Searcher, canonical_tree, dense_pi, make_engine
from fake_model import FAMILIES, ILLEGAL_MASS_ACTIONS, family_eval, fake_logits_values
from oracle import oracle as O

KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
POSITIONS = {"start": (O.STARTING_FEN, 31), "kiwipete": (KIWIPETE, 32)}  # name -> (fen, salt of its evaluator)
CONFIGS = [(1.5, 0.1), (4.0, 0.0), (4.0, 0.1)]  # (widen_coeff, dirichlet_alpha)
SIMS, BATCH, SEED = 120, 8, 9
SWEEP = [(f, w, a, p) for f in FAMILIES for (w, a) in CONFIGS for p in POSITIONS]
SWEEP_IDS = [f"{f}-w{w}-a{a}-{p}" for f, w, a, p in SWEEP]

DEGENERATE_SEARCHES = {e["case"]["name"]: e for e in G.load_degenerate_searches()}
DEGENERATE_SEARCH_NAMES = list(DEGENERATE_SEARCHES)


# ---- A1. searches the unmodified reference executed -----------------------------------------------------------------------
def check_degenerate_golden_search(backend, name):
    EC.check_golden_search(backend, name, DEGENERATE_SEARCHES)


# ---- A2. every family x config x position against the oracle ----------------------------------------------------------------
def _cfg(widen, alpha, sims=SIMS):
    return dict(num_simulations=sims, batch_size=BATCH, widen_coeff=widen, dirichlet_alpha=alpha)


@functools.lru_cache(maxsize=None)
def oracle_search(family, widen, alpha, pos):
    """The oracle's search of one sweep case: computed once, shared by the tests that need it, never modified."""
    fen, salt = POSITIONS[pos]
    b = O.Board(fen)
    trk = O.PyTracker(); trk.add_board(b)
    return O.run_mcts(b, [], trk, family_eval(family, salt), np.random.RandomState(SEED), O.default_config(**_cfg(widen, alpha)))


def check_family_vs_oracle(backend, family, widen, alpha, pos):
    fen, salt = POSITIONS[pos]
    r = oracle_search(family, widen, alpha, pos)
    eng = make_engine(backend, 1, _cfg(widen, alpha))
    eng.reset([0], [fen], [None])
    res = Searcher(backend, eng).search([1], [family_eval(family, salt)], [np.random.RandomState(SEED)], alpha)
    exp = {"/".join(k): list(v) for k, v in O.canonical_tree(r["nodes"]).items()}
    got = canonical_tree(eng.debug_tree(0))
    assert set(got) == set(exp), "the trees hold different nodes"
    for k in exp:  # [n, q bits, prior bits, child count]
        assert got[k] == exp[k], (k, got[k], exp[k])
    assert np.array_equal(dense_pi(res, 0).view(np.uint32), r["pi"].view(np.uint32))
    assert E.move_to_uci(int(res["best_move"][0])) == O.move_to_uci(r["best"])
    assert int(eng.status()["term_sims"][0]) == r["n_terminal_sims"]
    eng.close()


# ---- A3. the edge is in the inputs: asserted on the ORACLE's trees --------------------------------------------------------------
TINY = np.float32(2.0 ** -126)  # smallest normal binary32


def _created_priors(family, widen, alpha):
    return np.array([nd["prior"] for p in POSITIONS for nd in oracle_search(family, widen, alpha, p)["nodes"][1:]], np.float32)


def check_edge_conditions():
    """Floors at less than half of what was measured with these salts (peak: 113 zero and 29 denormal priors of 338 created nodes;
    illegal_mass: 331 of 331 zero)."""
    pr = _created_priors("peak", 4.0, 0.0)
    zeros, denormals = int((pr == 0).sum()), int(((pr > 0) & (pr < TINY)).sum())
    print(f"peak (4.0, 0.0): {len(pr)} created nodes, {zeros} with prior 0, {denormals} with a denormal prior")
    assert zeros >= 50 and denormals >= 10
    pr = _created_priors("illegal_mass", 4.0, 0.0)
    print(f"illegal_mass (4.0, 0.0): {len(pr)} created nodes, {int((pr == 0).sum())} with prior 0")
    assert len(pr) >= 100 and np.all(pr == 0)
    for fen, _ in POSITIONS.values():  # the eight boosted actions leave the board: legal nowhere
        assert not {O.move_to_index(m) for m in O.Board(fen).legal_moves()} & set(ILLEGAL_MASS_ACTIONS)


# ---- A4. short games: root normalisation with noise and the temperature turn over sparse pis -----------------------------------
def check_family_games(backend, family):
    EC.check_multi_game_vs_oracle(backend, n_games=2, plies=3, sims=40, batch=8, eval_fn_for=lambda salt: family_eval(family, salt))


# ---- B. non-finite rows: the contract at BO_ST_NAN_SCORE ---------------------------------------------------------------------------
B_SIMS, B_BATCH, B_ALPHA = 60, 8, 0.1
B_FENS, B_SALTS, B_SEEDS = [O.STARTING_FEN, KIWIPETE], [51, 52], [7, 8]  # slot 0 gets the poisoned rows, slot 1 a clean net
WIDENS = [1.5, 4.0]
PROBS_POISONS = ["row_nan", "one_nan", "one_inf", "value_nan", "value_inf"]
LOGITS_POISONS = ["logit_nan", "logit_inf", "logits_all_ninf"]
# (a value is consumed at leaves only: the root's evaluation gives priors, its value is not backed up -- no root case for the value poisons)
POISON_CASES = [(k, p, w) for k, ps in (("probs", PROBS_POISONS), ("logits", LOGITS_POISONS)) for p in ps
                for w in ("root", "from4") if not (p.startswith("value") and w == "root")]
POISON_IDS = [f"{k}-{p}-{w}" for k, p, w in POISON_CASES]


def fen_of_planes(row):
    """The position an input row encodes: its last history block (planes 98..109) and the scalar planes 112..119."""
    board = [None] * 64
    for t, sym in enumerate("PNBRQK"):
        for pl, s_ in ((98 + 2 * t, sym), (99 + 2 * t, sym.lower())):
            for s in np.nonzero(row[pl].reshape(64))[0]:
                board[s] = s_
    ranks = []
    for r in range(7, -1, -1):
        out, gap = "", 0
        for f in range(8):
            c = board[8 * r + f]
            if c is None:
                gap += 1
            else:
                out, gap = out + (str(gap) if gap else "") + c, 0
        ranks.append(out + (str(gap) if gap else ""))
    castling = "".join(c for c, pl in zip("KQkq", (113, 114, 115, 116)) if row[pl, 0, 0]) or "-"
    ep = np.nonzero(row[119].reshape(64))[0]
    ep = "abcdefgh"[ep[0] % 8] + str(ep[0] // 8 + 1) if len(ep) else "-"
    return f"{'/'.join(ranks)} {'w' if row[112, 0, 0] else 'b'} {castling} {ep} {int(row[117, 0, 0])} {int(row[118, 0, 0])}"


def legal_indices(row):
    return sorted(O.move_to_index(m) for m in O.Board(fen_of_planes(row)).legal_moves())


def _poison(name, row, value, legal):
    """Poisons one policy row in place; returns the row's value."""
    if name == "row_nan":
        row[:] = np.nan
    elif name in ("one_nan", "logit_nan"):
        row[legal[0]] = np.nan
    elif name in ("one_inf", "logit_inf"):
        row[legal[0]] = np.inf
    elif name == "logits_all_ninf":
        row[:] = -np.inf
    elif name == "illegal_nan":  # the negative control: an action that leaves the board is never read from a leaf's row
        assert ILLEGAL_MASS_ACTIONS[0] not in legal
        row[ILLEGAL_MASS_ACTIONS[0]] = np.nan
    elif name == "value_nan":
        value = np.nan
    elif name == "value_inf":
        value = np.inf
    else:
        raise KeyError(name)
    return value


def _engine(backend, G, widen, fast_L):
    if not fast_L:
        return make_engine(backend, G, dict(num_simulations=B_SIMS, batch_size=B_BATCH, widen_coeff=widen, dirichlet_alpha=B_ALPHA))
    from engine_harness import emu_call

    kw = dict(num_simulations=B_SIMS, dirichlet_alpha=B_ALPHA, fast=True, leaves_per_step=fast_L, max_plies=256)
    return emu_call(E.Engine, G, **kw) if backend == "emu" else E.Engine(G, **kw)


def run_slots(backend, slots, widen, kind, fast_L=0, poison=None, when=None):
    """One search in every slot (slots: indices into B_FENS), rows evaluated by the hash net; `poison` spoils the rows of the FIRST slot at
    its root evaluation (when == "root") or from its 4th evaluation on ("from4").  Returns the engine, the steps taken and the status
    words read right after each step that consumed a poisoned row."""
    import torch

    G, L = len(slots), fast_L or 1
    eng = _engine(backend, G, widen, fast_L)
    eng.reset(list(range(G)), [B_FENS[s] for s in slots], [None] * G)
    nl, _, _ = eng.root_info()
    noise = np.zeros((G, E.MAX_LEGAL), dtype=np.float64)
    for g, s in enumerate(slots):
        noise[g, :nl[g]] = np.random.RandomState(B_SEEDS[s]).dirichlet([B_ALPHA] * int(nl[g]))
    nn_in, pol, val = Buf(backend, (G * L, 120, 8, 8)), Buf(backend, (G * L, E.NUM_ACTIONS)), Buf(backend, (G * L,))
    eng.search_begin([1] * G, noise, nn_in.ptr)
    k, steps, n_eval0, poisoned, seen = E.POLICY_NONE, 0, 0, False, []
    while True:
        eng.step(pol.ptr, val.ptr, k, nn_in.ptr)
        steps += 1
        if poisoned:
            seen.append(eng.status_bits().copy())
            poisoned = False
        running, _, mask = eng.poll()
        if not running:
            break
        assert steps <= 2 * B_SIMS + 4, "the search does not end"
        planes = nn_in.numpy()
        p, v = np.zeros((G * L, E.NUM_ACTIONS), np.float32), np.zeros(G * L, np.float32)
        for g, s in enumerate(slots):
            logits, vv = fake_logits_values(planes[g * L:(g + 1) * L], 6.0, B_SALTS[s])
            p[g * L:(g + 1) * L] = logits if kind == "logits" else torch.softmax(torch.from_numpy(logits), dim=1).numpy()
            v[g * L:(g + 1) * L] = vv
        if poison and (fast_L or mask[0]):
            n_eval0 += 1
            if (when == "root" and n_eval0 == 1) or (when == "from4" and n_eval0 >= 4):
                for r in range(L):
                    if planes[r, 98:110].any():  # (fast mode: a row no leaf has used yet is ignored by the engine as well)
                        v[r] = _poison(poison, p[r], v[r], legal_indices(planes[r]))
                poisoned = True
        pol.set(p); val.set(v)
        k = E.POLICY_LOGITS if kind == "logits" else E.POLICY_PROBS
    return eng, steps, seen


def _slot_result(eng, g):
    res = eng.result()
    return dict(tree=eng.debug_tree(g), pi=dense_pi(res, g).view(np.uint32).tolist(), best=int(res["best_move"][g]))


def _same(a, b):
    key = lambda t: [(nd["parent"], nd["n"], G.f32bits(nd["q"]), G.f32bits(nd["prior"]), nd["move"], nd["n_children"]) for nd in t]
    return key(a["tree"]) == key(b["tree"]) and a["pi"] == b["pi"] and a["best"] == b["best"]


@functools.lru_cache(maxsize=None)
def clean_run(backend, slots, widen, kind, fast_L):
    eng, _, _ = run_slots(backend, list(slots), widen, kind, fast_L)
    assert eng.check_status() == 0 and not eng.status_bits().any(), "finite rows are never flagged"
    out = [_slot_result(eng, g) for g in range(len(slots))]
    eng.close()
    return out


def check_tree_invariants(nodes, fen):
    """Every prior and q finite; every node reached by a move that is legal in its parent's position (by the oracle); sibling moves
    distinct; no more children than legal moves."""
    kids = {}
    for i, nd in enumerate(nodes):
        assert np.isfinite(nd["prior"]) and np.isfinite(nd["q"]), (i, nd)
        if nd["parent"] >= 0:
            kids.setdefault(nd["parent"], []).append(i)
    board = O.Board(fen)

    def walk(i):
        ch = kids.get(i, [])
        legal = {O.move_to_uci(m) for m in board.legal_moves()}
        ucis = [E.move_to_uci(nodes[c]["move"]) for c in ch]
        assert len(set(ucis)) == len(ucis), ("duplicate sibling moves", i, ucis)
        assert set(ucis) <= legal, ("moves that are not legal here", i, sorted(set(ucis) - legal))
        assert len(ch) <= len(legal)
        for c, u in zip(ch, ucis):
            board.push(u)
            walk(c)
            board.pop()

    walk(0)


def check_poisoned_search(backend, kind, poison, when, widen, fast_L=0):
    eng, steps, seen = run_slots(backend, [0, 1], widen, kind, fast_L, poison, when)
    assert seen, "no poisoned row was consumed"
    for st in seen:  # read right after the step that consumed the row
        assert st[0] & E.ST_NAN_SCORE and st[1] == 0, st
    assert steps <= 2 * B_SIMS + 4
    try:
        eng.check_status()
        raise AssertionError("check_status() did not raise")
    except E.EngineError as err:
        assert "game slot 0" in str(err) and "NaN" in str(err), str(err)
    assert int(eng.result()["total"][0]) == B_SIMS and int(eng.result()["total"][1]) == B_SIMS  # both searches ran to their end
    assert _same(_slot_result(eng, 1), clean_run(backend, (1,), widen, kind, fast_L)[0]), "the clean slot differs from a run of its own"
    check_tree_invariants(eng.debug_tree(0), B_FENS[0])
    eng.close()


def check_illegal_index_nan_is_not_read(backend, widen, fast_L=0):
    """The negative control: a NaN at an action that is legal nowhere, in every leaf row from the 4th evaluation on, is never read --
    both trees equal the clean run's and no slot is flagged."""
    eng, _, seen = run_slots(backend, [0, 1], widen, "probs", fast_L, "illegal_nan", "from4")
    assert seen and not eng.status_bits().any() and eng.check_status() == 0
    clean = clean_run(backend, (0, 1), widen, "probs", fast_L)
    for g in range(2):
        assert _same(_slot_result(eng, g), clean[g]), g
    assert _same(clean[1], clean_run(backend, (1,), widen, "probs", fast_L)[0])  # (and a slot does not depend on its neighbour)
    eng.close()


def check_rollout_with_nan_net(backend):
    """The product path: a Rollout on 4 games, 32 simulations, whose net returns NaN logits for the rows whose plane sum is odd (while all
    32 men are on the board: the positions with an en-passant square).  After one ply the status check raises and names it."""
    import contextlib

    import torch
    from betaone_amd.rollout import Rollout
    from engine_harness import emulator_backend

    class OddRowsNaN(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(3)
            self.a = torch.nn.Parameter(torch.randn(120 * 64, 16, generator=g) * 0.05)
            self.b = torch.nn.Parameter(torch.randn(16, 4672, generator=g))
            self.register_buffer("nan_rows", torch.zeros((), dtype=torch.int64))

        def forward(self, x):
            f = x.flatten(1)
            h = torch.tanh(f @ self.a)
            odd = torch.remainder(f.sum(dim=1), 2.0) == 1.0
            self.nan_rows.add_(odd.sum())
            logits = torch.where(odd[:, None], torch.full_like(h[:, :1], float("nan")), h @ self.b)
            return logits, torch.tanh(h.sum(dim=1, keepdim=True))

    emu = backend == "emu"
    with emulator_backend() if emu else contextlib.nullcontext():
        net = OddRowsNaN().to("cpu" if emu else "cuda:0").eval()
        kw = dict(device="cpu", use_graph=False) if emu else dict(device="cuda:0")
        ro = Rollout(net, 4, num_simulations=32, mcts_batch_size=8, **kw)
        ro.start_games(list(range(4)), list(range(4)), [np.random.RandomState(s) for s in range(4)])
        try:
            ro.play_ply()
            ro.eng.check_status()
            raise AssertionError("the status check did not raise")
        except E.EngineError as err:
            assert "NaN" in str(err), str(err)
        assert int(net.nan_rows) > 0
        assert (ro.eng.status_bits() & E.ST_NAN_SCORE).any()
        ro.close()
