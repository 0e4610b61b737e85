"""tests/analyse_cases.py -- TEST HELPER: bodies shared by tests/test_analyse_emu.py (wave emulator) and tests/test_analyse_gpu.py (MI355X)
for the analysis path (csrc/bo_analyse.h, betaone_amd/analyse.py): a corpus of PGN games, a slot set up from the device against the
same slot set up from strings, a NumPy restatement of the principal-variation rule."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

import engine_harness as H
import pgn_util as U
from betaone_amd import engine as E

FENS = [None, None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12", "4k3/8/8/8/8/8/8/4K2R b K - 7 33"]  # tests/test_pgn_emu.py
REPETITION = ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "e2e4", "e7e5", "f1c4"]  # plays on past the draw
MATE = ["f2f3", "e7e5", "g2g4", "d8h4"]
EP_FEN = "4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 2"
EP_GAME = ["e5d6", "e8d7", "e1e2", "d7d6"]


def _sans(fen, moves):
    b = U.chess.Board(fen) if fen else U.chess.Board()
    out = []
    for u in moves:
        m = U.chess.Move.from_uci(u)
        out.append(U.san(b, m))
        b.push(m)
    return out


def make_corpus(seed=7, n_random=40, max_plies=120, long_plies=70):
    """(games [(fen, uci moves)], PGN text): n_random random games over both kinds of root (lengths 0..max_plies), then the hand-made
    ones -- a threefold repetition that plays on, a mate, a [FEN] with an en-passant square, a game longer than 64 plies, a game of
    one position.  No eval comments: a plain corpus."""
    rng = random.Random(seed)
    games, text = [], []

    def add(fen, mv, sans, res, headers):
        games.append((fen, list(mv)))
        text.append(U.write_game(sans, [None] * len(mv), res, fen=fen, headers=headers))

    for i in range(n_random):
        fen = FENS[i % len(FENS)]
        mv, _, sans, res = U.random_game(rng, fen=fen, max_plies=rng.randint(0, max_plies), eval_p=0.0, book_p=0.0)
        add(fen, mv, sans, res, {"Event": f"random {i}", "White": "a \\\"quoted\\\" name", "Annotator": "nobody"})
    add(None, REPETITION, _sans(None, REPETITION), "*", {"Event": "repetition", "Result": "*"})
    add(None, MATE, _sans(None, MATE), "0-1", {"Event": "mate", "Result": "0-1"})
    add(EP_FEN, EP_GAME, _sans(EP_FEN, EP_GAME), "1/2-1/2", {"Event": "en passant"})
    for _ in range(200):
        mv, _, sans, res = U.random_game(rng, fen=None, max_plies=120, eval_p=0.0, book_p=0.0)
        if len(mv) >= long_plies:
            break
    assert len(mv) > 64
    add(None, mv, sans, res, {"Event": "long"})
    add(None, [], [], "*", {"Event": "one position"})
    return games, "".join(text)


def flat_eval(planes):
    """Every move equally likely, every position worth 0: visit counts tie."""
    n = planes.shape[0]
    return np.full((n, E.NUM_ACTIONS), np.float32(1.0 / E.NUM_ACTIONS), np.float32), np.zeros(n, np.float32)


def softmax_eval(salt, scale=5.0):
    from fake_model import fake_logits_values

    def fn(planes):
        logits, v = fake_logits_values(planes, scale, salt)
        x = logits.astype(np.float64)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), v
    return fn


class IntBuf:
    """An int32 / int64 / uint8 device array with a raw address (numpy on the emulator, torch on the GPU)."""

    def __init__(self, backend, arr):
        arr = np.ascontiguousarray(arr)
        if backend == "emu":
            self.a, self.t = arr.copy(), None
            self.ptr = self.a.ctypes.data
        else:
            import torch

            self.t = torch.from_numpy(arr.copy()).to("cuda:0")
            self.ptr = self.t.data_ptr()

    def numpy(self):
        if self.t is None:
            return self.a
        import torch

        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def run_searches(backend, eng, nn_in, policy, value, fns, begin):
    """begin() starts the searches; -> (planes after the first step [G,120,8,8], bo_search_result).  fns[g]: slot g's evaluator."""
    G = eng.G
    begin()
    eng.step(0, 0, E.POLICY_NONE, nn_in.ptr)
    first = nn_in.numpy().copy()
    planes = first
    while True:
        running, requested, mask = eng.poll()
        if running == 0:
            break
        pol, val = np.zeros((G, E.NUM_ACTIONS), np.float32), np.zeros(G, np.float32)
        for g in np.nonzero(mask)[0]:
            p, v = fns[g](planes[g:g + 1])
            pol[g], val[g] = p[0], v[0]
        policy.set(pol)
        value.set(val)
        eng.step(policy.ptr, value.ptr, E.POLICY_PROBS, nn_in.ptr)
        planes = nn_in.numpy()
    return first, eng.result()


def slot_state(eng, g):
    """Everything the comparison of two set-ups looks at in slot g."""
    pos, mv = eng.export_game(g)
    return dict(positions=[bytes(p) for p in pos], moves=list(mv), tree=H.canonical_tree(eng.debug_tree(g)))


def walk_pv(nodes, legal, cap=E.PV_CAP):
    """The rule of include/betaone_engine.h (bo_analysis.pv) restated over bo_debug_tree's nodes: -> (pv moves, a tie was seen)."""
    pv, node, tie = [], 0, False
    while len(pv) < cap:
        nd = nodes[node]
        if nd["n_children"] <= 0:
            break
        kids = list(range(nd["first_child"], nd["first_child"] + nd["n_children"]))
        best = max(nodes[k]["n"] for k in kids)
        if best <= 0:
            break
        top = [k for k in kids if nodes[k]["n"] == best]
        tie = tie or len(top) > 1
        pick = min(top, key=(lambda k: legal.index(nodes[k]["move"])) if node == 0 else (lambda k: k))
        pv.append(int(nodes[pick]["move"]))
        node = pick
    return pv, tie


def analysis_records(backend, eng, played):
    G = eng.G
    pl = IntBuf(backend, np.asarray(played, np.int32))
    out = IntBuf(backend, np.zeros((G, 32), np.int32))
    eng.analysis_result(pl.ptr, out.ptr)
    return out.numpy().copy().view(E.ANALYSIS_DTYPE).reshape(G)


def make_engines(backend, G, sims, batch, max_plies):
    cfg = dict(num_simulations=sims, batch_size=batch, dirichlet_alpha=0.0)
    a, b = H.make_engine(backend, G, cfg, max_plies=max_plies), H.make_engine(backend, G, cfg, max_plies=max_plies)
    a.root_values(True)
    b.root_values(True)
    return a, b


def check_setup_and_analysis(backend, games, text, G=64, sims=24, batch=8, oracle_every=0):
    """(a), (b), (d) and, for every oracle_every-th root, (c) of the analysis issue, for EVERY (game, ply) of the corpus."""
    import torch

    from betaone_amd import analyse as A

    lib = H.emu_lib() if backend == "emu" else E.load_hip_library()
    dev = torch.device("cpu" if backend == "emu" else "cuda:0")
    ing = A.Ingested(lib, dev, "corpus", text.encode())
    ing.finish(lib, dev)
    assert ing.n_games == len(games) and set(ing.status.tolist()) == {0}
    assert ing.n_plies.tolist() == [len(mv) for _, mv in games]
    N = ing.n_roots
    assert N == sum(len(mv) for _, mv in games)
    max_plies = max(len(mv) for _, mv in games) + 2
    ea, eb = make_engines(backend, G, sims, batch, max_plies)
    bufs = [(H.Buf(backend, (G, 120, 8, 8)), H.Buf(backend, (G, E.NUM_ACTIONS)), H.Buf(backend, (G,))) for _ in range(2)]
    # pretraining's planes of every root (bo_pgn_sample: the live tracker)
    gs = IntBuf(backend, ing.tok_off[ing.w_game].astype(np.int32))
    ks = IntBuf(backend, ing.w_ply.astype(np.int32))
    states = H.Buf(backend, (N, 120, 8, 8))
    pi_i, z_o = IntBuf(backend, np.zeros(N, np.int32)), H.Buf(backend, (N,))
    pi_v, z_in = H.Buf(backend, (N,)), H.Buf(backend, (ing.T,))
    assert lib.bo_pgn_sample(ing.pos.data_ptr(), ing.act.data_ptr(), z_in.ptr, N, gs.ptr, ks.ptr, states.ptr, pi_i.ptr, pi_v.ptr, z_o.ptr, 0) == 0
    sample_planes = states.numpy()
    slots = IntBuf(backend, np.arange(G, dtype=np.int32))
    compared = searched = ties = oracle_n = code2 = 0
    for b0 in range(0, N, G):
        ids = list(range(b0, min(N, b0 + G)))
        n = len(ids)
        fens = [games[ing.w_game[i]][0] for i in ids]
        mvs = [" ".join(games[ing.w_game[i]][1][:ing.w_ply[i]]) or None for i in ids]
        # evaluators: the hand-made games and every fifth root get the flat one (ties)
        fns = [flat_eval if (i % 5 == 0 or ing.w_game[i] >= len(games) - 5) else softmax_eval(100 + i) for i in ids] + [flat_eval] * (G - n)
        ea.reset(list(range(n)), fens, mvs)
        first = IntBuf(backend, np.concatenate([ing.tok_off[ing.w_game[ids]], np.zeros(G - n, np.int64)]))
        ply = IntBuf(backend, np.concatenate([ing.w_ply[ids], np.full(G - n, -1, np.int32)]).astype(np.int32))
        eb.reset_dev(n, slots.ptr, ing.pos.data_ptr(), ing.T, first.ptr, ply.ptr)
        ia, ib = ea.root_info(), eb.root_info()
        for k in range(3):
            assert np.array_equal(ia[k][:n], ib[k][:n]), ("root_info", k)
        term = ia[1][:n]
        go = np.zeros(G, np.int32)
        go[:n] = term == 0
        want = IntBuf(backend, np.concatenate([np.ones(n, np.int32), np.zeros(G - n, np.int32)]))
        fa, ra = run_searches(backend, ea, *bufs[0], fns, lambda: ea.search_begin(go, None, bufs[0][0].ptr))
        fb, rb = run_searches(backend, eb, *bufs[1], fns, lambda: eb.search_begin_dev(want.ptr, bufs[1][0].ptr))
        va, vb = ea.search_root_value(), eb.search_root_value()
        played = np.concatenate([ing.moves[ids], np.full(G - n, -1, np.int32)])
        rec = analysis_records(backend, eb, played)
        legal_all = None
        for j, i in enumerate(ids):
            sa, sb = slot_state(ea, j), slot_state(eb, j)
            assert sa == sb, (ing.w_game[i], ing.w_ply[i])   # positions incl. ep_key, played moves, the whole tree
            assert sb["moves"] == [int(m) for m in ing.moves[i - ing.w_ply[i]:i]]
            r = rec[j]
            assert int(r["terminal"]) == int(term[j]) and int(r["n_legal"]) == int(ia[0][j]) and int(r["ply"]) == int(ing.w_ply[i])
            compared += 1
            if term[j] != 0:
                code2 += int(term[j] == 2)
                assert int(r["phase"]) == E.PH_IDLE and int(r["pv_len"]) == 0 and int(r["best_move"]) == -1
                continue
            searched += 1
            assert np.array_equal(fa[j].view(np.uint32), fb[j].view(np.uint32))                      # (a) the NN input row
            assert np.array_equal(fb[j].view(np.uint32), sample_planes[i].view(np.uint32))           # (b) pretraining's planes
            for key in ("n", "best_idx", "best_move", "total"):
                assert ra[key][j] == rb[key][j], key
            m = int(ra["n"][j])
            assert np.array_equal(ra["idx"][j, :m], rb["idx"][j, :m]) and np.array_equal(ra["val"][j, :m].view(np.uint32), rb["val"][j, :m].view(np.uint32))
            assert va[j:j + 1].view(np.uint32)[0] == vb[j:j + 1].view(np.uint32)[0]
            # (d) the record against a NumPy walk over the tree
            nodes = eb.debug_tree(j)
            legal = eb.movegen([eb.export_game(j)[0][-1]])[0][0]
            pv, tie = walk_pv(nodes, legal)
            ties += int(tie)
            assert int(r["phase"]) == E.PH_DONE and int(r["status"]) == 0 and int(r["sims_done"]) == sims
            assert int(r["total_visits"]) == int(rb["total"][j]) and int(r["best_move"]) == int(rb["best_move"][j])
            assert r["root_value"].view(np.uint32) == vb[j:j + 1].view(np.uint32)[0]
            assert [int(x) for x in r["pv"][:int(r["pv_len"])]] == pv and (not pv or pv[0] == int(r["best_move"]))
            if int(r["total_visits"]) == 0:
                assert int(r["pv_len"]) == 0
            kids = [k for k in range(nodes[0]["first_child"], nodes[0]["first_child"] + nodes[0]["n_children"]) if nodes[k]["move"] == played[j]]
            assert int(r["played_is_child"]) == len(kids)
            if kids:
                assert int(r["played_visits"]) == nodes[kids[0]]["n"] and r["played_q"].view(np.uint32) == np.float32(nodes[kids[0]]["q"]).view(np.uint32)
            else:
                assert int(r["played_visits"]) == 0 and float(r["played_q"]) == 0.0
            if oracle_every and searched % oracle_every == 0:                                          # (c) the oracle, from the same stack
                oracle_n += 1
                check_against_oracle(games[ing.w_game[i]], int(ing.w_ply[i]), fns[j], sims, batch, nodes, rb, j, vb[j])
    assert compared == N
    return dict(compared=compared, searched=searched, ties=ties, oracle=oracle_n, code2=code2)


def check_against_oracle(game, ply, fn, sims, batch, nodes, res, j, root_q):
    from oracle import oracle as O

    fen, moves = game
    b = O.Board(fen) if fen else O.Board()
    trk = O.PyTracker()
    trk.add_board(b)
    for u in moves[:ply]:
        b.push(u)
        trk.add_board(b)
    pos = b.positions()
    r = O.run_mcts(b, pos[max(0, len(pos) - 8):-1], trk, fn, np.random.RandomState(0),
                   O.default_config(num_simulations=sims, batch_size=batch, dirichlet_alpha=0.0))
    exp = {"/".join(k): list(v) for k, v in O.canonical_tree(r["nodes"]).items()}
    assert H.canonical_tree(nodes) == exp
    assert E.move_to_uci(int(res["best_move"][j])) == O.move_to_uci(r["best"])
    assert np.array_equal(H.dense_pi(res, j).view(np.uint32), r["pi"].view(np.uint32))
    assert np.float32(r["nodes"][0]["q"]).view(np.uint32) == np.float32(root_q).view(np.uint32)


def check_capacity(backend):
    """(e): a root beyond max_plies gets the status bit and is not searched, a range that leaves the array is refused, the slots next
    to them are what the set-up from strings makes them."""
    import torch

    from betaone_amd import analyse as A

    games, text = make_corpus(seed=3, n_random=2, max_plies=30, long_plies=70)
    lib = H.emu_lib() if backend == "emu" else E.load_hip_library()
    dev = torch.device("cpu" if backend == "emu" else "cuda:0")
    ing = A.Ingested(lib, dev, "corpus", text.encode())
    ing.finish(lib, dev)
    long_g = len(games) - 2
    assert len(games[long_g][1]) > 64
    G, cap = 4, 20
    ea, eb = make_engines(backend, G, 8, 8, cap)
    o = int(ing.tok_off[long_g])
    first = IntBuf(backend, np.array([o, o, ing.T - 3, o], np.int64))
    ply = IntBuf(backend, np.array([5, cap, 10, cap - 1], np.int32))      # fine | ply + 1 > max_plies | leaves the array | the last ply that fits
    slots = IntBuf(backend, np.arange(G, dtype=np.int32))
    eb.reset_dev(G, slots.ptr, ing.pos.data_ptr(), ing.T, first.ptr, ply.ptr)
    st = eb.status_bits()
    assert st.tolist() == [0, E.ST_PLY_OVERFLOW, 128, 0]
    nl, term, pl = eb.root_info()
    assert term[1] == -1 and term[2] == -1 and pl.tolist() == [5, 0, 0, cap - 1]
    mv = games[long_g][1]
    ea.reset([0], [None], [" ".join(mv[:5])])
    assert slot_state(ea, 0) == slot_state(eb, 0)
    nn = H.Buf(backend, (G, 120, 8, 8))
    want = IntBuf(backend, np.ones(G, np.int32))
    eb.search_begin_dev(want.ptr, nn.ptr)
    eb.step(0, 0, E.POLICY_NONE, nn.ptr)
    running, _, mask = eb.poll()
    assert mask.tolist() == [1, 0, 0, 1]                                     # the refused slots are not searched
    rec = analysis_records(backend, eb, [-1] * G)
    assert rec["terminal"].tolist()[1:3] == [-1, -1] and rec["status"].tolist() == [0, E.ST_PLY_OVERFLOW, 128, 0] and rec["phase"].tolist() == [1, 0, 0, 1]
    # what the host can know it refuses itself
    bad = lambda rc: rc == -1 and lib.bo_last_error()
    assert bad(lib.bo_games_reset_dev(eb.h, G + 1, slots.ptr, ing.pos.data_ptr(), ing.T, first.ptr, ply.ptr, 0))
    assert bad(lib.bo_games_reset_dev(eb.h, G, slots.ptr, ing.pos.data_ptr(), 0, first.ptr, ply.ptr, 0))
    assert bad(lib.bo_games_reset_dev(eb.h, G, None, ing.pos.data_ptr(), ing.T, first.ptr, ply.ptr, 0))
    return True
