"""tests/uci_cases.py -- backend-independent bodies of the tests of the interactive front end on the FAST search mode (emu on CPU, hip
on GPU): bo_search_info against a host walk over Engine.debug_tree, bo_search_stop on fast-mode engines against tests/fast_reference.py,
and the UCI protocol of betaone_amd/uci.py in-process.

A stopped fast search is compared with the restatement run for num_simulations = sims_done: the step in flight leaves nothing in the
tree (csrc/bo_info.h).  Every comparison of trees and records is bit for bit."""
from __future__ import annotations

import functools

import numpy as np

import test_fast_mode_emu as FM
from betaone_amd import engine as E
from engine_harness import Buf, emu_call
from fake_model import family_eval
from fast_reference import canonical_from_engine
from oracle import oracle as O

START = O.STARTING_FEN
KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
KRK_MATES = "k7/8/1K6/8/8/8/8/7R w - - 0 1"
MATED = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"  # fool's mate: white is mated
SALT = 7


def logits_eval(salt=SALT, scale=6.0):
    """planes -> (fake_model.fake_logits_values' logits as float32 softmax probabilities, values)"""
    return FM.softmax_eval(salt, scale)


class IBuf:
    """int32 [G, INFO_WORDS] device buffer with a raw address; records() -> the G records as E.INFO_DTYPE."""

    def __init__(self, backend, G):
        self.backend, self.G = backend, G
        if backend == "emu":
            self.a = np.full((G, E.INFO_WORDS), -7, dtype=np.int32)
            self.ptr = self.a.ctypes.data
        else:
            import torch

            self.t = torch.full((G, E.INFO_WORDS), -7, dtype=torch.int32, device="cuda:0")
            self.ptr = self.t.data_ptr()

    def records(self):
        if self.backend == "emu":
            a = self.a.copy()
        else:
            import torch

            torch.cuda.synchronize()
            a = self.t.cpu().numpy()
        return a.view(E.INFO_DTYPE).reshape(self.G)


def make_engine(backend, G, sims, L, opts=None, arena=0):
    kw = dict(num_simulations=sims, dirichlet_alpha=0.0, fast=True, leaves_per_step=L, max_plies=256, fast_arena_granules=arena)
    eng = emu_call(E.Engine, G, **kw) if backend == "emu" else E.Engine(G, **kw)
    if opts:
        eng.fast_options(**opts)
    return eng


def drive(backend, eng, G, L, eval_fn, after_step=None, max_steps=None, go=None, bufs=None):
    """search_begin + steps with an external evaluator.  after_step(k) runs behind the k-th step; it may return True to leave the loop
    (the search is then still running).  -> (steps made, buffers)"""
    nn_in, pol, val = bufs or (Buf(backend, (G * L, 120, 8, 8)), Buf(backend, (G * L, E.NUM_ACTIONS)), Buf(backend, (G * L,)))
    eng.search_begin(go or [1] * G, None, nn_in.ptr)
    kind, steps = E.POLICY_NONE, 0
    while True:
        eng.step(pol.ptr, val.ptr, kind, nn_in.ptr)
        steps += 1
        if after_step is not None and after_step(steps):
            break
        running, _, _ = eng.poll()
        if not running or (max_steps is not None and steps >= max_steps):
            break
        p, v = eval_fn(nn_in.numpy())
        pol.set(p); val.set(v)
        kind = E.POLICY_PROBS
        assert steps < 10000
    return steps, (nn_in, pol, val)


# ---- 1. bo_search_info against a host walk --------------------------------------------------------------------------------------
def info_walk(nodes, n_lines):
    """The rule of include/betaone_engine.h (bo_search_info_rec) restated over Engine.debug_tree's nodes (fast mode: breadth-first,
    children in record order, padding left out): -> (lines [(move, visits, w bits, prior bits, pv)], a tie among the root's visited children)"""
    root = nodes[0]
    if root["terminal"] != 0:
        return [], False
    kids = list(range(root["first_child"], root["first_child"] + root["n_children"]))
    visited = [i for i in kids if nodes[i]["n"] > 0]
    order = sorted(visited, key=lambda i: (-nodes[i]["n"], i))[:min(n_lines, E.INFO_LINES)]
    tie = len({nodes[i]["n"] for i in visited}) < len(visited)
    lines = []
    for i in order:
        pv, node = [nodes[i]["move"]], i
        while len(pv) < E.INFO_PV:
            nd = nodes[node]
            if nd["terminal"] != 0 or nd["n_children"] == 0:
                break
            ch = list(range(nd["first_child"], nd["first_child"] + nd["n_children"]))
            best = min(ch, key=lambda c: (-nodes[c]["n"], c))
            if nodes[best]["n"] <= 0:
                break
            node = best
            pv.append(nodes[node]["move"])
        nd = nodes[i]
        lines.append((nd["move"], nd["n"], int(np.float32(nd["q"]).view(np.uint32)), int(np.float32(nd["prior"]).view(np.uint32)), pv))
    return lines, tie


def check_info_record(eng, ibuf, g, what):
    """bo_search_info of slot g for 1, 3 and 8 lines, field for field against the walk and the engine's own state; -> the 8-line walk"""
    nodes = eng.debug_tree(g)
    st = eng.status_bits()
    nl, term, _ = eng.root_info()
    dbg, _paths = eng.debug_fast(g)
    out = None
    for n in (1, 3, 8):
        eng.search_info(n, ibuf.ptr)
        r = ibuf.records()[g]
        lines, tie = info_walk(nodes, n) if term[g] == 0 else ([], False)
        assert int(r["status"]) == int(st[g]) and int(r["terminal"]) == int(term[g]) and int(r["n_legal"]) == int(nl[g]), (what, n)
        assert int(r["root_visits"]) == nodes[0]["n"] and int(r["arena_top"]) == dbg["top"], (what, n)
        assert int(r["arena_granules"]) > 0 and int(r["watch"]) == 0 and not r["reserved"].any(), (what, n)
        assert int(r["n_lines"]) == len(lines), (what, n, int(r["n_lines"]), len(lines))
        for i in range(E.INFO_LINES):
            ln = r["line"][i]
            if i < len(lines):
                mv, vis, wb, pb, pv = lines[i]
                got = (int(ln["move"]), int(ln["visits"]), int(ln["w"].view(np.uint32)), int(ln["prior"].view(np.uint32)), int(ln["pv_len"]))
                assert got == (mv, vis, wb, pb, len(pv)), (what, n, i, got, lines[i])
                assert ln["pv"][:len(pv)].tolist() == pv and int(ln["pv"][0]) == mv and not ln["pv"][len(pv):].any(), (what, n, i)
                assert not ln["reserved"].any()
            else:
                assert not np.frombuffer(ln.tobytes(), np.int32).any(), (what, n, i)  # words beyond n_lines are 0
        out = (lines, tie, r.copy())
    return out


INFO_CASES = list(FM.CASES)
INFO_IDS = ["start-64-L8", "ruy-150-L16", "krk-mates-120-L8", "repetitions-100-L4", "fifty-60-L8", "wide218-48-L8"]


def check_info_after_search(backend, fen, moves, sims, L, every_step=False):
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [fen], [" ".join(moves) or None])
    ibuf = IBuf(backend, 1)

    def hook(k):
        check_info_record(eng, ibuf, 0, ("step", k))
        return False

    drive(backend, eng, 1, L, logits_eval(), after_step=hook if every_step else None)
    eng.check_status()
    lines, _tie, r = check_info_record(eng, ibuf, 0, "end")
    res = eng.result()
    assert int(r["phase"]) == E.PH_DONE and int(r["sims_done"]) == sims
    assert len(lines) >= 1 and lines[0][0] == int(res["best_move"][0])  # line[0].move is bo_search_result's best move
    assert sum(1 for nd in eng.debug_tree(0)[1:1 + eng.debug_tree(0)[0]["n_children"]] if nd["n"] > 0) >= len(lines)
    eng.close()


def check_info_edge_roots(backend):
    """A mated root, a root that is not expanded yet (before any search, and while its own evaluation is outstanding), a root with fewer
    visited children than the lines asked for."""
    L = 4
    eng = make_engine(backend, 3, 5, L)
    eng.reset([0, 1, 2], [MATED, START, START], [None, None, None])
    ibuf = IBuf(backend, 3)
    eng.search_info(8, ibuf.ptr)
    r = ibuf.records()
    assert r["phase"].tolist() == [E.PH_IDLE] * 3 and r["n_lines"].tolist() == [0, 0, 0] and r["terminal"].tolist() == [1, 0, 0]
    assert r["n_legal"].tolist() == [0, 20, 20] and r["sims_done"].tolist() == [0, 0, 0] and r["root_visits"].tolist() == [0, 0, 0]

    def hook(k):
        if k == 1:  # the roots' own rows are outstanding: nothing is expanded
            eng.search_info(8, ibuf.ptr)
            q = ibuf.records()
            assert q["phase"].tolist() == [E.PH_DONE, E.PH_RUN, E.PH_RUN] and q["n_lines"].tolist() == [0, 0, 0]
        for g in range(3):
            check_info_record(eng, ibuf, g, ("edge", k, g))
        return False

    drive(backend, eng, 3, L, logits_eval(), after_step=hook)
    for g in range(3):
        lines, _tie, r = check_info_record(eng, ibuf, g, ("edge end", g))
        assert len(lines) == (0 if g == 0 else int(r["n_lines"]))
    lines, _tie, r = check_info_record(eng, ibuf, 1, "few")
    assert 1 <= int(r["n_lines"]) <= 5 < E.INFO_LINES  # five simulations: fewer visited children than the eight lines asked for
    eng.close()


def check_info_deep_line(backend):
    """A peaked evaluator with values of 0 runs down one line: the main variation is deeper than BO_INFO_PV and is cut there."""
    sims, L = 140, 4
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [KIWIPETE], [None])
    drive(backend, eng, 1, L, family_eval("peak", 31, value="v_zero", peak_scale=800.0))
    ibuf = IBuf(backend, 1)
    lines, _tie, r = check_info_record(eng, ibuf, 0, "deep")
    nodes = eng.debug_tree(0)
    depth, node = 0, 0
    while nodes[node]["n_children"] and nodes[node]["terminal"] == 0:  # the most-visited line's real length
        ch = range(nodes[node]["first_child"], nodes[node]["first_child"] + nodes[node]["n_children"])
        node = min(ch, key=lambda c: (-nodes[c]["n"], c))
        if nodes[node]["n"] <= 0:
            break
        depth += 1
    assert depth > E.INFO_PV, depth  # (the case's precondition)
    assert int(r["line"][0]["pv_len"]) == E.INFO_PV == len(lines[0][4])
    eng.close()


def check_info_tied_counts(backend):
    """Uniform priors (no legal move holds mass): root children with equal visit counts; the earlier one in legal-move order comes first."""
    sims, L = 12, 4
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [START], [None])
    drive(backend, eng, 1, L, family_eval("illegal_mass", 31))
    ibuf = IBuf(backend, 1)
    lines, tie, r = check_info_record(eng, ibuf, 0, "ties")
    assert tie and int(r["n_lines"]) == E.INFO_LINES
    vis = [ln[1] for ln in lines]
    assert vis == sorted(vis, reverse=True) and len(set(vis)) < len(vis)
    assert lines[0][0] == int(eng.result()["best_move"][0])
    eng.close()


def check_info_refuses_reference_engines(backend):
    import pytest

    kw = dict(num_simulations=16, mcts_batch_size=8)
    eng = emu_call(E.Engine, 1, **kw) if backend == "emu" else E.Engine(1, **kw)
    eng.reset([0])
    ibuf = IBuf(backend, 1)
    with pytest.raises(E.EngineError, match="fast-mode engines only"):
        eng.search_info(1, ibuf.ptr)
    eng.close()


# ---- 2. bo_search_info is read-only ----------------------------------------------------------------------------------------------
def _result_block(eng):
    res = eng.result()
    return {k: v.tobytes() for k, v in res.items()}


def check_info_is_read_only(backend):
    fen, moves, sims, L = FM.CASES[1]
    out = []
    for look in (False, True):
        eng = make_engine(backend, 1, sims, L)
        eng.reset([0], [fen], [" ".join(moves)])
        ibuf = IBuf(backend, 1)

        def hook(_k):
            for n in (1, 8):
                eng.search_info(n, ibuf.ptr)
            return False

        steps, _ = drive(backend, eng, 1, L, logits_eval(), after_step=hook if look else None)
        out.append((steps, canonical_from_engine(eng.debug_tree(0), E.move_to_uci), _result_block(eng), eng.debug_fast(0)[0]["top"],
                    {k: v.tolist() for k, v in eng.status().items()}))
        eng.close()
    assert out[0] == out[1]


# ---- 3. bo_search_stop on fast-mode engines ---------------------------------------------------------------------------------------
def _compare_with_reference(eng, g, ref, what):
    got, want = canonical_from_engine(eng.debug_tree(g), E.move_to_uci), ref.canonical()
    if got != want:
        diff = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
        raise AssertionError((what, len(diff), "paths differ; first:", diff[0], got.get(diff[0]), want.get(diff[0])))
    res = eng.result()
    visits = [v for _m, v in ref.visits()]
    n = int(res["n"][g])
    assert int(res["total"][g]) == sum(visits), what
    if sum(visits) > 0:
        assert n == sum(v > 0 for v in visits), what
        assert E.move_to_uci(int(res["best_move"][g])) == ref.visits()[int(np.argmax(visits))][0], what
    else:  # no visit yet: pi is uniform over the legal moves, the best move is the first
        assert n == len(visits) and E.move_to_uci(int(res["best_move"][g])) == ref.visits()[0][0], what
    assert abs(float(res["val"][g, :n].sum()) - 1.0) < 1e-6, what


STOP_CASES = [(START, (), 96, 8, 2), (START, (), 96, 8, 3), (START, (), 96, 8, 6), (START, ("e2e4", "e7e5"), 120, 16, 4),
              (START, ("d2d4",), 64, 4, 9)]
STOP_IDS = [f"L{L}-k{k}" for _f, _m, _s, L, k in STOP_CASES]


def check_stop_after_k_steps(backend, fen, moves, sims, L, k):
    """Stop behind the k-th step (k >= 2: the root is expanded): sims_done is a whole number of steps, tree and result are the
    restatement's for sims = sims_done; a second search on the slot continues in that tree; stopping it again changes nothing."""
    fn = logits_eval()
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [fen], [" ".join(moves) or None])
    _, bufs = drive(backend, eng, 1, L, fn, max_steps=k)
    assert eng.poll()[0] == 1  # (still running: the stop is the one under test)
    inflight, _ = eng.debug_fast(0)
    assert inflight["n_rows"] > 0 and inflight["n_step"] > 0
    done = eng.search_stop()
    assert int(done[0]) == (k - 2) * L and int(done[0]) % L == 0
    assert eng.poll()[0] == 0
    dbg, _ = eng.debug_fast(0)
    assert dbg["n_rows"] == 0 and dbg["n_step"] == 0 and dbg["top"] == inflight["top"]
    eng.check_status()
    ref = FM.reference_for(fen, list(moves), fn, int(done[0]), L, use_noise=False)
    ref.search(None)
    _compare_with_reference(eng, 0, ref, "stopped")
    before = (canonical_from_engine(eng.debug_tree(0), E.move_to_uci), _result_block(eng))
    assert eng.search_stop().tolist() == [int(done[0])]  # a finished slot: untouched
    assert (canonical_from_engine(eng.debug_tree(0), E.move_to_uci), _result_block(eng)) == before
    # the next search on the slot continues: the restatement's search() called twice
    drive(backend, eng, 1, L, fn, bufs=bufs)
    eng.check_status()
    ref.sims = sims
    ref.search(None)
    _compare_with_reference(eng, 0, ref, "continued")
    eng.close()


def check_stop_before_the_root_is_expanded(backend):
    """k = 1: only the root's own row is outstanding.  It is dropped like any other row: the root stays unexpanded, no simulation is
    counted, pi is uniform -- and the next search starts like a fresh one."""
    fn, sims, L = logits_eval(), 48, 8
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [START], [None])
    _, bufs = drive(backend, eng, 1, L, fn, max_steps=1)
    inflight, _ = eng.debug_fast(0)
    assert inflight["n_rows"] == 1 and inflight["n_step"] == 0 and int(inflight["row_slot"][0]) == 0
    assert eng.search_stop().tolist() == [0] and eng.poll()[0] == 0
    t = eng.debug_tree(0)
    assert len(t) == 1 and t[0]["n"] == 0 and t[0]["terminal"] == -1
    res = eng.result()
    assert int(res["n"][0]) == 20 and int(res["total"][0]) == 0
    legal = [O.move_to_uci(m) for m in O.Board(START).legal_moves()]
    assert E.move_to_uci(int(res["best_move"][0])) == legal[0]
    drive(backend, eng, 1, L, fn, bufs=bufs)
    ref = FM.reference_for(START, [], fn, sims, L, use_noise=False)
    ref.search(None)
    _compare_with_reference(eng, 0, ref, "after a stop at k = 1")
    eng.close()


def check_stop_with_shared_rows_and_known_terminals_in_flight(backend):
    """King and rook against king: the search is stopped behind the first step whose simulations in flight share a row AND include a hit
    on a known mate or draw (found on the control block, bo_debug_fast)."""
    fn, sims, L = family_eval("peak", 7, peak_scale=30.0), 150, 8  # (a peaked policy: descents of one step end in the same leaf)
    eng = make_engine(backend, 1, sims, L)
    eng.reset([0], [KRK_MATES], [None])
    seen = {}

    def hook(k):
        d, _ = eng.debug_fast(0)
        rows = d["sim_row"][:d["n_step"]]
        live = rows[rows >= 0]
        if (rows < 0).any() and len(set(live.tolist())) < len(live) and eng.poll()[0] == 1:
            seen.update(k=k, n_step=d["n_step"], n_rows=d["n_rows"])
            return True
        return False

    drive(backend, eng, 1, L, fn, after_step=hook)
    assert seen, "no step with shared rows and known-terminal simulations in flight: the case lost its point"
    done = eng.search_stop()
    assert int(done[0]) % L == 0 and 0 < int(done[0]) < sims
    eng.check_status()
    ref = FM.reference_for(KRK_MATES, [], fn, int(done[0]), L, use_noise=False)
    ref.search(None)
    _compare_with_reference(eng, 0, ref, seen)
    assert int(eng.status()["term_sims"][0]) == ref.n_term_sims
    eng.close()


def check_stop_idle_and_masked_slots(backend):
    """G = 3: slot 1 is stopped behind the third step, slot 2 is idle (not begun); slot 0 runs on to the tree it builds without any
    stop, slot 2 stays idle."""
    fn, sims, L, G = logits_eval(), 72, 8, 3
    fens, mvs = [START, KIWIPETE, START], [None, None, "e2e4"]
    trees = []
    for with_stop in (False, True):
        eng = make_engine(backend, G, sims, L)
        eng.reset([0, 1, 2], fens, mvs)
        stopped = {}

        def hook(k):
            if with_stop and k == 3:
                stopped["done"] = eng.search_stop([0, 1, 1])
            return False

        drive(backend, eng, G, L, fn, after_step=hook, go=[1, 1, 0])
        eng.check_status()
        ibuf = IBuf(backend, G)
        eng.search_info(3, ibuf.ptr)
        r = ibuf.records()
        assert r["phase"].tolist() == [E.PH_DONE, E.PH_DONE, E.PH_IDLE]
        trees.append([canonical_from_engine(eng.debug_tree(g), E.move_to_uci) for g in range(G)])
        if with_stop:
            assert stopped["done"].tolist() == [L, L, 0]  # (behind the third step every running search has one step backed up)
            assert r["sims_done"].tolist() == [sims, L, 0]
            ref = FM.reference_for(KIWIPETE, [], fn, L, L, use_noise=False)
            ref.search(None)
            _compare_with_reference(eng, 1, ref, "masked stop")
        eng.close()
    assert trees[0][0] == trees[1][0] and trees[0][2] == trees[1][2] and len(trees[1][2]) == 1
    assert trees[0][1] != trees[1][1]


def check_reference_semantics_stop_unchanged(backend):
    """A reference-semantics engine interrupted between two steps still returns the oracle's result for NUM_SIMULATIONS = sims_done."""
    from engine_harness import make_engine as make_ref_engine

    fen, moves, batch = START, "e2e4 e7e5 g1f3 b8c6 f1b5".split(), 16
    cfg = dict(num_simulations=200, batch_size=batch)
    eng = make_ref_engine(backend, 1, cfg)
    eng.reset([0], [fen], [" ".join(moves)])
    fn = logits_eval(8)
    nl, _term, _ = eng.root_info()
    noise = np.zeros((1, E.MAX_LEGAL))
    noise[0, :nl[0]] = np.random.RandomState(3).dirichlet([0.1] * int(nl[0]))
    nn_in, pol, val = Buf(backend, (1, 120, 8, 8)), Buf(backend, (1, E.NUM_ACTIONS)), Buf(backend, (1,))
    eng.search_begin([1], noise, nn_in.ptr)
    kind = E.POLICY_NONE
    for _ in range(4):
        eng.step(pol.ptr, val.ptr, kind, nn_in.ptr)
        assert eng.poll()[0] == 1
        p, v = fn(nn_in.numpy())
        pol.set(p); val.set(v)
        kind = E.POLICY_PROBS
    done = int(eng.search_stop()[0])
    assert 0 < done < cfg["num_simulations"]
    eng.check_status()
    res = eng.result()
    b = O.Board(fen)
    trk = O.PyTracker(); trk.add_board(b)
    for u in moves:
        b.push(u); trk.add_board(b)
    pos = b.positions()
    r = O.run_mcts(b, pos[max(0, len(pos) - 8):-1], trk, fn, np.random.RandomState(3), O.default_config(num_simulations=done, batch_size=batch))
    pi = np.zeros(E.NUM_ACTIONS, np.float32)
    n = int(res["n"][0])
    pi[res["idx"][0, :n]] = res["val"][0, :n]
    assert E.move_to_uci(int(res["best_move"][0])) == O.move_to_uci(r["best"])
    assert np.array_equal(pi.view(np.uint32), r["pi"].view(np.uint32))
    eng.close()


# ---- 4. the protocol, in-process through UciEngine.handle ----------------------------------------------------------------------------
NET_SHAPE = dict(emu=(1, 0, 16), hip=(1, 1, 64))  # (residual blocks, SE blocks, filters)
UCI_OPTIONS = dict(emu=dict(Leaves=4, MaxNodes=4000), hip=dict(Leaves=8, MaxNodes=20000))


@functools.lru_cache(maxsize=None)
def make_net(backend):
    import torch

    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = NET_SHAPE[backend]
    try:
        torch.manual_seed(5)
        net = network.PolicyValueNet().eval()
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    return net.to("cuda:0") if backend == "hip" else net


class Session:
    """One UciEngine driven line by line; cmd() returns what it printed once the search thread has carried the lines out."""

    def __init__(self, backend, **options):
        from engine_harness import emulator_backend

        from betaone_amd.uci import UciEngine

        self.backend, self.lines = backend, []
        self.cm = emulator_backend() if backend == "emu" else None
        if self.cm:
            self.cm.__enter__()
        self.u = UciEngine(out=self.lines.append, model=make_net(backend), device="cuda:0", options=dict(UCI_OPTIONS[backend], **options))

    def cmd(self, *lines, wait=True):
        for ln in lines:
            self.u.handle(ln)
        if wait:
            self.u.wait()
        out, self.lines[:] = list(self.lines), []
        return out

    def close(self):
        self.u.close()
        if self.cm:
            self.cm.__exit__(None, None, None)


def _field(line, name):
    t = line.split()
    return t[t.index(name) + 1]


def _pv(line):
    t = line.split()
    return t[t.index("pv") + 1:]


def _stable(lines):
    """Output without what depends on the wall clock (`time` and `nps`)."""
    out = []
    for ln in lines:
        t = ln.split()
        for k in ("time", "nps"):
            if ln.startswith("info depth") and k in t:
                i = t.index(k)
                del t[i:i + 2]
        out.append(" ".join(t))
    return out


def _legal(fen, moves):
    b = O.Board(fen)
    for u in moves:
        b.push(u)
    return [O.move_to_uci(m) for m in b.legal_moves()]


def check_uci_handshake(backend):
    s = Session(backend)
    try:
        out = s.cmd("uci")
        assert out[0].startswith("id name ") and out[-1] == "uciok"
        names = [ln.split()[2] for ln in out if ln.startswith("option name ")]
        assert names == ["MultiPV", "Leaves", "MaxNodes", "MoveOverhead", "Model"] and not any("onder" in ln for ln in out)
        assert s.u.eng is None  # engine, net and tuning wait for isready
        assert s.cmd("isready") == ["readyok"] and s.u.eng is not None
        assert s.cmd("xyzzy", "") == []  # unknown input is ignored
    finally:
        s.close()


def _go_nodes(backend, n=64, **options):
    s = Session(backend, **options)
    try:
        return s.cmd("isready", "position startpos", f"go nodes {n}"), s.u.L
    finally:
        s.close()


def check_uci_go_nodes(backend):
    out, L = _go_nodes(backend)
    infos = [ln for ln in out if ln.startswith("info depth")]
    best = [ln for ln in out if ln.startswith("bestmove")]
    assert infos and len(best) == 1 and out[-1] == best[0]
    mv = best[0].split()[1]
    last = [ln for ln in infos if _field(ln, "multipv") == "1"][-1]
    assert _pv(last)[0] == mv and mv in _legal(START, [])
    assert int(_field(last, "depth")) == len(_pv(last)) >= 1
    nodes = int(_field(last, "nodes"))
    assert nodes >= 64 and nodes % L == 0 and nodes - 64 < L  # the first step boundary with sims_done >= 64
    assert 0 <= int(_field(last, "hashfull")) <= 1000 and abs(int(_field(last, "cp"))) <= 9999
    again, _ = _go_nodes(backend)
    assert _stable(again)[-2:] == _stable(out)[-2:] == _stable([last, best[0]])  # the same bestmove and the same final info line
    assert len({ln for ln in _stable(again) + _stable(out) if " nodes 64 " in ln}) == 1  # (lines in between come once a second)


def check_uci_multipv(backend):
    s = Session(backend)
    try:
        out = s.cmd("setoption name MultiPV value 3", "isready", "position startpos", "go nodes 64")
        last = [ln for ln in out if ln.startswith("info depth")][-3:]
        assert [_field(ln, "multipv") for ln in last] == ["1", "2", "3"]
        ibuf = IBuf(backend, 1)
        s.u.eng.search_info(3, ibuf.ptr)
        r = ibuf.records()[0]
        vis = [int(r["line"][i]["visits"]) for i in range(3)]
        assert int(r["n_lines"]) == 3 and vis == sorted(vis, reverse=True) and vis[2] > 0
        assert [_pv(ln)[0] for ln in last] == [E.move_to_uci(int(r["line"][i]["move"])) for i in range(3)]
        assert out[-1] == "bestmove " + _pv(last[0])[0]
    finally:
        s.close()


def check_uci_infinite_and_stop(backend):
    """`go infinite` answers only behind `stop`, exactly once -- also when MaxNodes ended the search long before."""
    s = Session(backend, MaxNodes=48)
    try:
        s.cmd("isready", "position startpos")
        s.cmd("go infinite", wait=False)
        assert s.u.parked.wait(timeout=120)  # the search reached MaxNodes and waits for `stop`
        assert not any(ln.startswith("bestmove") for ln in s.lines)
        s.u.handle("isready")
        assert s.lines[-1] == "readyok"  # answered at once during a search
        out = s.cmd("stop")
        assert sum(ln.startswith("bestmove") for ln in out) == 1 and s.u.last_search["stopped_by"] == "maxnodes"
        assert s.u.last_search["nodes"] == 48
        # and a search that `stop` itself ends
        s.u.handle("setoption name MaxNodes value 4000")
        s.cmd("go infinite", wait=False)
        out = s.cmd("stop")
        assert sum(ln.startswith("bestmove") for ln in out) == 1 and s.u.last_search["stopped_by"] in ("stop", "maxnodes")
        assert out[-1].split()[1] in _legal(START, [])
    finally:
        s.close()


def check_uci_tree_reuse(backend):
    s = Session(backend)
    try:
        out = s.cmd("isready", "position startpos moves e2e4", "go nodes 96")
        last = [ln for ln in out if ln.startswith("info depth")][-1]
        pv = _pv(last)
        assert len(pv) >= 2 and not any("tree reused" in ln for ln in out)
        moves = ["e2e4"] + pv[:2]
        out = s.cmd("position startpos moves " + " ".join(moves), "go nodes 32")
        assert any(ln.startswith("info string tree reused") for ln in out) and s.u.last_search["reused"] > 0
        assert out[-1].split()[1] in _legal(START, moves)
        # a second go on the unchanged position continues in the tree of the first
        before = s.u.last_search["root_visits"]
        s.cmd("go nodes 32")
        assert s.u.last_search["reused"] == before and s.u.last_search["root_visits"] > before
        # the slot's game stack, tracker and planes are those of a fresh reset with the same move list
        eng = s.u.eng
        fresh = make_engine(backend, 1, 64, s.u.L)
        fresh.reset([0], [START], [" ".join(moves)])
        got, want = [], []
        for e, dst in ((eng, got), (fresh, want)):
            pos, mv = e.export_game(0)
            n = len(mv)
            enc = Buf(backend, (n + 1, 120, 8, 8))
            e.encode_game(0, 0, n + 1, enc.ptr)  # every ply and the root, with the slot's tracker
            dst.extend([[bytes(pos[k]) for k in range(n + 1)], mv, enc.numpy().tobytes(), [a.tolist() for a in e.root_info()]])
        assert got == want and got[1] == [uci_parse(m) for m in moves]
        fresh.close()
        # ucinewgame drops the tree
        out = s.cmd("ucinewgame", "position startpos moves " + " ".join(moves), "go nodes 32")
        assert not any("tree reused" in ln for ln in out) and s.u.last_search["reused"] == 0
    finally:
        s.close()


def uci_parse(text):
    from betaone_amd.uci import parse_move

    return parse_move(text)


def check_uci_illegal_move_and_mated_root(backend):
    s = Session(backend)
    try:
        out = s.cmd("isready", "position startpos moves e2e4 e7e5 e1e3 g8f6", "go nodes 16")
        assert any(ln.startswith("info string illegal move e1e3") for ln in out)
        assert s.u.have == (START, ["e2e4", "e7e5"]) and out[-1].split()[1] in _legal(START, ["e2e4", "e7e5"])
        out = s.cmd("position startpos moves e2e4 zz", "go nodes 16")  # another game, an unparsable move
        assert any(ln.startswith("info string illegal move zz") for ln in out) and s.u.have == (START, ["e2e4"])
        out = s.cmd("position startpos moves f2f3 e7e5 g2g4 d8h4", "go movetime 1000")
        assert out[-1] == "bestmove 0000" and any(ln.startswith("info string the root is terminal: checkmate") for ln in out)
        out = s.cmd(f"position fen {MATED}", "go depth 3")
        assert out[-1] == "bestmove 0000" and any("go depth is not supported" in ln for ln in out)
    finally:
        s.close()


# ---- 5. the clock ---------------------------------------------------------------------------------------------------------------------
CLOCK_TABLE = [  # (go line, white to move, MoveOverhead, ms or None)
    ("movetime 1000", True, 0, 950.0),
    ("movetime 1000", False, 10, 940.0),
    ("wtime 60000 btime 30000 winc 1000 binc 2000", True, 0, 2900.0),
    ("wtime 60000 btime 30000 winc 1000 binc 2000", False, 0, 2800.0),
    ("wtime 60000 btime 30000 winc 1000 binc 2000 movestogo 20", False, 50, 2750.0),
    ("wtime 600 btime 600", True, 0, 100.0),          # the floor of 100 ms
    ("wtime 600 btime 600", True, 30, 70.0),
    ("btime 90000", True, 0, 5000.0),                  # no time for the side to move: 5 s
    ("", False, 10, 4990.0),
    ("depth 5", True, 0, 5000.0),
    ("infinite", True, 0, None),
    ("nodes 800", True, 0, None),
    ("nodes 800 movetime 200", True, 0, 190.0),
    ("movetime 2 ", True, 10, 1.0),                    # at least 1 ms is left
    ("movetime 3000 wtime 1000", True, 0, 2850.0),     # movetime first
]


def check_clock_table():
    from betaone_amd.uci import parse_go, time_limit_ms

    for line, white, overhead, want in CLOCK_TABLE:
        got = time_limit_ms(parse_go(line.split()), white, overhead)
        assert (got is None) == (want is None) and (want is None or abs(got - want) < 1e-9), (line, white, overhead, got, want)
    assert parse_go("searchmoves e2e4 d2d4 nodes 5 ponder".split()) == dict(searchmoves=True, nodes=5, ponder=True)
