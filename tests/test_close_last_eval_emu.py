"""CPU tests (wave emulator; Rollout's eager loop with close_last_eval set by hand, as captured graphs set it): a search's last leaf evaluation only adds the remaining visits along the requested leaf's path as far as pi,
the move and the records can tell, so Rollout._eval_and_step_n ends a search's expected iterations with bo_k_search_close (csrc/bo_tree.h)
in its place.  Closing on (the default) against BETAONE_CLOSE_LAST_EVAL=0: the same games -- moves, pi indices and bits, z, terminal
code -- with one evaluation less per searched ply; and at the Engine level the close against the real evaluation + step: the same visit
counts of the root's children, the same result, and every game the close may not touch bit-unchanged."""
import math

import numpy as np
import pytest

import engine_harness as H
from fake_model import FakeNet, fake_logits_values

# tests/test_baseline_configs_gpu.py LATE_GAME_FENS: terminal bursts, the MCTS_BATCH_SIZE-simulation yield, claimable draws, games that end
LATE_GAME_FENS = [
    "6k1/5ppp/8/8/8/8/5PPP/3R2K1 w - - 0 40",          # back-rank mate in one: terminal bursts from the first search on
    "7k/5Q2/5K2/8/8/8/8/8 w - - 10 70",                 # several mates in one side by side, stalemating moves among them
    "8/8/4k3/8/8/3K4/8/6R1 w - - 98 80",                # halfmove clock 98: claimable fifty-move draws in the tree
    "k7/8/1K6/8/8/8/8/7R w - - 96 60",                  # mate in one AND the 50-move claim close
    "8/5k2/8/8/8/2K5/8/4R3 b - - 90 75",                # black to move, long reversible chains (repetition claims)
    "r1bq1rk1/pp2bppp/2n1pn2/3p4/3P1B2/2PBPN2/PP1N1PPP/R2QK2R w KQ - 4 29",  # a middlegame that crosses the temperature threshold (fullmove 30) after three plies
]


def _play(monkeypatch, close, *, sims, batch, G=4, plies=8, fens=None, expected_evals=None, record_values=False, cohorts=1):
    """-> (games by id: (moves, [(pi indices, pi bits)], [z], terminal), NN forwards per play_ply call, close launches, root values)"""
    from betaone_amd.rollout import CohortRollout, Rollout

    monkeypatch.setenv("BETAONE_CLOSE_LAST_EVAL", "1" if close else "0")
    with H.emulator_backend():
        kw = dict(num_simulations=sims, mcts_batch_size=batch, device="cpu", use_graph=False, rng_mode="native", policy_kind="logits",
                  max_game_moves=300, record_values=record_values)
        ro = CohortRollout(FakeNet(), G, cohorts=cohorts, **kw) if cohorts > 1 else Rollout(FakeNet(), G, **kw)
        parts = ro.parts if cohorts > 1 else [ro]
        n_close = [0]
        for p in parts:
            # (without captured graphs a Rollout keeps the last evaluation by default: the eager loop closes where it is told to)
            assert p.close_allowed == (close and not record_values) and not p.close_last_eval
            p.close_last_eval = p.close_allowed
            if expected_evals is not None:
                p.expected_evals = expected_evals  # fewer iterations enqueued than a search needs: the close meets searches with batches to go

            def counted(stream=0, real=p.eng.search_close):
                n_close[0] += 1
                return real(stream)
            p.eng.search_close = counted
        ro.start_games(list(range(G)), list(range(G)), [900 + g for g in range(G)], fens=[fens[g % len(fens)] for g in range(G)] if fens else None)
        fins, per_ply = {}, []
        for _ in range(plies):
            f0 = ro.n_forward
            ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f))
            per_ply.append(ro.n_forward - f0)
        if cohorts > 1:
            ro.drain()
        for p in parts:
            p.eng.check_status()
            for g in range(p.G):
                if p.games[g] is not None:
                    f = p._finish(g, 0)
                    fins[f.game_id] = f
        ro.close()
    games = {gid: (list(f.moves), [(np.asarray(i).tolist(), np.asarray(v, np.float32).view(np.uint32).tolist()) for i, v in f.pis],
                   [f.z(i) for i in range(len(f.pis))], f.terminal) for gid, f in fins.items()}
    values = {gid: None if f.root_values is None else np.asarray(f.root_values, np.float32).view(np.uint32).tolist() for gid, f in fins.items()}
    return games, per_ply, n_close[0], values


@pytest.mark.parametrize("sims,batch", [(64, 16),   # whole batches only
                                        (40, 16),   # a last batch of 8
                                        (32, 16),   # the last batch exactly full: S - sims_done == B at the close
                                        (10, 16)])  # a single batch: one plain iteration behind the root's
def test_closing_plays_the_same_games_with_one_evaluation_less(monkeypatch, sims, batch):
    """Games from the start position: no terminal simulations within these plies, so every search takes exactly its expected
    iterations -- 1 + ceil(S / B) evaluations per ply without the close, ceil(S / B) with it."""
    a, fa, ca, _ = _play(monkeypatch, False, sims=sims, batch=batch)
    b, fb, cb, _ = _play(monkeypatch, True, sims=sims, batch=batch)
    assert len(a) == 4 and a == b
    assert all(len(m) == 8 and len(pis) == 8 for m, pis, _, _ in a.values())
    n = math.ceil(sims / batch)
    assert ca == 0
    # (the first call holds the root's evaluation too and enqueues the root evaluation of the second ply's searches; from then on every
    # call counts one search's worth: the next root's evaluation + the leaves')
    assert fa == [2 + n] + [1 + n] * 7
    if n >= 2:
        assert cb == 8 and [x - y for x, y in zip(fa, fb)] == [1] * 8
    else:  # one iteration per search: plain.  (Only the first call, whose iterations begin with the root's, has two and ends with the close.)
        assert cb == 1 and [x - y for x, y in zip(fa, fb)] == [1] + [0] * 7


def test_closing_from_late_positions_leaves_ineligible_games_to_the_redo(monkeypatch):
    """Mates in one, claimable draws and reversible chains: searches absorb runs of terminal simulations, yield after MCTS_BATCH_SIZE of them,
    finish early or late -- at the close some are done, some wait for their last evaluation, some are in the middle of a run (no leaf
    requested) or have batches to go.  The close takes the second kind only; the single iterations behind the turn finish the rest.
    A ply then costs one forward less; or, when a game the close had to leave needs k more iterations, one more: without the close the
    first of the k is the expected iterations' last one and k - 1 turns are made again, with it k are, and a turn made again enqueues
    the next roots' evaluation again (1 + 2 (k - 1) against 2 k forwards)."""
    kw = dict(sims=40, batch=16, G=6, plies=10, fens=LATE_GAME_FENS)
    a, fa, _, _ = _play(monkeypatch, False, **kw)
    b, fb, cb, _ = _play(monkeypatch, True, **kw)
    assert len(a) >= 6 and a == b
    assert any(t in (1, 2) for *_, t in a.values())  # games ended by rule inside the run
    print("forwards per ply, close off / on:", fa, fb)
    assert cb > 0 and all(abs(x - y) <= 1 for x, y in zip(fa, fb)) and sum(fb) < sum(fa)
    c, _, cc, _ = _play(monkeypatch, True, cohorts=2, **kw)  # (two cohorts of three games, each part closing for itself)
    d, _, _, _ = _play(monkeypatch, False, cohorts=2, **kw)
    assert c == d and cc > 0


def test_close_meets_searches_with_batches_to_go(monkeypatch):
    """expected_evals lowered to 3 (1 + ceil(64 / 16) = 5 are needed): the close comes up behind the first leaf evaluation, when every
    search has three batches to go -- it must leave them alone, and the turn's redo finishes them with real evaluations."""
    kw = dict(sims=64, batch=16, plies=6)
    a, fa, _, _ = _play(monkeypatch, False, **kw)
    b, fb, cb, _ = _play(monkeypatch, True, expected_evals=3, **kw)
    assert a == b and cb == 6
    assert all(y >= x for x, y in zip(fa, fb))  # nothing was eligible: every search was evaluated in full (and turns were made again)


def test_closing_is_off_when_root_values_are_recorded(monkeypatch):
    """v_i is the root's q after the LAST backup: with record_values the close is off whatever the switch says, and a Rollout that is
    told to close all the same is refused by the engine."""
    from betaone_amd import engine as E
    from betaone_amd.rollout import Rollout

    kw = dict(sims=40, batch=16, plies=6, record_values=True)
    a, fa, ca, va = _play(monkeypatch, False, **kw)
    b, fb, cb, vb = _play(monkeypatch, True, **kw)
    assert a == b and va == vb and all(v is not None and len(v) == 6 for v in va.values())
    assert ca == cb == 0 and fa == fb and fa[1:] == [1 + math.ceil(40 / 16)] * 5
    with H.emulator_backend():
        ro = Rollout(FakeNet(), 2, num_simulations=40, mcts_batch_size=16, device="cpu", use_graph=False, rng_mode="native", record_values=True)
        ro.close_last_eval = True
        ro.start_games([0, 1], [0, 1], [1, 2])
        with pytest.raises(E.EngineError, match="root values"):
            ro.play_ply()
        ro.close()


# ---- Engine level -------------------------------------------------------------------------------------------------------------------

def _engine_at_last_evaluation(S, B, fens):
    """An engine whose searches have been stepped (fake net keyed by planes, probabilities at the seam) until no game that is still
    running has more than one batch to go.  -> (engine, buffers, evaluate())"""
    from betaone_amd import engine as E

    G = len(fens)
    eng = E.Engine(G, num_simulations=S, mcts_batch_size=B, dirichlet_alpha=0.0, max_plies=256)
    eng.reset(list(range(G)), fens)
    nn_in, policy, value = H.Buf("emu", (G, 120, 8, 8)), H.Buf("emu", (G, E.NUM_ACTIONS)), H.Buf("emu", (G,))

    def evaluate():
        logits, v = fake_logits_values(nn_in.numpy())
        ex = np.exp(logits - logits.max(axis=1, keepdims=True))
        policy.set((ex / ex.sum(axis=1, keepdims=True)).astype(np.float32))
        value.set(v)

    eng.search_begin(np.ones(G, np.int32), None, nn_in.ptr)
    eng.step(policy.ptr, value.ptr, E.POLICY_NONE, nn_in.ptr)
    for _ in range(4 * (2 + S // B)):
        st = eng.debug_search_state()
        run = st["phase"] == E.PH_RUN
        if not (run & ((S - st["sims_done"] > B) | (st["req_node"] == 0))).any():
            break
        evaluate()
        eng.step(policy.ptr, value.ptr, E.POLICY_PROBS, nn_in.ptr)
    else:
        raise AssertionError("searches did not reach their last batch")
    return eng, (nn_in, policy, value), evaluate


def _run_to_end(eng, bufs, evaluate, S, B):
    from betaone_amd import engine as E

    for _ in range(4 * (2 + S // B)):
        if eng.poll()[0] == 0:
            break
        evaluate()
        eng.step(bufs[1].ptr, bufs[2].ptr, E.POLICY_PROBS, bufs[0].ptr)
    assert eng.poll()[0] == 0
    eng.check_status()


def _root_children(eng, g):
    nodes = eng.debug_tree(g)
    fc, nc = nodes[0]["first_child"], nodes[0]["n_children"]
    return [(nd["move"], nd["n"]) for nd in nodes[fc:fc + nc]]


@pytest.mark.parametrize("S,B", [(40, 16), (32, 16), (64, 16)])
def test_engine_close_counts_the_visits_of_the_last_evaluation(S, B):
    from betaone_amd import engine as E

    fens = [None, None] + LATE_GAME_FENS  # (slots 0 and 1: the same game twice -- the close must treat equal states equally)
    G = len(fens)
    with H.emulator_backend():
        real, bufs_r, eval_r = _engine_at_last_evaluation(S, B, fens)
        closed, bufs_c, eval_c = _engine_at_last_evaluation(S, B, fens)
        st0 = closed.debug_search_state()
        assert all((real.debug_search_state()[k] == st0[k]).all() for k in st0)
        eligible = (st0["phase"] == E.PH_RUN) & (st0["req_node"] > 0) & (st0["rows"] == 0) & (S - st0["sims_done"] <= B)
        assert eligible[:2].all() and (st0["sims_done"][:2] == B * ((S - 1) // B)).all()
        assert not eligible.all()  # late positions: done already, or in the middle of a run of terminal simulations
        before = [closed.debug_tree(g) for g in range(G)]

        closed.search_close()
        st1 = closed.debug_search_state()
        for g in range(G):
            after = closed.debug_tree(g)
            if eligible[g]:
                assert st1["phase"][g] == E.PH_DONE and st1["sims_done"][g] == S and st1["rows"][g] == 0 and st1["req_node"][g] == -1
                assert st1["n_nodes"][g] == st0["n_nodes"][g] and after[0]["n"] == before[g][0]["n"] + S - st0["sims_done"][g]
                assert [nd["q"].tobytes() for nd in after] == [nd["q"].tobytes() for nd in before[g]]  # no q moved
            else:  # bit-unchanged
                assert all(st1[k][g] == st0[k][g] for k in st0)
                assert after == before[g]

        # the same searches with the real evaluation + step; games neither path has finished yet are stepped on in both engines
        _run_to_end(real, bufs_r, eval_r, S, B)
        _run_to_end(closed, bufs_c, eval_c, S, B)
        ra, rb = real.result(), closed.result()
        for g in range(G):
            assert _root_children(real, g) == _root_children(closed, g), g
        for k in ra:
            assert ra[k].tobytes() == rb[k].tobytes(), k
        assert (real.debug_search_state()["sims_done"] == closed.debug_search_state()["sims_done"]).all()
        real.close()
        closed.close()


def test_engine_close_is_refused_where_its_result_would_be_read():
    from betaone_amd import engine as E

    with H.emulator_backend():
        eng = E.Engine(1, num_simulations=16, mcts_batch_size=8, max_plies=64)
        eng.root_values(True)
        with pytest.raises(E.EngineError, match="root values"):
            eng.search_close()
        eng.close()
        fast = E.Engine(1, num_simulations=16, mcts_batch_size=8, max_plies=64, fast=True, leaves_per_step=4)
        with pytest.raises(E.EngineError, match="reference-semantics"):
            fast.search_close()
        fast.close()
