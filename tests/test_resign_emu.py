"""CPU tests (wave emulator): resignation and per-ply root values.

The device-made turn (bo_k_turn_sample / bo_k_turn_play with flag bit 3) and the host-made turn (bo_search_root_value + the rule in
rollout.py) resign the same games at the same plies and report the same v_i bits; v_i is the root's q_value as the reference's
update_recursive leaves it (checked against the oracle's tree, terminal-simulation bursts included); resignation off plays the games
of a Rollout built without the new arguments; BOG2 records, z of a resigned game and the betaone_amd.resign report."""
import io
import json

import numpy as np
import pytest

import engine_cases as EC
import engine_harness as H
from fake_model import FakeNet
from oracle import oracle as O


def _play(device_turn, *, G=6, plies=40, sims=40, batch=16, temperature=(3, 1.0, 0.1), max_game_moves=30, cohorts=1, n_games=14,
          expected_evals=None, rng_mode="native", **rkw):
    from betaone_amd.rollout import CohortRollout, Rollout

    with H.emulator_backend():
        kw = dict(num_simulations=sims, mcts_batch_size=batch, device="cpu", use_graph=False, rng_mode=rng_mode, policy_kind="logits",
                  temperature=temperature, max_game_moves=max_game_moves, **rkw)
        ro = CohortRollout(FakeNet(), G, cohorts=cohorts, **kw) if cohorts > 1 else Rollout(FakeNet(), G, **kw)
        parts = ro.parts if cohorts > 1 else [ro]
        for p in parts:
            p.device_turn = device_turn
            if expected_evals is not None:
                p.expected_evals = expected_evals
        seeds = lambda gid: 700 + gid if rng_mode == "native" else np.random.RandomState(700 + gid)
        ro.start_games(list(range(G)), list(range(G)), [seeds(g) for g in range(G)])
        nxt, fins = [G], {}

        def refill(slot):
            if nxt[0] >= n_games:
                return None
            gid = nxt[0]
            nxt[0] += 1
            return gid, seeds(gid), None

        for _ in range(plies):
            ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f), refill=refill)
        if cohorts > 1:
            ro.drain()
        states = []
        if rng_mode == "native":
            for p in parts:
                for g in range(p.G):
                    st = p.eng.rng_get_state(g)
                    states.append(st[1][:8].tolist() + [int(st[2])])
        for p in parts:
            p.eng.check_status()
        ro.close()
    return fins, states


def _key(fins):
    out = {}
    for gid, f in fins.items():
        rv = None if f.root_values is None else np.asarray(f.root_values, np.float32).view(np.uint32).tolist()
        out[gid] = (list(f.moves), [(np.asarray(i).tolist(), np.asarray(v, np.float32).view(np.uint32).tolist()) for i, v in f.pis],
                    f.terminal, f.outcome, rv, f.resign_check)
    return out


def _first_firing(v, t, k):
    """NumPy restatement of the rule: the first ply i with v[j] < t for j = i, i - 2, ..., i - 2 (k - 1) (all >= 0), else None."""
    below = np.asarray(v, np.float32) < np.float32(t)
    for i in range(len(below)):
        js = [i - 2 * m for m in range(k)]
        if js[-1] >= 0 and all(below[j] for j in js):
            return i
    return None


RESIGN = dict(resign_threshold=-0.02, resign_check_fraction=0.25)


@pytest.mark.parametrize("k", [1, 2])
def test_device_turn_resigns_like_the_host_turn(k):
    a, sa = _play(False, resign_plies=k, **RESIGN)
    b, sb = _play(True, resign_plies=k, **RESIGN)
    assert _key(a) == _key(b) and sa == sb
    resigned = [f for f in a.values() if f.terminal == 3]
    assert len(a) >= 10 and resigned, "the case must make games resign"
    assert any(f.terminal == 0 for f in a.values())  # and some run into the move limit
    for f in a.values():
        assert f.root_values is not None and len(f.root_values) == len(f.moves) == len(f.pis)
        fire = _first_firing(f.root_values, RESIGN["resign_threshold"], k)
        if f.resign_check:
            assert f.terminal != 3
        elif f.terminal == 3:
            # ended before the search at ply len(moves), which fired: no earlier ply fires
            assert fire is None and f.outcome == 1.0
        else:
            assert fire is None, (f.game_id, fire)


def test_device_turn_resigns_like_the_host_turn_in_cohorts_and_with_redos():
    a, sa = _play(False, resign_plies=2, **RESIGN)
    b, sb = _play(True, resign_plies=2, expected_evals=2, **RESIGN)  # 1 + ceil(40 / 16) = 4 needed: turns come up early and are made again
    assert _key(a) == _key(b) and sa == sb
    c, _ = _play(True, resign_plies=2, cohorts=2, **RESIGN)
    assert _key(c) == _key(a)


def test_python_rng_mode_resigns_the_same_games():
    a, _ = _play(False, resign_plies=1, **RESIGN)
    p, _ = _play(False, resign_plies=1, rng_mode="python", **RESIGN)
    ka, kp = _key(a), _key(p)
    common = set(ka) & set(kp)  # (the two modes hand finished games over at different points of a ply)
    assert len(common) >= 10 and any(ka[g][2] == 3 for g in common)
    assert {g: ka[g] for g in common} == {g: kp[g] for g in common}


def test_resign_off_plays_the_games_of_a_plain_rollout():
    base, sb = _play(True)
    for kw in (dict(resign_threshold=None), dict(record_values=True)):
        for dt in (True, False):
            got, sg = _play(dt, **kw)
            kb, kg = _key(base), _key(got)
            assert {g: v[:4] for g, v in kb.items()} == {g: v[:4] for g, v in kg.items()} and sb == sg
            if kw.get("record_values"):
                assert all(v[4] is not None for v in kg.values())
            else:
                assert all(v[4] is None for v in kg.values())


def test_check_games_are_a_fixed_subset_of_ids():
    from betaone_amd.rollout import resign_check_game

    ids = [g for g in range(10000) if resign_check_game(g, 0.1)]
    assert 900 <= len(ids) <= 1100
    assert ids == [g for g in range(10000) if resign_check_game(g, 0.1)]
    assert not any(resign_check_game(g, 0.0) for g in range(1000)) and all(resign_check_game(g, 1.0) for g in range(1000))


def test_resign_parameters_are_refused_where_out_of_scope():
    from betaone_amd.rollout import Rollout

    with H.emulator_backend():
        with pytest.raises(ValueError, match="fast"):
            Rollout(FakeNet(), 2, num_simulations=16, mcts_batch_size=8, device="cpu", use_graph=False, fast=True, resign_threshold=-0.9)

        class Pair(FakeNet):
            is_pair = True

        with pytest.raises(ValueError, match="two-net"):
            Rollout(Pair(), 2, num_simulations=16, mcts_batch_size=8, device="cpu", use_graph=False, resign_threshold=-0.9)


@pytest.mark.parametrize("case", EC.LONG_TERMINAL_RUN_CASES[:3], ids=lambda c: c[0].split()[0][:12])
def test_root_value_is_the_oracle_root_q(case):
    """v_i = the root's q_value as update_recursive leaves it: the oracle's root q bit for bit, also when hundreds of simulations end in
    known terminal leaves (the step kernel's register-resident burst, which before kept the root's visit count only)."""
    import test_fast_mode_emu as T

    fen, moves, sims, batch = case
    cfg = dict(num_simulations=sims, batch_size=batch)
    eng = H.make_engine("emu", 1, cfg)
    with H.emulator_backend():
        eng.root_values(True)
        eng.reset([0], [fen], [" ".join(moves) or None])
        fn = T.softmax_eval(3, scale=4.0)
        H.Searcher("emu", eng).search([1], [fn], [np.random.RandomState(5)], 0.1)
        b = O.Board(fen)
        trk = O.PyTracker(); trk.add_board(b)
        pos = b.positions()
        r = O.run_mcts(b, pos[max(0, len(pos) - 8):-1], trk, fn, np.random.RandomState(5), O.default_config(**cfg))
        assert r["n_terminal_sims"] >= sims // 2
        q_oracle = np.float32(r["nodes"][0]["q"])
        q_tree = np.float32(eng.debug_tree(0)[0]["q"])
        v = eng.search_root_value()[0]
        assert q_oracle.view(np.uint32) == q_tree.view(np.uint32) == np.float32(v).view(np.uint32)
        eng.close()


def test_root_value_is_the_oracle_root_q_in_mid_game_searches():
    from fake_model import fake_logits_values

    def fn(planes):
        logits, v = fake_logits_values(planes, 6.0, 17)
        x = logits.astype(np.float64)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), v

    moves = "e2e4 e7e5 g1f3 b8c6 f1b5 a7a6".split()
    cfg = dict(num_simulations=120, batch_size=16)
    with H.emulator_backend():
        eng = H.make_engine("emu", 1, cfg)
        eng.root_values(True)
        eng.reset([0], [None], [" ".join(moves)])
        H.Searcher("emu", eng).search([1], [fn], [np.random.RandomState(3)], 0.1)
        b = O.Board(O.STARTING_FEN)
        trk = O.PyTracker(); trk.add_board(b)
        for u in moves:
            b.push(u); trk.add_board(b)
        pos = b.positions()
        r = O.run_mcts(b, pos[max(0, len(pos) - 8):-1], trk, fn, np.random.RandomState(3), O.default_config(**cfg))
        assert np.float32(r["nodes"][0]["q"]).view(np.uint32) == np.float32(eng.search_root_value()[0]).view(np.uint32)
        assert r["nodes"][0]["q"] != 0.0
        eng.close()


def _games_for_records():
    a, _ = _play(True, resign_plies=1, **RESIGN)
    return a


def test_bog2_round_trip_and_bog1_unchanged():
    from betaone_amd import records as R

    fins = _games_for_records()
    for f in fins.values():
        blob = R.pack_game(f)
        assert blob[:4] == b"BOG2"
        g = R.unpack_games(blob)[0]
        assert g["n_plies"] == len(f.moves) and g["terminal"] == f.terminal and g["outcome"] == f.outcome
        assert np.array_equal(g["root_values"].view(np.uint32), np.asarray(f.root_values, np.float32).view(np.uint32))
        assert g["resign"] is True and g["resign_check"] == f.resign_check
        assert R.scan_games(blob) == [(f.game_id, len(f.moves), 0, len(blob))]
        # the same game without values is BOG1, byte for byte as before
        f1 = type(f)(**{**f.__dict__, "root_values": None, "resign_check": False, "resign": False})
        b1 = R.pack_game(f1)
        assert b1[:4] == b"BOG1" and len(blob) == len(b1) + 4 + 4 * len(f.moves)
        g1 = R.unpack_games(b1)[0]
        assert g1["root_values"] is None and g1["moves"].tolist() == g["moves"].tolist()
    mixed = b"".join(R.pack_game(f) for f in fins.values()) + b1
    assert len(R.unpack_games(mixed)) == len(fins) + 1 and len(R.scan_games(mixed)) == len(fins) + 1


def test_z_of_a_resigned_game():
    """outcome 1.0, z by self_play.py:202 unchanged: +1 on the plies with white to move, -1 on the others (the reference's quirk kept)."""
    fins = _games_for_records()
    f = next(f for f in fins.values() if f.terminal == 3)
    assert f.outcome == 1.0
    for i in range(len(f.pis)):
        assert f.z(i) == (1.0 if f.positions[i].turn == 1 else -1.0)


def _game(gid, values, terminal, check, n=None):
    return dict(game_id=gid, n_plies=len(values) if n is None else n, terminal=terminal, outcome=1.0 if terminal in (1, 3) else 0.0,
                root_values=np.asarray(values, np.float32), resign=True, resign_check=check, positions=None)


def test_resign_report_on_hand_built_games():
    from betaone_amd import resign as RS

    games = [
        _game(0, [0.1, -0.2, 0.3, -0.95, 0.9, -0.97], 3, False),  # resigned after 6 plies (black's v at ply 5 would fire again)
        _game(1, [0.0, 0.0, -0.96, 0.5, 0.1, 0.2, 0.3], 2, True),  # check game: white's v fired at ply 2, the game was drawn -> false positive
        _game(2, [0.0, -0.5, 0.2, -0.99, 0.4], 1, True),           # check game: black fired at ply 3 and black ends mated (5 plies, white moved last)
        _game(3, [0.1, 0.1, 0.1, 0.1], 2, True),                   # check game: never fires
        _game(4, [0.2, 0.3, 0.4, 0.5], 1, False),                  # full game, mate
    ]
    rep = RS.report(games, threshold=-0.9, plies=1)
    assert rep["games"] == 5 and rep["resigned"] == 1 and rep["plies"] == 6 + 7 + 5 + 4 + 4
    assert rep["mean_plies_resigned"] == 6.0 and rep["mean_plies_full"] == (7 + 5 + 4 + 4) / 4
    assert rep["check_games"] == 3 and rep["check_fired"] == 2 and rep["false_positives"] == 1
    assert abs(rep["false_positive_rate"] - 1 / 3) < 1e-12
    rows = {r["threshold"]: r for r in rep["table"]}
    assert rows[-0.98]["false_positive_rate"] == 0.0                  # only game 2's -0.99 fires, and black was mated
    assert rows[-0.98]["plies_saved"] == 5 - 3                        # game 2 would have ended at ply 3
    assert rows[-0.9]["false_positives"] == 1
    assert rep["recommended_threshold"] == max(t for t, r in rows.items() if r["false_positive_rate"] < 0.05)
    buf = io.StringIO()
    RS.print_report(rep, buf)
    assert "false positives" in buf.getvalue()


def test_resign_report_cli_reads_every_rank(tmp_path):
    from betaone_amd import records as R
    from betaone_amd import resign as RS

    fins = list(_games_for_records().values())
    d = tmp_path / "iter_0"
    R.save_games(R.compact_path(str(tmp_path), 0, 0), fins[: len(fins) // 2])
    R.save_games(R.compact_path(str(tmp_path), 0, 1), fins[len(fins) // 2:])
    out = io.StringIO()
    rep = RS.main([str(d), "--threshold", str(RESIGN["resign_threshold"]), "--json"], out=out)
    assert rep["games"] == len(fins) and rep["resigned"] == sum(f.terminal == 3 for f in fins)
    assert json.loads(out.getvalue().strip().splitlines()[-1])["games"] == len(fins)


def check_pgn_eval_comments(games, text, sims):
    """Every move of a game with root values carries "{e/S 0.00s}" with e from v_i; resigned games the winner's result and a last
    "{White resigns}" / "{Black resigns}"; the comments parse back (PGN reader) to float32(-eval_to_value(e)), within 2e-3 of -v_i."""
    import re

    from betaone_amd import pgn as P
    from betaone_amd import pgn_write as W
    from pgn_reference import eval_target

    from types import SimpleNamespace

    games = [SimpleNamespace(moves=list(g["moves"]), root_values=g["root_values"], terminal=int(g["terminal"]), positions=g["positions"])
             if isinstance(g, dict) else g for g in games]
    bodies = re.split(r"\n\n(?=\[Event)", text.strip())
    assert len(bodies) == len(games)
    ex = P.parse_text(text).export()
    assert ex["status"].tolist() == [0] * len(games)
    n_checked = 0
    for k, g in enumerate(games):
        n = len(g.moves)
        body = bodies[k]
        coms = re.findall(r"\{([^}]*)\}", body)
        rv = np.asarray(g.root_values, np.float32)
        want = [W.eval_text(v, sims) for v in rv]
        if g.terminal == 3:
            side = "White" if g.positions[n].turn == 1 else "Black"
            assert coms == want + [f"{side} resigns"]
            assert f'[Result "{"0-1" if side == "White" else "1-0"}"]' in body and '[Termination "normal"]' in body
        else:
            assert coms == want
        a = int(ex["tok_off"][k])
        assert int(ex["tok_off"][k + 1]) - a == n
        for i in range(n):
            if g.terminal == 3 and i == n - 1:
                assert ex["has_eval"][a + i] == 0  # (its comments join to a text the pattern rejects: no sample from the last move)
                continue
            assert ex["has_eval"][a + i] == 1
            t = ex["target"][a + i]
            assert np.float32(t).view(np.uint32) == eval_target(want[i]).view(np.uint32)
            if abs(float(rv[i])) < 0.999:
                assert abs(float(t) + float(rv[i])) < 2e-3
                n_checked += 1
    return n_checked


def test_pgn_eval_comments_round_trip():
    from betaone_amd import pgn_write as W

    games = sorted(_games_for_records().values(), key=lambda f: f.game_id)
    f = io.StringIO()
    with H.emulator_backend():
        W.write_pgn(f, games, tags={"Event": "resign"}, device="cpu", sims=40)
        n = check_pgn_eval_comments(games, f.getvalue(), 40)
    assert n > 50
    # a game without root values is written as before (no comments)
    g0 = type(games[0])(**{**games[0].__dict__, "root_values": None, "terminal": 0, "resign": False})
    f2 = io.StringIO()
    with H.emulator_backend():
        W.write_pgn(f2, [g0], device="cpu")
    assert "{" not in f2.getvalue()


def test_eval_text_format():
    from betaone_amd import pgn_write as W

    assert W.eval_text(np.float32(0.0), 100) == "+0.00/100 0.00s"
    assert W.eval_text(np.float32(1.0), 7) == "+99.99/7 0.00s" and W.eval_text(np.float32(-1.0), 7) == "-99.99/7 0.00s"
    v = np.float32(-0.3)
    e = 2.0 * np.log((1.0 + float(v)) / (1.0 - float(v)))
    assert W.eval_text(v, 5) == f"{e:+.2f}/5 0.00s"
