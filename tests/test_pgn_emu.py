"""CPU tests (library host code + wave emulator) of PGN pretraining: the tokeniser and eval targets (csrc/bo_pgn.h) on a hand-written
fixture, SAN resolution by bo_k_pgn_replay, a round trip of random games whose samples must be bit-identical to a restatement of the
reference's PGNDataset.parse, the reference batch order, and `python -m betaone_amd.pretrain` end to end with a tiny net."""
import json
import os
import random

import numpy as np
import pytest
import torch

import engine_harness as H
import pgn_reference as RF
import pgn_util as U

from betaone_amd import pgn as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_tokeniser_and_evals_on_the_fixture():
    exp = json.load(open(os.path.join(GOLDEN, "g7_pgn_cases.json")))["games"]
    pg = P.parse_text(open(os.path.join(GOLDEN, "g7_pgn_cases.pgn"), "rb").read(), H.emu_lib())
    x = pg.export()
    assert pg.n_games == len(exp)
    for g, e in enumerate(exp):
        a, b = x["tok_off"][g], x["tok_off"][g + 1]
        assert P.STATUS_NAMES[x["status"][g]] == e["status"], g
        assert [P.token_str(t) for t in x["tokens"][a:b]] == e["tokens"], g
        assert sorted(int(i) for i in np.nonzero(x["has_eval"][a:b])[0]) == sorted(int(i) for i in e["evals"]), g
        for i, ev in e["evals"].items():
            assert "0x%08x" % int(_bits(x["target"][a + int(i)])) == ev["z_bits"], (g, i)
            assert "0x%08x" % int(_bits(RF.eval_target(ev["comment"]))) == ev["z_bits"]  # (the test-side restatement agrees)
    roots = x["roots"]
    assert roots[1].turn == 1 and roots[2].turn == 0 and roots[2].halfmove_clock == 3 and roots[2].fullmove_number == 40


def test_chunked_parsing_matches_one_pass():
    """The text cut anywhere: the games of the first piece are complete ones, the rest comes with the next piece."""
    lib = H.emu_lib()
    text = open(os.path.join(GOLDEN, "g7_pgn_cases.pgn"), "rb").read()
    whole = P.parse_text(text, lib).export()
    for cut in (1, 57, 200, 333, len(text) - 3):
        blocks, off, buf = [], 0, text[:cut]
        pg, used = P.parse_chunk(lib, buf, 0, False)
        blocks.append(pg.export())
        buf = buf[used:] + text[cut:]
        pg, used = P.parse_chunk(lib, buf, 0, True)
        assert used == len(buf)
        blocks.append(pg.export())
        assert np.concatenate([b["status"] for b in blocks]).tolist() == whole["status"].tolist(), cut
        assert np.concatenate([b["tokens"] for b in blocks]).tolist() == whole["tokens"].tolist(), cut
        assert np.concatenate([b["target"] for b in blocks]).view(np.uint32).tolist() == whole["target"].view(np.uint32).tolist()
    # max_tokens: blocks of whole games
    pg, used = P.parse_chunk(lib, text, 0, True, -1, 5)
    assert pg.n_games == 1 and pg.n_tokens == 7 and used < len(text)


def _moves(fen, games):
    """PGN of single-token games from fen -> per game (status, plies, action indices)."""
    text = "".join(f'[FEN "{fen}"]\n\n{san} *\n\n' for san in games)
    with H.emulator_backend():
        r = P.replay_games(P.parse_text(text), device="cpu")
    return [(P.STATUS_NAMES[r["status"][g]], int(r["n_plies"][g]), int(r["act"][r["tok_off"][g]])) for g in range(len(games))]


def _idx(uci):
    from betaone_amd import dropin

    dropin.install()
    import chess
    import utils

    return utils.move_to_index(chess.Move.from_uci(uci))


@pytest.mark.parametrize("fen,cases", [
    # three queens reach e1: file, rank and square disambiguation
    ("2k5/8/8/8/4Q2Q/K7/8/7Q w - - 0 1", [("Qee1", "e4e1"), ("Qh4e1", "h4e1"), ("Q1e1", "h1e1"), ("Qxe1", "ambiguous"), ("Qe1", "ambiguous"),
                                          ("Qhe1", "ambiguous"), ("Q4e1", "ambiguous"), ("Qh4-e1+", "h4e1"), ("Qa1e1", "illegal"),
                                          ("h4e1", "h4e1")]),
    # promotions with and without '=', underpromotions, captures; no promotion piece or a king: nothing matches
    ("1n2k3/P7/8/8/8/8/8/4K3 w - - 0 1", [("a8=Q", "a7a8q"), ("a8Q", "a7a8q"), ("a8=N", "a7a8n"), ("axb8=R", "a7b8r"), ("axb8b", "a7b8b"),
                                          ("a7b8=q+", "a7b8q"), ("a8", "illegal"), ("a8=K", "illegal"), ("a7a8", "illegal")]),
    ("4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 2", [("exd6", "e5d6"), ("ed6", "e5d6"), ("e5d6", "e5d6"), ("d6", "illegal")]),
    ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", [("O-O", "e1g1"), ("0-0", "e1g1"), ("O-O-O", "e1c1"), ("0-0-0+", "e1c1"), ("e1g1", "e1g1"),
                                              ("e1c1", "e1c1"), ("Kg1", "e1g1"), ("O-O#", "e1g1")]),
    ("r3k2r/8/8/8/8/8/8/R3K2R b KQkq - 0 1", [("O-O", "e8g8"), ("O-O-O", "e8c8"), ("0-0-0", "e8c8"), ("e8g8", "e8g8")]),
    ("r3k2r/8/8/8/8/8/8/R3K2R w - - 0 1", [("O-O", "illegal"), ("O-O-O", "illegal")]),
    ("r1bqkb1r/pppp1ppp/2n2n2/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - 4 4", [("Qxf7#", "h5f7"), ("Qxf7", "h5f7"), ("Bxf7+", "c4f7"),
                                                                           ("Nf3", "g1f3"), ("Nc3", "b1c3"), ("Ne2", "g1e2"), ("N1e2", "g1e2")]),
])
def test_san_resolution(fen, cases):
    got = _moves(fen, [s for s, _ in cases])
    for (san, want), (st, n, act) in zip(cases, got):
        if want in ("illegal", "ambiguous"):
            assert (st, n) == (want, 0), san
        else:
            assert (st, n, act) == ("ok", 1, _idx(want)), san


def test_bad_tokens_end_the_game_and_keep_earlier_samples():
    text = ("1. e4 {+0.1/1 0.1s} e5 {+0.2/1 0.1s} 2. Nf3 {+0.3/1 0.1s} Ke6 {+0.4/1 0.1s} 3. d4 *\n\n"
            '[FEN "4k3/8/8/8/8/8/8/1N2KN2 w - - 0 1"]\n\n1. Ke2 {+0.1/1 0.1s} Kd7 {+0.2/1 0.1s} 2. Nd2 {+0.3/1 0.1s} *\n\n'
            "1. e4 {+0.1/1 0.1s} e5 {+0.1/1 0.1s} 2. -- {+0.5/1 0.1s} 2... Nc6 *\n\n"
            '[Variant "Chess960"]\n\n1. e4 {+0.1/1 0.1s} e5 {+0.1/1 0.1s} *\n')
    with H.emulator_backend():
        r = P.replay_games(P.parse_text(text), device="cpu")
    assert [P.STATUS_NAMES[s] for s in r["status"]] == ["illegal", "ambiguous", "null_move", "variant"]
    assert r["n_plies"].tolist() == [3, 2, 2, 0]
    off = r["tok_off"]
    assert r["smp"][off[0]:off[0] + 3].tolist() == [1, 1, 0]   # ply 2's sample needed move 3 (Ke6) replayed
    assert r["smp"][off[1]:off[1] + 2].tolist() == [1, 0]
    assert r["smp"][off[2]:off[2] + 2].tolist() == [1, 0]
    assert _bits(r["z"][off[0]:off[0] + 2]).tolist() == _bits([RF.eval_target("+0.2/1 0.1s"), RF.eval_target("+0.3/1 0.1s")]).tolist()


# ---- round trip -------------------------------------------------------------------------------------------------------------------
FENS = [None, None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12", "4k3/8/8/8/8/8/8/4K2R b K - 7 33"]


def make_corpus(seed, n_games, max_plies=80):
    """(games [(fen, uci moves, comments)], PGN text) of random legal games: castling, promotions, en passant, FEN roots, and a
    shuffling game that repeats positions."""
    rng = random.Random(seed)
    games, text = [], []
    for i in range(n_games):
        fen = FENS[i % len(FENS)]
        mv, cm, sans, res = U.random_game(rng, fen=fen, max_plies=rng.randint(1, max_plies))
        games.append((fen, mv, cm))
        text.append(U.write_game(sans, cm, res, fen=fen, headers={"Event": f"g{i}"}))
    # knights out and back: position repeats; ply 4's live repetition count (1) differs from the end-of-game one (2)
    mv = ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "f3g1", "f6g8", "e2e4"]
    b = U.chess.Board()
    sans = []
    for u in mv:
        sans.append(U.san(b, U.chess.Move.from_uci(u)))
        b.push(U.chess.Move.from_uci(u))
    cm = ["+0.1/1 0.1s"] * len(mv)
    games.append((None, mv, cm))
    text.append(U.write_game(sans, cm, "*"))
    return games, "".join(text)


def expected_samples(games):
    return [s for g in games for s in RF.samples(*g)]


def check_batch(states, idx, val, z, exp):
    s, i, v, zz = (t.cpu().numpy() for t in (states, idx, val, z))
    assert s.shape[0] == len(exp)
    for b, (planes, a, t) in enumerate(exp):
        assert np.array_equal(_bits(s[b]), _bits(planes)), b
        assert int(i[b, 0]) == a and float(v[b, 0]) == 1.0, b
        assert int(_bits(zz[b, 0])) == int(_bits(t)), b


def test_round_trip_is_bit_identical_to_the_reference_parse(tmp_path):
    games, text = make_corpus(11, 200)
    (tmp_path / "c.pgn").write_text(text)
    with H.emulator_backend():
        pg = P.parse_text(text)
        r = P.replay_games(pg, device="cpu")
        assert set(r["status"].tolist()) == {0} and pg.n_games == len(games)
        # every move comes back
        for g, (fen, mv, _) in enumerate(games):
            a = r["tok_off"][g]
            assert int(r["n_plies"][g]) == len(mv)
            assert r["act"][a:a + len(mv)].tolist() == [_idx(u) for u in mv], g
        ing = P.PgnIngest([str(tmp_path)], device="cpu", window_plies=1 << 15, workers=1)
        refs = list(ing.sample_refs(1 << 30))
        assert len(refs) == 1
        exp = expected_samples(games)
        assert ing.counts["samples"] == len(exp) and ing.counts["ok"] == len(games)
        check_batch(*ing.batch(*refs[0]), exp)
    # the repeating game: the live tracker is what the reference encodes, and it is not the end-of-game one
    fen, mv, _ = games[-1]
    live = RF.samples(fen, mv, games[-1][2])[4][0]
    assert not np.array_equal(live, RF.end_of_game_planes(fen, mv, 4))


def test_reference_batch_order_over_uneven_files(tmp_path):
    """order="reference": DataLoader(PGNDataset(sorted paths), batch_size=B, num_workers=3) -- worker w reads files w, w+3, ...,
    batches of B per worker (the last partial one kept), round-robin over the workers that still have data."""
    W, B = 3, 16
    files = []
    for f, n in enumerate([3, 9, 1, 6, 2, 0, 4]):
        games, text = make_corpus(100 + f, n, max_plies=40) if n else ([], "")
        p = tmp_path / f"f{f:02d}.pgn"
        p.write_text(text)
        files.append((str(p), games))
    streams = [[s for p, g in files[w::W] for s in expected_samples(g)] for w in range(W)]
    batches = [[st[i:i + B] for i in range(0, len(st), B)] for st in streams]
    order, active = [], list(range(W))
    cur = [0] * W
    while active:
        for w in list(active):
            if cur[w] >= len(batches[w]):
                active.remove(w)
                continue
            order.append(batches[w][cur[w]])
            cur[w] += 1
    with H.emulator_backend():
        ing = P.PgnIngest([str(tmp_path)], device="cpu", window_plies=1 << 14, workers=W, block_tokens=300)
        got = list(ing.loader(B))
    assert len(got) == len(order)
    for (s, i, v, z), exp in zip(got, order):
        check_batch(s, i, v, z, exp)


def test_shuffle_order_draws_from_the_window(tmp_path):
    games, text = make_corpus(5, 30, max_plies=40)
    (tmp_path / "a.pgn").write_text(text)
    with H.emulator_backend():
        a = [np.stack(r) for r in P.PgnIngest([str(tmp_path)], device="cpu", window_plies=2048, order="shuffle", seed=3, block_tokens=256).sample_refs(32)]
        b = [np.stack(r) for r in P.PgnIngest([str(tmp_path)], device="cpu", window_plies=2048, order="shuffle", seed=3, block_tokens=256).sample_refs(32)]
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert sum(x.shape[1] for x in a) == len(expected_samples(games))


# ---- the command line ------------------------------------------------------------------------------------------------------------
def _tiny(monkeypatch):
    from betaone_amd import dropin

    dropin.install()
    import config

    monkeypatch.setattr(config, "RESIDUAL_BLOCKS", 1)
    monkeypatch.setattr(config, "SE_RESIDUAL_BLOCKS", 0)
    monkeypatch.setattr(config, "CONV_FILTERS", 16)
    return config


def test_pretrain_command_end_to_end(tmp_path, monkeypatch, capsys):
    from betaone_amd import pretrain

    config = _tiny(monkeypatch)
    monkeypatch.setattr(config, "MID_EPOCH_CHECKPOINT", 4)
    games, text = make_corpus(21, 12, max_plies=50)
    data = tmp_path / "pgn"
    data.mkdir()
    (data / "a.pgn").write_text(text)
    import gzip

    with gzip.open(data / "b.pgn.gz", "wt") as f:
        f.write(text)
    n = 2 * len(expected_samples(games))
    with H.emulator_backend():
        assert pretrain.main([str(data), "--count", "--batch", "8", "--device", "cpu"]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"samples": n, "steps": -(-n // 8)}
        save = tmp_path / "ck"
        out = tmp_path / "s.json"
        assert pretrain.main([str(data), "--save-dir", str(save), "--batch", "8", "--max-steps", "11", "--log-every", "5", "--workers", "2",
                              "--out", str(out), "--device", "cpu", "--no-amp"]) == 0
        s = json.load(open(out))
        assert s["steps"] == 11 and s["counts"]["ok"] >= 12 and [iv["steps"] for iv in s["intervals"]] == [5, 5, 1]
        assert s["checkpoint_writes_after_batch"] == [1, 5, 9]       # (i - 1) % 4 == 0
        assert os.path.exists(save / "pretrained.pth")
        # no mid-run write once best_model.pth exists
        torch.save({}, save / "best_model.pth")
        assert pretrain.main([str(data), "--save-dir", str(save), "--batch", "8", "--max-steps", "6", "--out", str(out), "--device", "cpu",
                              "--no-amp", "--init", str(save / "pretrained.pth")]) == 0
        assert json.load(open(out))["checkpoint_writes_after_batch"] == []


def test_pretrain_loss_falls_on_a_repeated_corpus(tmp_path, monkeypatch):
    from betaone_amd import pretrain

    _tiny(monkeypatch)
    games, text = make_corpus(31, 4, max_plies=30)
    for i in range(12):
        (tmp_path / f"r{i:02d}.pgn").write_text(text)
    out = tmp_path / "s.json"
    with H.emulator_backend():
        assert pretrain.main([str(tmp_path), "--save-dir", str(tmp_path / "ck"), "--batch", "16", "--log-every", "10", "--workers", "1",
                              "--t-max", "1000", "--out", str(out), "--device", "cpu", "--no-amp"]) == 0
    iv = json.load(open(out))["intervals"]
    assert len(iv) >= 3 and iv[-1]["loss"] < 0.8 * iv[0]["loss"]
