"""CPU tests (wave emulator) of the analysis path: game slots set up from positions that are already on the device
(bo_games_reset_dev, csrc/bo_analyse.h) against the same slots set up from FEN + UCI strings, the roots' planes against pretraining's,
the searches against the CPU oracle, the analysis record (bo_analysis_result) against a NumPy walk over the tree, the capacity checks,
and `python -m betaone_amd.analyse` end to end with a tiny net, closing the loop into `pretrain`."""
import json
import os
import re

import numpy as np
import pytest
import torch

import analyse_cases as AC
import engine_harness as H
import pgn_reference as RF

from betaone_amd import engine as E
from betaone_amd import pgn as P


def test_setup_from_the_device_equals_setup_from_strings_every_ply():
    """(a) + (b) + (c) + (d): every ply of every game of the corpus; played[] is recovered from consecutive positions and IS compared
    (bo_game_export's moves).  ~120 of the roots also go through the oracle."""
    games, text = AC.make_corpus()
    assert len(games) >= 45 and max(len(m) for _, m in games) > 64 and min(len(m) for _, m in games) == 0
    st = AC.check_setup_and_analysis("emu", games, text, G=64, sims=24, batch=8, oracle_every=15)
    assert st["compared"] == sum(len(m) for _, m in games)
    assert st["oracle"] >= 100, st
    assert st["code2"] >= 2, st      # the repetition game plays on past claimable draws: roots with code 2 in the middle of a game
    assert st["ties"] >= 1, st       # the tie rule of the principal variation was exercised


def test_capacity_and_ranges():
    assert AC.check_capacity("emu")


def test_entry_points_refuse_what_they_do_not_cover():
    with H.emulator_backend():
        fast = E.Engine(2, num_simulations=8, fast=True, leaves_per_step=4, max_plies=32)
        noisy = E.Engine(2, num_simulations=8, max_plies=32)
        plain = E.Engine(2, num_simulations=8, dirichlet_alpha=0.0, max_plies=32)
    a = np.zeros(64, np.int64)
    for call in (lambda: fast.reset_dev(1, a.ctypes.data, a.ctypes.data, 1, a.ctypes.data, a.ctypes.data),
                 lambda: fast.search_begin_dev(a.ctypes.data, a.ctypes.data), lambda: fast.analysis_result(0, a.ctypes.data),
                 lambda: noisy.search_begin_dev(a.ctypes.data, a.ctypes.data),   # Dirichlet noise cannot be handed in
                 lambda: plain.analysis_result(0, a.ctypes.data)):               # root values are off
        with pytest.raises(E.EngineError):
            call()


def test_spans_name_each_game_s_text():
    games, text = AC.make_corpus(seed=2, n_random=3, max_plies=20)
    lib = H.emu_lib()
    data = text.encode()
    pg = P.parse_text(data, lib)
    import ctypes as C

    b, e = np.zeros(pg.n_games, np.int64), np.zeros(pg.n_games, np.int64)
    assert lib.bo_pgn_spans(pg.h, b.ctypes.data_as(C.POINTER(C.c_int64)), e.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert pg.n_games == len(games) and b[0] == 0 and all(b[i + 1] >= e[i] for i in range(len(b) - 1)) and e[-1] <= len(data)
    from betaone_amd import analyse as A

    for g in range(pg.n_games):
        chunk = data[b[g]:e[g]]
        assert chunk.startswith(b"[Event ")
        tags = dict(A.game_tags(chunk))
        assert tags["Event"] == (f"random {g}" if g < 3 else tags["Event"])
        assert P.parse_text(chunk, lib).n_games == 1
    assert dict(A.game_tags(data[b[0]:e[0]]))["White"] == 'a "quoted" name'
    # '%' escape lines and ';' comments in front of a game are outside its span; between its tags they are skipped
    pre = b"% an escape line\n; a comment\n\n"
    pg2 = P.parse_text(pre + data, lib)
    b2, e2 = np.zeros(pg2.n_games, np.int64), np.zeros(pg2.n_games, np.int64)
    assert lib.bo_pgn_spans(pg2.h, b2.ctypes.data_as(C.POINTER(C.c_int64)), e2.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    assert (b2 - len(pre)).tolist() == b.tolist() and (e2 - len(pre)).tolist() == e.tolist()
    assert A.game_tags(b'; c\n[Event "x"]\n% esc\n[Site "y"]\n\n1. e4 *') == [("Event", "x"), ("Site", "y")]


def _tiny(monkeypatch):
    from betaone_amd import dropin

    dropin.install()
    import config

    monkeypatch.setattr(config, "RESIDUAL_BLOCKS", 1)
    monkeypatch.setattr(config, "SE_RESIDUAL_BLOCKS", 0)
    monkeypatch.setattr(config, "CONV_FILTERS", 16)
    import network

    torch.manual_seed(5)
    return config, network.PolicyValueNet().eval()


def check_command_outputs(lib, text, out_pgn, jsonl, report, sims, movegen):
    """(f): the annotated PGN against the input, the JSONL and the report."""
    src, ann = P.parse_text(text.encode(), lib).export(), P.parse_text(open(out_pgn, "rb").read(), lib).export()
    assert ann["status"].tolist() == src["status"].tolist() and ann["tok_off"].tolist() == src["tok_off"].tolist()
    assert ann["tokens"].tolist() == src["tokens"].tolist()                      # the same games, the same tokens
    lines = [json.loads(l) for l in open(jsonl)]
    rep = json.load(open(report))
    assert len(lines) == len(src["tokens"]) == rep["replayed_moves"]                # one line per replayed move
    assert rep["positions_analysed"] + rep["positions_not_searched"] == rep["replayed_moves"]
    searched = np.array([l["searched"] for l in lines], bool)
    assert rep["positions_analysed"] == int(searched.sum()) and (~searched).sum() >= 2
    assert all(l["terminal"] != 0 for l, s in zip(lines, searched) if not s) and all(l["terminal"] == 0 for l, s in zip(lines, searched) if s)
    assert ann["has_eval"].astype(bool).tolist() == searched.tolist()               # claim-draw and mate roots have no comment
    body = re.sub(r'\[[A-Za-z0-9_]+ "(?:[^"\\]|\\.)*"\]', "", open(out_pgn).read())
    comments = re.findall(r"\{([^}]*)\}", body)
    assert len(comments) == int(searched.sum()) and all(c.endswith(f"/{sims} 0.00s") for c in comments)
    want = np.array([RF.eval_target(c) for c in comments], np.float32)              # -value_of(e) for the e printed, DESIGN "Eval comments"
    assert np.array_equal(ann["target"][searched].view(np.uint32), want.view(np.uint32))
    for l in lines:                                                                 # the values behind the comments
        if l["searched"]:
            assert l["best"] == (l["pv"][0] if l["pv"] else l["best"]) and l["visits"] == sims
    out = open(out_pgn).read()
    for tag in ('[Event "repetition"]', '[Annotator "nobody"]', '[White "a \\"quoted\\" name"]', '[Result "0-1"]', '[Event "one position"]'):
        assert tag in out, tag
    assert out.index('[Event "random 0"]') < out.index('[Site "?"]') < out.index('[Annotator "nobody"]')   # Seven Tag Roster first
    legal = movegen(lines)
    for l, lg in zip(lines, legal):
        if l["searched"]:
            assert l["best"] in lg and l["played"] in lg
    return lines, rep


def test_the_command_end_to_end_and_into_pretrain(tmp_path, monkeypatch, capsys):
    from betaone_amd import analyse as A
    from betaone_amd import pretrain

    config, net = _tiny(monkeypatch)
    games, text = AC.make_corpus(seed=9, n_random=3, max_plies=14, long_plies=66)
    games, text = games[:-2] + games[-1:], None                                    # (the long game is left to the GPU test)
    import pgn_util as U

    text = "".join(U.write_game(AC._sans(f, m), [None] * len(m), "0-1" if m == AC.MATE else "*", fen=f,
                                headers={"Event": ev, **({"Result": "0-1"} if m == AC.MATE else {}),
                                         **({"White": 'a \\"quoted\\" name', "Annotator": "nobody"} if ev.startswith("random") else {})})
                   for (f, m), ev in zip(games, ["random 0", "random 1", "random 2", "repetition", "mate", "en passant", "one position"]))
    src = tmp_path / "in.pgn"
    src.write_text(text)
    ck = tmp_path / "net.pth"
    torch.save(net.state_dict(), ck)
    sims = 12
    monkeypatch.setattr(config, "MCTS_BATCH_SIZE", 8)
    outs = []
    with H.emulator_backend():
        for run in range(2):
            o, j, r = (tmp_path / f"{n}{run}" for n in ("out.pgn", "pos.jsonl", "report.json"))
            assert A.main([str(src), "--model", str(ck), "-o", str(o), "--sims", str(sims), "--slots", "16", "--jsonl", str(j), "--report", str(r),
                           "--device", "cpu"]) == 0
            outs.append((o, j, r))
        assert "[analyse] games 7" in capsys.readouterr().out
        assert open(outs[0][0], "rb").read() == open(outs[1][0], "rb").read() and open(outs[0][1], "rb").read() == open(outs[1][1], "rb").read()
        eng = E.Engine(1, num_simulations=1, max_plies=8)

        def movegen(lines):
            ing = A.Ingested(H.emu_lib(), torch.device("cpu"), "in", text.encode())
            ing.finish(H.emu_lib(), torch.device("cpu"))
            pos = A.ring_to_positions(ing.pos_host[:ing.n_roots])
            mv, _ = eng.movegen([pos[i] for i in range(ing.n_roots)])
            return [[E.move_to_uci(m) for m in row] for row in mv]

        lines, rep = check_command_outputs(H.emu_lib(), text, *outs[0], sims, movegen)
        assert rep["games_read"] == 7 and rep["games_skipped"] == 0
        # refusals
        with pytest.raises(ValueError):
            A.analyse_games(text, net, sims=sims, slots=16, device="cpu", fast=True)
        with pytest.raises(ValueError):
            A.analyse_games(text, net, sims=sims, slots=16, device="cpu", resign_threshold=-0.9)
        # the loop this closes: one pretraining step over the annotated file draws samples from it
        data = tmp_path / "pgn"
        data.mkdir()
        os.replace(outs[0][0], data / "annotated.pgn")
        assert pretrain.main([str(src), "--count", "--batch", "8", "--device", "cpu"]) == 0
        assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["samples"] == 0     # the plain corpus cannot be used at all
        assert pretrain.main([str(data), "--count", "--batch", "8", "--device", "cpu"]) == 0
        n = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["samples"]
        assert n > 0
        out = tmp_path / "s.json"
        assert pretrain.main([str(data), "--save-dir", str(tmp_path / "ck"), "--batch", "8", "--max-steps", "1", "--workers", "1", "--out", str(out),
                              "--device", "cpu", "--no-amp"]) == 0
        s = json.load(open(out))
        assert s["steps"] == 1 and s["counts"]["samples"] >= 8


def test_slot_reuse_small_batches_equal_one_batch(monkeypatch):
    """(g) on the emulator: the same roots in different slots and batch compositions give the same records."""
    from betaone_amd import analyse as A

    config, _ = _tiny(monkeypatch)
    monkeypatch.setattr(config, "MCTS_BATCH_SIZE", 8)

    class HashNet(torch.nn.Module):  # a stand-in net whose rows do not depend on the batch they are evaluated in (tests/fake_model.py)
        def forward(self, x):
            from fake_model import fake_logits_values

            logits, v = fake_logits_values(x.numpy(), 5.0, 11)
            return torch.from_numpy(logits), torch.from_numpy(v)

    net = HashNet()
    games, text = AC.make_corpus(seed=4, n_random=2, max_plies=10, long_plies=66)
    import pgn_util as U

    text = "".join(U.write_game(AC._sans(f, m), [None] * len(m), "*", fen=f) for f, m in games[:4])
    n_roots = sum(len(m) for _, m in games[:4])
    with H.emulator_backend():
        a = A.analyse_games(text, net, sims=10, slots=4, device="cpu")
        b = A.analyse_games(text, net, sims=10, slots=max(8, n_roots), device="cpu")
    assert a["report"]["batches"] > 3 and b["report"]["batches"] == 1
    for ga, gb in zip(a["games"], b["games"]):
        assert ga["plies"].tobytes() == gb["plies"].tobytes()


def test_a_search_that_needs_more_iterations_is_searched_again(monkeypatch):
    """The pipeline enqueues a fixed number of evaluate -> step iterations per batch.  A search that is still running when its record is
    written (forced here: two iterations where five are needed) has lost its slot to the next batch; its root is searched again from
    scratch and stepped until it has finished -- the same records, bit for bit, as a run whose searches all finish in time."""
    from betaone_amd import analyse as A

    config, _ = _tiny(monkeypatch)
    monkeypatch.setattr(config, "MCTS_BATCH_SIZE", 8)

    class HashNet(torch.nn.Module):
        def forward(self, x):
            from fake_model import fake_logits_values

            logits, v = fake_logits_values(x.numpy(), 5.0, 11)
            return torch.from_numpy(logits), torch.from_numpy(v)

    games, text = AC.make_corpus(seed=4, n_random=2, max_plies=10, long_plies=66)
    import pgn_util as U

    text = "".join(U.write_game(AC._sans(f, m), [None] * len(m), "*", fen=f) for f, m in games[:5])   # incl. the repetition and the mate
    with H.emulator_backend():
        want = A.analyse_games(text, HashNet(), sims=32, slots=4, device="cpu")
        got = A.analyse_games(text, HashNet(), sims=32, slots=4, device="cpu", iterations=2)
    assert want["report"]["roots_searched_again"] == 0
    assert got["report"]["roots_searched_again"] == got["report"]["positions_analysed"] == want["report"]["positions_analysed"] > 8
    assert got["report"]["positions_not_searched"] == want["report"]["positions_not_searched"] >= 2
    for ga, gb in zip(want["games"], got["games"]):
        assert ga["plies"].tobytes() == gb["plies"].tobytes(), ga["index"]
