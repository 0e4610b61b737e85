"""GPU tests of PGN export on the MI355X: bo_k_san_render's SAN slots and state bytes for a 2 000-game seeded corpus are bit-identical
to the wave emulator's, the PGN round-trips through the device ingest, `match --pgn` between two 10x128 checkpoints parses back to
the JSON's moves, and `selfplay_main --records compact` + the converter round-trip."""
import io
import json

import numpy as np
import pytest
import torch

import pgn_util as U
import test_pgn_write_emu as T
from betaone_amd import pgn as P
from betaone_amd import pgn_write as W

pytestmark = pytest.mark.gpu
chess = U.chess


@pytest.fixture(scope="module")
def corpus():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return T.corpus(23, 2000, 120)


def _acts(moves):
    from betaone_amd import dropin

    dropin.install()
    import utils

    return [utils.move_to_index(chess.Move(m & 63, (m >> 6) & 63, (m >> 12) or None)) for m in moves]


def test_san_and_states_match_the_emulator(corpus):
    games = [g for _, g, _ in corpus]
    gpu = W.render_san(games, device="cuda:0", max_positions=1 << 16)  # (several launches)
    emu = T.render(games)
    for a, b, (_, _, sans) in zip(gpu, emu, corpus):
        assert np.array_equal(a.san, b.san) and np.array_equal(a.state, b.state), a.game_id
        assert a.sans() == sans, a.game_id


def test_round_trip_through_the_device_ingest(corpus):
    games = [g for _, g, _ in corpus]
    f = io.StringIO()
    W.write_pgn(f, games, device="cuda:0")
    r = P.replay_games(P.parse_text(f.getvalue()), device="cuda:0")
    assert r["status"].tolist() == [0] * len(games)
    for k, g in enumerate(games):
        a, n = int(r["tok_off"][k]), len(g["moves"])
        assert int(r["n_plies"][k]) == n
        assert r["act"][a:a + n].tolist() == _acts(g["moves"]), k


def test_match_pgn_between_two_checkpoints(tmp_path):
    from betaone_amd import match as M
    from test_match_gpu import _net

    pa, pb = tmp_path / "a.pth", tmp_path / "b.pth"
    torch.save(_net(10, 0, 128).state_dict(), pa)
    torch.save(_net(10, 0, 128, salt=1).state_dict(), pb)
    op = tmp_path / "openings.txt"
    op.write_text("startpos ; e2e4 e7e5\nrnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1\n")
    out, pgn = tmp_path / "match.json", tmp_path / "match.pgn"
    assert M.main([str(pa), str(pb), "--games", "4", "--slots", "4", "--sims", "16", "--mcts-batch", "8", "--openings", str(op),
                   "--max-game-moves", "40", "--out", str(out), "--pgn", str(pgn)]) == 0
    res = json.loads(out.read_text())
    text = pgn.read_text()
    r = P.replay_games(P.parse_text(text), device="cuda:0")
    assert r["status"].tolist() == [0] * 4
    for k, g in enumerate(res["games"]):
        a = int(r["tok_off"][k])
        want = [T.enc(chess.Move.from_uci(u)) for u in g["moves"]]
        assert r["act"][a:a + len(want)].tolist() == _acts(want) and int(r["n_plies"][k]) == len(want), k
    assert text.count("{book}") == 2 * sum(1 for g in res["games"] if g["prefix"])


def test_selfplay_compact_records_convert(tmp_path):
    from betaone_amd import dropin
    from betaone_amd import records as R
    from betaone_amd import selfplay_main as M

    dropin.install()
    import config
    import network

    keys = ("RESIDUAL_BLOCKS", "SE_RESIDUAL_BLOCKS", "CONV_FILTERS", "NUM_SIMULATIONS", "MCTS_BATCH_SIZE", "DATA_DIR", "MAX_GAME_MOVES")
    saved = {k: getattr(config, k) for k in keys}
    try:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 3, 1, 64
        torch.manual_seed(0)
        model = network.PolicyValueNet().to("cuda").eval()
        config.NUM_SIMULATIONS, config.MCTS_BATCH_SIZE, config.MAX_GAME_MOVES = 50, 48, 30
        config.DATA_DIR = str(tmp_path / "data")
        M.run_iteration(model, 1, n_games=6, n_slots=6, log=lambda s: None, records="compact")
    finally:
        for k, v in saved.items():
            setattr(config, k, v)
    path = R.compact_path(str(tmp_path / "data"), 1, 0)
    games = sorted(R.load_games(path), key=lambda g: g["game_id"])
    out = tmp_path / "it1.pgn"
    assert W.main([path, "-o", str(out), "--date", "2026.10.15"]) == 0
    r = P.replay_games(P.parse_text(out.read_bytes()), device="cuda:0")
    assert r["status"].tolist() == [0] * len(games) and len(games) == 6
    for k, g in enumerate(games):
        a, n = int(r["tok_off"][k]), int(g["n_plies"])
        assert int(r["n_plies"][k]) == n and r["act"][a:a + n].tolist() == _acts(g["moves"].tolist()), k
