"""GPU test: `match --pgn` on the MI355X marks exactly the opening's prefix moves of every game with {book}, for prefixes of several
lengths, and each game parses back to the JSON's moves."""
import json
import re

import pytest
import torch

import pgn_util as U
from betaone_amd import pgn as P

pytestmark = pytest.mark.gpu
chess = U.chess


def test_book_comments_sit_on_each_games_prefix(tmp_path):
    from betaone_amd import dropin
    from betaone_amd import match as M
    from test_match_gpu import _net

    dropin.install()
    import utils

    pa, pb = tmp_path / "a.pth", tmp_path / "b.pth"
    torch.save(_net(2, 1, 64).state_dict(), pa)
    torch.save(_net(2, 1, 64, salt=1).state_dict(), pb)
    op = tmp_path / "openings.txt"
    op.write_text("startpos ; e2e4 e7e5 g1f3\nstartpos ; d2d4\nstartpos\n"
                  "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1 ; c7c5 g1f3\n")
    out, pgn = tmp_path / "match.json", tmp_path / "match.pgn"
    assert M.main([str(pa), str(pb), "--games", "8", "--slots", "8", "--sims", "16", "--mcts-batch", "8", "--openings", str(op),
                   "--max-game-moves", "30", "--out", str(out), "--pgn", str(pgn)]) == 0
    games = json.loads(out.read_text())["games"]
    text = pgn.read_text()
    r = P.replay_games(P.parse_text(text), device="cuda:0")
    assert r["status"].tolist() == [0] * len(games)
    movetexts = text.split("\n\n")[1::2]
    assert len(movetexts) == len(games)
    for k, g in enumerate(games):
        a = int(r["tok_off"][k])
        want = [utils.move_to_index(chess.Move.from_uci(u)) for u in g["moves"]]
        assert r["act"][a:a + len(want)].tolist() == want and int(r["n_plies"][k]) == len(want), k
        words = [w for w in movetexts[k].split() if not re.match(r"^\d+\.", w)]
        flags = [i for i, w in enumerate(words) if w == "{book}"]
        assert flags == [2 * i + 1 for i in range(len(g["prefix"].split()))], k   # after each prefix move, and nowhere else
