"""CPU tests (library host code + wave emulator) of PGN export: the SAN of every legal move of seeded and hand-made positions
(bo_k_san_render) against tests/pgn_util.san, a round trip of random games through write_pgn and the PGN ingest, the tag and movetext
format, the integrity errors, `match --pgn` under a stand-in rollout, and the .bog converter."""
import io
import json
import random
import re

import numpy as np
import pytest

import engine_cases as EC
import engine_harness as H
import pgn_util as U
from betaone_amd import match as M
from betaone_amd import pgn as P
from betaone_amd import pgn_write as W

chess = U.chess


def bo_pos(b):
    """bo_position of a shim Board, with the key's ep square resolved (what the engine exports)."""
    return EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1)


def enc(m):
    return m.from_square | m.to_square << 6 | (m.promotion or 0) << 12


def game_from(fen, ucis, gid=0):
    """A record-like game (positions, moves, terminal) and the oracle's SAN list."""
    b = chess.Board(fen) if fen else chess.Board()
    pos, mv, sans = [bo_pos(b)], [], []
    for u in ucis:
        m = chess.Move.from_uci(u)
        sans.append(U.san(b, m))
        mv.append(enc(m))
        b.push(m)
        pos.append(bo_pos(b))
    term = 1 if b.is_checkmate() else 2 if b.is_game_over(claim_draw=False) else 0
    return {"game_id": gid, "positions": pos, "moves": mv, "terminal": term}, sans


def render(games):
    with H.emulator_backend():
        return W.render_san(games, device="cpu")


HAND = [
    "2k5/8/8/8/4Q2Q/K7/8/7Q w - - 0 1",                                       # three queens: file, rank, square
    "k7/8/8/1N3N2/8/1N3N2/8/K3R2R w - - 0 1",                                # knights and rooks on shared files / ranks
    "r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1",
    "1n2k3/P1P5/8/8/8/8/8/4K3 w - - 0 1",                                    # capture-promotions with check
    "kr6/2P5/K7/8/8/8/8/1R6 w - - 0 1",                                      # capture-promotion mate
    "4k3/8/8/3pP3/8/8/8/4K3 w - d6 0 2",                                     # en passant
    "5k2/8/8/8/8/8/8/4K2R w K - 0 1",                                        # O-O+
    "3k4/8/8/8/8/8/8/R3K3 w Q - 0 1",                                        # O-O-O+
    "4rkr1/4p1p1/8/8/8/8/8/4K2R w K - 0 1",                                  # O-O#
    "k7/8/1Q6/8/8/8/8/7K w - - 0 1",                                         # stalemating moves
    "r1bqkb1r/pppp1ppp/2n2n2/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - 4 4",   # Qxf7#
]


def test_san_of_every_legal_move():
    rng = random.Random(3)
    fens = list(HAND)
    for i in range(120):
        mv, _, _, _ = U.random_game(rng, fen=[None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12"][i % 2], max_plies=rng.randint(0, 60))
        b = chess.Board() if i % 2 == 0 else chess.Board("r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12")
        for u in mv:
            b.push_uci(u)
        fens.append(b.fen())
    games, want = [], []
    for fen in fens:
        for m in chess.Board(fen).legal_moves:
            g, s = game_from(fen, [m.uci()], len(games))
            games.append(g)
            want.append(s[0])
    got = [r.sans()[0] for r in render(games)]
    bad = [(g["game_id"], w, s) for g, w, s in zip(games, want, got) if w != s]
    assert not bad, bad[:10]
    # the hand-made cases render what they were made for
    for must in ("Qee1", "Qh4e1", "Q1e1", "Nf5d4", "N3h4", "Nbd2", "Rhf1", "axb8=Q+", "cxb8=Q#", "cxb8=R#", "exd6", "O-O+", "O-O-O+",
                 "O-O#", "Qxf7#", "Qc7"):                            # (Qc7 stalemates: no suffix)
        assert must in got, must


FENS = [None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R b KQkq - 0 12", "4k3/8/8/8/8/8/8/4K2R b K - 7 33"]


def corpus(seed, n, max_plies=80):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        fen = FENS[i % len(FENS)]
        mv, _, _, _ = U.random_game(rng, fen=fen, max_plies=rng.randint(1, max_plies))
        out.append((fen,) + game_from(fen, mv, 1000 + i))
    return out


def test_round_trip_through_the_ingest():
    games = corpus(7, 300)
    f = io.StringIO()
    with H.emulator_backend():
        W.write_pgn(f, [g for _, g, _ in games], tags={"Event": "rt"})
        text = f.getvalue()
        r = P.replay_games(P.parse_text(text), device="cpu")
    assert r["status"].tolist() == [0] * len(games)
    words = re.findall(r"\n\n(.*?)(?:1-0|0-1|1/2-1/2|\*)\n", text, flags=re.S)
    for k, (fen, g, sans) in enumerate(games):
        n = len(g["moves"])
        a = int(r["tok_off"][k])
        assert int(r["n_plies"][k]) == n
        pos = r["pos"][a:a + n].view(np.uint64)[:, :8]
        want = np.array([list(p.bb) for p in g["positions"][:n]], dtype=np.uint64)
        assert np.array_equal(pos, want), k
        toks = [w for w in words[k].split() if not re.match(r"^\d+\.", w)]
        assert toks == sans, k
    # the action indices are those of the moves
    from betaone_amd import dropin

    dropin.install()
    import utils

    fen, g, _ = games[5]
    a = int(r["tok_off"][5])
    assert r["act"][a:a + len(g["moves"])].tolist() == [utils.move_to_index(chess.Move(m & 63, (m >> 6) & 63, (m >> 12) or None))
                                                       for m in g["moves"]]


def test_format():
    g1, _ = game_from("4k3/8/8/8/8/8/8/4K2R b K - 7 33", ["e8d7"] + ["h1h2", "d7d6", "h2h1", "d6d7"] * 12, 5)
    g2, _ = game_from(None, ["f2f3", "e7e5", "g2g4", "d8h4"], 6)            # fool's mate: terminal 1
    g3, _ = game_from("k7/8/1Q6/8/8/8/8/7K w - - 0 1", ["b6c7"], 7)         # stalemate: terminal 2
    g1["terminal"] = 0                                                       # (stopped by the move limit)
    assert (g2["terminal"], g3["terminal"]) == (1, 2)
    f = io.StringIO()
    with H.emulator_backend():
        W.write_pgn(f, [g1, g2, g3], tags=[{"Event": 'say "hi" \\ bye', "Round": 1}, {"Round": 2}, {"Round": 3, "Annotator": "x"}])
    text = f.getvalue()
    blocks = text.split("\n\n")
    heads = [re.findall(r'^\[(\w+) "((?:[^"\\]|\\.)*)"\]$', b, flags=re.M) for b in blocks[0::2]]
    order = ["Event", "Site", "Date", "Round", "White", "Black", "Result"]
    assert [k for k, _ in heads[0]] == order + ["SetUp", "FEN", "Termination", "PlyCount"]
    assert [k for k, _ in heads[1]] == order + ["Termination", "PlyCount"]
    assert [k for k, _ in heads[2]] == order + ["SetUp", "FEN", "Termination", "PlyCount", "Annotator"]
    h0, h1, h2 = (dict(h) for h in heads[:3])
    assert h0["Event"] == 'say \\"hi\\" \\\\ bye'
    assert h0["FEN"] == chess.Board("4k3/8/8/8/8/8/8/4K2R b K - 7 33").fen() and h0["PlyCount"] == "49"
    assert re.match(r"^\d{4}\.\d\d\.\d\d$", h0["Date"])
    assert (h0["Result"], h0["Termination"]) == ("*", "unterminated")
    assert (h1["Result"], h1["Termination"]) == ("0-1", "normal")
    assert (h2["Result"], h2["Termination"]) == ("1/2-1/2", "normal")
    assert blocks[1].startswith("33... Kd7 34. Rh2") and blocks[1].rstrip().endswith("*")
    assert blocks[3] == "1. f3 e5 2. g4 Qh4# 0-1" and blocks[5].strip() == "1. Qc7 1/2-1/2"
    assert all(len(line) <= 79 for line in text.splitlines())
    assert text.endswith("\n\n")


def test_errors_name_game_and_ply():
    g, _ = game_from(None, ["e2e4", "e7e5", "g1f3", "b8c6"], 42)
    bad = dict(g, moves=list(g["moves"]))
    bad["moves"][2] = enc(chess.Move.from_uci("g1g3"))
    with pytest.raises(ValueError, match=r"game 42 ply 2: illegal"):
        render([bad])
    bad = dict(g, positions=list(g["positions"]))
    bad["positions"][3] = g["positions"][1]
    with pytest.raises(ValueError, match=r"game 42 ply 2: mismatch"):
        render([bad])
    with pytest.raises(ValueError, match=r"game 42 ply 4"):
        with H.emulator_backend():
            W.write_pgn(io.StringIO(), [dict(g, terminal=1)])


# ---- match --pgn ----------------------------------------------------------------------------------------------------------------
from test_match_cpu import StandInRollout  # noqa: E402


class _Fin:
    def __init__(self, game_id, slot, positions, moves, terminal, first_ply):
        self.game_id, self.slot, self.positions, self.moves, self.terminal, self.first_ply = game_id, slot, positions, moves, terminal, first_ply


class PgnStandIn(StandInRollout):
    """The stand-in rollout, finishing every game with a real random game from its opening (seeded by the game id)."""

    def play_ply(self, on_finished=None, refill=None):
        def fin(f):
            gid = self.slot[f.slot][0]
            mg = self.sched.admitted[gid]
            b = chess.Board(mg.fen) if mg.fen else chess.Board()
            ucis = mg.moves.split()
            for u in ucis:
                b.push_uci(u)
            more, _, _, _ = U.random_game(random.Random(gid), fen=b.fen(), max_plies=self.lengths[gid])
            g, _ = game_from(mg.fen, ucis + more, gid)
            on_finished(_Fin(gid, f.slot, g["positions"], g["moves"], g["terminal"], len(ucis)))
        return super().play_ply(on_finished=fin, refill=refill)


def _play(finished):
    openings = [(None, ""), (None, "e2e4 e7e5 g1f3"), ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", "c7c5")]
    n, slots, cohorts = 12, 4, 2
    sched = M.MatchScheduler(openings, n, slots, cohorts)
    lengths = {g: 5 + 7 * (g % 5) for g in range(n)}
    ro = PgnStandIn(sched, slots, cohorts, lengths)
    return M.play_match(ro, sched, step_of=lambda s: ro.step[s // ro.Gc] + 1, finished=finished)


def test_match_pgn():
    plain = _play(None)
    fins = {}
    played = _play(fins)
    assert json.dumps(plain["games"]) == json.dumps(played["games"])
    f = io.StringIO()
    with H.emulator_backend():
        M.write_match_pgn(f, played, fins, "a.pth", "b.pth", device="cpu", date="2026.01.02")
        text = f.getvalue()
        r = P.replay_games(P.parse_text(text), device="cpu")
    assert r["status"].tolist() == [0] * len(played["games"])
    from betaone_amd import dropin

    dropin.install()
    import utils

    movetexts = text.split("\n\n")[1::2]
    for k, g in enumerate(played["games"]):
        a = int(r["tok_off"][k])
        want = [utils.move_to_index(chess.Move.from_uci(u)) for u in g["moves"]]
        assert r["act"][a:a + len(want)].tolist() == want and int(r["n_plies"][k]) == len(want)
        pre = len(g["prefix"].split())
        words = [w for w in movetexts[k].split() if not re.match(r"^\d+\.", w)]
        flags = [i for i, w in enumerate(words) if w == "{book}"]
        assert flags == [2 * i + 1 for i in range(pre)], k          # after each prefix move, and nowhere else
    heads = re.findall(r'\[Round "([^"]*)"\]\n\[White "([^"]*)"\]\n\[Black "([^"]*)"\]', text)
    assert [h[0] for h in heads] == [f"{g['opening'] + 1}.{g['game_id'] % 2 + 1}" for g in played["games"]]
    assert heads[0][1] == {"A": "A (a.pth)", "B": "B (b.pth)"}[played["games"][0]["white"]]
    # the {book} comment is no eval: pretraining takes no sample from the prefix
    assert not any(P.parse_text(text, H.emu_lib()).export()["has_eval"])


# ---- the converter -------------------------------------------------------------------------------------------------------------
def test_converter_on_bog_files(tmp_path):
    from betaone_amd import records

    games = corpus(17, 24, 60)
    d = tmp_path / "iter_3"
    d.mkdir()

    class Fin:
        def __init__(self, g):
            self.game_id, self.moves, self.positions, self.terminal = g["game_id"], g["moves"], g["positions"], g["terminal"]
            self.outcome, self.first_ply = 0.0, 0
            self.pis = [(np.array([0], np.int32), np.array([1.0], np.float32))] * len(g["moves"])

    rev = [Fin(g) for _, g, _ in games][::-1]  # written out of id order
    records.save_games(str(d / "games_rank1.bog"), rev[:10])
    records.save_games(str(d / "games_rank0.bog"), rev[10:])
    outs = []
    with H.emulator_backend():
        for k in range(2):
            out = tmp_path / f"o{k}.pgn"
            assert W.main([str(d), "-o", str(out), "--date", "2026.10.15", "--device", "cpu", "--event", "it3"]) == 0
            outs.append(out.read_bytes())
        r = P.replay_games(P.parse_text(outs[0]), device="cpu")
    assert outs[0] == outs[1]
    text = outs[0].decode()
    rounds = [int(x) for x in re.findall(r'\[Round "(\d+)"\]', text)]
    ids0 = sorted(f.game_id for f in rev[10:])
    ids1 = sorted(f.game_id for f in rev[:10])
    assert rounds == ids0 + ids1                                   # (path, game_id) order
    byid = {g["game_id"]: g for _, g, _ in games}
    from betaone_amd import dropin

    dropin.install()
    import utils

    assert r["status"].tolist() == [0] * len(rounds)
    for k, gid in enumerate(rounds):
        mv = byid[gid]["moves"]
        a = int(r["tok_off"][k])
        assert r["act"][a:a + len(mv)].tolist() == [utils.move_to_index(chess.Move(m & 63, (m >> 6) & 63, (m >> 12) or None)) for m in mv]
    assert '[Event "it3"]' in text and "selfplay_main --records compact" in _help()


def _help():
    import contextlib

    f = io.StringIO()
    with contextlib.redirect_stdout(f), pytest.raises(SystemExit):
        W.main(["--help"])
    return " ".join(f.getvalue().split())
