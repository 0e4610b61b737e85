"""tests/tablebase_cases.py -- checks of the endgame tablebases (betaone_amd/tablebase.py, csrc/bo_tb.h), shared by the wave-emulator
tests (test_tablebase_emu.py) and the MI355X tests (test_tablebase_gpu.py): the same bodies, parameterised by backend ("emu" / "hip").

The references: the published DTM maxima (KQK 10 moves, KRK 16, KPK 28, KBNK 33), and the oracle's rules -- an entry's code must follow
from its children's codes (looked up through the HOST index function, sub-tables, mirror and insufficient material handled in Python),
with the oracle's legal moves as the children.  The device's own verify kernel proves the whole table given the device move generator;
the sample over the oracle ties that generator to independent rules."""
import contextlib
import ctypes as C
import functools

import numpy as np

import engine_harness as H
from betaone_amd import engine as E
from betaone_amd import tablebase as TB
from oracle import oracle as O

PUBLISHED_MAX_WIN_PLIES = {"KQK": 19, "KRK": 31, "KPK": 55, "KBNK": 65}  # 10, 16, 28 and 33 moves
DEVICE = {"emu": "cpu", "hip": "cuda:0"}


def backend_ctx(backend):
    return H.emulator_backend() if backend == "emu" else contextlib.nullcontext()


@functools.lru_cache(maxsize=None)
def built(backend, materials):
    """TableSet with `materials` and their closure, built once and shared (nobody changes it); .payload[name] = the host copy."""
    with backend_ctx(backend):
        ts = TB.build(list(materials), None, DEVICE[backend])
        ts.payload = {name: t.download() for name, t in ts.tables.items()}
    return ts


def check_complete_build(backend, ts, name, all_strong_wins):
    """verify 0, a second build with the same bytes, the published maximum, the weak side's largest loss even and <= maximum + 1."""
    t = ts.tables[name]
    with backend_ctx(backend):
        info = t.info()
        assert info["complete"] and t.verify() == 0
        # a second build, in a table of its own bound to the same sub-tables
        again = TB.Table(name, t.subs, DEVICE[backend])
        passes = again.build()
        info2 = again.info()
        again.close()
    s, w = info["strong_to_move"], info["weak_to_move"]
    print(f"{TB.stats_line(info)}; {info['passes']} passes, {t.seconds:.3f} s")
    assert info2["fnv1a"] == info["fnv1a"]
    if info["n_men"] <= 3:  # (the host's byte loop: the small tables only)
        assert info["fnv1a"] == TB.fnv1a(ts.payload[name].astype("<u2").tobytes())
    assert passes == info["passes"]
    assert s["max_win_ply"] == PUBLISHED_MAX_WIN_PLIES[name], (name, s)
    assert w["max_loss_ply"] % 2 == 0 and w["max_loss_ply"] <= PUBLISHED_MAX_WIN_PLIES[name] + 1, (name, w)
    assert s["losses"] == 0 and w["wins"] == 0  # (a lone king never wins)
    if all_strong_wins:
        assert s["wins"] == s["legal"] and s["draws"] == 0, (name, s)


def pos_bitboards(p):
    return [p.pawns, p.knights, p.bishops, p.rooks, p.queens, p.kings, p.occ[1], p.occ[0]], p.turn == 1


def host_code(payload, bb, white_to_move):
    name, idx = TB.position_index(bb, white_to_move)
    return 1 if name is None else int(payload[name][idx])


def bellman(payload, board):
    """The code of the board's position from its children's codes, with the oracle's moves."""
    L = O.lib()
    moves = board.legal_moves()
    if not moves:
        return 2 if L.bo_is_check(C.byref(board.pos)) else 1
    min_loss, worst = None, -1
    for m in moves:
        board.push(m)
        c = host_code(payload, *pos_bitboards(board.pos))
        board.pop()
        assert c != 0, (board.fen(), O.move_to_uci(m))
        if c == 1:
            worst = 1 << 20
        elif (c - 2) & 1:
            worst = max(worst, c - 2)
        else:
            min_loss = c - 2 if min_loss is None else min(min_loss, c - 2)
    if min_loss is not None:
        return 2 + min_loss + 1
    return 1 if worst == 1 << 20 else 2 + worst + 1


def check_against_the_oracle(payload, name, n_sample, seed=0):
    """A fixed-seed sample of legal entries: the Bellman rule with the oracle's moves; every code-2 entry is the oracle's checkmate."""
    T = payload[name]
    legal = np.nonzero(T)[0]
    pick = np.random.RandomState(seed).choice(legal, size=min(n_sample, len(legal)), replace=False)
    L = O.lib()
    bad = []
    for idx in pick.tolist():
        b = O.Board(TB.entry_fen(name, idx))
        want = bellman(payload, b)
        if want != int(T[idx]):
            bad.append((idx, b.fen(), int(T[idx]), want))
    for idx in np.nonzero(T == 2)[0].tolist():
        b = O.Board(TB.entry_fen(name, idx))
        if b.legal_moves() or not L.bo_is_check(C.byref(b.pos)):
            bad.append((idx, b.fen(), 2, "not checkmate"))
    assert not bad, (name, len(bad), bad[:5])
    return len(pick)


def bo_position(bb, white_to_move, castling=0):
    p = E.BoPosition()
    for i in range(8):
        p.bb[i] = bb[i]
    p.turn, p.castling, p.ep_square, p.ep_key, p.halfmove_clock, p.fullmove_number = int(white_to_move), castling, -1, -1, 0, 1
    return p


def check_probe(backend, ts, names, n_sample=2000, seed=1):
    pos, want = [], []
    for name in names:
        T = ts.payload[name]
        legal = np.nonzero(T)[0]
        for idx in np.random.RandomState(seed).choice(legal, size=min(n_sample, len(legal)), replace=False).tolist():
            bb, wtm = TB.entry_bitboards(name, idx)
            pos.append(bo_position(bb, wtm))
            pos.append(bo_position(*TB.mirror(bb, wtm)))
            want += [int(T[idx])] * 2
    with backend_ctx(backend):
        codes, status = ts.probe_codes(pos)
    assert (status == TB.COVERED).all()
    assert codes.tolist() == want


def check_probe_statuses(backend, ts):
    fens = ["8/8/8/4k3/8/8/PP6/K6R w - - 0 1",        # 5 men
            "4k3/8/8/8/8/8/8/4K2R w K - 0 1",          # castling rights
            "4k3/4p3/8/8/8/8/4P3/4K3 w - - 0 1",       # KPKP
            "4k3/8/8/8/8/8/8/2B1KB2 w - - 0 1",        # KBBK: no table loaded
            "4k3/8/8/8/8/8/8/2B1K3 b - - 0 1",         # KBK: insufficient material, a draw without a table
            "4k3/8/8/8/8/8/8/4K3 w - - 0 1"]           # KK
    with backend_ctx(backend):
        wdl, dtm, status = ts.probe([TB.position_from_fen(f) for f in fens])
    assert status.tolist() == [TB.TOO_MANY_MEN, TB.CASTLING, TB.PAWNS_BOTH, TB.NO_TABLE, TB.COVERED, TB.COVERED]
    assert wdl.tolist() == [0] * 6 and dtm.tolist() == [-1, -1, -1, -1, 0, 0]


def check_missing_sub_table(backend):
    with backend_ctx(backend):
        try:
            TB.Table("KPK", [], DEVICE[backend])
        except E.EngineError as e:
            assert "KQK" in str(e), e
            lib = E.load_hip_library()
            h = C.c_void_p()
            assert lib.bo_tb_create(0, b"KPK", None, 0, C.byref(h)) == -5 and not h.value  # BO_E_STATE
            return
    raise AssertionError("KPK was created without KQK")


# ---- rescoring: a synthetic .bog file ---------------------------------------------------------------------------------------------------
class Fin:
    """What records.pack_game reads of a finished game."""

    def __init__(self, gid, fen, ucis, terminal, values=False):
        b = O.Board(fen)
        pos = [b.pos.copy()]
        self.moves = []
        for u in ucis:
            m = O.move_from_uci(u)
            assert m.tup() in [x.tup() for x in b.legal_moves()], (fen, u)
            self.moves.append(m.from_sq | m.to_sq << 6 | m.promo << 12)
            b.push(m)
            pos.append(b.pos.copy())
        import engine_cases as EC

        self.positions = [EC.to_bo_position(p, -1) for p in pos]
        self.game_id, self.first_ply, self.terminal = gid, 0, terminal
        self.outcome = 1.0 if terminal in (1, 3) else 0.0
        self.pis = [(np.array([i % 7], np.int32), np.array([1.0], np.float32)) for i in range(len(ucis))]
        self.root_values = np.linspace(-0.5, 0.5, len(ucis)).astype(np.float32) if values else None
        self.resign, self.resign_check = values, False


KRK_START = "8/8/8/8/8/2k5/2P5/K6R b - - 0 40"   # ...Kxc2 enters KRK with white, the winner, to move
SHUFFLE = ["h1h8", "c2c3", "h8h1", "c3c2"]
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


def synthetic_games():
    return [Fin(10, KRK_START, ["c3c2"] + SHUFFLE * 5, 0),                 # through KRK, played on to the move limit
            Fin(11, KRK_START, ["c3c2", "h1d1", "c2d1"], 2),               # the rook is blundered: drawn from ply 2 on
            Fin(12, START, ["e2e4", "e7e5", "g1f3", "b8c6"], 0),           # never leaves the middlegame
            Fin(13, KRK_START, ["c3c2"] + SHUFFLE * 2, 0, values=True)]    # a BOG2 game


def check_rescore(backend, ts, tmp_path, complete=True):
    """The report's counts, the cut plies, untouched games byte for byte, and every written record through unpack_games,
    GpuReplayBuffer.add and write_pgn.  complete: ts holds the complete KRK table -- white wins at ply 1, black is lost at ply 2, and
    is only drawn there once the rook hangs.  Otherwise KRK's classification only (checkmates, everything else reads as a draw): every
    covered game is cut as drawn at its first covered ply."""
    import io

    from betaone_amd import pgn_write as W
    from betaone_amd import records as R

    fins = synthetic_games()
    blobs = [R.pack_game(f) for f in fins]
    src, out = tmp_path / "iter_0", tmp_path / "out"
    src.mkdir()
    (src / "games_rank0.bog").write_bytes(blobs[0] + blobs[1])
    (src / "games_rank1.bog").write_bytes(blobs[2] + blobs[3])
    with backend_ctx(backend):
        rep = TB.rescore(str(src), ts, write=str(out))
    cut = 2 if complete else 1
    assert (rep["games"], rep["positions"]) == (4, sum(len(f.moves) + 1 for f in fins)) == (4, 41)
    assert rep["games_covered"] == 3 and rep["mean_first_covered_ply"] == 1.0
    # complete: the table says white wins at ply 1; the records say unfinished, drawn, unfinished
    assert rep["disagree"] == (3 if complete else 0)
    assert rep["games_cut"] == 3 and rep["plies_saved"] == (21 - cut) + (3 - cut) + (9 - cut)
    assert "3 games reach a covered position (mean ply 1.0)" in TB.report_text(rep)
    got0, got1 = (out / "games_rank0.bog").read_bytes(), (out / "games_rank1.bog").read_bytes()
    g = R.unpack_games(got0) + R.unpack_games(got1)
    assert [x["game_id"] for x in g] == [10, 11, 12, 13]
    lost = (cut, 3, 1.0) if complete else (cut, 2, 0.0)  # black, to move at ply 2 of the complete table, resigned
    assert [(x["n_plies"], x["terminal"], x["outcome"]) for x in g] == [lost, (cut, 2, 0.0), (4, 0, 0.0), lost]
    assert got1[:len(blobs[2])] == blobs[2]                                   # the untouched game, byte for byte
    assert got0[:4] == b"BOG1" and got1[len(blobs[2]):][:4] == b"BOG2"        # BOG1 stays BOG1
    assert g[3]["root_values"].tolist() == fins[3].root_values[:cut].tolist() and g[3]["resign"] and g[0]["root_values"] is None
    for x, f in zip(g, fins):
        n = x["n_plies"]
        assert x["moves"].tolist() == f.moves[:n] and len(x["pis"]) == n
        assert bytes(x["positions"]) == b"".join(bytes(p) for p in f.positions[:n + 1])
    with backend_ctx(backend):
        text = io.StringIO()
        W.write_pgn(text, g, device=DEVICE[backend], sims=50)
        assert text.getvalue().count('[Result "1-0"]') == (2 if complete else 0)
        assert text.getvalue().count('[Result "1/2-1/2"]') == (1 if complete else 3)
        buf = R.GpuReplayBuffer(64, device=DEVICE[backend])
        assert buf.add(g) == 0 and len(buf) == sum(x["n_plies"] for x in g)
        buf.close()
    return rep
