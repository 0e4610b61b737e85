"""tests/anchor_cases.py -- checks of the anchor opponent (betaone_amd/anchor.py, csrc/bo_anchor.h), shared by the wave-emulator
tests (test_anchor_emu.py) and the MI355X tests (test_anchor_gpu.py): the same bodies, parameterised by backend.

The reference is the definition (DESIGN.md "Anchor opponent") written down once more in Python: a negamax over the oracle's rules
(bo_legal_moves / bo_push / bo_is_check) to a fixed depth, with the static evaluation restated from the text.  It shares no code with
the device.  Every comparison is of exact integers; the expected figures are recomputed here, never pinned; a set only asserts that
the reference shows the class it is there for."""
import ctypes as C
import functools
import io
import re
import types

import numpy as np

import engine_harness as H
import mate_cases as MC
from betaone_amd import anchor as A
from betaone_amd import engine as E
from oracle import oracle as O
from test_oracle_rules import PERFT

MATE = 30000
KIWIPETE = PERFT[1][0]
MANY_MOVES = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"   # 218 legal moves: four mask words, loops past 64 and 128
KPK = "8/8/8/4k3/8/4K3/4P3/8 w - - 0 1"
MATED_IN_2 = "7k/p4K1p/7P/8/8/8/8/6R1 b - - 0 1"       # ...a6 / ...a5, then Rg8#
HANGING_QUEEN = "4k3/8/8/3q4/8/8/8/3RK3 w - - 0 1"     # Rxd5 wins a queen for nothing
POISONED = "4k3/8/2p5/3p4/8/8/8/3QK3 w - - 0 1"        # Qxd5 wins a pawn at depth 1 and loses the queen to cxd5 at depth 2
INNER_TERMINALS = "7k/8/6K1/8/8/5Q2/8/8 w - - 0 1"      # Qf8 mates, Qf7 stalemates: both are entries of level 1 at depth 3
MATE_IN_1_OPENING = "6k1/5ppp/8/8/8/8/5PPP/R5K1 w - - 0 1"   # Ra8#
_CLOCKS = 8


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def ev_of(bb, white_to_move) -> int:
    """ev from the text: bb = pawns, knights, bishops, rooks, queens, kings, white, black."""
    no_queens = bb[4] == 0
    total = 0
    for kind in range(6):
        x = bb[kind]
        while x:
            sq = (x & -x).bit_length() - 1
            x &= x - 1
            white = bool(bb[6] >> sq & 1)
            f, rank = sq & 7, sq >> 3
            r = rank if white else 7 - rank
            e = min(f, 7 - f)
            d = e + min(r, 7 - r)
            t = (100 + 2 * (r - 1) ** 2 + 3 * e, 300 + 8 * d, 320 + 4 * d, 500 + (20 if r == 6 else 0), 900 + 2 * d,
                 8 * d if no_queens else -6 * r)[kind]
            total += t if white == bool(white_to_move) else -t
    return total


def ev_pos(p) -> int:
    return ev_of([p.pawns, p.knights, p.bishops, p.rooks, p.queens, p.kings, p.occ[1], p.occ[0]], p.turn == 1)


def ev_bo(q) -> int:
    return ev_of([int(v) for v in q.bb], q.turn == 1)


_memo = {}


def ref_val(p, ply, depth) -> int:
    key = (bytes(p)[:-_CLOCKS], ply, depth)
    v = _memo.get(key)
    if v is None:
        arr, k = MC._moves(p)
        if k == 0:
            v = -(MATE - ply) if O.lib().bo_is_check(C.byref(p)) else 0
        elif ply == depth:
            v = ev_pos(p)
        else:
            v = max(-ref_val(MC._after(p, arr[i]), ply + 1, depth) for i in range(k))
        _memo[key] = v
    return v


def ref_entries(p, levels) -> int:
    """Frontier entries of `levels` levels from p (transpositions counted as the walk meets them)."""
    if levels == 1:
        return 1
    arr, k = MC._moves(p)
    return 1 + sum(ref_entries(MC._after(p, arr[i]), levels - 1) for i in range(k))


@functools.lru_cache(maxsize=None)
def ref_root(fen, depth):
    board = O.Board(fen)  # (alive while its position is copied)
    p = board.pos.copy()
    arr, k = MC._moves(p)
    if k == 0:
        st = "checkmated" if O.lib().bo_is_check(C.byref(p)) else "stalemated"
        return types.SimpleNamespace(status=st, n_moves=0, moves=[], scores=[], score=0, best=None, n_best=0, entries=0)
    moves = [O.move_to_uci(arr[i]) for i in range(k)]
    scores = [-ref_val(MC._after(p, arr[i]), 1, depth) for i in range(k)]
    score = max(scores)
    return types.SimpleNamespace(status="ok", n_moves=k, moves=moves, scores=scores, score=score, best=moves[scores.index(score)],
                                 n_best=scores.count(score), entries=ref_entries(p, depth))


def ev_fens():
    """Check 1's positions: the perft suite's, every position one ply below them, the 218-move position, KRK / KQK / KPK roots."""
    fens = [p[0] for p in PERFT] + [MANY_MOVES, MC.KRK, MC.KQK, KPK, MC.STALE_TRAP]
    for p in PERFT:
        fens += list(MC.below(p[0], 1))
    return fens


def krk_roots():
    return tuple(sorted(set(MC.below(MC.KRK, 2))))


# ---- the device ---------------------------------------------------------------------------------------------------------------------
def _on(backend, fn, *a, **kw):
    if backend == "emu":
        with H.emulator_backend():
            return fn(*a, device="cpu", **kw)
    return fn(*a, device="cuda:0", **kw)


@functools.lru_cache(maxsize=None)
def run(backend, fens, depth, capacity=A.DEFAULT_CAPACITY, as_positions=False):
    """A.search with scores on the backend; `fens` a FEN or a tuple of FENs.  Cached and shared: nobody changes a result."""
    f = list(fens) if isinstance(fens, tuple) else [fens]
    roots = MC.to_bo_positions(f) if as_positions else f
    res = _on(backend, A.search, roots, depth, scores=True, capacity=capacity)
    return res if isinstance(fens, tuple) else res[0]


def facts(r):
    """What two runs of a root must agree on (everything but the call's own nodes, splits and time)."""
    return (r.status, r.score, r.best, r.n_best, r.n_moves, tuple(r.move_words), tuple(r.scores))


def check_ev(backend, fens):
    """Check 1: bo_anchor_eval against the Python ev; the turn toggled; the colours flipped."""
    from symmetry_cases import flip_fen

    fens = list(fens)
    arr = MC.to_bo_positions(fens)
    got = _on(backend, A.evaluate, arr)
    want = [ev_bo(q) for q in arr]
    assert got.tolist() == want
    kings = {(int(q.bb[4]) == 0) for q in arr}
    assert kings == {True, False}, "both king terms must occur"
    assert len(set(want)) > 50 and max(abs(v) for v in want) < 15000  # (the set is no row of equal numbers)
    # the other side to move: the same men, the opposite sign (where the side to move is not in check, and without an ep square)
    quiet = [i for i, f in enumerate(fens) if not O.lib().bo_is_check(C.byref(O.Board(f).pos.copy()))]
    assert len(quiet) > len(fens) // 2
    tog = MC.to_bo_positions([fens[i] for i in quiet])
    for q in tog:
        q.turn ^= 1
        q.ep_square = -1
    assert _on(backend, A.evaluate, tog).tolist() == [-want[i] for i in quiet]
    flipped = MC.to_bo_positions([flip_fen(f) for f in fens])
    assert _on(backend, A.evaluate, flipped).tolist() == want
    return want


def check_values(backend, fens, depth, **kw):
    """Check 2: score, best, n_best, n_moves, status and the whole scores row of every root, and the call's nodes."""
    fens = tuple(fens)
    res = run(backend, fens, depth, **kw)
    entries = 0
    for f, r in zip(fens, res):
        want = ref_root(f, depth)
        entries += want.entries
        assert r.status == want.status, (f, r.status, want.status)
        assert (r.n_moves, r.score, r.n_best, r.best) == (want.n_moves, want.score, want.n_best, want.best), (f, depth, r, want)
        assert r.moves == want.moves and r.scores == want.scores, (f, depth)
        assert r.depth == depth
    print(f"{len(fens)} roots, depth {depth}: {res[0].nodes} nodes, {res[0].splits} splits, {res[0].seconds:.3f} s")
    assert res[0].nodes == entries and all(r.nodes == entries for r in res)
    return res


NAMED = [(MC.EP_MATE, 1), (MC.PROMO_KEYS, 1), (MC.STALE_TRAP, 3), (MC.KRK, 3), (MATED_IN_2, 2), (MATED_IN_2, 3), (HANGING_QUEEN, 1),
         (POISONED, 1), (POISONED, 2), (INNER_TERMINALS, 3), (MANY_MOVES, 1), (MANY_MOVES, 2)]


def check_named(backend, fen, depth):
    """Check 2 on one named position: the reference's figures, and what the position is there for."""
    r = check_values(backend, (fen,), depth)[0]
    by = dict(zip(r.moves, r.scores))  # (what the position is there for: the reference agreed above, so it sees it too)
    if fen == MC.EP_MATE:
        assert (r.best, r.score, r.n_best) == ("f5g6", MATE - 1, 1)
    if fen == MC.PROMO_KEYS:
        assert r.score == MATE - 1 and r.n_best > 1 and len(r.best) == 5 and r.best == [m for m in r.moves if by[m] == r.score][0]
    if fen == MC.STALE_TRAP:
        assert by["f7f8q"] == 0 and by["f7f8r"] == MATE - 3 == r.score
    if fen == MC.KRK:
        assert r.score == MATE - 3 and r.n_best == 2
    if fen == MATED_IN_2:
        assert r.score == -(MATE - 2) and r.n_best == r.n_moves
    if fen == HANGING_QUEEN:
        assert r.best == "d1d5" and r.score > 400
    if fen == POISONED:
        assert (r.best == "d1d5") == (depth == 1) and (depth == 1 or by["d1d5"] < 0 < r.score)
    if fen == INNER_TERMINALS:  # a mated and a stalemated entry on level 1 of a depth-3 walk: the count kernel's terminal path
        assert by["f3f8"] == MATE - 1 and by["f3f7"] == 0
        assert {MC.ref_root(f, 1).status for f in MC.below(fen, 1)} == {"ok", "checkmated", "stalemated"}
    if fen == MANY_MOVES:
        assert r.n_moves == 218
    return r


def check_chunking(backend, fens, depth, capacities):
    """Check 3: identical results, scores and nodes at every capacity; each of them must have split a level."""
    fens = tuple(fens)
    base = run(backend, fens, depth)
    assert base[0].splits == 0
    for cap in capacities:
        got = run(backend, fens, depth, capacity=cap)
        print(f"capacity {cap}: {got[0].splits} splits, {got[0].nodes} nodes")
        assert got[0].splits > 0, cap
        assert [facts(r) for r in got] == [facts(r) for r in base], cap
        assert got[0].nodes == base[0].nodes, cap


def check_batch_invariance(backend, fens, depth):
    """Check 4: each root alone equals the root inside the batch; FEN and bo_position input agree; two identical raw calls return
    identical bytes."""
    fens = tuple(fens)
    batch = run(backend, fens, depth)
    for f, r in zip(fens, batch):
        assert facts(run(backend, f, depth)) == facts(r), f
    as_pos = run(backend, fens, depth, as_positions=True)
    assert [facts(r) for r in as_pos] == [facts(r) for r in batch] and all(r.fen is None for r in as_pos)

    def raw():
        lib = H.emu_lib() if backend == "emu" else E.load_hip_library()
        arr = (C.c_char_p * len(fens))(*[f.encode() for f in fens])
        out = (A.BoAnchorResult * len(fens))()
        words = np.zeros((len(fens), A.MAX_MOVES), np.int32)
        vals = np.zeros((len(fens), A.MAX_MOVES), np.int32)
        splits = C.c_int64(-1)
        assert lib.bo_anchor(0, len(fens), arr, None, depth, 256, 0, C.addressof(out), words.ctypes.data, vals.ctypes.data, C.byref(splits), None) == 0
        return bytes(out), words.tobytes(), vals.tobytes(), splits.value

    first = raw()
    assert first == raw()
    words = np.frombuffer(first[1], np.int32).reshape(len(fens), -1)
    vals = np.frombuffer(first[2], np.int32).reshape(len(fens), -1)
    for i, r in enumerate(batch):  # beyond n_moves: -1 and INT32_MIN
        assert words[i, :r.n_moves].tolist() == r.move_words and (words[i, r.n_moves:] == -1).all()
        assert vals[i, :r.n_moves].tolist() == r.scores and (vals[i, r.n_moves:] == -(1 << 31)).all()


# ---- the game loop ------------------------------------------------------------------------------------------------------------------
def _net():
    import torch

    from fake_model import FakeNet

    class Net(torch.nn.Module):
        def forward(self, x):
            l, v = FakeNet(scale=6.0, salt=9)(x)
            return l.to(x.device), v.to(x.device)

    return Net()


def play(backend, openings, n_games, n_slots, sims, depth, max_game_moves, margin=0):
    """(played, finished games by id, summary, PGN text) of a net-versus-anchor match of tests/fake_model.py's net."""
    from betaone_amd import match as M

    dev = "cpu" if backend == "emu" else "cuda:0"

    def go():
        ro = A.AnchorRollout(_net(), n_slots, depth, margin, num_simulations=sims, mcts_batch_size=8, max_game_moves=max_game_moves,
                             temperature=(2, 1.0, 0.1), device=dev, use_graph=False)
        fins = {}
        try:
            played = M.play_match(ro, M.MatchScheduler(openings, n_games, n_slots, 1), step_of=lambda s: 0, finished=fins)
        finally:
            ro.close()
        f = io.StringIO()
        M.write_match_pgn(f, played, fins, A.anchor_name(depth, margin), "fake", device=dev, date="2026.01.02")
        return played, fins, M.summarize(played, with_pairs=True), f.getvalue()

    if backend == "emu":
        with H.emulator_backend():
            return go()
    return go()


def check_games(openings, n_games, depth, played, fins, st, text):
    """Check 7 on a finished match: the anchor's plies are the reference's best moves, net plies and anchor plies alternate, each
    opening is played once with each colour, summarize counts every game once, the PGN reads back."""
    import pgn_util as U

    games = played["games"]
    assert sorted(g["game_id"] for g in games) == list(range(n_games)) and sorted(fins) == list(range(n_games))
    assert st["games"] == n_games == st["wins"] + st["draws"] + st["losses"]
    whites = {}
    for g in games:
        whites.setdefault((g["game_id"] // 2, g["opening"]), []).append(g["white"])
    assert all(sorted(w) == ["A", "B"] for w in whites.values()), whites
    anchor_plies = 0
    for g in games:
        fin = fins[g["game_id"]]
        pre = len(g["prefix"].split())
        assert fin.first_ply == pre and len(fin.pis) == len(fin.moves) - pre
        board = O.Board(g["fen"])
        for i, w in enumerate(fin.moves):
            uci = E.move_to_uci(w)
            assert uci in [O.move_to_uci(m) for m in board.legal_moves()], (g["game_id"], i, uci)
            if i >= pre:
                white_to_move = board.pos.turn == 1
                anchor = white_to_move == (g["white"] == "A")
                idx, val = fin.pis[i - pre]
                assert (len(idx) == 0) == anchor, (g["game_id"], i)  # (so the movers alternate: the side to move does)
                if anchor:
                    anchor_plies += 1
                    assert uci == ref_root(board.fen(), depth).best, (g["game_id"], i, uci, board.fen())
            board.push(O.move_from_uci(uci))
    assert anchor_plies >= n_games
    heads = re.findall(r'\[White "([^"]*)"\]\n\[Black "([^"]*)"\]', text)
    name = {"A": f"A ({A.anchor_name(depth, 0)})", "B": "B (fake)"}
    assert heads == [(name[g["white"]], name[g["black"]]) for g in games]
    movetexts = text.split("\n\n")[1::2]
    assert len(movetexts) == n_games
    for g, mt in zip(games, movetexts):  # the SAN of every move, replayed through the oracle's shim
        b = U.chess.Board(g["fen"])
        toks = [w for w in re.sub(r"\{[^}]*\}", " ", mt).split() if not re.match(r"^\d+\.", w)]
        assert toks[-1] in ("1-0", "0-1", "1/2-1/2", "*")
        ucis = g["moves"]  # (the prefix included)
        assert len(toks) - 1 == len(ucis), (g["game_id"], toks, ucis)
        for tok, u in zip(toks, ucis):
            m = U.chess.Move.from_uci(u)
            assert tok == U.san(b, m), (g["game_id"], tok, u)
            b.push(m)
    return anchor_plies


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def cli(backend, argv):
    """(exit status, output) of python -m betaone_amd.anchor's main on the backend."""
    out = io.StringIO()
    dev = ["--device", "cpu" if backend == "emu" else "cuda:0"]
    if backend == "emu":
        with H.emulator_backend():
            rc = A.main(list(argv) + dev, out)
    else:
        rc = A.main(list(argv) + dev, out)
    return rc, out.getvalue()


def check_cli_best(backend, tmp_path):
    """Check 8a: `anchor best` on a FEN (text, scores, JSON) and on a small EPD file."""
    import json

    want = ref_root(MC.STALE_TRAP, 3)
    rc, text = cli(backend, ["best", MC.STALE_TRAP, "--depth", "3", "--scores"])
    print(text)
    lines = text.splitlines()
    assert rc == 0 and lines[0] == f"Best f7f8r (mate in 2, score {MATE - 3}), 1 of {want.n_moves} moves reach it."
    assert lines[1] == " ".join(f"{m} {v}" for m, v in zip(want.moves, want.scores)) and lines[2].startswith(f"depth 3: {want.entries} nodes, ")
    rc, text = cli(backend, ["best", POISONED, "--depth", "2", "--json"])
    d = json.loads(text)
    two = ref_root(POISONED, 2)
    assert rc == 0 and (d["best"], d["score"], d["n_best"], d["nodes"]) == (two.best, two.score, two.n_best, two.entries) and "scores" not in d
    epd = tmp_path / "suite.epd"
    epd.write_text(f"# three positions\n{' '.join(MC.EP_MATE.split()[:4])} bm f5g6;\n{MC.MATED}\n{HANGING_QUEEN} id \"queen\";\n")
    rc, text = cli(backend, ["best", "--epd", str(epd), "--depth", "1"])
    print(text)
    lines = text.splitlines()
    q = ref_root(HANGING_QUEEN, 1)
    assert rc == 0 and len(lines) == 4
    assert ":2: " in lines[0] and f"best f5g6 (mate in 1, score {MATE - 1})" in lines[0]
    assert ":3: " in lines[1] and lines[1].endswith("the side to move is checkmated")
    assert ":4: " in lines[2] and f"best {q.best} ({q.score:+d} cp, score {q.score})" in lines[2]
    assert lines[3].startswith("3 positions at depth 1; 2 nodes in ")


def check_cli_match(backend, tmp_path):
    """Check 8b: `anchor match` through main with a hash-initialised checkpoint: a summary line, a JSON file and a PGN file."""
    import json

    import torch

    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = (1, 0, 64) if backend == "emu" else (2, 1, 128)
    try:
        net = hash_init_(network.PolicyValueNet())
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    ckpt, out, pgn, book = tmp_path / "net.pth", tmp_path / "result.json", tmp_path / "games.pgn", tmp_path / "book.txt"
    torch.save(net.state_dict(), ckpt)
    book.write_text(f"{MC.KRK}\n")
    rc, text = cli(backend, ["match", str(ckpt), "--depth", "2", "--margin", "15", "--games", "2", "--slots", "2", "--sims", "8",
                             "--mcts-batch", "8", "--openings", str(book), "--max-game-moves", "6", "--out", str(out), "--pgn", str(pgn)])
    print(text)
    assert rc == 0
    last = text.splitlines()[-1]
    assert re.match(r"^\[anchor\] net vs anchor\(depth=2,margin=15\): \+\d+ =\d+ -\d+  score \d\.\d{3}  Elo \S+ \[\S+, \S+\] \(pentanomial\)  "
                    r"LOS \d\.\d{3}  \d+ plies/s$", last), last
    d = json.loads(out.read_text())
    assert d["a"] == "anchor(depth=2,margin=15)" and d["summary"]["games"] == 2 and len(d["games"]) == 2
    assert {g["white"] for g in d["games"]} == {"A", "B"} and d["summary"]["anchor_plies"] >= 2
    assert pgn.read_text().count('[Event "BetaOne match"]') == 2 and "A (anchor(depth=2,margin=15))" in pgn.read_text()
