"""tests/anchor_q_cases.py -- checks of the anchor's quiescence search (bo_anchor_q, csrc/bo_anchor.h, betaone_amd/anchor.py), shared by
the wave-emulator tests (test_anchor_q_emu.py) and the MI355X tests (test_anchor_q_gpu.py): the same bodies, parameterised by backend.

The reference is the definition (DESIGN.md "Anchor opponent", quiescence) written down once more in Python over the oracle's rules:
    tactical moves of P    all legal moves if P is in check, else the legal moves that capture (the destination holds an enemy man, or a
                           pawn leaves its file onto an empty square: en passant) or promote, in the oracle's order
    qs(P, p, q)            -(MATE - p) / 0 without a legal move; ev(P) if q == 0; else the maximum of the floor (ev(P); -MATE in check)
                           and of -qs(P.m, p + 1, q - 1) over the tactical moves
    val(P, p)              -(MATE - p) / 0 without a legal move; qs(P, D, Q) at p == D; else the maximum over the moves of -val
with a memo of (position without clocks, ply, q).  It reuses anchor_cases.ev_pos and mate_cases._moves / _after and shares no code with
the device.  Every comparison is of exact integers; the expected figures are recomputed here, never pinned.  While it runs the
reference records which KINDS of quiescence node it met (KINDS: kind -> the first example), for the test of the classes."""
import ctypes as C
import functools
import io
import json
import re
import types

import numpy as np

import anchor_cases as AC
import engine_harness as H
import mate_cases as MC
from betaone_amd import anchor as A
from betaone_amd import engine as E
from oracle import oracle as O

MATE = AC.MATE
KIWIPETE, MANY_MOVES, POISONED, HANGING_QUEEN = AC.KIWIPETE, AC.MANY_MOVES, AC.POISONED, AC.HANGING_QUEEN
BACK_RANK = "r2r2k1/5ppp/8/8/8/8/3R1PPP/3R2K1 w - - 0 1"   # Rxd8+ Rxd8 Rxd8#: the mate lies inside the quiescence plies at (1, 2)
EP_BELOW = "4k3/8/8/8/4p3/8/3P4/4K3 w - - 0 1"             # after d2d4 the node at the horizon has the en passant capture exd3
PROMO_BELOW = "8/2P4k/8/8/8/8/8/K7 b - - 0 1"              # after any king move the node at the horizon has four quiet promotions
SUITE = tuple(p[0] for p in AC.PERFT)
# the named positions: anchor_cases' (each once) and the three above
NAMED = tuple(dict.fromkeys(f for f, _ in AC.NAMED)) + (BACK_RANK, EP_BELOW, PROMO_BELOW)
_CLOCKS = 8
KINDS = {}


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _seen(kind, p, ply, q):
    KINDS.setdefault(kind, (bytes(p)[:-_CLOCKS], ply, q))


def _check(p) -> bool:
    return bool(O.lib().bo_is_check(C.byref(p)))


def _en_passant(p, m) -> bool:
    return bool(p.pawns >> m.from_sq & 1) and (m.from_sq & 7) != (m.to_sq & 7) and not ((p.occ[0] | p.occ[1]) >> m.to_sq & 1)


def _tactical(p, m, chk) -> bool:
    return chk or bool(p.occ[1 - p.turn] >> m.to_sq & 1) or _en_passant(p, m) or m.promo != 0


_memo_qs, _memo_val, _memo_ent = {}, {}, {}


def ref_qs(p, ply, q, depth) -> int:
    key = (bytes(p)[:-_CLOCKS], ply, q, depth)
    v = _memo_qs.get(key)
    if v is None:
        arr, k = MC._moves(p)
        chk = _check(p)
        if k == 0:
            v = -(MATE - ply) if chk else 0
            if chk and ply > depth:
                _seen("mated above D", p, ply, q)
            if not chk:
                _seen("stalemated at D or below", p, ply, q)
        elif q == 0:
            v = AC.ev_pos(p)
        else:
            v = -MATE if chk else AC.ev_pos(p)
            tact = [i for i in range(k) if _tactical(p, arr[i], chk)]
            if chk:
                _seen("in check with moves", p, ply, q)
            elif not tact:
                _seen("stand pat only", p, ply, q)
            for i in tact:
                m = arr[i]
                if not chk:
                    if _en_passant(p, m):
                        _seen("en passant", p, ply, q)
                    if m.promo and not (p.occ[1 - p.turn] >> m.to_sq & 1):
                        _seen("quiet promotion", p, ply, q)
                        if m.promo != 5:
                            _seen("quiet under-promotion", p, ply, q)
                    if i >= 64:
                        _seen("tactical move beyond index 64", p, ply, q)
                        if q >= 2 and len(tact) < i + 1:  # (an inner quiescence level: the expand kernel ranks it below its index)
                            _seen("compacted from beyond index 64", p, ply, q)
                v = max(v, -ref_qs(MC._after(p, m), ply + 1, q - 1, depth))
        _memo_qs[key] = v
    return v


def ref_val(p, ply, depth, q) -> int:
    if ply == depth:
        return ref_qs(p, ply, q, depth)
    key = (bytes(p)[:-_CLOCKS], ply, depth, q)
    v = _memo_val.get(key)
    if v is None:
        arr, k = MC._moves(p)
        if k == 0:
            v = -(MATE - ply) if _check(p) else 0
        else:
            v = max(-ref_val(MC._after(p, arr[i]), ply + 1, depth, q) for i in range(k))
        _memo_val[key] = v
    return v


def ref_entries(p, level, depth, q) -> int:
    """Frontier entries of levels `level` .. depth + q - 1 below p, itself included (transpositions counted as the walk meets them:
    the memo is of (position, level), which the count is a function of)."""
    if level == depth + q - 1:
        return 1
    key = (bytes(p)[:-_CLOCKS], level, depth, q)
    v = _memo_ent.get(key)
    if v is None:
        arr, k = MC._moves(p)
        chk = _check(p) if level >= depth else True  # (a full-width level: every move)
        v = 1 + sum(ref_entries(MC._after(p, arr[i]), level + 1, depth, q) for i in range(k) if _tactical(p, arr[i], chk))
        _memo_ent[key] = v
    return v


@functools.lru_cache(maxsize=None)
def ref_root(fen, depth, q):
    board = O.Board(fen)  # (alive while its position is copied)
    p = board.pos.copy()
    arr, k = MC._moves(p)
    if k == 0:
        st = "checkmated" if _check(p) else "stalemated"
        return types.SimpleNamespace(status=st, n_moves=0, moves=[], scores=[], score=0, best=None, n_best=0, entries=0)
    moves = [O.move_to_uci(arr[i]) for i in range(k)]
    scores = [-ref_val(MC._after(p, arr[i]), 1, depth, q) for i in range(k)]
    score = max(scores)
    return types.SimpleNamespace(status="ok", n_moves=k, moves=moves, scores=scores, score=score, best=moves[scores.index(score)],
                                 n_best=scores.count(score), entries=ref_entries(p, 0, depth, q))


# ---- the device ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run(backend, fens, depth, q, capacity=A.DEFAULT_CAPACITY, as_positions=False):
    """A.search with scores and quiesce=q on the backend; `fens` a FEN or a tuple of FENs.  Cached and shared: nobody changes a result."""
    f = list(fens) if isinstance(fens, tuple) else [fens]
    roots = MC.to_bo_positions(f) if as_positions else f
    res = AC._on(backend, A.search, roots, depth, quiesce=q, scores=True, capacity=capacity)
    return res if isinstance(fens, tuple) else res[0]


def check_values(backend, fens, depth, q, **kw):
    """Check 1: status, n_moves, score, best, n_best and the whole scores row of every root, and the call's nodes."""
    fens = tuple(fens)
    res = run(backend, fens, depth, q, **kw)
    entries = 0
    for f, r in zip(fens, res):
        want = ref_root(f, depth, q)
        entries += want.entries
        assert r.status == want.status, (f, r.status, want.status)
        assert (r.n_moves, r.score, r.n_best, r.best) == (want.n_moves, want.score, want.n_best, want.best), (f, depth, q, r, want)
        assert r.moves == want.moves and r.scores == want.scores, (f, depth, q)
        assert (r.depth, r.quiesce) == (depth, q)
        assert all(-MATE <= v <= MATE for v in r.scores)  # (an int16 holds every value)
    print(f"{len(fens)} roots, depth {depth}, quiesce {q}: {res[0].nodes} nodes, {res[0].splits} splits, {res[0].seconds:.3f} s")
    assert res[0].nodes == entries and all(r.nodes == entries for r in res)
    return res


def check_classes(roots):
    """Check 2: over `roots` ((fen, depth, q) triples, the ones the value tests compare) the reference met every kind of node."""
    for f, d, q in roots:
        ref_root(f, d, q)
    kinds = ["in check with moves", "mated above D", "stalemated at D or below", "stand pat only", "en passant", "quiet promotion",
             "quiet under-promotion", "tactical move beyond index 64", "compacted from beyond index 64"]
    assert [k for k in kinds if k not in KINDS] == [], sorted(KINDS)
    assert KINDS["mated above D"][1] > 1
    back = ref_root(BACK_RANK, 1, 2)  # a root whose score is a mate found inside the quiescence plies
    assert back.score == MATE - 3 and 1 < MATE - back.score <= 1 + 2
    assert ref_root(BACK_RANK, 1, 0).score < MATE - 8 and ref_root(BACK_RANK, 1, 1).score < MATE - 8


def check_purpose(backend):
    """Check 3: what quiescence is for."""
    assert run(backend, POISONED, 1, 0).best == "d1d5" == ref_root(POISONED, 1, 0).best
    one = run(backend, POISONED, 1, 1)
    assert one.best != "d1d5" and one.best == ref_root(POISONED, 1, 1).best
    by = dict(zip(one.moves, one.scores))
    assert by["d1d5"] < 0 <= one.score  # (the queen is lost one ply behind the horizon)
    for q in (0, 1, 2, 3):
        assert run(backend, HANGING_QUEEN, 1, q).best == "d1d5" and run(backend, HANGING_QUEEN, 1, q).score > 400
    r = run(backend, BACK_RANK, 1, 2)
    assert r.score == MATE - 3 == ref_root(BACK_RANK, 1, 2).score
    mating = [i for i, v in enumerate(r.scores) if v == r.score]
    assert 0 < len(mating) < r.n_moves
    assert A.candidates(r, 2 * MATE) == mating  # (MATE - depth would let the margin, and with it every move, in: the mate lies at ply 3)
    assert r.score < MATE - r.depth and r.score >= MATE - (r.depth + r.quiesce)
    rng = np.random.RandomState(3)
    assert {A.pick(r, 2 * MATE, rng) for _ in range(16)} == {r.move_words[i] for i in mating}


def _raw(backend, fens, depth, q, capacity=256):
    """The bytes of one raw call: bo_anchor_q, or bo_anchor if q is None."""
    lib = H.emu_lib() if backend == "emu" else E.load_hip_library()
    arr = (C.c_char_p * len(fens))(*[f.encode() for f in fens])
    out = (A.BoAnchorResult * len(fens))()
    words = np.zeros((len(fens), A.MAX_MOVES), np.int32)
    vals = np.zeros((len(fens), A.MAX_MOVES), np.int32)
    splits = C.c_int64(-1)
    tail = (capacity, 0, C.addressof(out), words.ctypes.data, vals.ctypes.data, C.byref(splits), None)
    rc = lib.bo_anchor(0, len(fens), arr, None, depth, *tail) if q is None else lib.bo_anchor_q(0, len(fens), arr, None, depth, q, *tail)
    assert rc == 0, lib.bo_last_error()
    return bytes(out), words.tobytes(), vals.tobytes(), splits.value


def check_q0(backend, fens, depths=(1, 2, 3)):
    """Check 4: bo_anchor_q(quiesce = 0) returns bo_anchor's bytes: results (nodes included), move words, scores and splits."""
    fens = tuple(fens)
    for d in depths:
        a, b = _raw(backend, fens, d, None), _raw(backend, fens, d, 0)
        assert a == b, d
        res = np.frombuffer(a[0], np.int32).reshape(len(fens), -1)
        assert (res[:, 4] > 0).any()  # (the batch is no row of terminal roots)


def check_chunking(backend, fens, depth, q, capacities):
    """Check 5: identical results, scores and nodes at every capacity; each of them must have split a level."""
    fens = tuple(fens)
    base = run(backend, fens, depth, q)
    assert base[0].splits == 0
    for cap in capacities:
        got = run(backend, fens, depth, q, capacity=cap)
        print(f"capacity {cap}: {got[0].splits} splits, {got[0].nodes} nodes")
        assert got[0].splits > 0, cap
        assert [AC.facts(r) for r in got] == [AC.facts(r) for r in base], cap
        assert got[0].nodes == base[0].nodes, cap


def check_batch_invariance(backend, fens, depth, q):
    """Check 6: each root alone equals the root inside the batch; FEN and bo_position input agree; two identical raw calls return
    identical bytes."""
    fens = tuple(fens)
    batch = run(backend, fens, depth, q)
    for f, r in zip(fens, batch):
        assert AC.facts(run(backend, f, depth, q)) == AC.facts(r), f
    as_pos = run(backend, fens, depth, q, as_positions=True)
    assert [AC.facts(r) for r in as_pos] == [AC.facts(r) for r in batch] and all(r.fen is None for r in as_pos)
    first = _raw(backend, fens, depth, q)
    assert first == _raw(backend, fens, depth, q)
    words = np.frombuffer(first[1], np.int32).reshape(len(fens), -1)
    vals = np.frombuffer(first[2], np.int32).reshape(len(fens), -1)
    for i, r in enumerate(batch):  # beyond n_moves: -1 and INT32_MIN
        assert words[i, :r.n_moves].tolist() == r.move_words and (words[i, r.n_moves:] == -1).all()
        assert vals[i, :r.n_moves].tolist() == r.scores and (vals[i, r.n_moves:] == -(1 << 31)).all()


# ---- the game loop and the command line ---------------------------------------------------------------------------------------------
def play(backend, openings, n_games, n_slots, sims, depth, q, max_game_moves):
    """(played, finished games by id, PGN text) of a match of tests/fake_model.py's net against anchor(depth, quiesce=q, margin 0)."""
    from betaone_amd import match as M

    dev = "cpu" if backend == "emu" else "cuda:0"

    def go():
        ro = A.AnchorRollout(AC._net(), n_slots, depth, 0, quiesce=q, num_simulations=sims, mcts_batch_size=8, max_game_moves=max_game_moves,
                             temperature=(2, 1.0, 0.1), device=dev, use_graph=False)
        fins = {}
        try:
            played = M.play_match(ro, M.MatchScheduler(openings, n_games, n_slots, 1), step_of=lambda s: 0, finished=fins)
        finally:
            ro.close()
        f = io.StringIO()
        M.write_match_pgn(f, played, fins, A.anchor_name(depth, 0, q), "fake", device=dev, date="2026.01.02")
        return played, fins, f.getvalue()

    if backend == "emu":
        with H.emulator_backend():
            return go()
    return go()


def check_games(n_games, depth, q, played, fins, text):
    """Check 8: every anchor ply of the match is the reference's pick for its root; the PGN names the anchor with its quiescence."""
    games = played["games"]
    assert sorted(g["game_id"] for g in games) == list(range(n_games))
    anchor_plies = 0
    for g in games:
        fin = fins[g["game_id"]]
        pre = len(g["prefix"].split())
        board = O.Board(g["fen"])
        for i, w in enumerate(fin.moves):
            uci = E.move_to_uci(w)
            if i >= pre:
                anchor = (board.pos.turn == 1) == (g["white"] == "A")
                assert (len(fin.pis[i - pre][0]) == 0) == anchor, (g["game_id"], i)
                if anchor:
                    anchor_plies += 1
                    assert uci == ref_root(board.fen(), depth, q).best, (g["game_id"], i, uci, board.fen())
            board.push(O.move_from_uci(uci))
    assert anchor_plies >= n_games
    name = f"anchor(depth={depth},quiesce={q},margin=0)"
    assert A.anchor_name(depth, 0, q) == name and text.count(f"A ({name})") == n_games
    return anchor_plies


def check_cli_best(backend, fen, depth, q):
    """`anchor best --quiesce Q` as JSON and as text."""
    want = ref_root(fen, depth, q)
    rc, text = AC.cli(backend, ["best", fen, "--depth", str(depth), "--quiesce", str(q), "--json"])
    d = json.loads(text)
    assert rc == 0 and (d["best"], d["score"], d["n_best"], d["nodes"], d["quiesce"]) == (want.best, want.score, want.n_best, want.entries, q)
    rc, text = AC.cli(backend, ["best", fen, "--depth", str(depth), "--quiesce", str(q), "--scores"])
    lines = text.splitlines()
    assert rc == 0 and lines[0].startswith(f"Best {want.best} (") and f"score {want.score})" in lines[0]
    assert lines[1] == " ".join(f"{m} {v}" for m, v in zip(want.moves, want.scores))
    assert lines[2].startswith(f"depth {depth}, quiesce {q}: {want.entries} nodes, ")
    rc, text = AC.cli(backend, ["best", fen, "--depth", str(depth), "--json"])  # without the option: no key, today's search
    d = json.loads(text)
    assert rc == 0 and "quiesce" not in d and (d["best"], d["score"], d["nodes"]) == (AC.ref_root(fen, depth).best, AC.ref_root(fen, depth).score,
                                                                                      AC.ref_root(fen, depth).entries)


def check_cli_match(backend, tmp_path, depth, q):
    """`anchor match --quiesce Q` through main with a hash-initialised checkpoint: the summary, the JSON and the PGN carry the new name,
    and with margin 0 every anchor move of the JSON's games is the reference's pick."""
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
    book.write_text(f"{POISONED}\n")
    rc, text = AC.cli(backend, ["match", str(ckpt), "--depth", str(depth), "--quiesce", str(q), "--games", "2", "--slots", "2", "--sims", "8",
                                "--mcts-batch", "8", "--openings", str(book), "--max-game-moves", "6", "--out", str(out), "--pgn", str(pgn)])
    print(text)
    assert rc == 0
    name = f"anchor(depth={depth},quiesce={q},margin=0)"
    lines = text.splitlines()
    assert lines[0].endswith(f" vs {name}") and re.match(r"^\[anchor\] net vs " + re.escape(name) + r": \+\d+ =\d+ -\d+  score \d\.\d{3}  ", lines[-1])
    d = json.loads(out.read_text())
    assert d["a"] == name and d["settings"]["quiesce"] == q and d["summary"]["games"] == 2 and len(d["games"]) == 2
    assert pgn.read_text().count(f"A ({name})") == 2
    n = 0
    for g in d["games"]:
        board = O.Board(g["fen"])
        for uci in g["moves"]:
            if (board.pos.turn == 1) == (g["white"] == "A"):
                n += 1
                assert uci == ref_root(board.fen(), depth, q).best, (g["game_id"], uci, board.fen())
            board.push(O.move_from_uci(uci))
    assert n >= 2
