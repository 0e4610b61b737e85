"""tests/mate_cases.py -- checks of the forced-mate solver on the device (betaone_amd/mate.py, csrc/bo_mate.h), shared by the
wave-emulator tests (test_mate_emu.py) and the MI355X tests (test_mate_gpu.py): the same bodies, parameterised by backend.

The reference is a definitional minimax over the oracle's rules (bo_legal_moves / bo_push / bo_is_check, the calls
perft_cases.oracle_walk uses): the value of a move is 1 if it mates, nothing if it stalemates, otherwise the maximum over the replies of
dtm + 2 if every reply is a proven mate within the budget, else 0; dtm of a position is the minimum over its moves' values, 0 if there
is none; the key moves are the moves that achieve it.  Draw rules are ignored on both sides.  Every comparison is of exact integers.
The expected figures are recomputed here, never pinned; a set only asserts that the reference finds each class it is there for."""
import ctypes as C
import functools
import types

import numpy as np

import engine_harness as H
from betaone_amd import engine as E
from betaone_amd import mate as M
from betaone_amd import records as R
from oracle import oracle as O
from test_oracle_rules import PERFT

KRK = "7k/8/5K2/8/8/8/8/R7 w - - 0 1"
KQK = "8/8/8/8/8/5K2/Q7/7k w - - 0 1"
SMOTHERED = "r2qkb1r/pp2nppp/3p4/2pNN1B1/2BnP3/3P4/PPP2PPP/R2bK2R w KQkq - 1 10"
EP_MATE = "8/5K1k/8/5Pp1/8/8/8/B1B5 w - g6 0 1"        # the en-passant capture is the only mate in 1
EP_GONE = "8/5K1k/8/5Pp1/8/8/8/B1B5 w - - 0 1"         # the same without the right: nothing within 2
STALE_TRAP = "8/5P1k/5K2/8/8/8/8/8 w - - 0 1"          # f8=Q is stalemate and must not count; dtm 3
PROMO_KEYS = "k7/2P5/1K6/8/8/8/8/8 w - - 0 1"          # mate in 1 by more than one promotion
KPK_5 = "k7/2K5/1P6/8/8/8/8/8 w - - 0 1"               # few moves a side: the cheapest walk to depth 5
MATED = "k6R/8/1K6/8/8/8/8/8 b - - 1 1"
STALEMATED = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
START = PERFT[0][0]
POS4, POS5 = PERFT[3][0], PERFT[5][0]
_CLOCKS = 8  # the last bytes of O.Pos: the two clocks, which no rule here reads


def word(m) -> int:
    return m.from_sq | m.to_sq << 6 | m.promo << 12


# ---- the reference ------------------------------------------------------------------------------------------------------------------
_memo = {}
_visited = [0]


def _moves(p):
    arr = (O.Move * O.MAX_MOVES)()
    n = O.lib().bo_legal_moves(C.byref(p), arr)
    return arr, n


def _after(p, m):
    c = p.copy()
    O.lib().bo_push(C.byref(c), m)
    return c


def ref_move_values(p, n):
    """Per legal move of p (oracle order): 1 it mates; 0 it stalemates or is not proven within n moves; else its distance."""
    L = O.lib()
    arr, k = _moves(p)
    _visited[0] += 1
    out, kids = [], []
    for i in range(k):
        c = _after(p, arr[i])
        if _moves(c)[1] == 0:
            out.append(1 if L.bo_is_check(C.byref(c)) else 0)
        else:
            out.append(None)
            kids.append((i, c))
    if n == 1 or 1 in out:  # (a mate in 1: the other moves' values are not asked for -- they are no keys)
        return [v or 0 for v in out]
    for i, c in kids:
        arr2, k2 = _moves(c)
        worst = 0
        for j in range(k2):
            d = ref_dtm(_after(c, arr2[j]), n - 1)
            if d == 0:
                worst = 0
                break
            worst = max(worst, d + 2)
        out[i] = worst
    return out


def ref_dtm(p, n) -> int:
    key = (bytes(p)[:-_CLOCKS], n)
    if key not in _memo:
        _memo[key] = min((v for v in ref_move_values(p, n) if v), default=0)
    return _memo[key]


@functools.lru_cache(maxsize=None)
def ref_root(fen, n):
    """What the solver must return for the root: status, dtm, n_moves, keys (UCI, oracle order), and the reference's own cost."""
    board = O.Board(fen)  # (alive while its position is copied)
    p = board.pos.copy()
    arr, k = _moves(p)
    if k == 0:
        return types.SimpleNamespace(status="checkmated" if O.lib().bo_is_check(C.byref(p)) else "stalemated", dtm=0, n_moves=0, keys=[], cost=1)
    before = _visited[0]
    dtm, keys = 0, []
    for it in range(1, n + 1):  # (the smallest budget that proves it: what `searched` reports)
        vals = ref_move_values(p, it)
        dtm = min((v for v in vals if v), default=0)
        if dtm:
            keys = [O.move_to_uci(arr[i]) for i in range(k) if vals[i] == dtm]
            break
    return types.SimpleNamespace(status="ok", dtm=dtm, n_moves=k, keys=keys, cost=_visited[0] - before + 1)


@functools.lru_cache(maxsize=None)
def below(fen, plies):
    """The FEN of every position `plies` plies below fen, in the oracle's move order (transpositions are kept: a batch may hold
    the same root twice)."""
    out = []

    def rec(b, d):
        if d == 0:
            out.append(b.fen())
            return
        for m in b.legal_moves():
            b.push(m)
            rec(b, d - 1)
            b.pop()

    rec(O.Board(fen), plies)
    return tuple(out)


def classes(fens, n):
    """{dtm: number of roots} by the reference (statuses other than ok under their name)."""
    out = {}
    for f in fens:
        r = ref_root(f, n)
        k = r.dtm if r.status == "ok" else r.status
        out[k] = out.get(k, 0) + 1
    return out


def cheapest(fens, n, per_class, want):
    """A subset the emulator can afford: of each class in `want` (dtm values) the `per_class` roots the reference spent least on."""
    out = []
    for d in want:
        have = sorted((f for f in set(fens) if ref_root(f, n).status == "ok" and ref_root(f, n).dtm == d), key=lambda f: (ref_root(f, n).cost, f))
        assert have, (d, "the reference finds no root of this class")
        out += have[:per_class]
    return tuple(out)


# ---- the device ---------------------------------------------------------------------------------------------------------------------
def to_bo_positions(fens):
    arr = (E.BoPosition * len(fens))()
    for i, f in enumerate(fens):
        board = O.Board(f)
        p = board.pos
        for k, v in enumerate([p.pawns, p.knights, p.bishops, p.rooks, p.queens, p.kings, p.occ[1], p.occ[0]]):
            arr[i].bb[k] = v
        c = p.castling
        arr[i].turn = p.turn
        arr[i].castling = (1 if c & (1 << 7) else 0) | (2 if c & 1 else 0) | (4 if c & (1 << 63) else 0) | (8 if c & (1 << 56) else 0)
        arr[i].ep_square, arr[i].ep_key = p.ep_square, -2
        arr[i].halfmove_clock, arr[i].fullmove_number = p.halfmove_clock, p.fullmove_number
    return arr


@functools.lru_cache(maxsize=None)
def run(backend, fens, n, pv=False, capacity=M.DEFAULT_CAPACITY, max_nodes=0, as_positions=False):
    """M.mate on the backend; `fens` a FEN or a tuple of FENs.  Cached: a result is computed once and shared (nobody changes it)."""
    f = list(fens) if isinstance(fens, tuple) else [fens]
    roots = to_bo_positions(f) if as_positions else f
    kw = dict(pv=pv, capacity=capacity, max_nodes=max_nodes)
    if backend == "emu":
        with H.emulator_backend():
            res = M.mate(roots, n, device="cpu", **kw)
    else:
        res = M.mate(roots, n, device="cuda:0", **kw)
    return res if isinstance(fens, tuple) else res[0]


def facts(r):
    """What two runs of a root must agree on (everything but the call's own nodes, splits and time)."""
    return (r.status, r.dtm, r.searched, r.n_moves, r.key, tuple(r.keys), None if r.pv is None else tuple(r.pv))


def check_values(backend, fens, n, **kw):
    """Check 1: dtm, n_keys, the key-move set, status, key and searched of every root against the reference."""
    fens = tuple(fens)
    res = run(backend, fens, n, **kw)
    print(f"{len(fens)} roots, N {n}: reference {classes(fens, n)}, {res[0].nodes} nodes, {res[0].splits} splits, {res[0].seconds:.3f} s")
    for f, r in zip(fens, res):
        want = ref_root(f, n)
        assert r.status == want.status, (f, r.status, want.status)
        assert (r.dtm, r.n_moves) == (want.dtm, want.n_moves), (f, r.dtm, want.dtm, r.n_moves, want.n_moves)
        assert r.keys == want.keys and len(r.keys) == len(r.key_words), (f, r.keys, want.keys)  # (same moves in the same order)
        assert r.key == (want.keys[0] if want.keys else None), (f, r.key)
        if want.status == "ok":
            assert r.searched == (r.mate_in if r.dtm else n), (f, r.searched)
        else:
            assert r.searched == 0 and r.dtm == 0, f
    return res


def check_pv(backend, fens, n, **kw):
    """Check 5: the line of every solved root is legal, has length dtm, ends in checkmate; every attacker move is a reference key move
    at the remaining distance and every reply has the reference's maximal remaining distance."""
    fens = tuple(fens)
    res = run(backend, fens, n, pv=True, **kw)
    L = O.lib()
    solved = 0
    for f, r in zip(fens, res):
        plain = ref_root(f, n)
        assert (r.dtm, r.keys) == (plain.dtm, plain.keys), f
        if not r.dtm:
            assert r.pv == [], f
            continue
        solved += 1
        assert len(r.pv) == r.dtm, (f, r.pv)
        board = O.Board(f)
        for ply, u in enumerate(r.pv):
            left = r.dtm - ply  # plies to mate before this move
            legal = board.legal_moves()
            ucis = [O.move_to_uci(m) for m in legal]
            assert u in ucis, (f, ply, u)
            p = board.pos.copy()
            if ply % 2 == 0:
                vals = ref_move_values(p, (left + 1) // 2)
                assert min(v for v in vals if v) == left and vals[ucis.index(u)] == left, (f, ply, u, vals)
                assert u == ucis[vals.index(left)], (f, ply, u, "not the lowest-index key move")
            else:
                ds = [ref_dtm(_after(p, m), left // 2) for m in legal]
                assert all(ds) and max(ds) == left - 1 and ds[ucis.index(u)] == left - 1, (f, ply, u, ds)
                assert u == ucis[ds.index(left - 1)], (f, ply, u, "not the lowest-index longest reply")
            board.push(u)
        end = board.pos.copy()
        assert _moves(end)[1] == 0 and L.bo_is_check(C.byref(end)), (f, r.pv)
    assert solved, "no solved root in the set"


def check_chunking(backend, fens, n, capacities, need_splits):
    """Check 2: identical results at every capacity; the capacities in need_splits must have split a level."""
    fens = tuple(fens)
    base = run(backend, fens, n)
    for cap in capacities:
        got = run(backend, fens, n, capacity=cap)
        print(f"capacity {cap}: {got[0].splits} splits, {got[0].nodes} nodes")
        if cap in need_splits:
            assert got[0].splits > 0, cap
        assert [facts(r) for r in got] == [facts(r) for r in base], cap
        assert got[0].nodes == base[0].nodes, cap


def check_batch_invariance(backend, fens, n):
    """Check 3: each root alone gives what it gives inside the batch; FEN input and bo_position input agree."""
    fens = tuple(fens)
    batch = run(backend, fens, n)
    cl = classes(fens, n)
    assert cl.get(1) and len(cl) > 1, cl  # (some roots resolve at n = 1 and drop out while others go on)
    for f, r in zip(fens, batch):
        assert facts(run(backend, f, n)) == facts(r), f
    as_pos = run(backend, fens, n, as_positions=True)
    assert [facts(r) for r in as_pos] == [facts(r) for r in batch]
    assert all(r.fen is None for r in as_pos)


def check_budget(backend, fens, n):
    """Check 4: max_nodes = 1 stops the call after the first iteration; two identical calls return identical bytes."""
    fens = tuple(fens)
    cl = classes(fens, n)
    assert cl.get(1) and any(k != 1 for k in cl), cl
    res = run(backend, fens, n, max_nodes=1)
    for f, r in zip(fens, res):
        want = ref_root(f, n)
        assert r.searched == 1, (f, r.searched)
        if want.dtm == 1:
            assert (r.dtm, r.keys) == (1, want.keys), f
        else:
            assert r.dtm == 0 and r.keys == [] and r.key is None, f
    assert res[0].nodes == len(fens)

    def raw():
        lib = H.emu_lib() if backend == "emu" else E.load_hip_library()
        arr = (C.c_char_p * len(fens))(*[f.encode() for f in fens])
        out = (M.BoMateResult * len(fens))()
        keys = np.full((len(fens), M.MAX_MOVES), -1, np.int32)
        line = np.full((len(fens), 2 * n - 1), -1, np.int32)
        splits = C.c_int64(-1)
        assert lib.bo_mate(0, len(fens), arr, None, n, 256, 0, M.PV, C.addressof(out), keys.ctypes.data, line.ctypes.data, C.byref(splits), None) == 0
        return bytes(out), keys.tobytes(), line.tobytes(), splits.value

    assert raw() == raw()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def cli(backend, argv):
    """(exit status, output) of python -m betaone_amd.mate's main on the backend."""
    import io

    out = io.StringIO()
    dev = ["--device", "cpu" if backend == "emu" else "cuda:0"]
    if backend == "emu":
        with H.emulator_backend():
            rc = M.main(list(argv) + dev, out)
    else:
        rc = M.main(list(argv) + dev, out)
    return rc, out.getvalue()


EPD_ROOT = KRK  # mate in 2 with two key moves, Kg6 and Kf7


def check_epd(backend, tmp_path):
    """Check 7a: a solved `dm 2` line with the right bm, a wrong dm, a wrong bm, a non-unique solution."""
    want = ref_root(STALE_TRAP, 2)
    assert want.dtm == 3 and want.keys == ["f7f8r"]
    two = ref_root(EPD_ROOT, 2)
    assert two.dtm == 3 and sorted(two.keys) == ["f6f7", "f6g6"]
    epd = tmp_path / "suite.epd"
    epd.write_text("# a mate suite\n"
                   f"{' '.join(STALE_TRAP.split()[:4])} dm 2; bm f8=R; id \"underpromotion\";\n"
                   f"{' '.join(STALE_TRAP.split()[:4])} dm 1; bm f8=R;\n"
                   f"{' '.join(STALE_TRAP.split()[:4])} dm 2; bm f8=Q+;\n"
                   f"{EPD_ROOT} dm 2; bm Kg6 f6f7;\n")
    rc, text = cli(backend, ["--epd", str(epd), "--moves", "2"])
    print(text)
    lines = text.splitlines()
    assert rc == 1 and len(lines) == 5
    assert ":2: ok " in lines[0] and "mate in 2, key f7f8r, unique" in lines[0]
    assert ":3: FAIL " in lines[1] and "mate in 2 (expected dm 1)" in lines[1]
    assert ":4: FAIL " in lines[2] and "bm f8=Q+ not among the key moves f7f8r" in lines[2]
    assert ":5: ok " in lines[3] and "not unique (2 keys)" in lines[3]
    assert lines[4].startswith("2 of 4 lines solved as stated")
    good = tmp_path / "good.epd"
    good.write_text(f"{EPD_ROOT} dm 2; bm Kf7;\n")
    rc, text = cli(backend, ["--epd", str(good)])
    assert rc == 0 and text.splitlines()[0].count(": ok ") == 1


def _game(gid, fen, ucis, outcome, terminal, pi_on):
    """A record of the oracle-played line `ucis` from fen; the pi of ply i is one entry on pi_on[i] (UCI), or on the played move."""
    b = O.Board(fen)
    fens, moves, pis = [b.fen()], [], []
    for i, u in enumerate(ucis):
        m = O.move_from_uci(u)
        assert u in [O.move_to_uci(x) for x in b.legal_moves()], (fen, i, u)
        target = O.move_from_uci(pi_on[i]) if pi_on and pi_on[i] else m
        pis.append((np.array([O.move_to_index(target)], np.int32), np.array([1.0], np.float32)))
        moves.append(word(m))
        b.push(m)
        fens.append(b.fen())
    game = types.SimpleNamespace(game_id=gid, terminal=terminal, outcome=float(outcome), moves=moves, positions=list(to_bo_positions(fens)),
                                 pis=pis, root_values=None)
    return game, fens


AUDIT_GAMES = (
    # the attacker plays a key move of the mate in 2 and wins (the pi of the first ply sits on the other key move)
    (KRK, ("f6g6", "h8g8", "a1a8"), 1.0, 1, ("f6f7", None, None)),
    # it misses the mate (the pi on the move played) and the game is drawn
    (KRK, ("a1a2", "h8g8", "a2a3"), 0.0, 0, None),
    # black has a choice and walks into a mate in 1; white gives it
    ("5k2/8/6K1/8/8/8/8/R7 b - - 0 1", ("f8g8", "a1a8"), 1.0, 1, None),
)


def check_audit(backend, tmp_path):
    """Check 7b: the audit's counts over three games against the reference."""
    n = 2
    games, lines = [], []
    for gid, (fen, ucis, outcome, terminal, pi_on) in enumerate(AUDIT_GAMES):
        g, fens = _game(50 + gid, fen, ucis, outcome, terminal, pi_on)
        games.append(g)
        lines.append((g, fens, ucis, outcome, pi_on))
    d = tmp_path / "data" / "iter_3"
    R.save_games(str(d / "games_rank0.bog"), games)
    want = {k: 0 for k in M.AUDIT_KEYS}
    by = {1: dict(want), 2: dict(want)}
    for g, fens, ucis, outcome, pi_on in lines:
        for i, u in enumerate(ucis):
            r, nxt = ref_root(fens[i], n), ref_root(fens[i + 1], n)
            if nxt.dtm:
                for b in (want, by[(nxt.dtm + 1) // 2]):
                    b["allowed"] += 1
            if not r.dtm:
                continue
            white = fens[i].split()[1] == "w"
            pi_u = pi_on[i] if pi_on and pi_on[i] else u
            for b in (want, by[(r.dtm + 1) // 2]):
                b["forced"] += 1
                b["played_key"] += 1 if u in r.keys else 0
                b["pi_top_key"] += 1 if pi_u in r.keys else 0
                b["pi_mass_on_keys"] += 1.0 if pi_u in r.keys else 0.0
                b["contradicted"] += 1 if (outcome if white else -outcome) <= 0 else 0
    print("reference:", want, by)
    assert want["forced"] >= 3 and 0 < want["played_key"] < want["forced"] and want["contradicted"] >= 1 and want["allowed"] >= 2
    assert by[1]["forced"] and by[2]["forced"] and 0 < want["pi_top_key"] < want["forced"]
    out_json = tmp_path / "audit.json"
    rc, text = cli(backend, ["audit", str(d), "--moves", str(n), "--json", str(out_json)])
    print(text)
    import json

    rep = json.loads(out_json.read_text())
    assert rc == 0 and rep["games"] == 3 and rep["records"] == sum(len(x[2]) for x in lines) and rep["files"] == 1
    assert rep["total"] == want and {int(k): v for k, v in rep["by_mate_in"].items()} == by
    assert f"contradicted targets {want['contradicted']}, allowed mates {want['allowed']}" in text.splitlines()[-1]
    assert [bytes(g["positions"]) for g in R.load_games(str(d / "games_rank0.bog"))] == [b"".join(bytes(p) for p in g.positions) for g in games]
