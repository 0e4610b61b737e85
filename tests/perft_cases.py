"""tests/perft_cases.py -- checks of perft on the device (betaone_amd/perft.py, csrc/bo_perft.h), shared by the wave-emulator tests
(test_perft_emu.py) and the MI355X tests (test_perft_gpu.py): the same bodies, parameterised by backend ("emu" / "hip").

The references: the published node counts (test_oracle_rules.PERFT), and a plain Python walk over the oracle's rules (oracle_walk) for
the move statistics and the ORDER checksum -- the walk hashes the oracle's ordered move lists, so a device list that holds the right
moves in another order fails it.  Agreement with the oracle is not agreement with python-chess (test_oracle_rules.py says what pins the
oracle's own order)."""
import ctypes as C
import functools

import numpy as np

import engine_harness as H
from betaone_amd import perft as P
from oracle import oracle as O
from test_oracle_rules import PERFT

START, KIWIPETE, POS3, POS5 = PERFT[0][0], PERFT[1][0], PERFT[2][0], PERFT[5][0]
EP_EVASION = "8/8/8/2k5/3Pp3/8/8/4K3 b - d3 0 1"      # black is in check from the pawn that just came to d4: exd3 e.p. takes the checker
PROMO_CHECK = "1n2k3/P1P5/8/8/8/8/8/4K3 w - - 0 1"     # promotions and capture-promotions, with check
STATS_FENS = [KIWIPETE, POS3, POS5, EP_EVASION, PROMO_CHECK]
MATED = "k6R/8/1K6/8/8/8/8/8 b - - 1 1"
STALEMATED = "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"
MASK = (1 << 64) - 1
FNV_BASIS, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3


@functools.lru_cache(maxsize=None)
def run(backend, fens, depth, divide=False, stats=False, order=False, capacity=P.DEFAULT_CAPACITY):
    """P.perft on the backend; `fens` a FEN or a tuple of FENs.  Cached: a result is computed once and shared (nobody changes it)."""
    f = list(fens) if isinstance(fens, tuple) else fens
    kw = dict(divide=divide, stats=stats, order=order, capacity=capacity)
    if backend == "emu":
        with H.emulator_backend():
            res = P.perft(f, depth, device="cpu", **kw)
    else:
        res = P.perft(f, depth, device="cuda:0", **kw)
    return res if isinstance(fens, tuple) else res[0]


def word(m) -> int:
    return m.from_sq | m.to_sq << 6 | m.promo << 12


@functools.lru_cache(maxsize=None)
def oracle_walk(fen, depth):
    """(nodes, stats, checksum) of perft(depth) by a walk over the oracle's rules, with the definitions of include/betaone_engine.h:
    stats over the positions at `depth` (captures / en passant / castles / promotions: the LAST move; checks, checkmates, stalemates:
    the position), checksum = sum mod 2^64 over the positions at depth 0 .. depth - 1 of the FNV-1a hash of the ordered move list."""
    L = O.lib()
    st = dict.fromkeys(P.STAT_NAMES, 0)
    acc = [0, 0]  # nodes, checksum
    if depth == 0:
        return 1, st, 0
    kid, kid_moves = O.Pos(), (O.Move * O.MAX_MOVES)()
    kid_ref, size = C.byref(kid), C.sizeof(O.Pos)

    def rec(p, d):
        arr = (O.Move * O.MAX_MOVES)()
        p_ref = C.byref(p)
        n = L.bo_legal_moves(p_ref, arr)
        raw = np.frombuffer(arr, dtype=np.uint8, count=4 * n).reshape(n, 4).astype(np.int64)
        words = (raw[:, 0] | raw[:, 1] << 6 | raw[:, 2] << 12).tolist()
        h = FNV_BASIS
        for w in words:
            h = ((h ^ w) * FNV_PRIME) & MASK
        acc[1] = (acc[1] + h) & MASK
        if d > 1:
            for i in range(n):
                c = p.copy()
                L.bo_push(C.byref(c), arr[i])
                rec(c, d - 1)
            return
        acc[0] += n
        their, occ = p.occ[1 - p.turn], p.occ[0] | p.occ[1]
        for i, w in enumerate(words):
            frm, to = w & 63, (w >> 6) & 63
            ep = bool(p.pawns >> frm & 1) and to == p.ep_square and (frm & 7) != (to & 7) and not occ >> to & 1
            st["captures"] += 1 if (their >> to & 1) or ep else 0
            st["en_passant"] += 1 if ep else 0
            st["castles"] += 1 if (p.kings >> frm & 1) and abs((to & 7) - (frm & 7)) == 2 else 0
            st["promotions"] += 1 if w >> 12 else 0
            C.memmove(kid_ref, p_ref, size)
            L.bo_push(kid_ref, arr[i])
            chk = L.bo_is_check(kid_ref) != 0
            none = L.bo_legal_moves(kid_ref, kid_moves) == 0
            st["checks"] += 1 if chk else 0
            st["checkmates"] += 1 if chk and none else 0
            st["stalemates"] += 1 if none and not chk else 0

    board = O.Board(fen)  # (alive while its position is copied)
    rec(board.pos.copy(), depth)
    return acc[0], st, acc[1]


def check_counts_and_divide(backend, fen, expected, depths):
    """Published counts; every divide sums to its total; the divide moves are the oracle's legal moves of the root in order; each
    divide count is the oracle's perft(d - 1) after that move."""
    b = O.Board(fen)
    legal = b.legal_moves()
    for d in depths:
        r = run(backend, fen, d, divide=True)
        assert r.nodes == expected[d - 1], (fen, d, r.nodes)
        assert sum(n for _, n in r.moves) == r.nodes, (fen, d)
        assert [u for u, _ in r.moves] == [O.move_to_uci(m) for m in legal], (fen, d)
        for (u, n), m in zip(r.moves, legal):
            b.push(m)
            want = b.perft(d - 1)
            b.pop()
            assert n == want, (fen, d, u, n, want)


def check_stats_and_order(backend, fen, depth):
    r = run(backend, fen, depth, divide=True, stats=True, order=True)
    nodes, st, cs = oracle_walk(fen, depth)
    print(f"{fen} depth {depth}: nodes {r.nodes} stats {r.stats} checksum {r.checksum:#018x} (oracle {nodes} {st} {cs:#018x})")
    assert r.nodes == nodes, (fen, depth)
    assert r.stats == st, (fen, depth, r.stats, st)
    assert r.checksum == cs, (fen, depth)


def same_result(a, b):
    assert (a.nodes, a.moves, a.stats, a.checksum) == (b.nodes, b.moves, b.stats, b.checksum), (a, b)
