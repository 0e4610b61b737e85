"""tests/symmetry_cases.py -- TEST HELPER for tests/test_symmetry_emu.py (wave emulator) and tests/test_symmetry_gpu.py (MI355X): board
symmetries in the replay samplers (csrc/bo_sym.h; GpuReplayBuffer.batch*(sym=...), loader(augment=...), train --augment,
validate --symmetry).  The bodies run on "cpu" under the emulator and on "cuda:0".

The oracle knows nothing of the bit tricks: it is the TRANSFORMED GAME PLAYED OUT.  The FEN and the UCI moves of a game are transformed
as text (flip_fen / mirror_fen / t_uci below), the game is replayed by the oracle's chess shim (pgn_util.chess), packed, added to a
buffer of its own and sampled PLAIN.  The pi indices are mapped by a table this file builds itself (action_table): an index is decoded
to its from square and its direction VECTOR, both are reflected, and the result is encoded again by the reference's move_to_index rule
restated here (m2i); the table is checked against m2i on all 1968 geometric (from, to, promotion) moves.

What may differ between sample(G, sym = colour) and sample(G'): plane 118, the fullmove number -- a game in which black moved first
counts one ahead on alternate plies, and the sampler keeps the record's own number.  Everything else is compared byte for byte."""
from __future__ import annotations

import ctypes as C
import functools
import json
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import merge_cases as MC
import value_mix_cases as VM

A = 4672
BO_E_ARG = -1
W = 4                     # the buffers' pi_width: rows of 1, 2 and 4 entries
START = MC.START
Q = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]     # (d rank, d file): N NE E SE S SW W NW
K = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)]
P = [(-1, 1), (0, 1), (1, 1)]                                                    # (d file, d rank towards promotion)
SAMPLERS = ("dense", "sparse", "sparse_q", "merged")


# ---- the move codec, restated, and the table ------------------------------------------------------------------------------------------

def m2i(fr, to, promo):
    """utils.move_to_index: promo None, or python-chess's piece type 2..5."""
    fr_r, fr_f, to_r, to_f = fr >> 3, fr & 7, to >> 3, to & 7
    dr, df = to_r - fr_r, to_f - fr_f
    if promo and promo != 5:
        d = P.index((df, dr)) if fr_r == 6 else P.index((df, -dr))
        return fr * 73 + 64 + (promo - 2) * 3 + d
    if (abs(dr), abs(df)) in ((1, 2), (2, 1)):
        return fr * 73 + 56 + K.index((dr, df))
    sr, sf = (dr > 0) - (dr < 0), (df > 0) - (df < 0)
    return fr * 73 + Q.index((sr, sf)) * 7 + max(abs(dr), abs(df)) - 1


def t_square(sq, t):
    return sq ^ (56 if t & 1 else 0) ^ (7 if t & 2 else 0)


@functools.lru_cache(maxsize=None)
def action_table(t):
    """table[a] = the index of the twin of move a: the from square reflected, the direction vector reflected (d rank -> -d rank under
    the colour flip, d file -> -d file under the file mirror; an underpromotion's direction is relative to the pawn's colour, so only
    the file mirror turns it), encoded again."""
    sr, sf = (-1 if t & 1 else 1), (-1 if t & 2 else 1)
    table = np.empty(A, dtype=np.int64)
    for a in range(A):
        fr, p = divmod(a, 73)
        if p < 56:
            dr, df = Q[p // 7]
            p2 = Q.index((sr * dr, sf * df)) * 7 + p % 7
        elif p < 64:
            dr, df = K[p - 56]
            p2 = 56 + K.index((sr * dr, sf * df))
        else:
            piece, d = divmod(p - 64, 3)
            p2 = 64 + 3 * piece + P.index((sf * P[d][0], P[d][1]))
        table[a] = t_square(fr, t) * 73 + p2
    return table


def geometric_moves():
    out = []
    for fr in range(64):
        for to in range(64):
            dr, df = (to >> 3) - (fr >> 3), (to & 7) - (fr & 7)
            if fr == to or not ((abs(dr), abs(df)) in ((1, 2), (2, 1)) or dr == 0 or df == 0 or abs(dr) == abs(df)):
                continue
            last = ((fr >> 3) == 6 and (to >> 3) == 7 or (fr >> 3) == 1 and (to >> 3) == 0) and abs(df) <= 1
            out += [(fr, to, pr) for pr in ((None, 5, 2, 3, 4) if last else (None,))]
    return out


def check_tables():
    """The test's table against the codec on every geometric move, and the product's host-side permutation against the table."""
    from betaone_amd import symmetry as S

    moves = geometric_moves()
    assert len(moves) == 1968
    for t in (0, 1, 2, 3):
        tab = action_table(t)
        assert sorted(tab.tolist()) == list(range(A)) and (tab[tab] == np.arange(A)).all()
        for fr, to, pr in moves:
            assert tab[m2i(fr, to, pr)] == m2i(t_square(fr, t), t_square(to, t), pr), (fr, to, pr, t)
        assert np.array_equal(S.action_permutation(t), tab)
    with pytest.raises(ValueError):
        S.action_permutation(4)
    assert S.transform_uci("a7b8b", 3) == t_uci("a7b8b", 3) == "h2g1b" and S.transform_uci("e2e4", 1) == "e7e5"
    for fen, _u, _t in SPECS:
        for t in (1, 2, 3):
            if t & 2 and fen.split()[2] != "-":
                with pytest.raises(ValueError):
                    S.transform_fen(fen, t)
            else:
                assert S.transform_fen(fen, t) == t_fen(fen, t)


# ---- text transforms ------------------------------------------------------------------------------------------------------------------

def t_uci(u, t):
    files, ranks = "abcdefgh", "12345678"
    sq = lambda f, r: (files[7 - files.index(f)] if t & 2 else f) + (ranks[7 - ranks.index(r)] if t & 1 else r)  # noqa: E731
    return sq(u[0], u[1]) + sq(u[2], u[3]) + u[4:]


def flip_fen(fen):
    board, turn, castling, ep, half, full = fen.split()
    board = "/".join(r.swapcase() for r in reversed(board.split("/")))
    castling = "-" if castling == "-" else "".join(c for c in "KQkq" if c.swapcase() in castling)
    ep = "-" if ep == "-" else ep[0] + "12345678"[7 - "12345678".index(ep[1])]
    return " ".join([board, "b" if turn == "w" else "w", castling, ep, half, full])


def mirror_fen(fen):
    board, turn, castling, ep, half, full = fen.split()
    assert castling == "-", "the file mirror of a position with castling rights is no chess position"
    board = "/".join(r[::-1] for r in board.split("/"))
    ep = "-" if ep == "-" else "abcdefgh"[7 - "abcdefgh".index(ep[0])] + ep[1]
    return " ".join([board, turn, castling, ep, half, full])


def t_fen(fen, t):
    fen = mirror_fen(fen) if t & 2 else fen
    return flip_fen(fen) if t & 1 else fen


# ---- the corpus -----------------------------------------------------------------------------------------------------------------------

# (FEN, the moves written by hand, plies of a seeded random tail)
SPECS = (
    # 0: white castles short, black long; both wings' rights are gone after ply 12
    (START, "e2e4 e7e5 g1f3 b8c6 f1c4 d7d6 e1g1 c8g4 d2d3 d8d7 b1c3 e8c8 c1e3 g8f6 h2h3 g4h5 a2a3 f8e7 f1e1 h8e8 d1d2 c8b8", 0),
    # 1: white castles long, black short
    (START, "d2d4 g8f6 b1c3 e7e6 c1g5 f8e7 d1d2 e8g8 e1c1 d7d5 e2e3 b8d7 g1f3 c7c5 f1d3 b7b6 h1e1 c8b7 c1b1 a8c8", 0),
    # 2: d7d5 can be taken en passant and is; e2e4 and d2d4 cannot
    (START, "e2e4 a7a6 e4e5 d7d5 e5d6 c7d6 d2d4 g8f6 g1f3 b8c6 f1d3 c8g4", 0),
    # 3: an underpromotion with capture, a promotion; no rights (a rook endgame)
    ("r1r3k1/1P3ppp/8/8/8/6P1/p4PKP/8 w - - 0 30", "b7a8n c8a8 g2f3 a2a1q f3e4 a1a4 e4e3 a4a3 e3e2", 6),
    # 4: a pawn endgame: a double push that can be taken en passant and is, a promotion
    ("8/p4k2/8/1P6/8/5K2/6PP/8 w - - 3 41", "f3e4 a7a5 b5a6 f7e6 a6a7 e6d6 a7a8q d6c5", 10),
    # 5: a rook endgame, black to move
    ("8/5pk1/R5p1/7p/7P/6P1/5PK1/1r6 b - - 5 45", "", 18),
    # 6: a middlegame whose kings have not moved but whose castling field is "-"
    ("r2qk2r/ppp2ppp/2npbn2/2b1p3/2B1P3/2NPBN2/PPP2PPP/R2QK2R w - - 4 8", "", 24),
    # 7: a knight shuffle: the start position three times, both repetition planes
    (START, "g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1 f6g8 e2e4 e7e5", 0),
    # 8: the same shuffle without rights: the repetition planes under the mirror
    ("4k1n1/pppp4/8/8/8/8/PPPP4/4K1N1 w - - 0 1", "g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1 f6g8 d2d4 d7d5", 0),
    # 9: four pi entries on every ply
    (START, "c2c4 e7e5 b1c3 g8f6 g2g3 d7d5 c4d5 f6d5 f1g2 d5b6", 4),
    # 10: black to move, all rights
    ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", "c7c5 g1f3", 12),
    # 11: the kings step out: no right after ply 4, then 24 plies in which the mirror applies
    (START, "e2e4 e7e5 e1e2 e8e7", 24),
)
NO_RIGHTS = (3, 4, 5, 6, 8)
WIDE = 9


def _line(fen, ucis, tail, seed):
    """The hand-written moves plus `tail` seeded random legal ones (none that ends the game)."""
    import pgn_util as U

    rng = random.Random(seed)
    b = U.chess.Board(fen)
    out = []
    for u in ucis.split():
        m = U.chess.Move.from_uci(u)
        assert b.is_legal(m), (fen, u)
        b.push(m)
        out.append(u)
    for _ in range(tail):
        legal = sorted(b.legal_moves, key=lambda m: m.uci())
        rng.shuffle(legal)
        for m in legal:
            b.push(m)
            if not b.is_game_over(claim_draw=True):
                break
            b.pop()
        else:
            raise AssertionError(f"{fen}: every move ends the game")
        out.append(m.uci())
    return out


def _replay(fen, ucis):
    """Positions (one more than moves), packed moves, and per ply what the properties below need, from the oracle's shim."""
    import engine_cases as EC
    import pgn_util as U

    b = U.chess.Board(fen)
    grab = lambda: EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1)  # noqa: E731
    pos, moves, info = [grab()], [], []
    for u in ucis:
        m = U.chess.Move.from_uci(u)
        assert b.is_legal(m), (fen, u)
        pawn = b.piece_type_at(m.from_square) == U.chess.PAWN
        info.append(SimpleNamespace(
            legal=sorted((x.from_square, x.to_square, x.promotion) for x in b.legal_moves), ep_square=b.ep_square, ep_legal=b.has_legal_en_passant(),
            ep_played=pawn and b.ep_square is not None and m.to_square == b.ep_square and (m.from_square & 7) != (m.to_square & 7),
            castle=b.piece_type_at(m.from_square) == U.chess.KING and abs((m.from_square & 7) - (m.to_square & 7)) == 2,
            white=bool(b.turn), wing="k" if (m.to_square & 7) > 4 else "q", promo=m.promotion,
            capture=b.piece_type_at(m.to_square) is not None, fen=b.fen(en_passant="fen")))
        moves.append(m.from_square | m.to_square << 6 | (m.promotion or 0) << 12)
        b.push(m)
        pos.append(grab())
    return pos, moves, info


def _pack(gid, pos, moves, pis, outcome, root_values):
    from betaone_amd import records as R

    fin = SimpleNamespace(game_id=gid, pis=pis, positions=pos, moves=moves, terminal=1 if outcome else 2, outcome=outcome)
    if root_values is not None:
        fin.root_values = root_values
    return R.unpack_games(R.pack_game(fin))[0]


@functools.lru_cache(maxsize=None)
def corpus():
    """A tuple of SimpleNamespace(game, fen, ucis, info): the dozen games.  pi of a ply: the move that was played first, then other legal
    moves, 1 or 2 entries in turn (4 in game WIDE) with random positive weights; outcomes +1, -1, 0 in turn; root values, unless
    gid % 4 == 3, all distinct over the corpus (multiples of 1/4096)."""
    nrng = np.random.default_rng(21)
    out, serial = [], 0
    for gid, (fen, ucis, tail) in enumerate(SPECS):
        line = _line(fen, ucis, tail, seed=100 + gid)
        pos, moves, info = _replay(fen, line)
        pis = []
        for i, (m, inf) in enumerate(zip(moves, info)):
            played = (m & 63, (m >> 6) & 63, (m >> 12) or None)
            others = [x for x in inf.legal if x != played]
            k = min(4 if gid == WIDE else 1 + (i + gid) % 2, 1 + len(others))
            pick = [played] + [others[j] for j in nrng.permutation(len(others))[:k - 1]]
            v = (nrng.random(k) + 0.05).astype(np.float32)
            pis.append((np.array([m2i(*x) for x in pick], dtype=np.int32), (v / v.sum()).astype(np.float32)))
        n = len(moves)
        rv = None
        if gid % 4 != 3:
            rv = (((np.arange(serial, serial + n) * 7) % 8191 - 4095) / 4096.0).astype(np.float32)
            serial += n
        outcome = (1.0, -1.0, 0.0)[gid % 3]
        out.append(SimpleNamespace(game=_pack(gid, pos, moves, pis, outcome, rv), fen=fen, ucis=line, info=info, pis=pis, outcome=outcome, rv=rv))
    return tuple(out)


def transformed(spec, t, gid=None, first=0):
    """The game `spec` from its ply `first` on under t, played out by the oracle: FEN and moves transformed as text, pi through the
    table, the outcome negated under the colour flip (z is the side to move's), the root values kept."""
    fen = spec.fen if first == 0 else spec.info[first].fen
    assert first == 0 or spec.info[first].ep_square is None
    pos, moves, _ = _replay(t_fen(fen, t), [t_uci(u, t) for u in spec.ucis[first:]])
    tab = action_table(t)
    pis = [(tab[ix].astype(np.int32), v) for ix, v in spec.pis[first:]]
    out = -spec.outcome if t & 1 else spec.outcome   # (a draw's 0.0 too: z keeps the sign of its zero, self_play.py:202)
    return _pack(spec.game["game_id"] if gid is None else gid, pos, moves, pis, out, None if spec.rv is None else spec.rv[first:])


def check_corpus():
    """Every property the checks lean on is in the corpus."""
    cs = corpus()
    assert len(cs) == 12 and all(9 <= len(c.ucis) <= 40 for c in cs)
    castles = {(i.white, i.wing) for c in cs for i in c.info if i.castle}
    assert castles == {(True, "k"), (True, "q"), (False, "k"), (False, "q")}
    ep = [i for c in cs for i in c.info if i.ep_square is not None]
    assert any(i.ep_legal for i in ep) and any(not i.ep_legal for i in ep) and any(i.ep_played for c in cs for i in c.info)
    assert any(i.ep_played for g in NO_RIGHTS for i in cs[g].info), "an en-passant square under the mirror"
    assert any(i.promo == 5 for c in cs for i in c.info)
    under = [(c, k) for c in cs for k, i in enumerate(c.info) if i.promo in (2, 3, 4) and i.capture]
    assert under and all(int(c.pis[k][0][0]) % 73 >= 64 for c, k in under)
    rep = [MC._key_bytes(p) for p in cs[7].game["positions"]]
    assert rep.count(rep[0]) == 3, "both repetition planes"
    assert any(c.fen.split()[1] == "b" for c in cs)
    assert all(cs[g].fen.split()[2] == "-" for g in NO_RIGHTS) and len(NO_RIGHTS) >= 3
    men = lambda f: sum(ch.isalpha() for ch in f.split()[0])  # noqa: E731
    assert set(cs[4].fen.split()[0].lower()) <= set("pk/12345678") and set(cs[5].fen.split()[0].lower()) <= set("prk/12345678") and men(cs[6].fen) > 20
    widths = {len(ix) for c in cs for ix, _ in c.pis}
    assert {1, 2, 4} <= widths and all(len(ix) == 4 for ix, _ in cs[WIDE].pis)
    assert any(c.rv is None for c in cs) and any(c.rv is not None for c in cs)
    rv = np.concatenate([c.rv for c in cs if c.rv is not None])
    assert np.unique(rv).size == rv.size
    ks = {k for c in cs for k in range(len(c.ucis))}
    assert {0, 1, 6, 7, 8} <= ks


# ---- sampling -------------------------------------------------------------------------------------------------------------------------

def _buffer(games, device):
    from betaone_amd import records as R

    buf = R.GpuReplayBuffer(sum(int(g["n_plies"]) + 1 for g in games) + 64, device=device, pi_width=W)
    assert buf.add(list(games)) == 0
    return buf


def _np(t):
    return t.detach().cpu().numpy()


def sample(buf, name, index, sym=None, merged=None):
    """One sampler's batch as numpy arrays: states [n,120,64]; pi (dense) or idx / val; z; q where the sampler has one; applied."""
    kw = {} if sym is None else {"sym": np.asarray(sym, dtype=np.int32)}
    if name == "dense":
        out = buf.batch(index, **kw)
        keys = ("states", "pi", "z")
    elif name == "sparse":
        out = buf.batch_sparse(index, **kw)
        keys = ("states", "idx", "val", "z")
    elif name == "sparse_q":
        out = buf.batch_sparse_q(index, **kw)
        keys = ("states", "idx", "val", "z", "q")
    else:
        out = buf.batch_merged(merged, index, **kw)
        keys = ("states", "idx", "val", "z", "q")
    assert len(out) == len(keys) + (sym is not None)
    d = {k: _np(v) for k, v in zip(keys, out)}
    d["states"] = d["states"].reshape(len(d["z"]), 120, 64)
    if sym is not None:
        assert out[-1].dtype == torch.int32 and tuple(out[-1].shape) == (len(d["z"]),)
        d["applied"] = _np(out[-1])
    return d


def _bits(a):
    return np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint32)


def _pairs(d, r):
    return sorted((int(i), int(np.float32(v).view(np.uint32))) for i, v in zip(d["idx"][r], d["val"][r]) if i >= 0)


def same_batch(got, want, what, planes=None, rows=None, sets=False, targets=True):
    """got's rows equal want's byte for byte: the planes `planes` (default all) and every target.  sets: idx / val per row as a set of
    (index, value bits) pairs (merged targets: a group's union is in ascending order of ITS indices)."""
    if rows is None:
        rows = np.arange(len(got["z"]))
    gr, wr = (np.asarray(rows[0]), np.asarray(rows[1])) if isinstance(rows, tuple) else (np.asarray(rows), np.asarray(rows))
    planes = np.arange(120) if planes is None else np.asarray(planes)
    gs, ws = _bits(got["states"][gr][:, planes]), _bits(want["states"][wr][:, planes])
    bad = np.nonzero((gs != ws).any(1))[0]
    if bad.size:
        first = int(planes[int(np.nonzero(gs[bad[0]] != ws[bad[0]])[0][0]) // 64])
        raise AssertionError(f"{what}: the states of {bad.size} rows differ, first row {int(gr[bad[0]])} at plane {first}")
    if not targets:
        return
    for k in ("pi", "z", "q") + (() if sets else ("idx", "val")):
        if k in got:
            g, w = got[k][gr], want[k][wr]
            assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), f"{what}: {k} differs in rows {np.nonzero((_bits(g) != _bits(w)).any(1))[0][:8].tolist()}"
    if sets and "idx" in got:
        for a, b in zip(gr, wr):
            assert _pairs(got, a) == _pairs(want, b), f"{what}: the pi entries of row {a}"


NOT_118 = np.array([p for p in range(120) if p != 118])


class Pair:
    """The corpus in a buffer and, per transform, the transformed corpus in a buffer of its own, each with its merge."""

    def __init__(self, device, games=None):
        self.device = device
        self.specs = corpus()
        self.games = [c.game for c in self.specs] if games is None else games
        self.buf = _buffer(self.games, device)
        self.merge = self.buf.merge_duplicates(key="input")
        self.n = len(self.buf)
        self.start = np.cumsum([0] + [int(g["n_plies"]) for g in self.games])
        self.rights = np.array([int(g["positions"][i].castling) != 0 for g in self.games for i in range(int(g["n_plies"]))])
        self.plain = {name: sample(self.buf, name, np.arange(self.n), merged=self.merge) for name in SAMPLERS}
        self._sym = {}

    def sym(self, name, t):
        if (name, t) not in self._sym:
            self._sym[name, t] = sample(self.buf, name, np.arange(self.n), sym=np.full(self.n, t), merged=self.merge)
        return self._sym[name, t]

    def rows_of(self, gids):
        return np.concatenate([np.arange(self.start[g], self.start[g + 1]) for g in gids])

    def close(self):
        self.merge.close()
        self.buf.close()


@functools.lru_cache(maxsize=2)
def pair(device):
    return Pair(device)


def _oracle(games, device):
    """Every record of `games` through the four plain samplers."""
    buf = _buffer(games, device)
    try:
        m = buf.merge_duplicates(key="input")
        try:
            return {name: sample(buf, name, np.arange(len(buf)), merged=m) for name in SAMPLERS}
        finally:
            m.close()
    finally:
        buf.close()


# ---- 1: colour flip = the flipped game ------------------------------------------------------------------------------------------------

def check_colour(device):
    p = pair(device)
    want = _oracle([transformed(c, 1) for c in p.specs], device)
    for name in SAMPLERS:
        got = p.sym(name, 1)
        assert (got["applied"] == 1).all()
        same_batch(got, want[name], f"{name}, colour flip", planes=NOT_118, sets=name == "merged")
        same_batch(got, p.plain[name], f"{name}, colour flip: plane 118", planes=[118], targets=False)
        if name == "dense":
            assert (got["states"][:, 112] != p.plain[name]["states"][:, 112]).all(), "the turn plane is toggled"
    assert any((want["dense"]["states"][:, 118] != p.plain["dense"]["states"][:, 118]).any(1)), "plane 118 of the flipped game runs ahead somewhere"
    return p.n


# ---- 2: file mirror = the mirrored game -----------------------------------------------------------------------------------------------

def check_mirror(device):
    p = pair(device)
    rows = p.rows_of(NO_RIGHTS)
    want = _oracle([transformed(p.specs[g], 2) for g in NO_RIGHTS], device)
    for name in SAMPLERS:
        got = p.sym(name, 2)
        assert (got["applied"][rows] == 2).all()
        same_batch(got, want[name], f"{name}, file mirror", rows=(rows, np.arange(rows.size)), sets=name == "merged")
        # with rights: applied is t & 1 exactly there, and those rows are the rows of sym = t & 1
        for t in (2, 3):
            got = p.sym(name, t)
            assert np.array_equal(got["applied"], np.where(p.rights, t & 1, t)), f"{name}: applied under {t}"
            held = np.nonzero(p.rights)[0]
            assert held.size > 50
            same_batch(got, p.plain[name] if t == 2 else p.sym(name, 1), f"{name}: rows with rights under {t}", rows=held)
    # after the last right is gone the mirror applies: against the mirrored (and flipped) continuation from that ply's FEN
    checked = 0
    for g in (0, 1, 11):
        spec = p.specs[g]
        n = len(spec.ucis)
        gone = min(k for k in range(n) if int(spec.game["positions"][k].castling) == 0)
        assert gone > 0 and n - gone >= 9 and not p.rights[p.start[g] + gone:p.start[g + 1]].any()
        for t in (2, 3):
            cont = _oracle([transformed(spec, t, first=gone)], device)
            ks = np.arange(7, n - gone)                                    # (records whose eight boards all lie in the continuation)
            rows = p.start[g] + gone + ks
            for name in SAMPLERS:
                got = p.sym(name, t)
                assert (got["applied"][rows] == t).all()
                same_batch(got, cont[name], f"{name}: game {g} from ply {gone} under {t}", rows=(rows, ks), planes=None if t == 2 else NOT_118,
                           sets=name == "merged")
                checked += rows.size
    assert checked > 100
    return checked


# ---- 3: both at once -------------------------------------------------------------------------------------------------------------------

def check_both(device):
    p = pair(device)
    rows = p.rows_of(NO_RIGHTS)
    want = _oracle([transformed(p.specs[g], 3) for g in NO_RIGHTS], device)
    for name in SAMPLERS:
        got = p.sym(name, 3)
        assert (got["applied"][rows] == 3).all()
        same_batch(got, want[name], f"{name}, both", rows=(rows, np.arange(rows.size)), planes=NOT_118, sets=name == "merged")
        same_batch(got, p.plain[name], f"{name}, both: plane 118", rows=rows, planes=[118], targets=False)


# ---- 4: nothing changes when off -------------------------------------------------------------------------------------------------------

def check_off(device):
    p = pair(device)
    for name in SAMPLERS:
        got = p.sym(name, 0)
        assert (got["applied"] == 0).all()
        same_batch(got, p.plain[name], f"{name}: sym all zero against today's entry point")
    buf, n = p.buf, p.n
    eq = lambda a, b: len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(_np(x)), _bits(_np(y))) for x, y in zip(a, b))  # noqa: E731
    for kw in (dict(), dict(sparse=True), dict(sparse=True, with_q=True), dict(sparse=True, merged=p.merge)):
        for how in (dict(steps=3), dict()):
            absent = list(buf.loader(16, seed=5, **how, **kw))
            none = list(buf.loader(16, seed=5, augment=None, **how, **kw))
            assert len(absent) == len(none) and all(eq(a, b) for a, b in zip(absent, none))
    # the same records in the same order: pi_val, z and q do not change under a symmetry, and the corpus's root values are distinct
    plain = list(buf.loader(16, seed=9, sparse=True, with_q=True))
    for augment, allowed in (("colour", {0, 1}), ("mirror", {0, 2}), ("both", {0, 1, 2, 3})):
        ld = buf.loader(16, seed=9, sparse=True, with_q=True, augment=augment)
        seen, untouched = set(), 0
        for a, b in zip(ld, plain):
            assert len(a) == 5 and all(np.array_equal(_bits(_np(a[k])), _bits(_np(b[k]))) for k in (2, 3, 4)), augment
            ap = _np(ld.last_applied)
            assert ap.shape == (a[0].shape[0],)
            seen |= set(ap.tolist())
            off = np.nonzero(ap == 0)[0]
            untouched += off.size
            assert np.array_equal(_bits(_np(a[0])[off]), _bits(_np(b[0])[off])) and np.array_equal(_np(a[1])[off], _np(b[1])[off])
            on = np.nonzero(ap != 0)[0]
            assert (_bits(_np(a[0])[on]) != _bits(_np(b[0])[on])).any(1).all(), "a transformed row has other planes"
        assert seen == allowed and untouched > 0, (augment, seen)
        assert int(ld.applied_counts.sum()) == n
    four = list(buf.loader(16, seed=9, sparse=True, augment="both"))
    dense = list(buf.loader(16, seed=9, augment="both"))
    mrg = list(buf.loader(16, seed=9, sparse=True, merged=p.merge, augment="both"))
    assert all(len(b) == 4 for b in four) and all(len(b) == 3 for b in dense) and all(len(b) == 5 for b in mrg)
    # the second generator is seeded: two loaders with one seed agree, and the dense, sparse and merged ones draw the same codes
    again = list(buf.loader(16, seed=9, sparse=True, augment="both"))
    assert all(eq(a, b) for a, b in zip(four, again))
    assert all(np.array_equal(_bits(_np(a[0])), _bits(_np(b[0]))) and np.array_equal(_bits(_np(a[0])), _bits(_np(c[0]))) for a, b, c in zip(four, dense, mrg))


# ---- 5: merged targets ---------------------------------------------------------------------------------------------------------------

def check_merged(device):
    """Exact copies with pis, outcomes and root values of their own: groups of three on every ply of two games."""
    cs = corpus()
    nrng = np.random.default_rng(4)
    games, flipped = [], []
    for gid, c in enumerate([cs[0], cs[2], cs[0], cs[4], cs[2], cs[0], cs[2], cs[8]]):
        pis = [(ix[nrng.permutation(len(ix))], v) for ix, v in c.pis]
        rv = (nrng.integers(-255, 256, size=len(c.ucis)) / 256.0).astype(np.float32) if gid % 3 else None
        spec = SimpleNamespace(game={"game_id": gid}, fen=c.fen, ucis=c.ucis, info=c.info, pis=pis, outcome=(1.0, -1.0, 0.0)[gid % 3], rv=rv)
        games.append(transformed(spec, 0))
        flipped.append(transformed(spec, 1))
    a, b = _buffer(games, device), _buffer(flipped, device)
    try:
        ma, mb = a.merge_duplicates(key="input"), b.merge_duplicates(key="input")
        try:
            n = len(a)
            assert ma.n_groups == mb.n_groups < n and ma.largest_group >= 3 and ma.counts.tolist() == mb.counts.tolist()
            assert ma.width == mb.width > 2
            got = sample(a, "merged", np.arange(n), sym=np.ones(n), merged=ma)
            want = sample(b, "merged", np.arange(n), merged=mb)
            same_batch(got, want, "merged targets under the colour flip", planes=NOT_118, sets=True)
            grouped = np.nonzero(ma.counts[ma.group_of(np.arange(n))] > 1)[0]
            assert grouped.size > 60
            return int(grouped.size)
        finally:
            ma.close()
            mb.close()
    finally:
        a.close()
        b.close()


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------

def check_refusals(device):
    from betaone_amd import engine as E

    p = pair(device)
    buf, lib = p.buf, p.buf.lib
    for bad in (4, -1):
        for name in SAMPLERS:
            with pytest.raises(E.EngineError, match="symmetry code"):
                sample(buf, name, [0, 1, 2], sym=[0, bad, 1], merged=p.merge)
    s, i, v, z, q = buf.batch_sparse_q(np.arange(4))
    ap = torch.zeros(4, dtype=torch.int32, device=s.device)
    idx = np.arange(4, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    codes = lambda c: np.asarray(c, dtype=np.int32).ctypes.data_as(E._I32P)  # noqa: E731
    before = _np(s).copy()
    assert lib.bo_replay_sample_sparse_q_sym(buf.h, 4, idx, codes([0, 1, 4, 0]), s.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), q.data_ptr(),
                                             ap.data_ptr(), None) == BO_E_ARG and b"0..3" in lib.bo_last_error()
    assert lib.bo_replay_sample_sparse_q_sym(buf.h, 4, idx, codes([0, 1, -1, 0]), s.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), q.data_ptr(),
                                             ap.data_ptr(), None) == BO_E_ARG
    assert lib.bo_replay_sample_sparse_q_sym(buf.h, 4, idx, None, s.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), q.data_ptr(),
                                             ap.data_ptr(), None) == BO_E_ARG
    assert np.array_equal(_np(s), before), "a refused call wrote the states"
    # applied may be NULL
    assert lib.bo_replay_sample_sparse_q_sym(buf.h, 4, idx, codes([1, 1, 1, 1]), s.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), q.data_ptr(),
                                             None, None) == 0
    assert np.array_equal(_bits(_np(s).reshape(4, 120, 64)), _bits(p.sym("sparse_q", 1)["states"][:4]))
    for name in SAMPLERS:
        for wrong in ([0], [0, 0, 0, 0]):
            with pytest.raises(ValueError):
                sample(buf, name, [0, 1, 2], sym=wrong, merged=p.merge)
    for aug in ("flip", "", "COLOUR", 1):
        with pytest.raises(ValueError):
            buf.loader(16, sparse=True, augment=aug)
    rng = np.random.default_rng(2)
    for n in (1, 65):
        index, sym = rng.integers(0, p.n, size=n), rng.integers(0, 4, size=n)
        for name in SAMPLERS:
            got = sample(buf, name, index, sym=sym, merged=p.merge)
            assert np.array_equal(got["applied"], np.where(p.rights[index], sym & 1, sym))
            for t in range(4):
                r = np.nonzero(got["applied"] == t)[0]
                if r.size:
                    same_batch(got, p.sym(name, t) if t else p.plain[name], f"{name}: a batch of {n} with mixed codes", rows=(r, index[r]))


# ---- 6b: one staging block under calls of every shape ------------------------------------------------------------------------------------

def check_staging(device):
    """The samplers share one staging block (rows slot, k and, where a sampler has them, sym and group; n ints each): calls of
    different row counts and batch sizes interleaved on ONE buffer, so the block grows, shrinks in use and changes its row offsets
    from call to call; then a refused call larger than anything staged before.  Every batch is compared bit for bit with the rows of
    the whole-corpus batches, which are taken only after the sequence has run."""
    from betaone_amd import engine as E

    p = pair(device)
    rng = np.random.default_rng(31)
    done = []

    def call(name, n, with_sym):
        index = rng.integers(0, p.n, size=n)
        sym = rng.integers(0, 4, size=n) if with_sym else None
        done.append((name, index, sym, sample(p.buf, name, index, sym=sym, merged=p.merge)))

    for name, n, with_sym in (("sparse", 3, False), ("merged", 130, True), ("dense", 1, False), ("sparse_q", 2, True), ("merged", 130, False),
                              ("dense", 65, True)):
        call(name, n, with_sym)
    bad = rng.integers(0, 4, size=200)
    bad[137] = 4
    with pytest.raises(E.EngineError, match="symmetry code 4 of sample 137"):
        sample(p.buf, "merged", rng.integers(0, p.n, size=200), sym=bad, merged=p.merge)
    call("sparse_q", 2, True)
    assert len(done) == 7
    for name, index, sym, got in done:
        what = f"{name}: a batch of {index.size}{' with mixed codes' if sym is not None else ''} among calls of other shapes"
        assert len(got["z"]) == index.size
        if sym is None:
            same_batch(got, p.plain[name], what, rows=(np.arange(index.size), index))
            continue
        assert np.array_equal(got["applied"], np.where(p.rights[index], sym & 1, sym)), what
        for t in range(4):
            r = np.nonzero(got["applied"] == t)[0]
            if r.size:
                same_batch(got, p.sym(name, t) if t else p.plain[name], what, rows=(r, index[r]))


# ---- 7: the commands -------------------------------------------------------------------------------------------------------------------

def _data(tmp_path):
    from betaone_amd import records as R

    data, init = str(tmp_path / "data"), str(tmp_path / "init.pth")
    R.save_games(R.compact_path(data, 0), VM._repack([c.game for c in corpus()]), append=False)
    VM.tiny_init(init)
    return data, init


def check_train_command(device, tmp_path, extra=()):
    from betaone_amd import train as T

    data, init = _data(tmp_path)
    n = sum(len(c.ucis) for c in corpus())
    common = ["--data-dir", data, "--init", init, "--batch", "16", "--device", device, "--iteration", "0", *extra]

    def run(name, *more):
        out = str(tmp_path / f"{name}.json")
        assert T.main(common + ["--save-dir", str(tmp_path / f"ck_{name}"), "--candidate", str(tmp_path / f"{name}.pth"), "--out", out, *more]) == 0
        return json.load(open(out))

    both = run("both", "--augment", "both", "--epochs", "2")
    assert both["augment"] == "both" and len(both["epochs"]) == 2
    assert all(np.isfinite([e["loss"], e["policy_loss"], e["value_loss"]]).all() for e in both["epochs"])
    trained = sum(e["samples"] for e in both["epochs"])
    counts = [both["applied_codes"][str(t)] for t in range(4)]
    assert trained == 2 * n and sum(counts) == trained and all(c > 0 for c in counts), counts
    for name, more in (("mix", ["--value-mix", "0.5"]), ("dense", ["--dense-loss"]),
                       ("held", ["--merge-duplicates", "input", "--merge-sample", "groups", "--holdout-fraction", "0.25"])):
        r = run(name, "--augment", "mirror", "--epochs", "1", *more)
        c = r["applied_codes"]
        assert c["1"] == c["3"] == 0 and c["0"] > c["2"] > 0 and c["0"] + c["2"] == sum(e["samples"] for e in r["epochs"]), (name, c)
        assert np.isfinite(r["epochs"][0]["loss"])
        if name == "held":
            assert np.isfinite(r["epochs"][0]["validation"]["policy_ce"])
    with pytest.raises(SystemExit) as ex:
        T.main(common + ["--save-dir", str(tmp_path / "ck_no"), "--augment", "rotate"])
    assert ex.value.code == 2
    # --augment none writes the bytes of the command without the flag
    with MC.deterministic_torch():
        for name, more in (("none", ["--augment", "none"]), ("absent", []), ("again", [])):
            assert T.main(common + ["--epochs", "1", "--save-dir", str(tmp_path / f"ck2_{name}"), "--candidate", str(tmp_path / f"w_{name}.pth"), *more]) == 0
    w = {k: MC._weights(str(tmp_path / f"w_{k}.pth")) for k in ("none", "absent", "again")}
    assert w["absent"] == w["again"], "two runs without the flag differ"
    assert w["none"] == w["absent"] and w["none"] != MC._weights(init)
    assert MC._weights(str(tmp_path / "both.pth")) != w["absent"]


def check_validate_command(device, tmp_path, extra=()):
    import contextlib
    import io
    import os

    from betaone_amd import validate as V

    data, init = _data(tmp_path)
    cs = corpus()
    n = sum(len(c.ucis) for c in cs)
    free = sum(int(c.game["positions"][i].castling) == 0 for c in cs for i in range(len(c.ucis)))
    out = str(tmp_path / "val.json")
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        assert V.main([os.path.join(data, "iter_0"), "--model", init, "--all", "--symmetry", "both", "--batch", "32", "--device", device, "--out", out,
                       *extra]) == 0
    text = text.getvalue()
    rep = json.load(open(out))["model"]
    assert rep["overall"]["records"] == n and 0 < free < n
    passes, cons = rep["symmetry"]["passes"], rep["symmetry"]["consistency"]
    assert [p["sym"] for p in passes] == [1, 2, 3] == [c["sym"] for c in cons]
    assert [p["overall"]["records"] for p in passes] == [n, free, free] == [c["records"] for c in cons]
    assert passes[1]["applied_codes"] == {"0": 0, "1": 0, "2": free, "3": 0}
    assert text.count("records      top1      top3") == 4 and "consistency" in text and all(name in text for name in V.SYMMETRY_NAMES.values())
    assert f"{free} of {n} records" in text
    for c in cons:   # a random net is no symmetric net
        assert c["kl"] > 0 and 0 <= c["top1_agreement"] <= 1 and c["value_abs_diff"] > 0
    for p in passes:
        assert np.isfinite(p["overall"]["policy_ce"]) and set(p["overall"]) == set(rep["overall"])


# ---- 8: consistency on nets with a known answer ----------------------------------------------------------------------------------------

def _destinations():
    """to[a] of every index (64 = off the board; an underpromotion is a white pawn's from rank 6 and a black pawn's from rank 1, no
    pawn's elsewhere), decoded with the vectors above."""
    to = np.full(A, 64, dtype=np.int64)
    for a in range(A):
        fr, p = divmod(a, 73)
        r, f = fr >> 3, fr & 7
        if p < 56:
            dr, df = Q[p // 7][0] * (p % 7 + 1), Q[p // 7][1] * (p % 7 + 1)
        elif p < 64:
            dr, df = K[p - 56]
        else:
            df, dr = P[(p - 64) % 3]
            dr = dr if r == 6 else -dr if r == 1 else 99
        if 0 <= r + dr < 8 and 0 <= f + df < 8:
            to[a] = (r + dr) * 8 + f + df
    return to


class ConstantNet(torch.nn.Module):
    """Logits that ignore the input: a fixed vector c; a fixed value."""

    def __init__(self, c):
        super().__init__()
        self.c = torch.nn.Parameter(torch.from_numpy(c))

    def forward(self, x):
        return self.c[None, :].expand(x.shape[0], -1), torch.full((x.shape[0], 1), 0.25, dtype=x.dtype, device=x.device)


class EquivariantNet(torch.nn.Module):
    """Logits read from the planes so that the twin position gives the twin move the same logit.  Per square, s = the pieces of the
    current board weighted by type, the side to move's once and the other side's seven times (the colour flip swaps the colours AND
    the turn); G[sq] = sum over sq' of s[sq'] k(|d rank|, |d file|) with an integer kernel, which both reflections leave alone;
    logit[a] = G[from(a)] + 3 G[to(a)] + 5 s[to(a)] + bias[a], from and to through this file's own decoding; the bias is -2^22 for a
    destination off the board and 1 + the piece for an underpromotion plane, which both reflections keep.
    Every quantity is a small integer, so float32 arithmetic is exact in any order, and T x gives bit for bit the permuted logits.
    The value is the material balance of the side to move."""

    def __init__(self):
        super().__init__()
        sq = np.arange(64)
        dr, df = np.abs((sq[:, None] >> 3) - (sq[None, :] >> 3)), np.abs((sq[:, None] & 7) - (sq[None, :] & 7))
        self.kernel = torch.nn.Parameter(torch.from_numpy(((8 - dr) * (9 - df) + dr * dr).astype(np.float32)))
        self.register_buffer("src", torch.from_numpy((np.arange(A) // 73).astype(np.int64)))
        self.register_buffer("dst", torch.from_numpy(_destinations()))
        self.w = torch.nn.Parameter(torch.tensor([1.0, 3.0, 4.0, 5.0, 9.0, 2.0]))
        plane = np.arange(A) % 73   # a move off the board never wins; an underpromotion differs from the promotion by its piece
        self.register_buffer("bias", torch.from_numpy(np.where(_destinations() == 64, -2.0 ** 22, np.where(plane >= 64, (plane - 64) // 3 + 1, 0)).astype(np.float32)))

    def forward(self, x):
        n = x.shape[0]
        cur = x[:, 98:110].reshape(n, 6, 2, 64)                       # [type][white, black][square]
        white_moves = x[:, 112].reshape(n, 64)[:, :1] > 0.5
        own = torch.where(white_moves[:, None, :], cur[:, :, 0], cur[:, :, 1])
        opp = torch.where(white_moves[:, None, :], cur[:, :, 1], cur[:, :, 0])
        s = ((own + 7.0 * opp) * self.w[None, :, None]).sum(1)      # [n, 64]
        g = s @ self.kernel
        pad = lambda t: torch.cat([t, torch.zeros((n, 1), dtype=t.dtype, device=t.device)], 1)  # noqa: E731
        logits = g[:, self.src] + 3.0 * pad(g)[:, self.dst] + 5.0 * pad(s)[:, self.dst] + self.bias[None, :]
        value = ((own - opp) * self.w[None, :, None]).sum((1, 2)) / 64.0
        return logits, value[:, None]


def check_consistency(device):
    """validate.symmetry_consistency on two nets whose answer is known.

    The bound.  Every figure is a float64 sum, here and there; eps = 2^-53, N = 4672.  A log-probability is x - max - log(sum exp): the
    sum of N exponentials is off by at most (N + 1) eps relative (one rounding per term and per addition, first order), its logarithm
    by that plus eps, and the two subtractions round once each: an absolute error of at most (N + 4) eps L per log-probability, L the
    largest magnitude among the logits and log-probabilities involved.  A term p (lp - lq) therefore carries at most 2 (N + 4) eps L p
    from its two log-probabilities, plus 3 eps of its own magnitude (exp, the difference, the product); over a row the p add up to 1,
    and adding N terms costs at most N eps of the sum S of their magnitudes: a row's KL is off by at most
        (2 (N + 4) L + (N + 3) S) eps.
    The mean over R equal or near-equal rows adds (R + 1) eps relative.  The implementation and this file's float64 reference each
    stay inside that, so they differ by at most twice it.  For the equivariant net both sides of every difference are bit-equal
    logits in another order, S is 0 up to the same errors, and the KL itself must be below the bound.  Agreements and value
    differences are exact: the logits and values of T x are bit for bit those of x."""
    from betaone_amd import validate as V

    p = pair(device)
    buf, eps = p.buf, 2.0 ** -53
    everything = np.arange(p.n)
    free = np.nonzero(~p.rights)[0]
    c = (np.random.default_rng(12).standard_normal(A) * 3.0).astype(np.float32)
    c64 = c.astype(np.float64)
    lp = c64 - c64.max() - np.log(np.exp(c64 - c64.max()).sum())
    const = ConstantNet(c).to(buf.device)
    for t in (1, 2, 3):
        index = free if t & 2 else everything
        lq = lp[action_table(t)]
        terms = np.exp(lp) * (lp - lq)
        want = float(terms.sum())
        L, S = float(max(np.abs(c64).max(), np.abs(lp).max())), float(np.abs(terms).sum())
        tol = 2.0 * (2 * (A + 4) * L + (A + 3) * S) * eps + (index.size + 1) * eps * abs(want)
        got = V.symmetry_consistency(const, buf, index, t, 32, False)
        assert got["sym"] == t and got["records"] == index.size
        assert want > 1.0 and abs(got["kl"] - want) <= tol, (t, got["kl"], want, tol)
        assert got["value_abs_diff"] == 0.0
        assert got["top1_agreement"] == float(action_table(t)[int(c.argmax())] == int(c.argmax()))
        if t & 2:   # records with rights drop the mirror bit and are left out
            assert V.symmetry_consistency(const, buf, everything, t, 32, False)["records"] == free.size
    eq = EquivariantNet().to(buf.device)
    with torch.no_grad():
        lg = eq(buf.batch_sparse(everything)[0])[0].double()
        top2 = lg.topk(2, dim=1).values
        assert bool((top2[:, 0] > top2[:, 1]).all()), "a tied best move: agreement would hang on the order of the indices"
        assert float(lg.abs().max()) < 2.0 ** 24 and bool((lg == lg.round()).all())
        L = float(max(lg.abs().max(), torch.log_softmax(lg, 1).abs().max()))
    for t in (1, 2, 3):
        index = free if t & 2 else everything
        got = V.symmetry_consistency(eq, buf, index, t, 32, False)
        assert got["records"] == index.size and got["top1_agreement"] == 1.0 and got["value_abs_diff"] == 0.0
        assert abs(got["kl"]) <= 2.0 * (2 * (A + 4) * L) * eps, (t, got["kl"], L)
    with pytest.raises(ValueError):
        V.symmetry_consistency(eq, buf, everything, 0, 32, False)
    with pytest.raises(ValueError):
        V.symmetry_consistency(eq, buf, [], 1, 32, False)
    # evaluate(sym=): the same metric table on the twin records; an equivariant net scores them alike
    plain, flipped = V.evaluate(eq, buf, everything, batch=32, amp=False), V.evaluate(eq, buf, everything, batch=32, amp=False, sym=1)
    assert flipped["sym"] == 1 and flipped["applied_codes"] == {"0": 0, "1": p.n, "2": 0, "3": 0} and "sym" not in plain
    for k in ("records", "policy_top1", "value_sign_accuracy", "mean_value"):   # (ranks below the first hang on ties among the logits)
        assert flipped["overall"][k] == plain["overall"][k], k
    assert abs(flipped["overall"]["policy_ce"] - plain["overall"]["policy_ce"]) <= 1e-5 * abs(plain["overall"]["policy_ce"])
