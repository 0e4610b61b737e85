"""tests/merge_cases.py -- TEST HELPER for tests/test_merge_emu.py (wave emulator) and tests/test_merge_gpu.py (MI355X): merged targets
of the replay buffer (csrc/bo_merge.h, GpuReplayBuffer.merge_duplicates).  The bodies run on "cpu" under the emulator and on "cuda:0".

The oracles know nothing of the implementation:
  input partition     buf.batch(every record) -> the state rows grouped by their bytes on the host
  position partition  the bytes of the current position's key fields (boards, turn, castling, legal en-passant square) from the games
  merged values       fractions.Fraction means over the members, taken from the games' pis, outcomes and root values
The bound on a merged value is one float32 ulp of the exact mean: the kernel rounds a float64 quotient once, and the quotient's own
error (a float64 sum of n float32 terms, one division) is below 2^-52 n of it, far inside half an ulp of float32 for every n here."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import hashlib
import json
import os
import random
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import value_mix_cases as VM

A = 4672
BO_E_ARG, BO_E_STATE = -1, -5
RES_CAP = 256
START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


# ---- games -------------------------------------------------------------------------------------------------------------------------

def _key_bytes(p) -> bytes:
    return b"".join(int(v).to_bytes(8, "little") for v in p.bb) + bytes([int(p.turn), int(p.castling), int(p.ep_key) + 1])


def _pool_pi(p, nrng):
    """1 or 2 actions out of a pool of 8 that the position fixes, with random positive weights: the unions of duplicates overlap."""
    pool = np.random.default_rng(int.from_bytes(hashlib.sha256(_key_bytes(p)).digest()[:8], "little")).choice(A, 8, replace=False)
    k = int(nrng.integers(1, 3))
    v = (nrng.random(k) + 0.05).astype(np.float32)
    return nrng.choice(pool, size=k, replace=False).astype(np.int32), (v / v.sum()).astype(np.float32)


def game_from_moves(gid, ucis, nrng, fen=None, valued=None, outcome=None, pi_of=_pool_pi):
    """An unpack_games dict of the game `ucis` from `fen`: outcome (+1, -1, 0)[gid % 3], root values (multiples of 1/256) unless
    gid % 4 == 3 (a BOG1 record), pis from pi_of(position, nrng)."""
    import engine_cases as EC
    import pgn_util as U
    from betaone_amd import records as R

    b = U.chess.Board(fen) if fen else U.chess.Board()
    pos = [EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1)]
    moves = []
    for u in ucis:
        m = U.chess.Move.from_uci(u)
        assert b.is_legal(m), (gid, u)
        moves.append(m.from_square | m.to_square << 6 | (m.promotion or 0) << 12)
        b.push(m)
        pos.append(EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1))
    n = len(moves)
    outcome = (1.0, -1.0, 0.0)[gid % 3] if outcome is None else outcome
    fin = SimpleNamespace(game_id=gid, pis=[pi_of(pos[i], nrng) for i in range(n)], positions=pos, moves=moves, terminal=1 if outcome else 2,
                          outcome=outcome)
    if (gid % 4 != 3) if valued is None else valued:
        fin.root_values = (nrng.integers(-255, 256, size=n) / 256.0).astype(np.float32)
    return R.unpack_games(R.pack_game(fin))[0]


def _continue(ucis, rng, n_more, avoid=None):
    """ucis plus n_more random legal moves; the first new move is not `avoid`."""
    import pgn_util as U

    b = U.chess.Board()
    for u in ucis:
        b.push(U.chess.Move.from_uci(u))
    out = list(ucis)
    for i in range(n_more):
        legal = [m for m in b.legal_moves if not (i == 0 and m.uci() == avoid)]
        if not legal or b.is_game_over(claim_draw=False):
            break
        m = rng.choice(legal)
        out.append(m.uci())
        b.push(m)
    return out


@functools.lru_cache(maxsize=None)
def family_corpus(seed=11):
    """About 40 games of 9 to 28 plies (module docstring of the issue's check 1): a base game with three exact copies; two siblings for
    each p in (0, 1, 3, 7, 8, 9, 12) that copy its first p plies and then diverge; two games that reach one position by transposed move
    orders and go on alike for 14 plies (their 8-board windows coincide again from ply 12 on); a game that returns to the start
    position twice; random games."""
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    base = []
    while len(base) < 24:
        base = _continue([], rng, 28)
    lines = [base, base, base[:20], base]
    for p in (0, 1, 3, 7, 8, 9, 12):
        for _ in range(2):
            lines.append(_continue(base[:p], rng, rng.randint(9, 16), avoid=base[p]))
    tail = None
    while tail is None or len(tail) < 18:
        tail = _continue(["g1f3", "g8f6", "b1c3", "b8c6"], rng, 14)
    lines += [tail, ["b1c3", "b8c6", "g1f3", "g8f6"] + tail[4:]]
    back = ["g1f3", "g8f6", "f3g1", "f6g8"]
    lines.append(_continue(back + back, rng, 10))
    while len(lines) < 40:
        g = _continue([], rng, rng.randint(9, 28))
        if len(g) >= 9:
            lines.append(g)
    games = [game_from_moves(gid, u, nrng) for gid, u in enumerate(lines)]
    assert any(g["root_values"] is None for g in games) and any(g["root_values"] is not None for g in games)
    return tuple(games)


def distinct_corpus(n_games=10, seed=3):
    """Games that differ at ply 0 and ever after: every game starts from a FEN of its own whose fullmove number no other game reaches."""
    import pgn_util as U

    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    games = []
    for gid in range(n_games):
        b = U.chess.Board()
        for u in _continue([], rng, 2):
            b.push(U.chess.Move.from_uci(u))
        fen = b.fen().split(" ")
        fen[5] = str(10 + 40 * gid)
        fen = " ".join(fen)
        ucis = U.random_game(rng, fen=fen, max_plies=rng.randint(9, 20), eval_p=0.0, book_p=0.0)[0]
        games.append(game_from_moves(gid, ucis, nrng, fen=fen))
    return games


def records_of(games):
    """Per record of the games in order: (actions, values, z, q, position) as the buffer has to hold them."""
    z, q, _ = VM.stored(games)
    out, at = [], 0
    for g in games:
        for i in range(int(g["n_plies"])):
            ix, v = g["pis"][i]
            out.append(SimpleNamespace(idx=np.asarray(ix, np.int32), val=np.asarray(v, np.float32), z=z[at], q=q[at], pos=g["positions"][i]))
            at += 1
    return out


# ---- oracles -----------------------------------------------------------------------------------------------------------------------

def partition(keys, index):
    """{lowest record index: ascending member list} of the records `index` grouped by keys[i]."""
    by = {}
    for i in sorted(int(x) for x in index):
        by.setdefault(keys[i], []).append(i)
    return {m[0]: m for m in by.values()}


def input_keys(buf, chunk=256):
    keys = []
    for a in range(0, len(buf), chunk):
        s = buf.batch(np.arange(a, min(len(buf), a + chunk)))[0].cpu().numpy()
        keys += [row.tobytes() for row in s.reshape(s.shape[0], -1)]
    return keys


def position_keys(recs):
    return [_key_bytes(r.pos) for r in recs]


def check_partition(merged, want, index):
    """The merge's groups are exactly `want`'s, for every record of index and none left out."""
    index = np.asarray(index, dtype=np.int64)
    reps = sorted(want)
    assert merged.n_groups == len(reps) and merged.n_records == index.size
    assert merged.representatives.tolist() == reps
    assert merged.counts.tolist() == [len(want[r]) for r in reps]
    got = merged.representative_of(index)
    rep_of = {i: r for r, m in want.items() for i in m}
    assert got.tolist() == [rep_of[int(i)] for i in index]
    at = {r: g for g, r in enumerate(reps)}
    assert merged.group_of(index).tolist() == [at[rep_of[int(i)]] for i in index]
    assert merged.largest_group == max(len(m) for m in want.values())
    assert merged.records_in_groups == sum(len(m) for m in want.values() if len(m) > 1)


def _ulp32(x: float) -> Fraction:
    return Fraction(float(np.spacing(np.float32(abs(x)))))


def _near(got, exact: Fraction, what):
    err = abs(Fraction(float(got)) - exact)
    assert err <= _ulp32(float(exact)), f"{what}: {float(got)!r} against {float(exact)!r}: off by {float(err):.3e}"


def check_values(buf, merged, recs, want, pi_width):
    """Every group's count, union, means and (for a group of one) copy, read through batch_merged at the representatives."""
    reps = sorted(want)
    s, idx, val, z, q = buf.batch_merged(merged, reps)
    s0 = buf.batch_sparse_q(reps)[0]
    assert VM.LC.same_bits(s, s0), "the states are not the records' own"
    idx, val, z, q = idx.cpu().numpy(), val.cpu().numpy(), z.cpu().numpy().reshape(-1), q.cpu().numpy().reshape(-1)
    unions = [sorted({int(a) for m in want[r] for a in recs[m].idx}) for r in reps]
    width = max([pi_width] + [len(u) if len(want[r]) > 1 else len(recs[r].idx) for r, u in zip(reps, unions)])
    assert merged.width == width == idx.shape[1] == val.shape[1]
    for g, r in enumerate(reps):
        mem = want[r]
        n = len(mem)
        if n == 1:
            rec = recs[r]
            k = len(rec.idx)
            assert idx[g, :k].tolist() == rec.idx.tolist() and (idx[g, k:] == -1).all(), f"group of record {r}"
            assert val[g, :k].view(np.uint32).tolist() == rec.val.view(np.uint32).tolist() and (val[g, k:].view(np.uint32) == 0).all()
            assert z[g:g + 1].view(np.uint32)[0] == np.float32(rec.z).view(np.uint32) and q[g:g + 1].view(np.uint32)[0] == np.float32(rec.q).view(np.uint32)
            continue
        u = unions[g]
        assert idx[g, :len(u)].tolist() == u and (idx[g, len(u):] == -1).all(), f"group of record {r}: {idx[g].tolist()} against {u}"
        assert (val[g, len(u):].view(np.uint32) == 0).all()
        tot = {a: Fraction(0) for a in u}
        for m in mem:
            for a, v in zip(recs[m].idx, recs[m].val):
                tot[int(a)] += Fraction(float(v))
        for e, a in enumerate(u):
            _near(val[g, e], tot[a] / n, f"group of record {r}, action {a}")
        _near(z[g], sum(Fraction(float(recs[m].z)) for m in mem) / n, f"group of record {r}: z")
        _near(q[g], sum(Fraction(float(recs[m].q)) for m in mem) / n, f"group of record {r}: q")
    return idx, val, z, q


def _buffer(games, device, pi_width=2, capacity=None):
    from betaone_amd import records as R

    buf = R.GpuReplayBuffer(capacity or sum(int(g["n_plies"]) + 1 for g in games) + 64, device=device, pi_width=pi_width)
    assert buf.add(list(games)) == 0
    return buf


# ---- 1, 2: the partition and the values ---------------------------------------------------------------------------------------------

def check_families(device):
    games = family_corpus()
    recs = records_of(games)
    buf = _buffer(games, device)
    try:
        n = len(buf)
        assert n == len(recs) and 9 <= min(int(g["n_plies"]) for g in games) and max(int(g["n_plies"]) for g in games) <= 28
        everything = np.arange(n)
        by_input, by_pos = partition(input_keys(buf), everything), partition(position_keys(recs), everything)
        mi, mp = buf.merge_duplicates(), buf.merge_duplicates(key="position")
        try:
            check_partition(mi, by_input, everything)
            check_partition(mp, by_pos, everything)
            assert mi.n_groups > mp.n_groups and mi.largest_group >= 4
            # records with k < 7, k = 7 and k > 7 that merge under `input`, and (the transposed pair from ply 12 on) from different histories
            start = np.cumsum([0] + [int(g["n_plies"]) for g in games])
            ks = {i - int(start[np.searchsorted(start, i, side="right") - 1]) for m in by_input.values() if len(m) > 1 for i in m}
            assert {0, 3, 7, 8, 12} <= ks
            # the transposed pair and the returned-to start position: one group under `position`, several under `input`
            a, b = int(start[18]) + 4, int(start[19]) + 4
            assert _key_bytes(recs[a].pos) == _key_bytes(recs[b].pos)
            assert mp.group_of(a) == mp.group_of(b) and mi.group_of(a) != mi.group_of(b)
            assert mi.group_of(a + 9) == mi.group_of(b + 9), "the 8-board windows of the transposed pair coincide from ply 12 on"
            g0 = int(start[20])
            assert mp.group_of(g0) == mp.group_of(g0 + 4) == mp.group_of(g0 + 8) == mp.group_of(0)
            # (its ply 0 has the start position's planes of every other game but for the end-of-game repetition count)
            assert len({mi.group_of(g0), mi.group_of(g0 + 4), mi.group_of(g0 + 8), mi.group_of(0)}) == 4
            check_values(buf, mi, recs, by_input, 2)
            check_values(buf, mp, recs, by_pos, 2)
            rep = mi.report()
            assert rep["groups"] == len(by_input) and rep["records"] == n and rep["largest_group"] == mi.largest_group
            assert sum(rep["histogram"].values()) == len(by_input)
            assert rep["histogram"]["2^0"] == sum(1 for m in by_input.values() if len(m) == 1)
            assert abs(rep["duplicate_share"] - sum(len(m) for m in by_input.values() if len(m) > 1) / n) < 1e-12
        finally:
            mi.close()
            mp.close()
        return len(by_input), len(by_pos)
    finally:
        buf.close()


# ---- 3: no duplicates, no difference --------------------------------------------------------------------------------------------------

def check_no_duplicates(device):
    games = distinct_corpus()
    buf = _buffer(games, device)
    try:
        n = len(buf)
        m = buf.merge_duplicates()
        try:
            assert m.n_groups == n == m.n_records and m.width == buf.pi_width and m.largest_group == 1 and m.records_in_groups == 0
            order = np.random.default_rng(1).permutation(n)
            got, want = buf.batch_merged(m, order), buf.batch_sparse_q(order)
            assert len(got) == 5 and all(a.dtype == b.dtype and a.shape == b.shape for a, b in zip(got, want))
            assert all(VM.LC.same_bits(a.float(), b.float()) for a, b in zip(got, want)) and torch.equal(got[1], want[1])
            for five, ref in zip(buf.loader(16, steps=3, seed=5, sparse=True, merged=m), buf.loader(16, steps=3, seed=5, sparse=True, with_q=True)):
                assert all(VM.LC.same_bits(a.float(), b.float()) for a, b in zip(five, ref))
            with pytest.raises(ValueError):
                buf.loader(16, sparse=False, merged=m)
        finally:
            m.close()
    finally:
        buf.close()


# ---- 4: index and hold-out ---------------------------------------------------------------------------------------------------------

def check_holdout(device):
    from betaone_amd import engine as E
    from betaone_amd import validate as V

    games = family_corpus()
    recs = records_of(games)
    train, held = V.holdout_games(list(games), 0.5, 1)
    assert train.size > 100 and held.size > 100
    buf = _buffer(games, device)
    try:
        keys = input_keys(buf)
        want = partition(keys, train)
        assert len(partition(keys, np.arange(len(buf)))) < len(want) + len(partition(keys, held)), "no group crosses the split: a weak corpus"
        m = buf.merge_duplicates(index=train)
        try:
            check_partition(m, want, train)
            assert set(m.representatives.tolist()) <= set(train.tolist())
            check_values(buf, m, recs, want, 2)   # the means over the training members only
            assert not m.covers(held).any() and m.covers(train).all()
            with pytest.raises(E.EngineError, match="not covered"):
                buf.batch_merged(m, held[:3])
            with pytest.raises(ValueError):
                m.group_of(held[:1])
            with pytest.raises(ValueError):
                buf.loader(16, sparse=True, merged=m)                                   # every record: some are held out
            with pytest.raises(ValueError):
                buf.loader(16, sparse=True, merged=m, index=np.concatenate([train[:5], held[:1]]))
            batches = list(buf.loader(16, sparse=True, merged=m, index=train, seed=2))
            assert sum(b[0].shape[0] for b in batches) == train.size and all(len(b) == 5 for b in batches)
        finally:
            m.close()
    finally:
        buf.close()


# ---- 5: probing --------------------------------------------------------------------------------------------------------------------

def shuffle_corpus():
    """Games of knight shuffles of different lengths that come back to the start position every four plies: one current position under
    many histories and counters."""
    nrng = np.random.default_rng(9)
    pats = [("g1f3", "g8f6", "f3g1", "f6g8"), ("b1c3", "b8c6", "c3b1", "c6b8"), ("g1f3", "b8c6", "f3g1", "c6b8"), ("b1c3", "g8f6", "c3b1", "f6g8"),
            ("g1h3", "g8h6", "h3g1", "h6g8"), ("b1a3", "b8a6", "a3b1", "a6b8"), ("g1h3", "b8a6", "h3g1", "a6b8")]
    return [game_from_moves(gid, list(p) * (8 + 2 * gid) + ["e2e4"], nrng) for gid, p in enumerate(pats)]


def check_probing(device):
    from betaone_amd import engine as E

    games = shuffle_corpus()
    recs = records_of(games)
    buf = _buffer(games, device)
    try:
        n = len(buf)
        everything = np.arange(n)
        by_input, by_pos = partition(input_keys(buf), everything), partition(position_keys(recs), everything)
        at_start = [i for i in range(n) if _key_bytes(recs[i].pos) == _key_bytes(recs[0].pos)]
        inputs_at_start = {by for by, m in by_input.items() if m[0] in at_start}
        assert len(inputs_at_start) >= 64 and by_pos[0] == at_start
        host = buf.merge_duplicates()
        t0 = host.table_slots
        host.close()
        assert t0 >= 2 * n and t0 & (t0 - 1) == 0
        t = t0
        while True:
            for key, want in (("input", by_input), ("position", by_pos)):
                m = buf.merge_duplicates(key=key, table_slots=t)
                try:
                    assert m.table_slots == t
                    check_partition(m, want, everything)
                finally:
                    m.close()
            if t >= 8 * n:
                break
            t *= 2
        # a table of exactly as many slots as there are groups still holds them; a smaller one overflows
        full = 1 << (len(by_pos) - 1).bit_length()
        m = buf.merge_duplicates(key="position", table_slots=full)
        check_partition(m, by_pos, everything)
        m.close()
        small = 64
        assert small < len(by_input)
        h = C.c_void_p()
        rc = buf.lib.bo_replay_merge_create_ex(buf.h, 0, None, 0, small, None, C.byref(h))
        assert rc == BO_E_STATE and b"overflow" in buf.lib.bo_last_error() and not h.value
        with pytest.raises(E.EngineError, match="overflow"):
            buf.merge_duplicates(table_slots=small)
        for bad in (3, -2, 1 << 31):
            assert buf.lib.bo_replay_merge_create_ex(buf.h, 0, None, 0, bad, None, C.byref(h)) == BO_E_ARG
        return len(inputs_at_start)
    finally:
        buf.close()


# ---- 6: contention -----------------------------------------------------------------------------------------------------------------

def check_contention(device, copies):
    """`copies` copies of one 12-ply game with pis and outcomes of their own: 12 groups of `copies`."""
    rng, nrng = random.Random(4), np.random.default_rng(4)
    line = []
    while len(line) < 12:
        line = _continue([], rng, 12)
    games = [game_from_moves(gid, line, nrng) for gid in range(copies)]
    recs = records_of(games)
    buf = _buffer(games, device)
    try:
        n = len(buf)
        assert n == 12 * copies
        want = {k: [k + 12 * c for c in range(copies)] for k in range(12)}
        first = buf.merge_duplicates()
        check_partition(first, want, np.arange(n))
        assert first.counts.tolist() == [copies] * 12
        cols = check_values(buf, first, recs, want, 2)
        again = buf.merge_duplicates()
        shuffled = buf.merge_duplicates(index=np.random.default_rng(6).permutation(n))
        try:
            for other in (again, shuffled):
                check_partition(other, want, other.index)
                for a, b in zip(cols, buf.batch_merged(other, sorted(want))[1:]):
                    assert np.array_equal(a.reshape(-1).view(np.uint32), b.cpu().numpy().reshape(-1).view(np.uint32)), "a column differs"
        finally:
            first.close()
            again.close()
            shuffled.close()
        return n
    finally:
        buf.close()


# ---- 7: life cycle -----------------------------------------------------------------------------------------------------------------

def check_wrap_around(device):
    """A ring of about three games, as in value_mix_cases.check_sampler: after it has come round, a merge follows the resident records."""
    from betaone_amd import engine as E
    from betaone_amd import records as R

    games = list(family_corpus()[:8])   # the base game, its copies and siblings: duplicates among whatever survives
    slots = sum(int(g["n_plies"]) + 1 for g in games[:3]) + 4
    small = R.GpuReplayBuffer(slots - 2, device=device, pi_width=2)
    try:
        added, used, checked, stale = [], 0, 0, None
        for rnd in range(2):
            for g in games:
                small.add([dict(g, game_id=100 * rnd + g["game_id"])])
                added.append(g)
                used += int(g["n_plies"]) + 1
                if stale is not None:
                    with pytest.raises(E.EngineError, match="stale merge"):
                        small.batch_merged(stale, [0])
                    stale.close()
                    stale = None
                if used <= slots or small.n_games < 2:
                    continue
                resident = added[-small.n_games:]
                recs = records_of(resident)
                n = len(small)
                assert n == len(recs)
                want = partition(input_keys(small), np.arange(n))
                m = small.merge_duplicates()
                check_partition(m, want, np.arange(n))
                check_values(small, m, recs, want, 2)
                checked += 1
                stale = m
        assert small.n_evicted > 0 and used > 2 * slots and checked >= 4
        if stale is not None:
            stale.close()
        return small.n_evicted
    finally:
        small.close()


def check_refusals(device):
    from betaone_amd import engine as E

    games = family_corpus()[:3]
    buf = _buffer(games, device)
    try:
        lib, n = buf.lib, len(buf)
        idx = lambda a: np.asarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        h = C.c_void_p()
        with pytest.raises(ValueError):
            buf.merge_duplicates(key="planes")
        with pytest.raises(ValueError):
            buf.merge_duplicates(index=[])
        assert lib.bo_replay_merge_create(buf.h, 0, None, 2, C.byref(h)) == BO_E_ARG and b"key" in lib.bo_last_error()
        assert lib.bo_replay_merge_create(buf.h, 0, None, -1, C.byref(h)) == BO_E_ARG
        assert lib.bo_replay_merge_create(None, 0, None, 0, C.byref(h)) == BO_E_ARG
        assert lib.bo_replay_merge_create(buf.h, 0, None, 0, None) == BO_E_ARG
        assert lib.bo_replay_merge_create(buf.h, 0, idx([0]), 0, C.byref(h)) == BO_E_ARG               # an empty index
        assert lib.bo_replay_merge_create(buf.h, 2, idx([0, n]), 0, C.byref(h)) == BO_E_ARG and b"out of range" in lib.bo_last_error()
        assert lib.bo_replay_merge_create(buf.h, 2, idx([0, -1]), 0, C.byref(h)) == BO_E_ARG
        assert lib.bo_replay_merge_create(buf.h, 3, idx([4, 2, 4]), 0, C.byref(h)) == BO_E_ARG and b"twice" in lib.bo_last_error()
        assert not h.value
        m = buf.merge_duplicates()
        s, i, v, z, q = buf.batch_merged(m, np.arange(4))
        good = (s.data_ptr(), i.data_ptr(), v.data_ptr(), z.data_ptr(), q.data_ptr())
        assert lib.bo_replay_sample_merged(buf.h, m.h, 4, idx([0, 1, 2, n]), *good, None) == BO_E_ARG and b"out of range" in lib.bo_last_error()
        assert lib.bo_replay_sample_merged(buf.h, None, 4, idx([0, 1, 2, 3]), *good, None) == BO_E_ARG
        assert lib.bo_replay_sample_merged(None, m.h, 4, idx([0, 1, 2, 3]), *good, None) == BO_E_ARG
        assert lib.bo_replay_sample_merged(buf.h, m.h, 0, idx([0]), *good, None) == BO_E_ARG
        assert lib.bo_replay_sample_merged(buf.h, m.h, 4, None, *good, None) == BO_E_ARG
        for k in range(5):
            args = list(good)
            args[k] = None
            assert lib.bo_replay_sample_merged(buf.h, m.h, 4, idx([0, 1, 2, 3]), *args, None) == BO_E_ARG
        assert lib.bo_replay_merge_info(None, None) == BO_E_ARG and lib.bo_replay_merge_groups(m.h, None, None) == BO_E_ARG
        other = _buffer(games, device)
        try:
            assert lib.bo_replay_sample_merged(other.h, m.h, 4, idx([0, 1, 2, 3]), *good, None) == BO_E_ARG and b"another buffer" in lib.bo_last_error()
        finally:
            other.close()
        # a merge made before buf.add is refused afterwards
        buf.add([dict(games[0], game_id=77)])
        with pytest.raises(E.EngineError, match="stale merge"):
            buf.batch_merged(m, np.arange(4))
        with pytest.raises(E.EngineError, match="stale merge"):
            next(iter(buf.loader(4, sparse=True, merged=m, index=np.arange(8))))
        m.close()
        with pytest.raises(ValueError):
            buf.batch_merged(m, np.arange(4))
        lib.bo_replay_merge_destroy(None)
    finally:
        buf.close()


def check_wide_union(device):
    """200 copies of one record, each with 2 random actions out of 4 672: a union above BO_RES_CAP is refused by name.  100 copies fit,
    and the merged width follows the union."""
    from betaone_amd import engine as E

    def any_two(p, nrng):
        return nrng.choice(A, size=2, replace=False).astype(np.int32), np.array([0.25, 0.75], dtype=np.float32)

    nrng = np.random.default_rng(8)
    lead = game_from_moves(0, ["d2d4", "d7d5"], nrng)                     # records 0, 1: record 1 is nobody's duplicate
    copies = [game_from_moves(1 + c, ["e2e4"], nrng, pi_of=any_two) for c in range(200)]
    buf = _buffer([lead] + copies, device)
    try:
        recs = records_of([lead] + copies)
        union = {int(a) for r in recs[2:] for a in r.idx} | {int(a) for a in recs[0].idx}
        assert len(union) > RES_CAP
        with pytest.raises(E.EngineError, match=r"the group of record 0 \(201 records\)"):
            buf.merge_duplicates()
        part = np.arange(101)
        want = {0: [0] + list(range(2, 101)), 1: [1]}
        m = buf.merge_duplicates(index=part)
        try:
            check_partition(m, want, part)
            check_values(buf, m, recs, want, 2)
            assert 100 < m.width <= 200
        finally:
            m.close()
    finally:
        buf.close()


# ---- 8: the command ----------------------------------------------------------------------------------------------------------------

def _weights(path):
    return {k: v.cpu().numpy().tobytes() for k, v in torch.load(path, map_location="cpu").items()}


@contextlib.contextmanager
def deterministic_torch():
    """torch's own kernels in their deterministic variants (MIOpen's convolution backward is not reproducible from run to run
    otherwise: two runs of `train` WITHOUT the option then differ in every tensor, and a byte-for-byte comparison says nothing)."""
    saved = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled(),
             torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = saved[:2]
        torch.use_deterministic_algorithms(saved[2], warn_only=saved[3])


def check_command(device, tmp_path, extra=()):
    from betaone_amd import records as R
    from betaone_amd import train as T
    from betaone_amd import validate as V

    games = list(family_corpus()[:12])
    data = str(tmp_path / "data")
    R.save_games(R.compact_path(data, 0), VM._repack(games), append=False)
    init = str(tmp_path / "init.pth")
    VM.tiny_init(init)
    loaded = T.load_window_games(T.iteration_files(data, 0)[0])
    train, held = V.holdout_games(loaded, 0.25, 0)
    assert held.size > 0 and train.size > 0
    buf = _buffer(loaded, device)
    try:
        keys = input_keys(buf)
    finally:
        buf.close()
    want = partition(keys, train)
    assert len(want) < train.size
    common = ["--data-dir", data, "--init", init, "--epochs", "1", "--batch", "16", "--device", device, "--iteration", "0", *extra]

    def run(name, *more):
        out = str(tmp_path / f"{name}.json")
        assert T.main(common + ["--save-dir", str(tmp_path / f"ck_{name}"), "--candidate", str(tmp_path / f"{name}.pth"), "--out", out,
                                *more]) == 0
        return json.load(open(out))

    rec = run("records", "--merge-duplicates", "input", "--holdout-fraction", "0.25")
    grp = run("groups", "--merge-duplicates", "input", "--holdout-fraction", "0.25", "--merge-sample", "groups")
    mix = run("mix", "--merge-duplicates", "input", "--holdout-fraction", "0.25", "--value-mix", "0.5", "--steps-per-epoch", "3")
    for r in (rec, grp, mix):
        mg = r["merge"]
        assert mg["key"] == "input" and mg["groups"] == len(want) and mg["records"] == int(train.size)
        assert mg["largest_group"] == max(len(m) for m in want.values())
        assert abs(mg["duplicate_share"] - sum(len(m) for m in want.values() if len(m) > 1) / train.size) < 1e-12
        assert sum(mg["histogram"].values()) == len(want) and r["held_out_records"] == int(held.size)
        assert "validation" in r["epochs"][0] and np.isfinite(r["epochs"][0]["loss"])
    assert rec["merge"]["sample"] == "records" and rec["epochs"][0]["samples"] == train.size and rec["epochs"][0]["steps"] == -(-train.size // 16)
    assert grp["merge"]["sample"] == "groups" and grp["epochs"][0]["samples"] == len(want) and grp["epochs"][0]["steps"] == -(-len(want) // 16)
    assert grp["merge"]["records_per_epoch"] == len(want) and rec["merge"]["records_per_epoch"] == train.size
    assert mix["epochs"][0]["steps"] == 3 and mix["value_mix"] == 0.5 and np.isfinite(mix["epochs"][0]["value_vs_q"])
    with pytest.raises(SystemExit) as ex:
        T.main(common + ["--save-dir", str(tmp_path / "ck_no"), "--merge-duplicates", "input", "--dense-loss"])
    assert ex.value.code == 2 and not os.path.exists(str(tmp_path / "ck_no"))


def check_command_without_duplicates(device, tmp_path, extra=()):
    """On the corpus of check_no_duplicates the option changes no weight: --merge-duplicates input --merge-sample records writes,
    byte for byte, what a run without it writes."""
    from betaone_amd import records as R
    from betaone_amd import train as T

    init = str(tmp_path / "init.pth")
    VM.tiny_init(init)
    data2 = str(tmp_path / "data2")
    R.save_games(R.compact_path(data2, 0), VM._repack(distinct_corpus(4)), append=False)
    common2 = ["--data-dir", data2, "--init", init, "--epochs", "1", "--batch", "16", "--device", device, "--iteration", "0", *extra]
    with deterministic_torch():
        for name, more in (("with", ["--merge-duplicates", "input", "--merge-sample", "records"]), ("without", []), ("again", [])):
            assert T.main(common2 + ["--save-dir", str(tmp_path / f"ck2_{name}"), "--candidate", str(tmp_path / f"w_{name}.pth"), *more]) == 0
    assert _weights(str(tmp_path / "w_without.pth")) == _weights(str(tmp_path / "w_again.pth")), "two runs without the option differ"
    assert _weights(str(tmp_path / "w_with.pth")) == _weights(str(tmp_path / "w_without.pth"))
    assert _weights(str(tmp_path / "w_with.pth")) != _weights(init)
