"""tests/book_cases.py -- TEST HELPER: bodies shared by tests/test_book_emu.py (wave emulator) and tests/test_book_gpu.py (MI355X) for the
opening-book path (csrc/bo_book.h, betaone_amd/book.py): a PGN corpus behind fixed prefixes, bo_book_insert against a NumPy / dict
restatement keyed by the entries' 68 key bytes, and the command's selection against a plain-Python restatement of its rules."""
from __future__ import annotations

import contextlib
import random

import numpy as np

import analyse_cases as AC
import engine_harness as H
import pgn_util as U
from betaone_amd import analyse as A
from betaone_amd import book as B
from betaone_amd import engine as E

F_KEY_MASK = 0x7F001F          # csrc/bo_chess.h: the side to move, the castling rights, the en-passant square where a capture is legal
GUARD = 8                      # guard elements on either side of every column
I64_MAX, I32_MAX = 2 ** 63 - 1, 2 ** 31 - 1
COLS = [(n, {"owner": np.int32, "first": np.int64, "sum_eval": np.int64}.get(n, np.int32), f) for n, _, f in B.COLUMNS]

# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
ORDER_A = ["e2e4", "e7e5", "g1f3", "b8c6"]                                   # one position ...
ORDER_B = ["g1f3", "b8c6", "e2e4", "e7e5"]                                   # ... by two move orders
NO_CASTLE = ORDER_A + ["h1g1", "g8f6", "g1h1", "f6g8"]                       # ORDER_A's pieces at ply 8, white's h1 right gone
EP_YES = ["e2e4", "a7a6", "e4e5", "h7h6", "g1f3", "d7d5"]                    # e5xd6 is legal
EP_NO = ["e2e3", "d7d6", "e3e4", "d6d5", "e4e5", "a7a6", "g1f3", "h7h6"]     # the same pieces, no en-passant capture
REPEAT = ["g1f3", "g8f6", "f3g1", "f6g8", "g1f3", "g8f6", "d2d4"]            # plies 1 and 5 are one position
OTHER = ["d2d4", "d7d5", "c2c4"]
PREFIXES = [ORDER_A, ORDER_B, NO_CASTLE, EP_YES, EP_NO, REPEAT, OTHER]
RESULTS = ["1-0", "0-1", "1/2-1/2", "*"]
WINDOW = (1, 10)


def make_corpus(seed=5, per_prefix=3, tail=8):
    """(games [(uci moves, result)], PGN text): per prefix `per_prefix` games that go on with random moves (eval comments on most), every
    game with a result token drawn from RESULTS."""
    rng = random.Random(seed)
    games, text = [], []
    for p, prefix in enumerate(PREFIXES):
        b = U.chess.Board()
        for u in prefix:
            b.push_uci(u)
        for k in range(per_prefix):
            mv, com, _, _ = U.random_game(rng, fen=b.fen(), max_plies=tail + k, eval_p=0.7, book_p=0.0)
            moves = prefix + mv
            comments = [U.random_eval_comment(rng) if rng.random() < 0.7 else None for _ in prefix] + com
            res = RESULTS[(p + k) % 4]
            games.append((moves, res))
            text.append(U.write_game(AC._sans(None, moves), comments, res, headers={"Event": f"prefix {p} game {k}"}))
    return games, "".join(text)


@contextlib.contextmanager
def backend_ctx(backend):
    if backend == "emu":
        with H.emulator_backend():
            yield "cpu"
    else:
        yield "cuda:0"


def corpus_of(backend, paths):
    with backend_ctx(backend) as dev:
        return B.Corpus([str(p) for p in paths], dev)


_CACHE = {}


def pgn_corpus(backend, tmp):
    """The corpus above ingested once per backend: (games, Corpus, ring bytes [capacity, 80], items of WINDOW with their evals)."""
    if backend not in _CACHE:
        games, text = make_corpus()
        path = tmp / "corpus.pgn"
        path.write_text(text)
        c = corpus_of(backend, [path])
        assert c.n_games == len(games) and c.g_moves.tolist() == [len(m) for m, _ in games]
        ring = c.pos.cpu().numpy().reshape(-1, 80).copy()
        it = c.items(*WINDOW)
        it["eval"] = c.ev.cpu().numpy()[it["entry"]]
        _CACHE[backend] = (games, c, ring, it, path)
    return _CACHE[backend]


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def key_of(ring, e):
    d = ring[e].view(A.DPOS_DTYPE)[0]
    return ring[e, :64].tobytes() + np.uint32(int(d["flags"]) & F_KEY_MASK).tobytes()


def restate(ring, it):
    """bo_book_insert in NumPy and a dict: -> (groups {key: dict(first, n, w, d, l, n_eval, min_ply, sum_eval)}, the key of every item or
    None where it is skipped, bad entries)."""
    groups, part, bad = {}, [], 0
    ev = it.get("eval")
    for i in range(len(it["entry"])):
        e = int(it["entry"][i])
        if e < 0 or e >= len(ring):
            bad += 1
            part.append(None)
            continue
        k = key_of(ring, e)
        if any(key_of(ring, e - j) == k for j in range(1, min(int(it["back"][i]), e) + 1)):
            part.append(None)
            continue
        g = groups.setdefault(k, dict(first=I64_MAX, n=0, w=0, d=0, l=0, n_eval=0, min_ply=I32_MAX, sum_eval=0))
        g["n"] += 1
        r = int(it["result"][i])
        if r in (1, 2, 3):
            g["wdl"[r - 1]] += 1
        if ev is not None and not np.isnan(ev[i]):
            q = int(np.rint(np.clip(np.float32(ev[i]), np.float32(-1), np.float32(1)) * np.float32(2 ** 20)))
            g["n_eval"] += 1
            g["sum_eval"] += q if int(ring[e].view(A.DPOS_DTYPE)[0]["flags"]) & 1 else -q
        g["min_ply"] = min(g["min_ply"], int(it["ply"][i]))
        g["first"] = min(g["first"], e)
        part.append(k)
    return groups, part, bad


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def lib_of(backend):
    return H.emu_lib() if backend == "emu" else E.load_hip_library()


def insert(backend, ring, it, T, flags=0, capacity=None, prefill=None):
    """One bo_book_insert call on guarded columns -> dict(columns [T], gid [n], status [2]); asserts that no guard element changed."""
    lib = lib_of(backend)
    n = len(it["entry"])
    rb = AC.IntBuf(backend, ring.reshape(-1))
    arg = {k: AC.IntBuf(backend, np.asarray(it[k], dt)) for k, dt in (("entry", np.int64), ("ply", np.int32), ("result", np.int32), ("back", np.int32))}
    ev = AC.IntBuf(backend, np.asarray(it["eval"], np.float32).view(np.int32)) if it.get("eval") is not None else None
    cols = {}
    for name, dt, fill in COLS:
        a = np.full(T + 2 * GUARD, 0x5A5A5A5A, dt)
        a[GUARD:GUARD + T] = fill if prefill is None else prefill[name]
        cols[name] = AC.IntBuf(backend, a)
    gid = AC.IntBuf(backend, np.full(n + 2 * GUARD, -99, np.int32))
    status = AC.IntBuf(backend, np.array([0, 0, -99, -99], np.int32))
    rc = lib.bo_book_insert(rb.ptr, len(ring) if capacity is None else capacity, n, *[arg[k].ptr for k in ("entry", "ply", "result")], ev.ptr if ev else None,
                            arg["back"].ptr, T, *[cols[name].ptr + GUARD * np.dtype(dt).itemsize for name, dt, _ in COLS], gid.ptr + 4 * GUARD,
                            status.ptr, flags, 0)
    assert rc == 0, lib.bo_last_error()
    out = {}
    for name, dt, _ in COLS:
        a = cols[name].numpy()
        assert (a[:GUARD] == dt(0x5A5A5A5A)).all() and (a[GUARD + T:] == dt(0x5A5A5A5A)).all(), name
        out[name] = a[GUARD:GUARD + T].copy()
    g = gid.numpy()
    assert (g[:GUARD] == -99).all() and (g[GUARD + n:] == -99).all()
    s = status.numpy()
    assert s[2] == -99 and s[3] == -99
    return dict(out, gid=g[GUARD:GUARD + n].copy(), status=s[:2].copy())


def by_first(t):
    """The occupied slots of a table, keyed by `first`: what does not depend on T or on the order of the items."""
    occ = np.nonzero(t["owner"] >= 0)[0]
    return {int(t["first"][s]): tuple(int(t[k][s]) for k in ("n", "w", "d", "l", "n_eval", "min_ply", "sum_eval")) for s in occ}


def check_against_restatement(t, ring, it):
    """Every column, the untouched slots and the gid partition of one call against restate()."""
    groups, part, bad = restate(ring, it)
    assert t["status"].tolist() == [0, bad]
    want = {g["first"]: tuple(g[k] for k in ("n", "w", "d", "l", "n_eval", "min_ply", "sum_eval")) for g in groups.values()}
    assert by_first(t) == want
    free = t["owner"] < 0
    assert int((~free).sum()) == len(groups)
    for name, _, fill in COLS:
        assert (t[name][free] == fill).all(), name
    slot_of = {}
    for i, k in enumerate(part):
        g = int(t["gid"][i])
        if k is None:
            assert g == -1, i
            continue
        assert 0 <= g < len(t["owner"]) and slot_of.setdefault(k, g) == g, i
        assert int(t["first"][g]) == groups[k]["first"]
    assert len(set(slot_of.values())) == len(slot_of)
    own = t["owner"][~free]
    assert all(part[o] is not None and slot_of[part[o]] == s for o, s in zip(own, np.nonzero(~free)[0]))   # owner: an item of the group
    return groups, part


def entry_of(c, games, moves, ply):
    """The ring entry of ply `ply` of the first game that begins with `moves`."""
    g = next(i for i, (m, _) in enumerate(games) if m[:len(moves)] == moves)
    return int(c.g_start[g]) + ply


def check_corpus_properties(games, c, ring, it):
    """What the issue wants of the restatement before anybody looks at the kernel."""
    groups, part, _ = restate(ring, it)
    assert sum(g["n"] >= 2 for g in groups.values()) >= 5
    a, b = entry_of(c, games, ORDER_A, 4), entry_of(c, games, ORDER_B, 4)
    ka = key_of(ring, a)
    assert ka == key_of(ring, b) and groups[ka]["n"] >= 2 * 3 and groups[ka]["min_ply"] == 4                # two move orders, one group
    nc = entry_of(c, games, NO_CASTLE, 8)
    assert ring[nc, :64].tobytes() == ring[a, :64].tobytes() and key_of(ring, nc) != ka                      # castling rights alone
    assert key_of(ring, nc) in groups and groups[key_of(ring, nc)]["min_ply"] == 8
    y, n = entry_of(c, games, EP_YES, 6), entry_of(c, games, EP_NO, 8)
    fy, fn = (int(ring[e].view(A.DPOS_DTYPE)[0]["flags"]) for e in (y, n))
    assert ring[y, :64].tobytes() == ring[n, :64].tobytes() and (fy ^ fn) & 0x1F == 0 and (fy >> 16) & 0x7F and not (fn >> 16) & 0x7F
    assert key_of(ring, y) != key_of(ring, n) and key_of(ring, y) in groups and key_of(ring, n) in groups  # e.p. legality alone
    r = entry_of(c, games, REPEAT, 1)
    assert key_of(ring, r) == key_of(ring, r + 4)
    i1, i5 = (int(np.nonzero(it["entry"] == e)[0][0]) for e in (r, r + 4))
    assert part[i1] is not None and part[i5] is None                                                        # the repetition counts once:
    assert groups[key_of(ring, r)]["n"] == sum(m[0] == "g1f3" for m, _ in games) == 6                       # every game that opens 1. Nf3, once
    assert any(g["n_eval"] > 0 and g["sum_eval"] != 0 for g in groups.values()) and any(g["w"] and g["d"] and g["l"] for g in groups.values())
    return groups


def check_pgn_corpus(backend, tmp):
    """(1) the PGN corpus against the restatement, with and without the per-wave combining."""
    games, c, ring, it, _ = pgn_corpus(backend, tmp)
    groups = check_corpus_properties(games, c, ring, it)
    n = len(it["entry"])
    assert n > 128 and n % 64 != 0                                   # more than one workgroup, a partial last wave
    tabs = []
    for flags in (0, B.NO_COMBINE):
        t = insert(backend, ring, it, B.next_pow2(2 * n), flags)
        check_against_restatement(t, ring, it)
        tabs.append(by_first(t))
    assert tabs[0] == tabs[1]
    no_ev = {k: v for k, v in it.items() if k != "eval"}             # eval_dev == NULL
    t = insert(backend, ring, no_ev, B.next_pow2(2 * n))
    check_against_restatement(t, ring, no_ev)
    assert (t["n_eval"] == 0).all() and (t["sum_eval"] == 0).all()
    return len(groups)


def synthetic_ring(n, seed, khash):
    rs = np.random.RandomState(seed)
    d = np.zeros(n, A.DPOS_DTYPE)
    d["bb"] = rs.randint(0, 2 ** 63, size=(n, 8), dtype=np.int64).astype(np.uint64)
    d["flags"] = rs.randint(0, 2, size=n).astype(np.uint32) | (rs.randint(0, 16, size=n).astype(np.uint32) << 1)
    d["khash"] = khash
    return d


def check_shared_khash(backend):
    """(2) distinct positions under ONE khash word are distinct groups (a probe chain as long as the table); one position under two
    khash words is two groups: the filter never lets the pair merge."""
    n_pos, copies = 48, 3
    d = synthetic_ring(n_pos, 1, 0xDEADBEEF)
    ring = np.tile(d, copies).view(np.uint8).reshape(-1, 80)          # every position three times, all with one khash
    N = len(ring)
    it = dict(entry=np.arange(N, dtype=np.int64), ply=(np.arange(N) % 7).astype(np.int32), result=(np.arange(N) % 4).astype(np.int32),
              back=np.zeros(N, np.int32), eval=np.linspace(-1.5, 1.5, N).astype(np.float32))
    for T in (64, 1024):
        t = insert(backend, ring, it, T)
        groups, _ = check_against_restatement(t, ring, it)
        assert len(groups) == n_pos and all(g["n"] == copies for g in groups.values())
    # the caller's error: entry 1 is entry 0 with another khash (both probe the same slot of a 4-slot table, and meet)
    two = synthetic_ring(2, 2, 8)
    two[1] = two[0]
    two["khash"] = [8, 12]
    t = insert(backend, two.view(np.uint8).reshape(-1, 80), dict(entry=np.arange(2, dtype=np.int64), ply=np.zeros(2, np.int32), result=np.ones(2, np.int32),
                                                               back=np.zeros(2, np.int32)), 4)
    assert sorted(t["gid"].tolist()) == [0, 1] and t["n"].tolist() == [1, 1, 0, 0] and t["status"].tolist() == [0, 0]


def prefix_with_groups(ring, it, want):
    """The longest prefix of the work list with exactly `want` groups."""
    seen, cut = set(), 0
    _, part, _ = restate(ring, it)
    for i, k in enumerate(part):
        if k is not None and k not in seen:
            if len(seen) == want:
                break
            seen.add(k)
        cut = i + 1
    assert len(seen) == want
    return {k: (v[:cut] if isinstance(v, np.ndarray) and k != "off" else v) for k, v in it.items()}


def check_table_sizes(backend, tmp):
    """(3) T below the group count overflows and writes nothing outside the columns; a full table, the smallest one that fits and a much
    larger one hold the same groups."""
    _, c, ring, it, path = pgn_corpus(backend, tmp)
    part = prefix_with_groups(ring, it, 64)
    groups, keys, _ = restate(ring, part)
    live = sum(k is not None for k in keys)
    t = insert(backend, ring, part, 32)                                # (insert() checks the guards)
    over = int(t["status"][0])
    assert over > 0 and int((t["gid"] == -2).sum()) == over and int((t["owner"] >= 0).sum()) == 32
    assert int(t["n"].sum()) + over == live                           # an overflow item contributes nothing, every other item once
    full = insert(backend, ring, part, 64)                             # T == the group count: every slot taken, probes wrap around
    assert int((full["owner"] >= 0).sum()) == 64
    check_against_restatement(full, ring, part)
    want = by_first(full)
    for T in (128, 1 << 16):
        t = insert(backend, ring, part, T)
        check_against_restatement(t, ring, part)
        assert by_first(t) == want
    # the library doubles a table that overflows: the same book from T = 4
    with backend_ctx(backend) as dev:
        kw = dict(min_ply=WINDOW[0], max_ply=WINDOW[1], min_games=2, max_bias=0.5, device=dev, corpus=c)
        a, b = B.build_book(None, t0=4, **kw), B.build_book(None, **kw)
    assert a["table_retries"] >= 5 and b["table_retries"] == 0 and a["text"] == b["text"] and a["kept"] >= 3
    return over


def check_order_independence(backend, tmp):
    """(4) the work list reversed and shuffled: the same groups."""
    _, _, ring, it, _ = pgn_corpus(backend, tmp)
    n = len(it["entry"])
    T = B.next_pow2(2 * n)
    want = by_first(insert(backend, ring, it, T))
    for perm in (np.arange(n)[::-1], np.random.RandomState(3).permutation(n)):
        p = {k: (np.ascontiguousarray(v[perm]) if isinstance(v, np.ndarray) and k != "off" else v) for k, v in it.items()}
        for flags in (0, B.NO_COMBINE):
            t = insert(backend, ring, p, T, flags)
            check_against_restatement(t, ring, p)
            assert by_first(t) == want


def check_refusals(backend):
    """(7) BO_E_ARG, n == 0, entries outside the ring."""
    lib = lib_of(backend)
    d = synthetic_ring(4, 4, 5)
    ring = d.view(np.uint8).reshape(-1, 80)
    it = dict(entry=np.array([0, 1, -1, 4, 2, 7], np.int64), ply=np.arange(6, dtype=np.int32), result=np.ones(6, np.int32), back=np.full(6, 9, np.int32))
    t = insert(backend, ring, it, 8)                                   # -1, 4 and 7 are outside [0, 4): counted, nothing read (back is cut at 0)
    assert t["status"].tolist() == [0, 3] and t["gid"][[2, 3, 5]].tolist() == [-1, -1, -1]
    check_against_restatement(t, ring, it)
    t = insert(backend, ring, dict(it, entry=np.arange(6, dtype=np.int64)), 8, capacity=0)   # an empty ring: every entry is bad
    assert t["status"].tolist() == [0, 6] and (t["owner"] == -1).all()
    pre = {name: np.arange(8).astype(dt) + 3 for name, dt, _ in COLS}
    t = insert(backend, ring, {k: v[:0] for k, v in it.items()}, 8, prefill=pre)             # n == 0: the columns are not touched
    assert all((t[name] == pre[name]).all() for name in pre) and t["status"].tolist() == [0, 0]
    a = AC.IntBuf(backend, np.zeros(64, np.int64))
    p = a.ptr
    good = [p, 4, 1, p, p, p, None, p, 8] + [p] * 11 + [0, 0]
    assert lib.bo_book_insert(*good) == 0

    def bad(i, v):
        args = list(good)
        args[i] = v
        return lib.bo_book_insert(*args)

    for i, v in ((8, 0), (8, 6), (8, -8), (8, 1 << 31), (1, -1), (2, -1), (2, 1 << 31), (20, 2), (0, None), (3, None), (7, None), (9, None), (17, None),
                 (18, None), (19, None)):
        assert bad(i, v) == -1 and lib.bo_last_error(), (i, v)          # BO_E_ARG
    args = list(good)
    args[2], args[9] = 0, None
    assert lib.bo_book_insert(*args) == -1                              # a NULL column is refused before n == 0 is looked at


# ---- selection, restated ---------------------------------------------------------------------------------------------------------------
def select_restated(groups, part, it, c, min_games, max_bias, max_eval, max_n, allow_nested):
    """The rules of the command over restate()'s groups, in plain Python: -> the `first` of the kept positions, in book order."""
    first_of = {k: g["first"] for k, g in groups.items()}
    cand = []
    for k, g in groups.items():
        dec = g["w"] + g["d"] + g["l"]
        if g["n"] < min_games or dec < 1 or abs((g["w"] + g["d"] / 2) / dec - 0.5) > max_bias:
            continue
        if max_eval is not None and g["n_eval"] > 0 and abs(g["sum_eval"] / 2 ** 20 / g["n_eval"]) > max_eval:
            continue
        cand.append((-g["n"], g["min_ply"], g["first"], k))
    kept, lines = [], {}
    for _, _, first, k in sorted(cand):
        if max_n is not None and len(kept) >= max_n:
            break
        game = int(np.searchsorted(c.g_start, first, side="right")) - 1
        i0 = int(it["off"][game])
        line = {p for p in part[i0:i0 + (first - int(c.g_start[game])) - it["lo"] + 1] if p is not None}
        if not allow_nested and any(k in lines[a] or a in line for a in kept):
            continue
        kept.append(k)
        lines[k] = line
    return [first_of[k] for k in kept]


def replay_fen(root, moves):
    b = U.chess.Board(root) if root != "startpos" else U.chess.Board()
    for u in moves.split():
        assert b.is_legal(U.chess.Move.from_uci(u)), (root, moves, u)
        b.push_uci(u)
    return b.fen()


def check_selection(backend, tmp, min_games=2, max_bias=0.5, max_eval=None, max_n=None, allow_nested=False):
    """(6) what the library keeps, and in which order, against select_restated()."""
    _, c, ring, it, _ = pgn_corpus(backend, tmp)
    groups, part, _ = restate(ring, it)
    want = select_restated(groups, part, it, c, min_games, max_bias, max_eval, max_n, allow_nested)
    with backend_ctx(backend) as dev:
        rep = B.build_book(None, min_ply=WINDOW[0], max_ply=WINDOW[1], min_games=min_games, max_bias=max_bias, max_eval=max_eval, max_n=max_n,
                           allow_nested=allow_nested, device=dev, corpus=c)
    assert [g["first"] for g in rep["kept_groups"]] == want and len(want) >= 2
    loose = select_restated(groups, part, it, c, 2, 0.5, None, None, True)
    strict = (min_games, max_bias, max_eval, max_n, allow_nested) != (2, 0.5, None, None, True)
    assert len(want) < len(loose) if strict else want == loose
    # every rule this case sets drops something on its own, the others left loose
    base = dict(min_games=2, max_bias=0.5, max_eval=None, max_n=None, allow_nested=True)
    for name, val in dict(min_games=min_games, max_bias=max_bias, max_eval=max_eval, max_n=max_n, allow_nested=allow_nested).items():
        if val != base[name]:
            alone = select_restated(groups, part, it, c, **dict(base, **{name: val}))
            assert len(alone) < len(loose) and set(alone) <= set(loose), name
    return want


def check_command_line(backend, tmp):
    """(6) the command on the PGN corpus: every line parses, replays with the oracle to the report's FEN, carries the restatement's counts;
    two runs give the same bytes; MatchScheduler takes the book."""
    import io
    import json

    from betaone_amd import match as M

    _, c, ring, it, path = pgn_corpus(backend, tmp)
    groups, part, _ = restate(ring, it)
    by = {g["first"]: g for g in groups.values()}
    outs = []
    with backend_ctx(backend) as dev:
        for k in range(2):
            book, rep, buf = tmp / f"book{k}_{backend}.txt", tmp / f"book{k}_{backend}.json", io.StringIO()
            args = [str(path), "-o", str(book), "--min-ply", str(WINDOW[0]), "--max-ply", str(WINDOW[1]), "--min-games", "2", "--max-bias", "0.5",
                    "--json", str(rep), "--device", dev]
            assert B.main(args, out=buf) == 0
            assert buf.getvalue().startswith(f"[book] games {c.n_games}  items {len(it['entry'])}  groups {len(groups)}  ")
            outs.append((book.read_bytes(), json.load(open(rep))))
    assert outs[0][0] == outs[1][0] and outs[0][1]["book"] == outs[1][1]["book"]
    text, rep = outs[0][0].decode(), outs[0][1]
    want = select_restated(groups, part, it, c, 2, 0.5, None, None, False)
    assert [b["first"] for b in rep["book"]] == want and rep["kept"] == len(want) >= 3 and rep["groups"] == len(groups)
    openings = M.parse_openings(text)
    lines = text.splitlines()
    assert len(openings) == len(lines) == len(want)
    for (fen, moves), line, b in zip(openings, lines, rep["book"]):
        g = by[b["first"]]
        assert fen is None and line.startswith("startpos ; ")            # every game of the corpus starts at the start position
        assert replay_fen("startpos", moves) == b["fen"]
        assert key_of(ring, b["first"])[:64] == ring[b["first"], :64].tobytes()
        assert (b["n"], b["w"], b["d"], b["l"], b["n_eval"], b["min_ply"]) == (g["n"], g["w"], g["d"], g["l"], g["n_eval"], g["min_ply"])
        assert f"# n={g['n']} w={g['w']} d={g['d']} l={g['l']} eval=" in line and line.endswith(f" ply={g['min_ply']}")
        assert (b["eval"] is None) == (g["n_eval"] == 0) and (g["n_eval"] == 0 or abs(b["eval"] - g["sum_eval"] / 2 ** 20 / g["n_eval"]) < 1e-12)
        # the moves played from the position: every counted game once
        assert sum(r["n"] for r in b["replies"]) == g["n"] and sum(r["w"] for r in b["replies"]) == g["w"]
        k = key_of(ring, b["first"])
        played = {}
        for i, p in enumerate(part):
            if p == k:
                u = E.move_to_uci(int(c.moves_at([it["entry"][i]])[0]))
                played[u] = played.get(u, 0) + 1
        assert {r["move"]: r["n"] for r in b["replies"]} == played
        assert all(U.chess.Board(b["fen"]).is_legal(U.chess.Move.from_uci(r["move"])) for r in b["replies"])
    sched = M.MatchScheduler(openings, 2 * len(openings), 4)
    assert len(sched.pending) == 2 * len(openings) and [o for o in sched.openings] == openings
    return rep


# ---- records -------------------------------------------------------------------------------------------------------------------------
def play_records(tmp):
    """Emulator self-play games saved without and with root values (tests/test_reanalyse_emu.py's games); terminal codes 1, 2, 3, 0, 4 are
    written into the headers in turn, so that every result occurs.  -> the two iteration directories."""
    import test_reanalyse_emu as TR
    from betaone_amd import records as R

    if "records" not in _CACHE:
        dirs = (TR._play(tmp, "book_bog1"), TR._play(tmp, "book_bog2", record_values=True))
        for d in dirs:
            p = d / "games_rank0.bog"
            buf = bytearray(p.read_bytes())
            for j, (_gid, _n, off, _size) in enumerate(R.scan_games(bytes(buf))):
                buf[off + 12:off + 16] = np.array([[1, 2, 3, 0, 4][j % 5]], np.int32).tobytes()
            p.write_bytes(bytes(buf))
        _CACHE["records"] = dirs
    return _CACHE["records"]


def restate_records(files, lo, hi):
    """The table of the records' window positions from records.load_games alone: {first: (n, w, d, l, n_eval, min_ply, sum_eval)}."""
    from betaone_amd import records as R

    groups, base = {}, 0
    for path in files:
        for g in R.load_games(str(path)):
            n, pos = g["n_plies"], g["positions"]
            res = {1: 3 if pos[n].turn == 1 else 1, 3: 3 if pos[n].turn == 1 else 1, 2: 2}.get(g["terminal"], 0)
            seen = set()
            for k in range(lo, min(hi, n - 1) + 1):
                p = pos[k]
                key = (bytes(p.bb), p.turn, p.castling, max(p.ep_key, -1))
                if key in seen:
                    continue
                seen.add(key)
                a = groups.setdefault(key, dict(first=base + k, n=0, w=0, d=0, l=0, n_eval=0, min_ply=k, sum_eval=0))
                a["n"] += 1
                if res:
                    a["wdl"[res - 1]] += 1
                if g["root_values"] is not None:
                    q = int(np.rint(np.clip(np.float32(g["root_values"][k]), np.float32(-1), np.float32(1)) * np.float32(2 ** 20)))
                    a["n_eval"] += 1
                    a["sum_eval"] += q if p.turn == 1 else -q
                a["min_ply"], a["first"] = min(a["min_ply"], k), min(a["first"], base + k)
            base += n + 1
    return {a["first"]: tuple(a[k] for k in ("n", "w", "d", "l", "n_eval", "min_ply", "sum_eval")) for a in groups.values()}


def check_records(backend, tmp):
    """(5) BOG1 and BOG2 files of the same games in one ring, with a PGN file in front of them."""
    d1, d2 = play_records(tmp)
    files = [d1 / "games_rank0.bog", d2 / "games_rank0.bog"]
    lo, hi = 0, 5
    want = restate_records(files, lo, hi)
    # (the games end with white to move, so terminals 1 and 3 are both black's wins; white's wins are the PGN corpus's and record_result's)
    assert sum(v[0] >= 2 for v in want.values()) >= 5 and any(v[2] for v in want.values())
    assert any(v[3] for v in want.values()) and any(0 < v[4] < v[0] and v[6] != 0 for v in want.values())   # only the BOG2 copy has evals
    c = corpus_of(backend, [d1, files[1]])                           # an iteration directory and a file
    assert c.n_games == 10 and (c.g_kind == B.KIND_BOG).all()
    tab = B.Table(c, c.items(lo, hi), t0=4)
    g = {k: v.cpu().numpy() for k, v in tab.groups().items()}
    got = {int(g["first"][i]): tuple(int(g[k][i]) for k in ("n", "w", "d", "l", "n_eval", "min_ply", "sum_eval")) for i in range(len(g["slot"]))}
    assert got == want and tab.retries > 0
    # the same records behind a PGN file: every entry index moves by the PGN's positions, nothing else changes
    _, pc, _, _, path = pgn_corpus(backend, tmp)
    mixed = corpus_of(backend, [path, d1, d2])
    assert mixed.capacity == pc.capacity + c.capacity and mixed.n_games == pc.n_games + 10
    with backend_ctx(backend) as dev:
        rep = B.build_book(None, min_ply=0, max_ply=4, min_games=2, max_bias=0.5, device=dev, corpus=mixed, allow_nested=True)
    recs = [k for k in rep["kept_groups"] if mixed.g_kind[k["game"]] == B.KIND_BOG]
    assert recs and all(replay_fen(k["root"], k["moves"]) == mixed.fens([k["first"]])[0] for k in rep["kept_groups"])
    return len(want)


# ---- contention (GPU) ------------------------------------------------------------------------------------------------------------------
LINE = ORDER_A + ["f1c4", "f8c5", "c2c3", "g8f6", "d2d4", "e5d4", "c3d4", "c5b4", "b1c3"]     # 13 moves, no position twice


def check_contention(backend, tmp, n_games=2048):
    """(4, GPU) n_games copies of one game: 12 * n_games items on 12 slots, in file order and shuffled, with and without combining."""
    comments = [None, "+0.50/10 0.100s"] + [None] * (len(LINE) - 2)                                 # move 1's comment: ply 0's eval, -value
    path = tmp / "one_line.pgn"
    path.write_text(U.write_game(AC._sans(None, LINE), comments, "1-0") * n_games)
    c = corpus_of(backend, [path])
    it = c.items(0, 11)
    it["eval"] = c.ev.cpu().numpy()[it["entry"]]
    n = len(it["entry"])
    assert c.n_games == n_games >= 2000 and n == 12 * n_games >= 20000 and n // 64 > 300            # hundreds of workgroups
    ring = c.pos.cpu().numpy().reshape(-1, 80)
    q = int(np.rint(np.float32(it["eval"][0]) * np.float32(2 ** 20)))
    assert q != 0 and np.isnan(it["eval"][1])
    perm = np.random.RandomState(9).permutation(n)
    for order in (None, perm):
        p = it if order is None else {k: (np.ascontiguousarray(v[order]) if isinstance(v, np.ndarray) and k != "off" else v) for k, v in it.items()}
        for flags in (0, B.NO_COMBINE):
            t = insert(backend, ring, p, 1 << 16, flags)
            assert t["status"].tolist() == [0, 0] and (t["gid"] >= 0).all()
            want = {ply: (n_games, n_games, 0, 0, n_games if ply == 0 else 0, ply, q * n_games if ply == 0 else 0) for ply in range(12)}
            assert by_first(t) == want, (order is None, flags)                                      # game 0's entries are 0 .. 11
    return n
