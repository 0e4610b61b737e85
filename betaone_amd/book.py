"""betaone_amd/book.py -- opening books from the games the pipeline already holds.

    python -m betaone_amd.book INPUT... -o book.txt [--min-ply 8] [--max-ply 16] [--min-games 10] [--max-bias 0.1] [--max-eval E]
           [--max N] [--allow-nested] [--json report.json] [--device cuda:0]

`match --openings FILE` needs a file of openings, and the machines this runs on cannot fetch one.  INPUT is any mix of PGN files or
directories (pretrain's input, pgn_write's output) and .bog files or iteration directories (self-play records).  Everything is ingested
into ONE ring of positions in device memory -- PGN through bo_pgn_parse / bo_pgn_replay, each file's games at their own slot offset,
records through bo_records_ring at an offset of the same buffer -- so an entry index names a position of the whole corpus.

Every position from which a game played a move, at a ply inside [--min-ply, --max-ply], is a work item.  bo_book_insert
(csrc/bo_book.h) groups the items by their exact transposition key, transpositions included, and gives each group integer aggregates:
games, white wins / draws / black wins, evals, the lowest ply, the first entry.  A game counts once per position.  The table starts at
the next power of two >= twice the item count and is doubled, and the call repeated, while items overflow.

Selection is torch operations on the table's columns ("Opening books"): enough games, at least one decided game, a score
near 50 %, optionally a mean eval near 0; most games first; lines that run through, or on from, a kept position are dropped unless
--allow-nested.  One line per kept position, in the format match.parse_openings reads:

    <root FEN | startpos> ; <uci moves to the position> # n=.. w=.. d=.. l=.. eval=.. ply=..

The same inputs in the same order give the same bytes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import analyse as A
from . import engine as E
from . import pgn as P
from . import records as R

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
RESULT_CODE = {"1-0": 1, "1/2-1/2": 2, "0-1": 3}   # bo_book_insert's result_dev; anything else: 0, unknown
EVAL_ONE = 1 << 20                                   # BO_BOOK_EVAL_ONE
NO_COMBINE = 1                                       # BO_BOOK_NO_COMBINE
COLUMNS = (("owner", torch.int32, -1), ("first", torch.int64, 2 ** 63 - 1), ("n", torch.int32, 0), ("w", torch.int32, 0), ("d", torch.int32, 0),
           ("l", torch.int32, 0), ("n_eval", torch.int32, 0), ("min_ply", torch.int32, 2 ** 31 - 1), ("sum_eval", torch.int64, 0))
KIND_PGN, KIND_BOG = 0, 1


def input_files(paths: Sequence[str]) -> List[Tuple[int, str]]:
    """(kind, file) in the order given: a directory contributes its PGN files (pgn.pgn_paths), then its *.bog files, each sorted."""
    out = []
    for p in ([paths] if isinstance(paths, str) else list(paths)):
        if os.path.isdir(p):
            out += [(KIND_PGN, f) for f in P.pgn_paths([p])]
            out += [(KIND_BOG, f) for f in sorted(glob.glob(os.path.join(p, "*" + R.COMPACT_SUFFIX)))]
        elif not os.path.exists(p):
            raise ValueError(f"book: {p}: no such file or directory")
        else:
            out.append((KIND_BOG if p.endswith(R.COMPACT_SUFFIX) else KIND_PGN, p))
    return out


def record_result(terminal: int, final_turn: int) -> int:
    """pgn_write.result_of's rule as a result code: terminals 1 (mate) and 3 (resignation) are a loss for the side to move in the final
    position, 2 is a draw, everything else is unknown."""
    if terminal in (1, 3):
        return 3 if final_turn == 1 else 1
    return 2 if terminal == 2 else 0


def next_pow2(x: int) -> int:
    return 1 << max(0, int(x) - 1).bit_length()


class Corpus:
    """Every input in one device ring.  pos: uint8 [capacity * 80] ring entries; act: int32 [capacity], the played action of a PGN entry;
    ev: float32 [capacity], the entry's eval seen by the side to move (NaN: none).  Per game: its first entry, the number of its
    positions that have a played move, its result code, its kind and its source file."""

    def __init__(self, inputs, device="cuda:0", lib=None):
        self.lib = lib or E.load_hip_library()
        self.dev = E.runtime_device(device)
        lib, dev = self.lib, self.dev
        t0 = time.perf_counter()
        self.files = input_files(inputs)
        parsed = []
        for kind, path in self.files:
            if kind == KIND_PGN:
                data = A._read(path)
                pg = P.parse_chunk(lib, data, 0, True)[0]
                parsed.append((data, pg, pg.n_tokens))
            else:
                with open(path, "rb") as fh:
                    buf = fh.read()
                index = R.scan_games(buf)
                parsed.append((buf, index, sum(n + 1 for _, n, _, _ in index)))
        cap = self.capacity = max(1, sum(p[2] for p in parsed))
        if cap >= 2 ** 31:
            raise ValueError("book: more than 2^31 - 1 positions in the inputs")
        self.t_parse = time.perf_counter() - t0
        t0 = time.perf_counter()
        self.pos = torch.zeros(cap * P.POSITION_BYTES, dtype=torch.uint8, device=dev)
        self.act = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.ev = torch.full((cap,), float("nan"), dtype=torch.float32, device=dev)
        z, smp = torch.zeros(cap, dtype=torch.float32, device=dev), torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_moves = np.full(cap, -1, np.int32)  # the move played from a record's entry
        self.seg_start, self.seg_kind = [], []
        starts, nmoves, results, kinds, srcs = [], [], [], [], []
        self.skipped = {"variant": 0, "bad_fen": 0}
        self.stopped_early = 0
        base = 0
        i64p = C.POINTER(C.c_int64)
        for f, ((kind, path), (data, h, size)) in enumerate(zip(self.files, parsed)):
            self.seg_start.append(base)
            self.seg_kind.append(kind)
            if kind == KIND_PGN:
                pg, G = h, h.n_games
                if G:
                    x = pg.export()
                    tok_off = x["tok_off"].astype(np.int64)
                    slot0 = base + tok_off[:-1]
                    n_plies, status = np.zeros(G, np.int32), np.zeros(G, np.int32)
                    scratch = torch.empty(max(pg.scratch_bytes, 16), dtype=torch.uint8, device=dev)
                    rc = lib.bo_pgn_replay(pg.h, slot0.ctypes.data_as(i64p), cap, scratch.data_ptr(), scratch.numel(), self.pos.data_ptr(),
                                           self.act.data_ptr(), z.data_ptr(), smp.data_ptr(), n_plies.ctypes.data_as(E._I32P),
                                           status.ctypes.data_as(E._I32P), A._stream(dev))
                    if rc != 0:
                        raise E.EngineError(f"bo_pgn_replay: {path}: {lib.bo_last_error().decode()}")
                    b, e = np.zeros(G, np.int64), np.zeros(G, np.int64)
                    if lib.bo_pgn_spans(pg.h, b.ctypes.data_as(i64p), e.ctypes.data_as(i64p)) != 0:
                        raise E.EngineError(f"bo_pgn_spans: {lib.bo_last_error().decode()}")
                    for g in range(G):
                        self.skipped["variant"] += int(status[g] == 1)
                        self.skipped["bad_fen"] += int(status[g] == 2)
                        self.stopped_early += int(status[g] >= 3)
                        text = data[int(b[g]):int(e[g])]
                        starts.append(int(slot0[g])); nmoves.append(int(n_plies[g])); kinds.append(KIND_PGN); srcs.append(f)
                        results.append(RESULT_CODE.get(A.game_result(text, A.game_tags(text)), 0))
                pg.close()
            else:
                mv, raw, evs, o_pos = memoryview(data), [], np.full(size, np.nan, np.float32), 0
                for _gid, n, off, _size in h:
                    head = np.frombuffer(mv[off:off + 24], np.int32)
                    v2 = head[0] == R.MAGIC2
                    o = off + 24 + (4 if v2 else 0)
                    body = np.frombuffer(mv[o:o + R.POS_BYTES * (n + 1)], np.uint8); o += R.POS_BYTES * (n + 1)
                    raw.append(body)
                    self.rec_moves[base + o_pos:base + o_pos + n] = np.frombuffer(mv[o:o + 4 * n], np.int32); o += 4 * n
                    if v2:
                        o += 4 * (n + 1) + 8 * int(head[5])
                        evs[o_pos:o_pos + n] = np.frombuffer(mv[o:o + 4 * n], np.float32)
                    turn = int(body.view(A.BOPOS_DTYPE)["turn"][n])
                    starts.append(base + o_pos); nmoves.append(n); kinds.append(KIND_BOG); srcs.append(f)
                    results.append(record_result(int(head[3]), turn))
                    o_pos += n + 1
                if size:
                    src = torch.from_numpy(np.concatenate(raw)).to(dev)
                    if lib.bo_records_ring(src.data_ptr(), size, self.pos.data_ptr() + base * P.POSITION_BYTES, A._stream(dev)) != 0:
                        raise E.EngineError(f"bo_records_ring: {path}: {lib.bo_last_error().decode()}")
                    self.ev[base:base + size] = torch.from_numpy(evs).to(dev)
                    if dev.type == "cuda":
                        torch.cuda.synchronize(dev)  # (src may go)
            base += size
        self.ev = torch.where(smp == 1, z, self.ev)  # a PGN entry's eval: z where the entry is a sample
        self.g_start, self.g_moves = np.array(starts, np.int64).reshape(-1), np.array(nmoves, np.int64).reshape(-1)
        self.g_result, self.g_kind = np.array(results, np.int32).reshape(-1), np.array(kinds, np.int32).reshape(-1)
        self.g_src = np.array(srcs, np.int32).reshape(-1)
        self.n_games = len(self.g_start)
        self.seg_start, self.seg_kind = np.array(self.seg_start, np.int64), np.array(self.seg_kind, np.int32)
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        self.t_replay = time.perf_counter() - t0

    # ---- the work list -----------------------------------------------------------------------------------------------------------
    def items(self, min_ply: int, max_ply: int) -> Dict[str, np.ndarray]:
        """Game-major, ply-minor: every (game, ply) with min_ply <= ply <= max_ply from which the game played a move."""
        lo = int(min_ply)
        cnt = np.maximum(np.minimum(int(max_ply), self.g_moves - 1) - lo + 1, 0)
        off = np.zeros(self.n_games + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        game = np.repeat(np.arange(self.n_games, dtype=np.int64), cnt)
        ply = lo + np.arange(len(game), dtype=np.int64) - off[:-1][game]
        return dict(game=game, ply=ply.astype(np.int32), entry=self.g_start[game] + ply, back=(ply - lo).astype(np.int32),
                    result=self.g_result[game].astype(np.int32), off=off, lo=lo)

    # ---- host read-outs ------------------------------------------------------------------------------------------------------------
    def entries(self, idx) -> np.ndarray:
        """Ring entries idx -> uint8 [len, 80] on the host."""
        idx = torch.as_tensor(np.asarray(idx, np.int64), device=self.dev)
        return self.pos.view(-1, P.POSITION_BYTES)[idx].cpu().numpy()

    def fens(self, idx) -> List[str]:
        idx = np.asarray(idx, np.int64).reshape(-1)
        if not len(idx):
            return []
        pos, buf, out = A.ring_to_positions(self.entries(idx)), C.create_string_buffer(128), []
        for i in range(len(idx)):
            if self.lib.bo_position_fen(C.byref(pos[i]), buf, 128) != 0:
                raise E.EngineError(f"bo_position_fen: {self.lib.bo_last_error().decode()}")
            out.append(buf.value.decode())
        return out

    def moves_at(self, idx) -> np.ndarray:
        """The move (from | to << 6 | promo << 12) the game played from each entry: the records' moves, bo_pgn_after on a PGN entry."""
        idx = np.asarray(idx, np.int64).reshape(-1)
        out = self.rec_moves[idx].copy() if len(idx) else np.zeros(0, np.int32)
        if not len(idx):
            return out
        pgn = self.seg_kind[np.searchsorted(self.seg_start, idx, side="right") - 1] == KIND_PGN
        for b0 in range(0, int(pgn.sum()), 1 << 30):
            sel = np.nonzero(pgn)[0][b0:b0 + (1 << 30)]
            d_idx = torch.from_numpy(idx[sel]).to(self.dev)
            mv = torch.zeros(len(sel), dtype=torch.int32, device=self.dev)
            if self.lib.bo_pgn_after(self.pos.data_ptr(), self.act.data_ptr(), self.capacity, len(sel), d_idx.data_ptr(), None, mv.data_ptr(),
                                     A._stream(self.dev)) != 0:
                raise E.EngineError(f"bo_pgn_after: {self.lib.bo_last_error().decode()}")
            out[sel] = mv.cpu().numpy()
        return out


class Table:
    """bo_book_insert's table for one work list: the columns (torch, on the device), gid per item (host), T, and how often T doubled."""

    def __init__(self, corpus: Corpus, items: Dict[str, np.ndarray], t0: Optional[int] = None, flags: int = 0):
        self.corpus, self.items = corpus, items
        lib, dev = corpus.lib, corpus.dev
        n = self.n_items = len(items["entry"])
        T = next_pow2(int(t0)) if t0 else next_pow2(max(2 * n, 1))
        d = {k: torch.from_numpy(np.ascontiguousarray(items[k])).to(dev) for k in ("entry", "ply", "result", "back")}
        ev = corpus.ev[d["entry"]] if n else torch.zeros(0, dtype=torch.float32, device=dev)
        gid = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
        self.retries = 0
        t_begin = time.perf_counter()
        while True:
            cols = {name: torch.full((T,), fill, dtype=dt, device=dev) for name, dt, fill in COLUMNS}
            status = torch.zeros(2, dtype=torch.int32, device=dev)
            rc = lib.bo_book_insert(corpus.pos.data_ptr(), corpus.capacity, n, d["entry"].data_ptr(), d["ply"].data_ptr(), d["result"].data_ptr(),
                                    ev.data_ptr() if n else None, d["back"].data_ptr(), T, *[cols[name].data_ptr() for name, _, _ in COLUMNS],
                                    gid.data_ptr(), status.data_ptr(), int(flags), A._stream(dev))
            if rc != 0:
                raise E.EngineError(f"bo_book_insert: {lib.bo_last_error().decode()}")
            over, bad = (int(v) for v in status.cpu().numpy())
            if bad:
                raise E.EngineError(f"bo_book_insert: {bad} work items name entries outside the ring")
            if not over:
                break
            if T >= 2 ** 30:
                raise E.EngineError("bo_book_insert: the table overflows at 2^30 slots")
            T *= 2
            self.retries += 1
        self.t_insert = time.perf_counter() - t_begin
        self.T, self.cols = T, cols
        self.gid = gid.cpu().numpy()[:n]

    def groups(self) -> Dict[str, torch.Tensor]:
        """The occupied slots: `slot` and every column at those slots."""
        slot = torch.nonzero(self.cols["owner"] >= 0).flatten()
        out = {name: self.cols[name][slot] for name, _, _ in COLUMNS}
        out["slot"] = slot
        return out


def select(table: Table, min_games: int = 10, max_bias: float = 0.1, max_eval: Optional[float] = None, max_n: Optional[int] = None,
           allow_nested: bool = False) -> Tuple[List[dict], int]:
    """(the kept groups in book order, how many groups qualified).  A group: slot, first, n, w, d, l, n_eval, sum_eval, min_ply, and game /
    ply of its representative -- the game that holds entry `first`."""
    g = table.groups()
    dec = (g["w"] + g["d"] + g["l"]).double()
    ok = (g["n"] >= int(min_games)) & (dec >= 1)
    score = (g["w"].double() + g["d"].double() / 2) / torch.clamp(dec, min=1.0)
    ok &= (score - 0.5).abs() <= float(max_bias)
    if max_eval is not None:
        mean = g["sum_eval"].double() / EVAL_ONE / torch.clamp(g["n_eval"], min=1).double()
        ok &= (g["n_eval"] == 0) | (mean.abs() <= float(max_eval))
    q = {k: v[ok] for k, v in g.items()}
    order = torch.argsort(q["first"])                                   # first is unique per group: the order is total
    order = order[torch.argsort(q["min_ply"][order], stable=True)]
    order = order[torch.argsort(q["n"][order], descending=True, stable=True)]
    q = {k: v[order].cpu().numpy() for k, v in q.items()}
    n_qual = len(q["slot"])
    c, it = table.corpus, table.items
    game = np.searchsorted(c.g_start, q["first"], side="right") - 1   # (games sit in the ring in increasing order of their first entry)
    ply = q["first"] - c.g_start[game] if n_qual else np.zeros(0, np.int64)
    lo = int(it["lo"])
    kept, kept_gids, covered = [], set(), set()
    for k in range(n_qual):
        if max_n is not None and len(kept) >= int(max_n):
            break
        slot = int(q["slot"][k])
        if not allow_nested:
            # L(X): the groups of the representative game's window items at plies up to X's ply
            i0 = int(it["off"][game[k]])
            line = {int(v) for v in table.gid[i0:i0 + int(ply[k]) - lo + 1] if v >= 0}
            if slot in covered or (line & kept_gids):
                continue
            covered |= line
        kept_gids.add(slot)
        kept.append(dict(slot=slot, game=int(game[k]), ply=int(ply[k]), **{name: int(q[name][k]) for name in
                                                                          ("first", "n", "w", "d", "l", "n_eval", "sum_eval", "min_ply")}))
    return kept, n_qual


def _uci(moves) -> str:
    return " ".join(E.move_to_uci(int(m)) for m in moves)


def eval_text(g: dict) -> str:
    return f"{g['sum_eval'] / EVAL_ONE / g['n_eval']:+.3f}" if g["n_eval"] else "-"


def book_lines(corpus: Corpus, kept: List[dict]) -> List[str]:
    """One line per kept group: the representative game's root, the moves to the position, the counts as a comment."""
    roots = corpus.fens([corpus.g_start[g["game"]] for g in kept])
    ent = np.concatenate([corpus.g_start[g["game"]] + np.arange(g["ply"]) for g in kept]).astype(np.int64) if kept else np.zeros(0, np.int64)
    mv, out, o = corpus.moves_at(ent), [], 0
    for g, fen in zip(kept, roots):
        g["root"], g["moves"] = ("startpos" if fen == START_FEN else fen), _uci(mv[o:o + g["ply"]])
        o += g["ply"]
        out.append(f"{g['root']} ; {g['moves']} # n={g['n']} w={g['w']} d={g['d']} l={g['l']} eval={eval_text(g)} ply={g['min_ply']}")
    return out


def replies(table: Table, kept: List[dict]) -> Dict[int, List[dict]]:
    """Per kept slot: the moves the games played from the position, with counts and white's score, most played first (host work over
    gid_out and the moves of the kept groups' items only)."""
    c, it = table.corpus, table.items
    idx = np.nonzero(np.isin(table.gid, np.array([g["slot"] for g in kept], np.int32)))[0] if kept else np.zeros(0, np.int64)
    mv = c.moves_at(it["entry"][idx])
    acc: Dict[int, Dict[int, List[int]]] = {}
    for i, m in zip(idx, mv):
        r = acc.setdefault(int(table.gid[i]), {}).setdefault(int(m), [0, 0, 0, 0])
        r[0] += 1
        if it["result"][i] in (1, 2, 3):
            r[int(it["result"][i])] += 1
    out = {}
    for slot, by in acc.items():
        rows = []
        for m, (n, w, d, l) in sorted(by.items(), key=lambda kv: (-kv[1][0], kv[0])):
            rows.append(dict(move=E.move_to_uci(m), n=n, w=w, d=d, l=l, score=((w + d / 2) / (w + d + l) if w + d + l else None)))
        out[slot] = rows
    return out


def build_book(inputs, out_path: Optional[str] = None, min_ply: int = 8, max_ply: int = 16, min_games: int = 10, max_bias: float = 0.1,
               max_eval: Optional[float] = None, max_n: Optional[int] = None, allow_nested: bool = False, json_path: Optional[str] = None,
               device="cuda:0", t0: Optional[int] = None, flags: int = 0, corpus: Optional[Corpus] = None) -> dict:
    """The whole command as a function -> the report (what --json writes, plus "lines" and "text")."""
    if min_ply < 0 or max_ply < min_ply:
        raise ValueError("book: 0 <= --min-ply <= --max-ply")
    c = corpus or Corpus(inputs, device)
    t = time.perf_counter()
    it = c.items(min_ply, max_ply)
    tab = Table(c, it, t0=t0, flags=flags)
    t_insert = time.perf_counter() - t
    t = time.perf_counter()
    kept, n_qual = select(tab, min_games, max_bias, max_eval, max_n, allow_nested)
    n_groups = int((tab.cols["owner"] >= 0).sum())
    t_select = time.perf_counter() - t
    t = time.perf_counter()
    lines = book_lines(c, kept)
    text = "".join(l + "\n" for l in lines)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    rep = dict(inputs=[p for _, p in c.files], window=[int(min_ply), int(max_ply)], games=int(c.n_games), games_skipped=dict(c.skipped),
               games_stopped_early=int(c.stopped_early), positions=int(c.capacity), items=int(tab.n_items),
               items_skipped=int((tab.gid == -1).sum()), groups=n_groups, table_slots=int(tab.T), table_retries=int(tab.retries),
               qualifying=int(n_qual), kept=len(kept))
    book = None
    if json_path:
        rp, fens = replies(tab, kept), c.fens([g["first"] for g in kept])
        book = [dict(fen=f, root=g["root"], moves=g["moves"], n=g["n"], w=g["w"], d=g["d"], l=g["l"], n_eval=g["n_eval"],
                     eval=(g["sum_eval"] / EVAL_ONE / g["n_eval"] if g["n_eval"] else None), min_ply=g["min_ply"], first=g["first"],
                     replies=rp.get(g["slot"], [])) for g, f in zip(kept, fens)]
    # (write: the lines, the book file and the report's positions; the report file itself is written after the clock is read)
    rep["seconds"] = dict(parse=c.t_parse, replay=c.t_replay, insert=t_insert, insert_calls=tab.t_insert, select=t_select,
                          write=time.perf_counter() - t)
    if json_path:
        with open(json_path, "w") as f:
            json.dump(dict(rep, book=book), f, indent=1)
            f.write("\n")
    return dict(rep, lines=lines, text=text, kept_groups=kept, table=tab)


def summary_text(rep: dict) -> str:
    s = rep["seconds"]
    return (f"[book] games {rep['games']}  items {rep['items']}  groups {rep['groups']}  qualifying {rep['qualifying']}  kept {rep['kept']}  "
            f"(parse {s['parse']:.3f} s, replay {s['replay']:.3f} s, insert {s['insert']:.3f} s, select {s['select']:.3f} s, write {s['write']:.3f} s)")


def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.book", description="opening books from PGN games and self-play records")
    ap.add_argument("inputs", nargs="+", metavar="INPUT", help="PGN files or directories, .bog files or iteration directories")
    ap.add_argument("-o", "--output", required=True, metavar="BOOK", help="one opening per line, as match --openings reads it")
    ap.add_argument("--min-ply", type=int, default=8, help="first ply of the window (plies count from a game's root, 0 = the root)")
    ap.add_argument("--max-ply", type=int, default=16, help="last ply of the window")
    ap.add_argument("--min-games", type=int, default=10, help="games that must reach a position")
    ap.add_argument("--max-bias", type=float, default=0.1, help="largest |white's score - 0.5| over the decided games")
    ap.add_argument("--max-eval", type=float, default=None, metavar="E", help="largest |mean eval| in white's view, where a position has evals")
    ap.add_argument("--max", type=int, default=None, dest="max_n", metavar="N", help="keep the first N positions")
    ap.add_argument("--allow-nested", action="store_true", help="keep positions that lie on, or continue, a kept position's line")
    ap.add_argument("--json", default=None, metavar="REPORT", help="counts, timings and, per kept position, its FEN and the moves played from it")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    try:
        rep = build_book(a.inputs, a.output, a.min_ply, a.max_ply, a.min_games, a.max_bias, a.max_eval, a.max_n, a.allow_nested, a.json, a.device)
    except (ValueError, OSError) as e:
        print(f"book: {e}", file=sys.stderr)
        return 2
    print(summary_text(rep), file=out)
    if not rep["kept"]:
        print(f"book: no position qualifies ({rep['groups']} groups from {rep['items']} items): {a.output} is empty; "
              "try a lower --min-games, a wider --max-bias or another window", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
