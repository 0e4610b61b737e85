"""betaone_amd/reanalyse.py -- fresh search targets for old self-play records.

    python -m betaone_amd.reanalyse DATA_DIR/iter_N [more ...] --model best.pth -o OUT_DIR
           [--sims S] [--slots G] [--pi-width W] [--fraction F --seed K] [--values]
           [--report report.json] [--device cuda:0]

A .bog record keeps the pi and the root value the net of its iteration produced.  This tool searches the stored positions again with
another net -- the current best -- and writes OUT_DIR/iter_N/<same file names>.bog with the new pi (and, for records with root
values, the new root values); header, positions, moves, terminal, outcome, game id and flags are kept, so every reader of .bog files
takes the output unchanged.  No game is replayed: the positions of a file are uploaded in one copy, become ring entries on the device
(bo_records_ring, csrc/bo_reanalyse.h) and from there on the path is analyse's -- slots set up from the device, searches begun on the
device, Rollout's captured evaluate -> step graph, one record per root read from double-buffered pinned memory with no host wait
(analyse.Analyser; Reanalyser below replaces its read-out by bo_reanalysis_result: a 16-word record and a pi row of --pi-width entries
per slot).  Dirichlet noise is off: a search is a function of its root and the net, so reanalysing with the net, simulation count,
search constants and slot count that played the games gives the input back byte for byte.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import analyse as A
from . import engine as E
from . import pgn as P
from . import records as R
from . import validate as V


def moves_to_actions(moves: np.ndarray) -> np.ndarray:
    """Action indices of moves (from | to << 6 | promo << 12): csrc/bo_chess.h move_to_index, on arrays."""
    m = np.asarray(moves, dtype=np.int64)
    fr, to, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    dr, df = (to >> 3) - (fr >> 3), (to & 7) - (fr & 7)
    adr, adf = np.abs(dr), np.abs(df)
    under = fr * 73 + 64 + (promo - 2) * 3 + (df + 1)
    k = np.where(dr == 2, np.where(df == 1, 0, 7), np.where(dr == 1, np.where(df == 2, 1, 6), np.where(dr == -1, np.where(df == 2, 2, 5),
                                                                                                        np.where(df == 1, 3, 4))))
    knight = fr * 73 + 56 + k
    sr, sf = np.sign(dr), np.sign(df)
    d = np.where(sr == 1, np.where(sf == 0, 0, np.where(sf == 1, 1, 7)), np.where(sr == 0, np.where(sf == 1, 2, 6),
                                                                                   np.where(sf == 1, 3, np.where(sf == 0, 4, 5))))
    queen = fr * 73 + d * 7 + (np.maximum(adr, adf) - 1)
    is_knight = ((adr == 1) & (adf == 2)) | ((adr == 2) & (adf == 1))
    return np.where((promo != 0) & (promo != 5), under, np.where(is_knight, knight, queen)).astype(np.int32)


class RecordFile:
    """One .bog file ingested for analyse.Analyser: pos (ring entries of every position of every game, game g's in entries tok_off[g] ..),
    the work list -- every (game, ply) with ply < n_plies of the selected games, in file order -- and the old pi on the device."""

    def __init__(self, lib, dev, path: str, iteration: int = 0, fraction: float = 1.0, seed: int = 0):
        self.name = self.path = path
        with open(path, "rb") as fh:
            buf = fh.read()
        self.index = R.scan_games(buf)
        self.buf = buf[:self.index[-1][2] + self.index[-1][3]] if self.index else b""  # (a truncated tail is cut, as complete_prefix_bytes does)
        G = self.n_games = len(self.index)
        mv = memoryview(self.buf)
        self.n_plies = np.array([g[1] for g in self.index], np.int32).reshape(G)
        self.game_ids = np.array([g[0] for g in self.index], np.int64).reshape(G)
        self.v2 = np.zeros(G, bool)
        self.body_off = np.zeros(G, np.int64)   # byte offset of positions[0]
        self.n_ent = np.zeros(G, np.int64)
        pos, moves, ptrs, idxs, vals, rvs = [], [], [], [], [], []
        for g, (_gid, n, off, _size) in enumerate(self.index):
            head = np.frombuffer(mv[off:off + 24], np.int32)
            self.v2[g] = head[0] == R.MAGIC2
            nent = int(head[5])
            o = off + 24 + (4 if self.v2[g] else 0)
            self.body_off[g], self.n_ent[g] = o, nent
            pos.append(np.frombuffer(mv[o:o + R.POS_BYTES * (n + 1)], np.uint8)); o += R.POS_BYTES * (n + 1)
            moves.append(np.frombuffer(mv[o:o + 4 * n], np.int32)); o += 4 * n
            ptr = np.frombuffer(mv[o:o + 4 * (n + 1)], np.int32); o += 4 * (n + 1)
            idxs.append(np.frombuffer(mv[o:o + 4 * nent], np.int32)); o += 4 * nent
            vals.append(np.frombuffer(mv[o:o + 4 * nent], np.float32)); o += 4 * nent
            rvs.append(np.frombuffer(mv[o:o + 4 * n], np.float32) if self.v2[g] else np.zeros(n, np.float32))
            if n and (ptr[0] != 0 or ptr[-1] != nent or (np.diff(ptr) < 0).any()):
                raise ValueError(f"reanalyse: {path}: game {_gid}: its pi offsets are not a partition of its pi entries")
            ptrs.append(ptr)
        self.tok_off = np.zeros(G + 1, np.int64)
        np.cumsum(self.n_plies.astype(np.int64) + 1, out=self.tok_off[1:])
        self.T = max(int(self.tok_off[-1]), 1)
        self.selected = np.array([V.is_held_out(iteration, int(gid), fraction, seed) for gid in self.game_ids], bool).reshape(G)
        sel_n = np.where(self.selected, self.n_plies, 0)
        self.w_game = np.repeat(np.arange(G, dtype=np.int64), sel_n)
        self.w_ply = (np.arange(len(self.w_game), dtype=np.int64) - np.repeat(np.cumsum(sel_n) - sel_n, sel_n)).astype(np.int32)
        self.n_roots = len(self.w_game)
        # per root of the FILE (every ply of every game, selected or not): its moves, old pi and old value, concatenated in file order
        cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dt)
        self.root_off = np.zeros(G + 1, np.int64)
        np.cumsum(self.n_plies, out=self.root_off[1:])
        self.ent_off = np.zeros(G + 1, np.int64)
        np.cumsum(self.n_ent, out=self.ent_off[1:])
        if int(self.ent_off[-1]) >= 2 ** 31:
            raise ValueError(f"reanalyse: {path}: more than 2^31 pi entries in one file")
        self.all_moves = cat(moves, np.int32)
        self.old_ptr = np.zeros(int(self.root_off[-1]) + 1, np.int32)
        for g in range(G):
            self.old_ptr[self.root_off[g] + 1:self.root_off[g + 1] + 1] = ptrs[g][1:] + self.ent_off[g]
        self.old_idx, self.old_val, self.old_rv = cat(idxs, np.int32), cat(vals, np.float32), cat(rvs, np.float32)
        self.w_root = self.root_off[self.w_game] + self.w_ply          # the work list's roots as indices into old_ptr
        self.moves = self.all_moves[self.w_root]                       # (Analyser's interface; the device gets action indices)
        self.actions = moves_to_actions(self.moves)
        # the device side: one upload of every position, one kernel
        t0 = time.perf_counter()
        raw = cat(pos, np.uint8)
        self.pos = torch.zeros(self.T * P.POSITION_BYTES, dtype=torch.uint8, device=dev)
        self.t_upload = self.t_ring = 0.0
        if len(raw):
            src = torch.from_numpy(raw.copy()).to(dev)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            self.t_upload = time.perf_counter() - t0
            t1 = time.perf_counter()
            if lib.bo_records_ring(src.data_ptr(), len(raw) // R.POS_BYTES, self.pos.data_ptr(), A._stream(dev)) != 0:
                raise E.EngineError(f"bo_records_ring: {lib.bo_last_error().decode()}")
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)  # (src may go; and the time below is the kernel's)
            self.t_ring = time.perf_counter() - t1
        self.old_dev = tuple(torch.from_numpy(a if len(a) else np.zeros(1, a.dtype)).to(dev) for a in (self.old_ptr, self.old_idx, self.old_val))

    def work_arrays(self, dev, G: int, order: Optional[np.ndarray] = None):
        """analyse.Ingested.work_arrays with the played ACTION and, fifth, each root's index into the file's old pi."""
        order = np.arange(self.n_roots) if order is None else np.asarray(order, dtype=np.int64)
        n = len(order)
        nb = max(1, -(-n // G))
        first, ply = np.zeros(nb * G, np.int64), np.full(nb * G, -1, np.int32)
        played, want, root = np.full(nb * G, -1, np.int32), np.zeros(nb * G, np.int32), np.full(nb * G, -1, np.int64)
        first[:n], ply[:n], played[:n], want[:n], root[:n] = self.tok_off[self.w_game[order]], self.w_ply[order], self.actions[order], 1, self.w_root[order]
        return tuple(torch.from_numpy(a).to(dev) for a in (first, ply, played, want, root)) + (nb,)


class Reanalyser(A.Analyser):
    """analyse.Analyser with bo_reanalysis_result as its read-out: per slot a bo_reanalysis record and a pi row of W entries, one pinned
    block [G, 16 + 2 W] per batch."""

    NAME = "reanalyse"
    RECORD_DTYPE = E.REANALYSIS_DTYPE

    def __init__(self, model, slots: int, sims: int, max_plies: int, device, pi_width: int = 8, **kw):
        self.W = int(pi_width)
        if not 1 <= self.W <= E.RES_CAP:
            raise ValueError(f"reanalyse: --pi-width must be 1 .. {E.RES_CAP}")
        super().__init__(model, slots, sims, max_plies, device, **kw)
        self.file: Optional[RecordFile] = None

    def _make_buffers(self, cuda: bool):
        G, W = self.G, self.W
        # one block per batch: [G * 16 record words | G * W pi indices | G * W pi values]
        self.out_dev = torch.zeros(G * (16 + 2 * W), dtype=torch.int32, device=self.dev)
        self.out_dev[G * 16:G * (16 + W)] = -1
        self.pinned = [torch.zeros(G * (16 + 2 * W), dtype=torch.int32, pin_memory=cuda) for _ in range(2)]
        self.batch_bytes = 4 * G * (16 + 2 * W)

    def _soft_bits(self) -> int:
        return self.eng.soft_status_bits() | E.ST_PI_OVERFLOW

    def begin_file(self, f: RecordFile):
        self.file = f
        self.pi_n = np.zeros(f.n_roots, np.int32)
        self.pi_idx = np.full((f.n_roots, self.W), -1, np.int32)
        self.pi_val = np.zeros((f.n_roots, self.W), np.float32)

    def _records(self, arrays, b: int, buf: int):
        G, W, f = self.G, self.W, self.file
        base = self.out_dev.data_ptr()
        self.eng.reanalysis_result(arrays[2].data_ptr() + 4 * b * G, arrays[4].data_ptr() + 8 * b * G, f.old_dev[0].data_ptr(), f.old_dev[1].data_ptr(),
                                   f.old_dev[2].data_ptr(), W, base, base + 4 * G * 16, base + 4 * G * (16 + W), A._stream(self.dev))
        self.pinned[buf].copy_(self.out_dev, non_blocking=True)
        self._recorded(buf)

    def _read(self, buf: int) -> np.ndarray:
        G, W = self.G, self.W
        blk = self.pinned[buf].numpy().copy()
        self._rows = (blk[G * 16:G * (16 + W)].reshape(G, W), blk[G * (16 + W):].view(np.float32).reshape(G, W))
        return blk[:G * 16].view(self.RECORD_DTYPE).reshape(G)

    def _took(self, ids: np.ndarray, rows: np.ndarray):
        # (a slot that did not search leaves its rows as the previous batch had them: only searched roots are read)
        self.pi_idx[ids], self.pi_val[ids] = self._rows[0][rows], self._rows[1][rows]


def _inputs(paths: Sequence[str]) -> List[tuple]:
    """[(iteration, directory, [files])] of DATA_DIR/iter_N directories, in the order given."""
    out = []
    for p in ([paths] if isinstance(paths, str) else list(paths)):
        m = re.search(r"iter_(\d+)$", os.path.normpath(p))
        if not m or not os.path.isdir(p):
            raise ValueError(f"reanalyse: {p}: not a DATA_DIR/iter_N directory")
        files = sorted(glob.glob(os.path.join(p, "*" + R.COMPACT_SUFFIX)))
        if not files:
            raise ValueError(f"reanalyse: {p} holds no compact records (*{R.COMPACT_SUFFIX})")
        out.append((int(m.group(1)), p, files))
    return out


def _inside(child: str, parent: str) -> bool:
    c, p = os.path.realpath(child), os.path.realpath(parent)
    return c == p or c.startswith(p.rstrip(os.sep) + os.sep)


def _write_file(f: RecordFile, rec: np.ndarray, an: Reanalyser, values: bool, out_path: str) -> None:
    """The file's games with the searched roots' pi (and root values) replaced; every other byte as in the input."""
    searched = rec["phase"] == E.PH_DONE
    new_n = np.minimum(rec["pi_n"], an.W)
    start = np.cumsum(np.where(f.selected, f.n_plies, 0)) - np.where(f.selected, f.n_plies, 0)   # a selected game's first work-list root
    parts = []
    for g, (gid, n, off, size) in enumerate(f.index):
        blob = f.buf[off:off + size]
        if not f.selected[g] or n == 0:                     # copied byte for byte
            parts.append(blob)
            continue
        w0, r0 = int(start[g]), int(f.root_off[g])
        s = searched[w0:w0 + n]
        counts = np.where(s, new_n[w0:w0 + n], np.diff(f.old_ptr[r0:r0 + n + 1]))
        ptr = np.zeros(n + 1, np.int32)
        np.cumsum(counts, out=ptr[1:])
        idx, val = np.zeros(int(ptr[-1]), np.int32), np.zeros(int(ptr[-1]), np.float32)
        for k in range(n):
            a, b = int(ptr[k]), int(ptr[k + 1])
            if s[k]:
                idx[a:b], val[a:b] = an.pi_idx[w0 + k, :b - a], an.pi_val[w0 + k, :b - a]
            else:                                           # not searched (a claim-draw or mate root, a refused slot): the old pi stays
                oa = int(f.old_ptr[r0 + k])
                idx[a:b], val[a:b] = f.old_idx[oa:oa + b - a], f.old_val[oa:oa + b - a]
        head = np.frombuffer(blob[:24], np.int32).copy()
        head[5] = len(idx)
        pre = int(f.body_off[g] - off)                      # the header (and a BOG2 record's flags)
        body_end = pre + R.POS_BYTES * (n + 1) + 4 * n      # ... positions and moves
        flags = blob[24:pre]
        rv = b""
        if f.v2[g] or values:
            rv = np.where(s, rec["root_value"][w0:w0 + n], f.old_rv[r0:r0 + n]).astype(np.float32).tobytes()
            if not f.v2[g]:                                 # BOG1 with --values: a BOG2 record, flags 0
                head[0], flags = R.MAGIC2, np.zeros(1, np.int32).tobytes()
        parts.append(b"".join([head.tobytes(), flags, blob[pre:body_end], ptr.tobytes(), idx.tobytes(), val.tobytes(), rv]))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "xb") as fh:
        fh.write(b"".join(parts))


def reanalyse_records(paths, model, out_dir: str, sims: Optional[int] = None, slots: int = 256, pi_width: int = 8, fraction: float = 1.0,
                      seed: int = 0, values: bool = False, device="cuda:0", use_graph: bool = True, mcts_batch_size: Optional[int] = None,
                      iterations: Optional[int] = None, **search_cfg) -> Dict:
    """Reanalyse the compact records of the DATA_DIR/iter_N directories `paths` with `model`; write out_dir/iter_N/<same names>.  Returns
    the report (a dict).  fraction / seed: only games with validate.holdout_hash(iteration, game_id, seed) < fraction * 2^64 are searched,
    the others are copied byte for byte.  values: records without root values are written as BOG2 (flags 0) with the new ones."""
    from . import pgn_write as W

    if search_cfg.pop("fast", False):
        raise ValueError("reanalyse: fast mode is not supported (the reference's search semantics only)")
    if getattr(model, "is_pair", False):
        raise ValueError("reanalyse: two-net reanalysis is not supported")
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("reanalyse: --fraction must lie in [0, 1]")
    if not 1 <= int(pi_width) <= E.RES_CAP:
        raise ValueError(f"reanalyse: --pi-width must be 1 .. {E.RES_CAP}")
    inputs = _inputs(paths)
    for _it, d, _files in inputs:
        if _inside(out_dir, d):
            raise ValueError(f"reanalyse: the output directory {out_dir} is, or lies inside, the input directory {d}")
    todo = []
    for it, d, files in inputs:
        for p in files:
            o = os.path.join(out_dir, f"iter_{it}", os.path.basename(p))
            if os.path.exists(o):
                raise ValueError(f"reanalyse: {o} exists already")
            todo.append((it, p, o))
    if len({o for _, _, o in todo}) != len(todo):
        raise ValueError("reanalyse: two inputs name the same iteration")
    if sims is None:
        sims = W._default_sims()
    t0 = time.perf_counter()
    lib = E.load_hip_library()
    dev = E.runtime_device(device)
    longest = 0
    for _it, p, _o in todo:  # the engine is sized once, for the longest game of all inputs (headers only)
        with open(p, "rb") as fh:
            longest = max([longest] + [g[1] for g in R.scan_games(fh.read())])
    from .nn_tune import best_inference_copy

    net = best_inference_copy(model, int(slots), dev) if hasattr(model, "for_inference") else model
    an = Reanalyser(net, slots, sims, longest + 2, dev, pi_width=pi_width, mcts_batch_size=mcts_batch_size, use_graph=use_graph,
                    iterations=iterations, **search_cfg)
    tot = dict(games=0, games_selected=0, roots=0, searched=0, kept=0, tv=0.0, agree=0, has_old=0, played=0.0, dq=0.0, flips=0, with_q=0)
    t_search = t_upload = t_ring = 0.0
    files_rep = []
    try:
        for it, p, o in todo:
            f = RecordFile(lib, dev, p, iteration=it, fraction=fraction, seed=seed)
            an.begin_file(f)
            t1 = time.perf_counter()
            rec = an.run(f)
            t_search += time.perf_counter() - t1
            t_upload, t_ring = t_upload + f.t_upload, t_ring + f.t_ring
            s = rec["phase"] == E.PH_DONE
            over = s & ((rec["status"] & E.ST_PI_OVERFLOW) != 0)
            if over.any():
                k = int(np.nonzero(over)[0][0])
                raise E.EngineError(f"reanalyse: {p} game {int(f.game_ids[f.w_game[k]])} ply {int(f.w_ply[k])}: the search's pi has "
                                    f"{int(rec['pi_n'][k])} entries, the rows hold {an.W}: raise --pi-width")
            _write_file(f, rec, an, values, o)
            ho = s & (rec["has_old"] != 0)
            tot["games"] += f.n_games
            tot["games_selected"] += int(f.selected.sum())
            tot["roots"] += int(f.n_plies.sum())
            tot["searched"] += int(s.sum())
            tot["kept"] += int(f.n_plies.sum()) - int(s.sum())
            tot["tv"] += float(rec["tv"][ho].astype(np.float64).sum())
            tot["agree"] += int(rec["agree"][ho].sum())
            tot["has_old"] += int(ho.sum())
            tot["played"] += float(rec["played_prob"][s].astype(np.float64).sum())
            q = s & f.v2[f.w_game]
            qo, qn = f.old_rv[f.w_root[q]].astype(np.float64), rec["root_value"][q].astype(np.float64)
            tot["dq"] += float(np.abs(qn - qo).sum())
            tot["flips"] += int(((qn > 0) != (qo > 0)).sum())
            tot["with_q"] += int(q.sum())
            files_rep.append(dict(input=p, output=o, games=f.n_games, roots_searched=int(s.sum()), upload_seconds=f.t_upload, ring_seconds=f.t_ring))
    finally:
        an.close()
    n_s, n_o, n_q = tot["searched"], tot["has_old"], tot["with_q"]
    return {
        "games": tot["games"], "games_reanalysed": tot["games_selected"], "roots": tot["roots"], "roots_searched": n_s, "roots_kept": tot["kept"],
        "roots_retried": an.n_retried, "mean_tv": tot["tv"] / n_o if n_o else None, "top1_agreement": tot["agree"] / n_o if n_o else None,
        "mean_played_prob": tot["played"] / n_s if n_s else None, "roots_with_values": n_q,
        "mean_abs_dq": tot["dq"] / n_q if n_q else None, "q_sign_changed_share": tot["flips"] / n_q if n_q else None,
        "sims": int(sims), "slots": int(slots), "pi_width": int(pi_width), "fraction": float(fraction), "seed": int(seed), "batches": an.n_batches,
        "batch_copy_bytes": an.batch_bytes, "seconds": time.perf_counter() - t0, "search_seconds": t_search, "upload_seconds": t_upload,
        "ring_seconds": t_ring, "roots_per_second": (n_s / t_search) if t_search > 0 else None, "files": files_rep,
    }


def summary_text(rep: Dict) -> str:
    f = lambda v, fmt: "-" if v is None else format(v, fmt)
    line = (f"[reanalyse] games {rep['games']} (reanalysed {rep['games_reanalysed']})  roots searched {rep['roots_searched']}, kept "
            f"{rep['roots_kept']}, retried {rep['roots_retried']}  mean tv {f(rep['mean_tv'], '.4f')}  top-1 agreement "
            f"{f(rep['top1_agreement'], '.3f')}  mean played prob {f(rep['mean_played_prob'], '.4f')}")
    if rep["roots_with_values"]:
        line += f"  mean |dq| {f(rep['mean_abs_dq'], '.4f')}  q sign changed {f(rep['q_sign_changed_share'], '.3f')}"
    return line + f"  {rep['seconds']:.1f} s, {f(rep['roots_per_second'], '.1f')} roots/s at {rep['sims']} simulations"


def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.reanalyse",
                                 description="Search the positions of self-play records again with a newer net; write records with the new pi and root values.")
    ap.add_argument("dirs", nargs="+", metavar="DATA_DIR/iter_N", help="directories with compact records")
    ap.add_argument("--model", required=True, metavar="CHECKPOINT.pth")
    ap.add_argument("-o", "--out", required=True, metavar="OUT_DIR", help="gets OUT_DIR/iter_N/<same file names>")
    ap.add_argument("--sims", type=int, default=None, help="simulations per position (default: config.NUM_SIMULATIONS)")
    ap.add_argument("--slots", type=int, default=256, help="roots searched together")
    ap.add_argument("--pi-width", type=int, default=8, metavar="W", help="most entries a new pi may have")
    ap.add_argument("--fraction", type=float, default=1.0, metavar="F", help="reanalyse this share of the games (chosen by validate.holdout_hash)")
    ap.add_argument("--seed", type=int, default=0, metavar="K")
    ap.add_argument("--values", action="store_true", help="give records without root values the new ones (they are written as BOG2)")
    ap.add_argument("--report", default=None, metavar="FILE")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from .match import build_net, load_state_dict

    try:
        dev = E.runtime_device(args.device)
        model = build_net(load_state_dict(args.model), dev)
        rep = reanalyse_records(args.dirs, model, args.out, sims=args.sims, slots=args.slots, pi_width=args.pi_width, fraction=args.fraction,
                                seed=args.seed, values=args.values, device=args.device)
    except (ValueError, E.EngineError) as ex:
        print(str(ex) if str(ex).startswith("reanalyse:") else f"reanalyse: {ex}", file=sys.stderr)
        return 2
    if args.report:
        with open(args.report, "w", encoding="utf-8") as fh:
            json.dump(rep, fh, indent=1)
            fh.write("\n")
    out.write(summary_text(rep) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
