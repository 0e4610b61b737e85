"""betaone_amd/perft.py -- perft on the GPU: node counts, divide, move statistics and a move-ORDER checksum.

perft(d) is the number of move sequences of length d from a position (python-chess Board perft: draw rules ignored, only a position
without legal moves ends a line) -- the tool one reaches for first to trust a move generator, or to time it.  The walk runs on the
device (bo_perft, csrc/bo_perft.h): the tree level by level in HBM, one wavefront per position, with the move generator and make_move
the searches run.

    perft("r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", 4, divide=True)[0].nodes    # 4085603
    python -m betaone_amd.perft --depth 6 --divide
    python -m betaone_amd.perft "FEN" --depth 5 --stats --order --json out.json
    python -m betaone_amd.perft --epd suite.epd --max-depth 5

stats=True counts, over the positions at depth d: captures (en passant included), en-passant captures, castling moves, promotions (each
by the LAST move), checks, checkmates and stalemates -- the breakdown the published perft tables give.  It makes every leaf and
generates its moves, where the plain count adds up the move counts of depth d - 1.  order=True returns the sum mod 2^64, over every
position at depth 0 .. d - 1, of the FNV-1a hash of its move list in generated order (h = 0xcbf29ce484222325; h = (h ^ m) *
0x100000001b3 per move word m = from | to << 6 | promo << 12): swap two moves anywhere in the tree and it changes.

capacity = positions per level buffer (>= 256).  A level whose children do not fit is walked in chunks; the results do not depend on
it, `splits` says how many extra chunks there were.

EPD mode reads the usual perft-suite lines `FEN ;D1 20 ;D2 400 ...`, runs every listed depth up to --max-depth, prints one line per
position and exits 1 if any count differs.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import engine as E

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
DEFAULT_CAPACITY = 1 << 23   # positions per level buffer: 96 bytes each, allocated as far as a level grows
MIN_CAPACITY, MAX_MOVES = 256, 256
DIVIDE, STATS, ORDER = 1, 2, 4  # BO_PERFT_* (include/betaone_engine.h)
STAT_NAMES = ("captures", "en_passant", "castles", "promotions", "checks", "checkmates", "stalemates")


class BoPerftResult(C.Structure):  # bo_perft_result
    _fields_ = [("nodes", C.c_uint64), ("checksum", C.c_uint64), ("stats", C.c_uint64 * 7), ("n_moves", C.c_int32), ("reserved", C.c_int32)]


@dataclass
class PerftResult:
    fen: str
    depth: int
    nodes: int
    moves: Optional[List[tuple]] = None      # divide: [(uci, nodes below it)] in generated order
    stats: Optional[Dict[str, int]] = None   # stats: STAT_NAMES -> count
    checksum: Optional[int] = None           # order
    splits: int = 0                          # of the whole call
    seconds: float = 0.0                     # of the whole call (the device call, synchronised)

    def to_json(self) -> dict:
        d = {"fen": self.fen, "depth": self.depth, "nodes": self.nodes, "splits": self.splits, "seconds": self.seconds}
        if self.moves is not None:
            d["divide"] = [[u, n] for u, n in self.moves]
        if self.stats is not None:
            d["stats"] = dict(self.stats)
        if self.checksum is not None:
            d["checksum"] = f"0x{self.checksum:016x}"
        return d


def perft(fens: Union[None, str, Sequence[Optional[str]]], depth: int, *, divide: bool = False, stats: bool = False, order: bool = False,
          capacity: int = DEFAULT_CAPACITY, device="cuda:0", lib=None) -> List[PerftResult]:
    """perft(depth) of every FEN (None = the start position) in one device call on torch's current stream of `device`."""
    lib = lib or E.load_hip_library()
    dev = E.runtime_device(device)
    if fens is None or isinstance(fens, str):
        fens = [fens]
    fens = [START_FEN if f is None else f for f in fens]
    n = len(fens)
    arr = (C.c_char_p * max(n, 1))(*[f.encode() for f in fens])
    res = (BoPerftResult * max(n, 1))()
    mv = np.full((n, MAX_MOVES), -1, np.int32)
    cnt = np.zeros((n, MAX_MOVES), np.uint64)
    splits = C.c_int64(0)
    flags = (DIVIDE if divide else 0) | (STATS if stats else 0) | (ORDER if order else 0)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
    else:
        stream = 0
    t0 = time.perf_counter()
    rc = lib.bo_perft(int(dev.index or 0), n, arr, int(depth), int(capacity), flags, C.addressof(res), mv.ctypes.data, cnt.ctypes.data,
                      C.byref(splits), stream)
    dt = time.perf_counter() - t0
    if rc != 0:
        msg = f"bo_perft: {lib.bo_last_error().decode()}"
        raise (ValueError if rc == -4 else E.EngineError)(msg)
    out = []
    for i in range(n):
        r = PerftResult(fens[i], int(depth), int(res[i].nodes), splits=int(splits.value), seconds=dt)
        if divide:
            k = int(res[i].n_moves)
            r.moves = [(E.move_to_uci(int(mv[i, j])), int(cnt[i, j])) for j in range(k)]
        if stats:
            r.stats = {name: int(res[i].stats[j]) for j, name in enumerate(STAT_NAMES)}
        if order:
            r.checksum = int(res[i].checksum)
        out.append(r)
    return out


def parse_epd(text: str) -> List[tuple]:
    """[(line number, fen, {depth: nodes})] of perft-suite lines `FEN ;D1 20 ;D2 400 ...` ('#' lines and blank lines are skipped)."""
    out = []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        parts = [p.strip() for p in line.split(";")]
        want = {}
        for p in parts[1:]:
            f = p.split()
            if len(f) != 2 or f[0][:1] not in "Dd" or not f[0][1:].isdigit() or not f[1].isdigit():
                raise ValueError(f"line {ln}: expected `D<depth> <nodes>`, got {p!r}")
            want[int(f[0][1:])] = int(f[1])
        out.append((ln, parts[0], want))
    return out


def run_epd(path: str, max_depth: Optional[int], capacity: int, device, out=None) -> int:
    out = out or sys.stdout
    suite = parse_epd(open(path).read())
    got = [dict() for _ in suite]
    depths = sorted({d for _, _, w in suite for d in w if max_depth is None or d <= max_depth})
    nodes, secs = 0, 0.0
    for d in depths:  # every position that lists this depth, in one call
        idx = [i for i, (_, _, w) in enumerate(suite) if d in w]
        res = perft([suite[i][1] for i in idx], d, capacity=capacity, device=device)
        for i, r in zip(idx, res):
            got[i][d] = r.nodes
        nodes += sum(r.nodes for r in res)
        secs += res[0].seconds
    bad = 0
    for (ln, fen, want), g in zip(suite, got):
        wrong = [d for d in sorted(g) if g[d] != want[d]]
        if wrong:
            bad += 1
            print(f"{path}:{ln}: FAIL {fen} " + " ".join(f"D{d} {g[d]} (expected {want[d]})" for d in wrong), file=out)
        else:
            print(f"{path}:{ln}: ok {fen} " + " ".join(f"D{d} {g[d]}" for d in sorted(g)), file=out)
    print(f"{len(suite) - bad} of {len(suite)} positions agree; {nodes} nodes in {secs:.3f} s", file=out)
    return 1 if bad else 0


def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.perft", description="perft on the GPU")
    ap.add_argument("fen", nargs="?", default=None, help="FEN (default: the start position)")
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--divide", action="store_true", help="the root's moves in generated order with the count below each")
    ap.add_argument("--stats", action="store_true", help="captures, e.p., castles, promotions, checks, checkmates, stalemates of the leaves")
    ap.add_argument("--order", action="store_true", help="order-sensitive checksum of every generated move list")
    ap.add_argument("--capacity", type=int, default=DEFAULT_CAPACITY, help="positions per level buffer (>= 256)")
    ap.add_argument("--json", default=None, metavar="OUT")
    ap.add_argument("--epd", default=None, metavar="SUITE", help="perft suite: lines `FEN ;D1 20 ;D2 400 ...`")
    ap.add_argument("--max-depth", type=int, default=None, help="EPD mode: skip deeper entries")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.epd:
        if a.fen or a.depth is not None:
            ap.error("--epd takes its positions and depths from the file")
        return run_epd(a.epd, a.max_depth, a.capacity, a.device, out)
    if a.depth is None:
        ap.error("--depth is required")
    fen = None if a.fen in (None, "startpos") else a.fen
    E.load_hip_library()  # (outside the timed call)
    r = perft(fen, a.depth, divide=a.divide, stats=a.stats, order=a.order, capacity=a.capacity, device=a.device)[0]
    if a.divide:
        for u, n in r.moves:
            print(f"{u}: {n}", file=out)
        print(file=out)
    print(f"Nodes searched: {r.nodes}", file=out)
    if r.stats is not None:
        print(" ".join(f"{k}={v}" for k, v in r.stats.items()), file=out)
    if r.checksum is not None:
        print(f"Order checksum: 0x{r.checksum:016x}", file=out)
    rate = r.nodes / r.seconds if r.seconds > 0 else 0.0
    print(f"{r.seconds:.3f} s, {rate / 1e6:.1f} M nodes/s" + (f", {r.splits} level splits" if r.splits else ""), file=out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r.to_json(), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
