"""betaone_amd/mate.py -- forced mates on the GPU: mate in N, EPD mate suites, and an audit of self-play records.

Is there a forced mate in at most N moves for the side to move, in how many plies (dtm), and by which first moves (the key moves)?
The search runs on the device (bo_mate, csrc/bo_mate.h): a full-width walk to depth 2 N - 1 over perft's frontier with an AND/OR
backup, deepened iteratively so every root leaves the batch at its exact distance.  Draw rules are ignored, as in perft and the
tablebases: only a position without legal moves ends a line.

    mate("r2qkb1r/pp2nppp/3p4/2pNN1B1/2BnP3/3P4/PPP2PPP/R2bK2R w KQkq - 1 10", moves=2, pv=True)[0].pv    # ['d5f6', 'g7f6', 'c4f7']
    python -m betaone_amd.mate "FEN" --moves 3 [--pv] [--json]
    python -m betaone_amd.mate --epd suite.epd [--moves N]
    python -m betaone_amd.mate audit DATA_DIR/iter_7 --moves 2 [--json out.json]

roots: a FEN, a sequence of FENs, or a ctypes array of engine.BoPosition (a record's positions as they are).  pv=True adds the
principal variation of every solved root -- the attacker plays the lowest-index key move, the defender the reply of longest
resistance -- and may cost as much as the solve.  max_nodes (0 = unlimited): the call stops before an iteration when the positions
visited so far exceed it; `searched` says how far each root got.

EPD mode reads `FEN dm N; bm MOVE [MOVE ...];` lines (a FEN of four or six fields; bm in SAN or UCI; other operations are ignored),
solves every line to the larger of its dm and --moves (3 when it has neither) and reports per line: solved or not, the distance found against
dm, whether every bm is a key move, and whether the solution is unique.  A line fails when no mate is found, the distance differs
from dm, or a bm is no key move; the exit status is 1 if any line fails.  A SAN bm is matched by what it states (piece, origin file /
rank, destination, promotion, castling) against the key moves.

Audit mode takes every stored position of every .bog game under the given directories as a root (one call per file) and reports, per
mate distance and in total: positions with a forced mate; how often the played move and the record's strongest pi entry are key moves
and the pi mass on key moves; CONTRADICTED TARGETS -- forced-mate positions whose game the side to move did not win; ALLOWED MATES --
records whose played move leaves the opponent a forced mate within N (read from the next position's result).  Records are only read.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import re
import sys
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import engine as E
from .perft import DEFAULT_CAPACITY, MAX_MOVES, START_FEN

PV = 1  # BO_MATE_PV (include/betaone_engine.h)
MAX_N = 16
STATUS_NAMES = ("ok", "checkmated", "stalemated", "not a position")


class BoMateResult(C.Structure):  # bo_mate_result
    _fields_ = [("status", C.c_int32), ("dtm", C.c_int32), ("searched", C.c_int32), ("n_moves", C.c_int32), ("n_keys", C.c_int32),
                ("key", C.c_int32), ("nodes", C.c_uint64)]


@dataclass
class MateResult:
    fen: Optional[str]                 # None for a BoPosition root
    status: str                        # STATUS_NAMES
    dtm: int                           # plies to mate, 0 = none found
    searched: int                      # the largest N completed for this root
    n_moves: int
    key: Optional[str] = None          # the lowest-index key move (UCI)
    keys: List[str] = field(default_factory=list)   # every key move, in generated order
    key_words: List[int] = field(default_factory=list)
    pv: Optional[List[str]] = None
    nodes: int = 0                     # positions visited, of the whole call
    splits: int = 0                    # of the whole call
    seconds: float = 0.0               # of the whole call

    @property
    def mate_in(self) -> int:
        """Moves to mate (0 = none found)."""
        return (self.dtm + 1) // 2

    def to_json(self) -> dict:
        d = {"fen": self.fen, "status": self.status, "dtm": self.dtm, "mate_in": self.mate_in, "searched": self.searched,
             "n_moves": self.n_moves, "key": self.key, "keys": list(self.keys), "nodes": self.nodes, "splits": self.splits,
             "seconds": self.seconds}
        if self.pv is not None:
            d["pv"] = list(self.pv)
        return d


def mate(roots: Union[str, Sequence[Optional[str]], C.Array], moves: int = 3, *, pv: bool = False, capacity: int = DEFAULT_CAPACITY,
         max_nodes: int = 0, device="cuda:0", lib=None) -> List[MateResult]:
    """Forced mates in at most `moves` moves of every root, in one device call on torch's current stream of `device`."""
    lib = lib or E.load_hip_library()
    dev = E.runtime_device(device)
    fens, arr, pos = None, None, None
    if isinstance(roots, C.Array) and getattr(roots, "_type_", None) is E.BoPosition:
        pos, n = roots, len(roots)
    else:
        if roots is None or isinstance(roots, str):
            roots = [roots]
        fens = [START_FEN if f is None else f for f in roots]
        n = len(fens)
        arr = (C.c_char_p * max(n, 1))(*[f.encode() for f in fens])
    res = (BoMateResult * max(n, 1))()
    width = max(2 * int(moves) - 1, 1)
    keys = np.full((max(n, 1), MAX_MOVES), -1, np.int32)
    line = np.full((max(n, 1), width), -1, np.int32)
    splits = C.c_int64(0)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
    else:
        stream = 0
    t0 = time.perf_counter()
    rc = lib.bo_mate(int(dev.index or 0), n, arr, C.addressof(pos) if pos is not None else None, int(moves), int(capacity), int(max_nodes),
                     PV if pv else 0, C.addressof(res), keys.ctypes.data, line.ctypes.data if pv else None, C.byref(splits), stream)
    dt = time.perf_counter() - t0
    if rc != 0:
        msg = f"bo_mate: {lib.bo_last_error().decode()}"
        raise (ValueError if rc == -4 else E.EngineError)(msg)
    out = []
    for i in range(n):
        r = res[i]
        words = [int(w) for w in keys[i, :int(r.n_keys)]]
        m = MateResult(fens[i] if fens is not None else None, STATUS_NAMES[int(r.status)], int(r.dtm), int(r.searched), int(r.n_moves),
                       E.move_to_uci(int(r.key)) if r.key >= 0 else None, [E.move_to_uci(w) for w in words], words,
                       nodes=int(r.nodes), splits=int(splits.value), seconds=dt)
        if pv:
            m.pv = [E.move_to_uci(int(w)) for w in line[i, :int(r.dtm)]]
        out.append(m)
    return out


# ---- EPD mate suites ---------------------------------------------------------------------------------------------------------------
def parse_epd(text: str) -> List[tuple]:
    """[(line number, fen, dm or None, [bm tokens])] of EPD lines `FEN op; op; ...` ('#' lines and blank lines are skipped).  The
    splitting on ';' is perft.parse_epd's; the operations here are words (dm N, bm MOVE ...), not depth counts."""
    out = []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        parts = [p.strip() for p in line.split(";")]
        head = parts[0].split()
        if len(head) < 4:
            raise ValueError(f"line {ln}: expected a FEN of at least four fields")
        k = 6 if len(head) >= 6 and head[4].isdigit() and head[5].isdigit() else 4
        fen = " ".join(head[:k]) + ("" if k == 6 else " 0 1")
        ops = [head[k:]] + [p.split() for p in parts[1:]]
        dm, bm = None, []
        for op in ops:
            if not op:
                continue
            if op[0] == "dm":
                if len(op) != 2 or not op[1].isdigit() or not 1 <= int(op[1]) <= MAX_N:
                    raise ValueError(f"line {ln}: expected `dm N` with N in 1..{MAX_N}")
                dm = int(op[1])
            elif op[0] == "bm":
                bm = op[1:]
        out.append((ln, fen, dm, bm))
    return out


_SAN = re.compile(r"^([KQRBN]?)([a-h]?)([1-8]?)x?([a-h][1-8])(?:=?([QRBNqrbn]))?$")
_UCI = re.compile(r"^[a-h][1-8][a-h][1-8][qrbn]?$")


def _piece_at(fen: str, sq: int) -> str:
    rows = fen.split()[0].split("/")
    f = 0
    for c in rows[7 - (sq >> 3)]:
        if c.isdigit():
            f += int(c)
            continue
        if f == (sq & 7):
            return c.upper()
        f += 1
    return ""


def bm_is_key(fen: str, bm: str, keys: Sequence[str]) -> bool:
    """Is the EPD move `bm` (UCI, or SAN matched by what it states) one of the key moves (UCI) of the position?"""
    t = bm.rstrip("+#!?")
    if _UCI.match(t):
        return t in keys
    if t in ("O-O", "0-0", "O-O-O", "0-0-0"):
        want = 2 if len(t) == 3 else -2
        return any(_piece_at(fen, _sq(k[:2])) == "K" and (_sq(k[2:4]) & 7) - (_sq(k[:2]) & 7) == want for k in keys)
    m = _SAN.match(t)
    if not m:
        return False
    piece, ff, fr, to, promo = m.group(1) or "P", m.group(2), m.group(3), m.group(4), (m.group(5) or "").lower()
    for k in keys:
        if k[2:4] != to or k[4:] != promo or _piece_at(fen, _sq(k[:2])) != piece:
            continue
        if (ff and k[0] != ff) or (fr and k[1] != fr):
            continue
        if piece == "K" and abs((_sq(k[2:4]) & 7) - (_sq(k[:2]) & 7)) == 2:
            continue  # (castling is written O-O)
        return True
    return False


def _sq(name: str) -> int:
    return (ord(name[1]) - ord("1")) * 8 + ord(name[0]) - ord("a")


def run_epd(path: str, moves: Optional[int], capacity: int, device, out=None) -> int:
    out = out or sys.stdout
    suite = parse_epd(open(path).read())
    depth = [max(dm or 0, moves or (0 if dm else 3)) for _, _, dm, _ in suite]
    res: List[Optional[MateResult]] = [None] * len(suite)
    nodes, secs = 0, 0.0
    for n in sorted(set(depth)):  # every line that asks for this distance, in one call
        idx = [i for i, d in enumerate(depth) if d == n]
        got = mate([suite[i][1] for i in idx], n, capacity=capacity, device=device)
        for i, r in zip(idx, got):
            res[i] = r
        nodes += got[0].nodes
        secs += got[0].seconds
    bad = 0
    for (ln, fen, dm, bm), r in zip(suite, res):
        notes = []
        if r.status != "ok":
            notes.append(r.status)
        elif not r.dtm:
            notes.append(f"no mate within {r.searched}")
        else:
            if dm is not None and r.mate_in != dm:
                notes.append(f"mate in {r.mate_in} (expected dm {dm})")
            wrong = [b for b in bm if not bm_is_key(fen, b, r.keys)]
            if wrong:
                notes.append("bm " + " ".join(wrong) + " not among the key moves " + " ".join(r.keys))
        ok = not notes
        bad += 0 if ok else 1
        tail = ""
        if r.status == "ok" and r.dtm:
            tail = f" mate in {r.mate_in}, key {' '.join(r.keys)}, " + ("unique" if len(r.keys) == 1 else f"not unique ({len(r.keys)} keys)")
        print(f"{path}:{ln}: {'ok' if ok else 'FAIL'} {fen}{tail}" + ("" if ok else ": " + "; ".join(notes)), file=out)
    print(f"{len(suite) - bad} of {len(suite)} lines solved as stated; {nodes} nodes in {secs:.3f} s", file=out)
    return 1 if bad else 0


# ---- audit of self-play records ----------------------------------------------------------------------------------------------------
AUDIT_KEYS = ("forced", "played_key", "pi_top_key", "pi_mass_on_keys", "contradicted", "allowed")


def bog_paths(args: Sequence[str]) -> List[str]:
    out = []
    for a in args:
        out += sorted(glob.glob(os.path.join(a, "*.bog"))) if os.path.isdir(a) else [a]
    return out


def audit(paths: Sequence[str], moves: int = 2, *, capacity: int = DEFAULT_CAPACITY, device="cuda:0") -> dict:
    """The report of the module docstring over the .bog files `paths`: {"moves", "files", "games", "records", "nodes", "seconds",
    "total": {AUDIT_KEYS}, "by_mate_in": {n: {AUDIT_KEYS}}}."""
    from . import records as R
    from .reanalyse import moves_to_actions

    blank = lambda: dict.fromkeys(AUDIT_KEYS, 0)
    rep = {"moves": int(moves), "files": 0, "games": 0, "records": 0, "nodes": 0, "seconds": 0.0, "total": blank(),
           "by_mate_in": {n: blank() for n in range(1, int(moves) + 1)}}
    for path in paths:
        games = R.load_games(path)
        rep["files"] += 1
        if not games:
            continue
        n_pos = sum(g["n_plies"] + 1 for g in games)
        arr = (E.BoPosition * n_pos)()
        at = 0
        for g in games:  # every stored position, the final one included (the next position of the last record)
            k = g["n_plies"] + 1
            C.memmove(C.addressof(arr) + at * C.sizeof(E.BoPosition), C.addressof(g["positions"]), k * C.sizeof(E.BoPosition))
            at += k
        res = mate(arr, moves, capacity=capacity, device=device)
        rep["nodes"] += res[0].nodes
        rep["seconds"] += res[0].seconds
        at = 0
        for g in games:
            n = g["n_plies"]
            rep["games"] += 1
            rep["records"] += n
            for i in range(n):
                r, nxt = res[at + i], res[at + i + 1]
                if nxt.dtm:
                    for b in (rep["total"], rep["by_mate_in"][nxt.mate_in]):
                        b["allowed"] += 1
                if not r.dtm:
                    continue
                z = g["outcome"] if g["positions"][i].turn == 1 else -g["outcome"]
                idx, val = g["pis"][i]
                acts = set(int(a) for a in moves_to_actions(np.array(r.key_words, np.int64)))
                on_key = [int(a) in acts for a in idx]
                top = bool(len(idx)) and on_key[int(np.argmax(val))]
                mass = float(sum(float(v) for v, k in zip(val, on_key) if k))
                for b in (rep["total"], rep["by_mate_in"][r.mate_in]):
                    b["forced"] += 1
                    b["played_key"] += 1 if int(g["moves"][i]) in r.key_words else 0
                    b["pi_top_key"] += 1 if top else 0
                    b["pi_mass_on_keys"] += mass
                    b["contradicted"] += 1 if z <= 0 else 0
            at += n + 1
    return rep


def print_audit(rep: dict, out=None):
    out = out or sys.stdout
    print(f"{rep['records']} records of {rep['games']} games in {rep['files']} files, mates within {rep['moves']} moves; "
          f"{rep['nodes']} nodes in {rep['seconds']:.3f} s", file=out)
    rows = [(f"mate in {n}", b) for n, b in sorted(rep["by_mate_in"].items())] + [("total", rep["total"])]
    for name, b in rows:
        f = max(b["forced"], 1)
        print(f"{name}: forced {b['forced']}, played a key move {b['played_key']}, strongest pi entry is a key move {b['pi_top_key']}, "
              f"mean pi mass on key moves {b['pi_mass_on_keys'] / f:.3f}, contradicted targets {b['contradicted']}, "
              f"allowed mates {b['allowed']}", file=out)


# ---- command line -------------------------------------------------------------------------------------------------------------------
def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "audit":
        ap = argparse.ArgumentParser(prog="python -m betaone_amd.mate audit", description="forced mates in self-play records")
        ap.add_argument("paths", nargs="+", help="DATA_DIR/iter_N directories or .bog files")
        ap.add_argument("--moves", type=int, default=2)
        ap.add_argument("--capacity", type=int, default=DEFAULT_CAPACITY)
        ap.add_argument("--json", default=None, metavar="OUT")
        ap.add_argument("--device", default="cuda:0")
        a = ap.parse_args(argv[1:])
        rep = audit(bog_paths(a.paths), a.moves, capacity=a.capacity, device=a.device)
        print_audit(rep, out)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rep, f, indent=1)
                f.write("\n")
        return 0
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.mate", description="forced mates on the GPU")
    ap.add_argument("fen", nargs="?", default=None, help="FEN (default: the start position)")
    ap.add_argument("--moves", type=int, default=None, help="mate in at most this many moves (default 3; EPD: for lines without dm)")
    ap.add_argument("--pv", action="store_true", help="the principal variation (may cost as much as the solve)")
    ap.add_argument("--max-nodes", type=int, default=0, help="stop before an iteration once this many positions were visited")
    ap.add_argument("--capacity", type=int, default=DEFAULT_CAPACITY, help="positions per level buffer (>= 256)")
    ap.add_argument("--json", action="store_true", help="print the result as JSON")
    ap.add_argument("--epd", default=None, metavar="SUITE", help="mate suite: lines `FEN dm N; bm MOVE;`")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.epd:
        if a.fen:
            ap.error("--epd takes its positions from the file")
        return run_epd(a.epd, a.moves, a.capacity, a.device, out)
    fen = None if a.fen in (None, "startpos") else a.fen
    E.load_hip_library()  # (outside the timed call)
    r = mate(fen, a.moves or 3, pv=a.pv, capacity=a.capacity, max_nodes=a.max_nodes, device=a.device)[0]
    if a.json:
        print(json.dumps(r.to_json()), file=out)
        return 0
    if r.status != "ok":
        print(f"The side to move is {r.status}." if r.status != "not a position" else "Not a position.", file=out)
    elif r.dtm:
        print(f"Mate in {r.mate_in} ({r.dtm} plies): {' '.join(r.keys)}" + (" (unique)" if len(r.keys) == 1 else ""), file=out)
        if r.pv is not None:
            print("pv " + " ".join(r.pv), file=out)
    else:
        print(f"No mate within {r.searched} moves.", file=out)
    rate = r.nodes / r.seconds if r.seconds > 0 else 0.0
    print(f"{r.nodes} nodes, {r.seconds:.3f} s, {rate / 1e6:.2f} M nodes/s" + (f", {r.splits} level splits" if r.splits else ""), file=out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
