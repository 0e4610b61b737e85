"""betaone_amd/tablebase.py -- endgame tablebases built and probed on the GPU, and self-play records rescored with them.

Distance to mate (DTM) in plies, 50-move rule ignored, no castling rights; 2 to 4 men, pawns on one side only (so no en passant).  The
tables are generated here (bo_tb_*, csrc/bo_tb.h): nothing is downloaded.  A material is named strong side first ("KQK", "KPK", "KBNK",
"KQKR"); the table serves the colour-swapped material through the mirror.  KK, KBK and KNK need no table: a probe answers draw.

    python -m betaone_amd.tablebase build KRK KPK KBNK --dir TB
    python -m betaone_amd.tablebase probe --dir TB "8/8/8/8/8/2k5/8/K2R4 w - - 0 1"
    python -m betaone_amd.tablebase verify --dir TB
    python -m betaone_amd.tablebase rescore DATA_DIR/iter_3 --dir TB --write OUT_DIR

Index (the host mirror of csrc/bo_tb.h): idx = ((stm * 64 + sq[0]) * 64 + sq[1]) ... over the piece list K, strong pieces, k, weak
pieces; stm 0 = the strong side (white in the table's frame) moves.  Code: 0 not a position, 1 draw, 2 + k mate in k plies (k even: the
side to move is mated in k, k odd: it mates in k).

File *.botb: a 64-byte little-endian header -- magic 'BOTB', version u16, men u16, name char[8], entries u32, passes u16, pad u16,
largest win ply [strong to move, weak to move] i16 x 2, largest loss ply i16 x 2, wins / draws / losses u32 x 2 each, FNV-1a (64 bit)
of the payload -- then entries x uint16.

rescore reads every *.bog file of a directory, probes every position of every game in one call and reports how many games reach a
covered position, how many recorded results disagree with the table there, and the plies an adjudication would save.  --write writes
the adjudicated records: a game is cut at the first covered ply j where the table says drawn or lost for the side to move, and written
as a game that ended there (a draw: terminal 2; a loss: the side to move resigned at P_j, terminal 3, outcome as rollout writes it).
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import os
import struct
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as E

ORDER = "QRBNP"
PIECE_TYPE = {"P": 1, "N": 2, "B": 3, "R": 4, "Q": 5, "K": 6}
MAX_MEN = 4
COVERED, NO_TABLE, TOO_MANY_MEN, CASTLING, PAWNS_BOTH, NOT_A_POSITION = range(6)  # BO_TB_*
STATUS_NAMES = ("covered", "no table loaded", "too many men", "castling rights", "pawns on both sides", "not a position")
MAGIC, VERSION, HEADER = b"BOTB", 1, struct.Struct("<4sHH8sIHH4h6IQ")
SUFFIX = ".botb"
FNV_BASIS, FNV_PRIME, MASK64 = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1
assert HEADER.size == 64


class BoTbSideStats(C.Structure):
    _fields_ = [("legal", C.c_uint64), ("wins", C.c_uint64), ("draws", C.c_uint64), ("losses", C.c_uint64), ("max_win_ply", C.c_int32),
                ("max_loss_ply", C.c_int32)]


class BoTbInfo(C.Structure):  # bo_tb_info
    _fields_ = [("n_entries", C.c_int64), ("n_men", C.c_int32), ("passes", C.c_int32), ("complete", C.c_int32), ("reserved", C.c_int32),
                ("fnv1a", C.c_uint64), ("side", BoTbSideStats * 2), ("material", C.c_char * 16)]


# ---- materials ------------------------------------------------------------------------------------------------------------------------
def parse(material: str) -> Tuple[str, str]:
    """"KQKR" -> ("Q", "R"): each side's pieces in the order Q R B N P."""
    m = material.strip().upper()
    if len(m) < 2 or m[0] != "K" or m.count("K") != 2 or any(c not in "KQRBNP" for c in m):
        raise ValueError(f"{material!r} is not a material: K, the strong side's pieces, K, the weak side's pieces")
    a, b = m[1:].split("K")
    key = lambda s: "".join(sorted(s, key=ORDER.index))
    return key(a), key(b)


def _name(a: str, b: str) -> str:
    """The name with the stronger side first: more men, then the better pieces in the order Q R B N P."""
    ka, kb = [ORDER.index(c) for c in a], [ORDER.index(c) for c in b]
    swap = len(b) > len(a) or (len(b) == len(a) and kb < ka)
    return "K" + b + "K" + a if swap else "K" + a + "K" + b


def canonical(material: str) -> str:
    return _name(*parse(material))


def needs_no_table(material: str) -> bool:
    a, b = parse(material)
    return (a + b) in ("", "B", "N")


def check_supported(material: str) -> str:
    a, b = parse(material)
    if 2 + len(a) + len(b) > MAX_MEN:
        raise ValueError(f"{material}: tables have 2 to {MAX_MEN} men")
    if "P" in a and "P" in b:
        raise ValueError(f"{material}: pawns on both sides need en passant in the table, which is not handled yet (a follow-up)")
    return _name(a, b)


def children(material: str) -> List[str]:
    """The other materials one move away: a capture, a promotion, a capture with promotion."""
    a, b = parse(material)
    srt = lambda s: "".join(sorted(s, key=ORDER.index))
    out = []
    for own, opp, flip in ((a, b, False), (b, a, True)):
        opps = [opp] + [opp[:i] + opp[i + 1:] for i in range(len(opp))]
        owns = [own] + ([srt(own.replace("P", q, 1)) for q in "QRBN"] if "P" in own else [])
        for o in owns:
            for p in opps:
                if (o, p) != (own, opp):
                    n = _name(p, o) if flip else _name(o, p)
                    if n not in out and n != _name(a, b):
                        out.append(n)
    return out


def closure(materials: Sequence[str]) -> List[str]:
    """The request with every sub-table it needs, each table behind its sub-tables: closure(["KPK"]) == ["KQK", "KRK", "KPK"]."""
    out: List[str] = []

    def visit(m):
        m = check_supported(m)
        if m in out or needs_no_table(m):
            return
        for c in children(m):
            visit(c)
        if m not in out:
            out.append(m)

    for m in materials:
        if needs_no_table(m):
            continue
        visit(m)
    return out


def piece_list(material: str) -> List[Tuple[int, bool]]:
    """[(piece type 1..6, belongs to the strong side)] in index order."""
    a, b = parse(material)
    return [(6, True)] + [(PIECE_TYPE[c], True) for c in a] + [(6, False)] + [(PIECE_TYPE[c], False) for c in b]


def n_entries(material: str) -> int:
    return 2 * 64 ** len(piece_list(material))


# ---- index (host mirror of csrc/bo_tb.h) ------------------------------------------------------------------------------------------------
def index(material: str, stm: int, squares: Sequence[int]) -> int:
    idx = stm
    for s in squares:
        idx = idx * 64 + s
    return idx


def decode(material: str, idx: int) -> Tuple[int, List[int]]:
    n = len(piece_list(material))
    return (idx >> (6 * n)) & 1, [(idx >> (6 * (n - 1 - s))) & 63 for s in range(n)]


def entry_bitboards(material: str, idx: int):
    """(bb[8], white to move) of an entry in the table's frame, or None when two men share a square."""
    stm, sq = decode(material, idx)
    if len(set(sq)) != len(sq):
        return None
    bb = [0] * 8
    for (pt, strong), s in zip(piece_list(material), sq):
        bb[pt - 1] |= 1 << s
        bb[6 if strong else 7] |= 1 << s
    return bb, stm == 0


def bitboards_fen(bb: Sequence[int], white_to_move: bool) -> str:
    rows = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for f in range(8):
            b = 1 << (8 * r + f)
            c = next((" PNBRQK"[i + 1] for i in range(6) if bb[i] & b), None)
            if c is None:
                gap += 1
                continue
            row += (str(gap) if gap else "") + (c if bb[6] & b else c.lower())
            gap = 0
        rows.append(row + (str(gap) if gap else ""))
    return "/".join(rows) + (" w" if white_to_move else " b") + " - - 0 1"


def entry_fen(material: str, idx: int) -> Optional[str]:
    e = entry_bitboards(material, idx)
    return None if e is None else bitboards_fen(*e)


def _bswap(x: int) -> int:
    return int.from_bytes(x.to_bytes(8, "little"), "big")


def mirror(bb: Sequence[int], white_to_move: bool):
    """Ranks flipped, colours and the side to move swapped."""
    m = [_bswap(x) for x in bb[:6]]
    return m + [_bswap(bb[7]), _bswap(bb[6])], not white_to_move


def position_index(bb: Sequence[int], white_to_move: bool):
    """(table name, index) of a position given as bitboards (pawns .. kings, white, black), the mirror applied where the strong side is
    black; (None, None) for insufficient material (KK, KBK, KNK: a draw)."""
    side = lambda occ: "".join(c * bin(bb[PIECE_TYPE[c] - 1] & occ).count("1") for c in ORDER)
    w, b = side(bb[6]), side(bb[7])
    if (w + b) in ("", "B", "N"):
        return None, None
    name = _name(w, b)
    if name != "K" + w + "K" + b:
        bb, white_to_move = mirror(bb, white_to_move)
    idx, taken = 0 if white_to_move else 1, 0
    for pt, strong in piece_list(name):
        c = bb[pt - 1] & bb[6 if strong else 7] & ~taken
        sq = (c & -c).bit_length() - 1  # identical men take their squares in ascending order
        taken |= 1 << sq
        idx = idx * 64 + sq
    return name, idx


def fnv1a(data: bytes) -> int:
    h = FNV_BASIS
    for b in data:
        h = ((h ^ b) * FNV_PRIME) & MASK64
    return h


def position_from_fen(fen: str) -> E.BoPosition:
    f = fen.split()
    p = E.BoPosition()
    r, c = 7, 0
    for ch in f[0]:
        if ch == "/":
            r, c = r - 1, 0
        elif ch.isdigit():
            c += int(ch)
        else:
            if ch.upper() not in PIECE_TYPE or not (0 <= r < 8 and 0 <= c < 8):
                raise ValueError(f"bad FEN: {fen!r}")
            b = 1 << (8 * r + c)
            p.bb[PIECE_TYPE[ch.upper()] - 1] |= b
            p.bb[6 if ch.isupper() else 7] |= b
            c += 1
    if len(f) < 2 or f[1] not in "wb":
        raise ValueError(f"bad FEN: {fen!r}")
    p.turn = 1 if f[1] == "w" else 0
    cas = f[2] if len(f) > 2 else "-"
    p.castling = sum(1 << "KQkq".index(x) for x in cas if x in "KQkq")
    ep = f[3] if len(f) > 3 else "-"
    p.ep_square = -1 if ep == "-" else (ord(ep[0]) - 97) + 8 * (int(ep[1]) - 1)
    p.ep_key = -2
    p.halfmove_clock = int(f[4]) if len(f) > 4 else 0
    p.fullmove_number = int(f[5]) if len(f) > 5 else 1
    return p


# ---- tables on the device -----------------------------------------------------------------------------------------------------------
def _check(lib, rc: int, who: str):
    if rc != 0:
        msg = f"{who}: {lib.bo_last_error().decode()}"
        raise (ValueError if rc in (-1, -3) else E.EngineError)(msg)


def _stream(dev) -> int:
    if dev.type == "cuda":
        return torch.cuda.current_stream(dev).cuda_stream
    return 0


def info_dict(i: BoTbInfo) -> dict:
    side = lambda s: dict(legal=int(s.legal), wins=int(s.wins), draws=int(s.draws), losses=int(s.losses), max_win_ply=int(s.max_win_ply),
                          max_loss_ply=int(s.max_loss_ply))
    return dict(material=i.material.decode(), n_entries=int(i.n_entries), n_men=int(i.n_men), passes=int(i.passes), complete=bool(i.complete),
                fnv1a=int(i.fnv1a), strong_to_move=side(i.side[0]), weak_to_move=side(i.side[1]))


def stats_line(d: dict) -> str:
    s, w = d["strong_to_move"], d["weak_to_move"]
    return (f"{d['material']}: strong to move {s['legal']} legal, {s['wins']} wins, {s['draws']} draws, {s['losses']} losses, largest win "
            f"{s['max_win_ply']} plies; weak to move {w['legal']} legal, {w['wins']} wins, {w['draws']} draws, {w['losses']} losses, "
            f"largest loss {w['max_loss_ply']} plies; fnv1a 0x{d['fnv1a']:016x}")


class Table:
    """One table on the device (a bo_tb handle).  `subs`: the Tables a capture or a promotion leads to (kept alive by this one)."""

    def __init__(self, material: str, subs: Sequence["Table"] = (), device="cuda:0", lib=None):
        self.lib = lib or E.load_hip_library()
        self.dev = E.runtime_device(device)
        self.subs = list(subs)
        arr = (C.c_void_p * max(1, len(self.subs)))(*[s.h for s in self.subs])
        h = C.c_void_p()
        self.h = None
        _check(self.lib, self.lib.bo_tb_create(int(self.dev.index or 0), canonical(material).encode(), arr, len(self.subs), C.byref(h)), "bo_tb_create")
        self.h = h
        self.material = canonical(material)  # (as the library names it)
        self.n_entries = n_entries(self.material)
        self.seconds = 0.0

    def build(self, max_passes: int = -1) -> int:
        passes = C.c_int32(0)
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        _check(self.lib, self.lib.bo_tb_build(self.h, int(max_passes), C.byref(passes), _stream(self.dev)), "bo_tb_build")
        self.seconds = time.perf_counter() - t0
        return int(passes.value)

    def verify(self) -> int:
        n = C.c_uint64(0)
        _check(self.lib, self.lib.bo_tb_verify(self.h, C.byref(n), _stream(self.dev)), "bo_tb_verify")
        return int(n.value)

    def info(self) -> dict:
        i = BoTbInfo()
        _check(self.lib, self.lib.bo_tb_stats(self.h, C.addressof(i)), "bo_tb_stats")
        return info_dict(i)

    def download(self) -> np.ndarray:
        a = np.empty(self.n_entries, np.uint16)
        _check(self.lib, self.lib.bo_tb_download(self.h, a.ctypes.data, a.size), "bo_tb_download")
        return a

    def upload(self, codes: np.ndarray, passes: int = 0):
        a = np.ascontiguousarray(codes, dtype=np.uint16)
        _check(self.lib, self.lib.bo_tb_upload(self.h, a.ctypes.data, a.size, int(passes)), "bo_tb_upload")

    def close(self):
        if getattr(self, "h", None):
            self.lib.bo_tb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- files --------------------------------------------------------------------------------------------------------------------------
def write_table(path: str, info: dict, codes: np.ndarray):
    s, w = info["strong_to_move"], info["weak_to_move"]
    head = HEADER.pack(MAGIC, VERSION, info["n_men"], info["material"].encode(), info["n_entries"], info["passes"], 0, s["max_win_ply"],
                       w["max_win_ply"], s["max_loss_ply"], w["max_loss_ply"], s["wins"], w["wins"], s["draws"], w["draws"], s["losses"],
                       w["losses"], info["fnv1a"])
    with open(path, "wb") as fh:
        fh.write(head)
        fh.write(np.ascontiguousarray(codes, dtype="<u2").tobytes())


def read_table(path: str) -> Tuple[dict, np.ndarray]:
    """(header fields, payload) of a *.botb file; a short file or a bad header raises ValueError.  The payload's checksum is compared by
    whoever uploads it (TableSet.load: the library hashes the payload)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if len(raw) < HEADER.size:
        raise ValueError(f"{path}: truncated (no header)")
    f = HEADER.unpack(raw[:HEADER.size])
    if f[0] != MAGIC or f[1] != VERSION:
        raise ValueError(f"{path}: not a tablebase file (magic {f[0]!r}, version {f[1]})")
    name = f[3].rstrip(b"\0").decode()
    if n_entries(name) != f[4] or len(piece_list(name)) != f[2]:
        raise ValueError(f"{path}: the header's entry count does not fit {name}")
    if len(raw) != HEADER.size + 2 * f[4]:
        raise ValueError(f"{path}: truncated ({len(raw) - HEADER.size} payload bytes of {2 * f[4]})")
    head = dict(material=name, n_men=f[2], n_entries=f[4], passes=f[5], fnv1a=f[17],
                strong_to_move=dict(max_win_ply=f[7], max_loss_ply=f[9], wins=f[11], draws=f[13], losses=f[15]),
                weak_to_move=dict(max_win_ply=f[8], max_loss_ply=f[10], wins=f[12], draws=f[14], losses=f[16]))
    return head, np.frombuffer(raw, dtype="<u2", offset=HEADER.size)


class TableSet:
    """Tables on one device, probed together."""

    def __init__(self, device="cuda:0", lib=None):
        self.lib = lib or E.load_hip_library()
        self.device = device
        self.dev = E.runtime_device(device)
        self.tables: Dict[str, Table] = {}

    def add(self, material: str) -> Table:
        """A new, empty table bound to the tables already in the set."""
        t = Table(material, list(self.tables.values()), self.device, self.lib)
        self.tables[t.material] = t
        return t

    @classmethod
    def load(cls, directory: str, device="cuda:0", lib=None) -> "TableSet":
        ts = cls(device, lib)
        files = {}
        for p in sorted(glob.glob(os.path.join(directory, "*" + SUFFIX))):
            head, codes = read_table(p)
            files[head["material"]] = (p, head, codes)
        for name in closure(list(files)):
            if name not in files:
                raise ValueError(f"{directory}: {name}{SUFFIX} is missing (a sub-table of a table that is there)")
            p, head, codes = files[name]
            t = ts.add(name)
            t.upload(codes, head["passes"])
            if t.info()["fnv1a"] != head["fnv1a"]:
                raise ValueError(f"{p}: wrong checksum (payload 0x{t.info()['fnv1a']:016x}, header 0x{head['fnv1a']:016x})")
        return ts

    def save(self, directory: str):
        os.makedirs(directory, exist_ok=True)
        for name, t in self.tables.items():
            write_table(os.path.join(directory, name + SUFFIX), t.info(), t.download())

    def probe_codes(self, positions) -> Tuple[np.ndarray, np.ndarray]:
        """(codes uint16, status int32) of bo_position records: a ctypes array, a list of BoPosition, or their bytes."""
        if isinstance(positions, (bytes, bytearray, memoryview)):
            raw = bytes(positions)
        elif isinstance(positions, C.Array):
            raw = bytes(positions)
        else:
            raw = b"".join(bytes(p) for p in positions)
        n = len(raw) // C.sizeof(E.BoPosition)
        codes, status = np.zeros(n, np.uint16), np.zeros(n, np.int32)
        hs = [t.h for t in self.tables.values()]
        arr = (C.c_void_p * max(1, len(hs)))(*hs)
        buf = C.create_string_buffer(raw, len(raw)) if n else None
        _check(self.lib, self.lib.bo_tb_probe(arr, len(hs), buf, n, codes.ctypes.data, status.ctypes.data, _stream(self.dev)), "bo_tb_probe")
        return codes, status

    def probe(self, positions) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(wdl, dtm_plies, status): wdl +1 / 0 / -1 for the side to move, dtm_plies the k of a mate (0 for a draw); a position that is
        not covered has wdl 0 and dtm_plies -1."""
        codes, status = self.probe_codes(positions)
        k = codes.astype(np.int32) - 2
        ok = status == COVERED
        wdl = np.where(ok & (codes >= 2), np.where(k & 1, 1, -1), 0).astype(np.int32)
        dtm = np.where(ok, np.where(codes >= 2, k, 0), -1).astype(np.int32)
        return wdl, dtm, status

    def close(self):
        for t in reversed(list(self.tables.values())):
            t.close()
        self.tables = {}


def build(materials: Sequence[str], out_dir: Optional[str] = None, device="cuda:0", lib=None, out=None) -> TableSet:
    """Builds `materials` and their sub-tables in closure order; writes NAME.botb into out_dir when given."""
    ts = TableSet(device, lib)
    for name in closure(materials):
        t = ts.add(name)
        passes = t.build()
        info = t.info()
        if out is not None:
            print(f"{name}: {passes} passes, {t.seconds:.3f} s", file=out)
            print(stats_line(info), file=out)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            write_table(os.path.join(out_dir, name + SUFFIX), info, t.download())
    return ts


# ---- rescoring records ----------------------------------------------------------------------------------------------------------------
class _Cut:
    """What records.pack_game reads of a finished game."""

    def __init__(self, g: dict, j: int, terminal: int):
        self.game_id, self.first_ply = g["game_id"], 0
        self.positions = [g["positions"][i] for i in range(j + 1)]
        self.moves = list(g["moves"][:j])
        self.pis = list(g["pis"][:j])
        self.terminal = terminal
        self.outcome = 1.0 if terminal in (1, 3) else 0.0  # as rollout's _finish writes a resigned game
        self.root_values = None if g["root_values"] is None else np.asarray(g["root_values"][:j], np.float32)
        self.resign, self.resign_check = g["resign"], g["resign_check"]


def _white_result(g: dict) -> int:
    if g["terminal"] in (1, 3):  # the side to move in the final position was mated / resigned
        return -1 if g["positions"][g["n_plies"]].turn == 1 else 1
    return 0


def rescore(iter_dir: str, ts: TableSet, write: Optional[str] = None) -> dict:
    from . import records as R

    files = []
    for p in sorted(glob.glob(os.path.join(iter_dir, "*" + R.COMPACT_SUFFIX))):
        with open(p, "rb") as fh:
            buf = fh.read()
        idx = R.scan_games(buf)
        end = idx[-1][2] + idx[-1][3] if idx else 0
        files.append((p, buf, idx, R.unpack_games(buf[:end])))
    games = [g for _, _, _, gs in files for g in gs]
    raw = b"".join(bytes(g["positions"]) for g in games)
    wdl, dtm, status = ts.probe(raw)  # every position of every game in one call
    rep = dict(games=len(games), positions=len(wdl), games_covered=0, first_covered_ply_sum=0, disagree=0, games_cut=0, plies_saved=0)
    off, cuts = 0, {}
    for gi, g in enumerate(games):
        n = g["n_plies"]
        st, w = status[off:off + n + 1], wdl[off:off + n + 1]
        off += n + 1
        cov = np.nonzero(st == COVERED)[0]
        if not len(cov):
            continue
        j0 = int(cov[0])
        rep["games_covered"] += 1
        rep["first_covered_ply_sum"] += j0
        table_white = int(w[j0]) * (1 if g["positions"][j0].turn == 1 else -1)
        if table_white != _white_result(g):
            rep["disagree"] += 1
        for j in range(j0, n + 1):
            if st[j] != COVERED:  # coverage ends (a promotion into a table that is not loaded): the game stays as it is
                break
            if w[j] <= 0:
                if j < n or g["terminal"] == 0:
                    cuts[gi] = (j, 2 if w[j] == 0 else 3)
                    rep["games_cut"] += 1
                    rep["plies_saved"] += n - j
                break
    rep["mean_first_covered_ply"] = rep["first_covered_ply_sum"] / rep["games_covered"] if rep["games_covered"] else 0.0
    if write:
        os.makedirs(write, exist_ok=True)
        gi = 0
        for p, buf, idx, gs in files:
            parts = []
            for (gid, n, o, size), g in zip(idx, gs):
                parts.append(R.pack_game(_Cut(g, *cuts[gi])) if gi in cuts else bytes(buf[o:o + size]))
                gi += 1
            with open(os.path.join(write, os.path.basename(p)), "wb") as fh:
                fh.write(b"".join(parts))
    return rep


def report_text(rep: dict) -> str:
    return (f"{rep['games']} games, {rep['positions']} positions\n"
            f"{rep['games_covered']} games reach a covered position (mean ply {rep['mean_first_covered_ply']:.1f})\n"
            f"{rep['disagree']} recorded results disagree with the table at the first covered ply\n"
            f"{rep['games_cut']} games would be cut, {rep['plies_saved']} plies saved\n")


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.tablebase", description="Endgame tablebases (DTM, 2 to 4 men) on the GPU")
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="build tables and the sub-tables they need")
    b.add_argument("materials", nargs="+")
    p = sub.add_parser("probe", help="probe FENs")
    p.add_argument("fens", nargs="+")
    v = sub.add_parser("verify", help="check every entry of every table against its children")
    r = sub.add_parser("rescore", help="rescore the compact records of one iteration")
    r.add_argument("iter_dir")
    r.add_argument("--write", default=None, metavar="OUT_DIR")
    for s in (b, p, v, r):
        s.add_argument("--dir", required=True, help="the directory of *.botb files")
        s.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.cmd == "build":
        try:
            ts = build(a.materials, a.dir, a.device, out=out)
        except ValueError as e:
            print(f"error: {e}", file=out)
            return 2
        ts.close()
        return 0
    ts = TableSet.load(a.dir, a.device)
    try:
        if a.cmd == "probe":
            wdl, dtm, status = ts.probe([position_from_fen(f) for f in a.fens])
            for f, w, d, s in zip(a.fens, wdl, dtm, status):
                if s != COVERED:
                    print(f"{f}: not covered ({STATUS_NAMES[s]})", file=out)
                elif w == 0:
                    print(f"{f}: draw", file=out)
                else:
                    print(f"{f}: {'win' if w > 0 else 'loss'} for the side to move, mate in {d} plies ({(d + 1) // 2} moves)", file=out)
            return 0
        if a.cmd == "verify":
            bad = 0
            for name, t in ts.tables.items():
                n = t.verify()
                bad += n
                print(f"{name}: {n} mismatches", file=out)
            return 1 if bad else 0
        rep = rescore(a.iter_dir, ts, a.write)
        out.write(report_text(rep))
        return 0
    finally:
        ts.close()


if __name__ == "__main__":
    sys.exit(main())
