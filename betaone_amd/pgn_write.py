"""betaone_amd/pgn_write.py -- games as PGN, with the SAN rendered on the GPU.

Every source of games in the project holds positions P_0..P_n and moves m_0..m_{n-1} (P_{i+1} the position after m_i): a
rollout.FinishedGame (.positions, .moves) and an unpacked compact record (records.unpack_games: "positions", "moves").  The SAN of
every move and the check / mate state of every position come from the device (bo_san_render, csrc/bo_san.h: one wave per position,
the legal moves from the same move generator as self-play; a move that is not legal, or whose next position is not the game's next
one, is an error).  The movetext is assembled by the library's host code (bo_pgn_movetext); Python only writes the tags.

    write_pgn(fh, games, tags={"Event": "match"})          # games: FinishedGame objects or unpacked records
    python -m betaone_amd.pgn_write DATA_DIR/iter_7/ -o iter7.pgn --date 2026.10.15

Results: terminal 1 (the side to move in the final position is mated; the device must confirm it) gives 1-0 / 0-1, terminal 2 gives
1/2-1/2, both with Termination "normal"; terminal 0 (the move limit) gives "*" and "unterminated"; terminal 3 (the side to move in the
final position resigned) gives the winner's result, Termination "normal" and a last comment "{White resigns}" / "{Black resigns}".

Eval comments: a game with root values (FinishedGame.root_values, BOG2 records) gets after each move m_i the comment
"{<e>/<S> 0.00s}", e = 2 ln((1 + v_i) / (1 - v_i)) pawns (the inverse of eval_to_value, train.py), "%+.2f" clamped to +-99.99, S the
simulations per search -- the pattern pretrain's PGN reader parses (DESIGN "Eval comments").
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import json
import os
import sys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import engine as E
from .pgn import STATUS_NAMES

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
SEVEN_TAGS = ("Event", "Site", "Date", "Round", "White", "Black", "Result")
ST_CHECK, ST_NO_MOVE = 0x1, 0x2  # state byte bits (include/betaone_engine.h, bo_san_render)
MAX_BATCH_POSITIONS = 1 << 20     # positions per bo_san_render launch (a longer game goes alone)
POS_BYTES = C.sizeof(E.BoPosition)


def _fields(g):
    """(game_id, positions, moves, terminal) of a FinishedGame or an unpacked record."""
    if isinstance(g, dict):
        return int(g["game_id"]), g["positions"], g["moves"], int(g["terminal"])
    return int(g.game_id), g.positions, g.moves, int(g.terminal)


def _root_values(g):
    return g.get("root_values") if isinstance(g, dict) else getattr(g, "root_values", None)


def eval_text(v, sims: int) -> str:
    """The eval comment of a root value v (float32, side to move): e = 2 ln((1 + v) / (1 - v)) pawns, %+.2f, clamped to +-99.99."""
    v = float(np.float32(v))
    if v >= 1.0:
        e = 99.99
    elif v <= -1.0:
        e = -99.99
    else:
        e = min(99.99, max(-99.99, 2.0 * np.log((1.0 + v) / (1.0 - v))))
    return f"{e:+.2f}/{int(sims)} 0.00s"


def _position_bytes(positions, n: int) -> bytes:
    raw = getattr(positions, "raw", None)  # engine.PositionList
    if raw is None and isinstance(positions, C.Array):
        raw = positions
    if raw is not None:
        return C.string_at(C.addressof(raw), n * POS_BYTES)
    return b"".join(bytes(p) for p in positions[:n])


class Rendered:
    """One game's device output: san [n, 8] (the SAN body of each move, NUL-padded), state [n + 1] (bit 0 check, bit 1 no legal
    move, per position)."""

    __slots__ = ("game_id", "san", "state")

    def __init__(self, game_id: int, san: np.ndarray, state: np.ndarray):
        self.game_id, self.san, self.state = game_id, san, state

    def sans(self) -> List[str]:
        """The moves' SAN with the check / mate suffix."""
        out = []
        for i in range(len(self.san)):
            s = bytes(self.san[i]).rstrip(b"\0").decode()
            nx = int(self.state[i + 1])
            out.append(s + ("#" if nx & ST_CHECK and nx & ST_NO_MOVE else "+" if nx & ST_CHECK else ""))
        return out

    def mated(self) -> bool:
        return (int(self.state[-1]) & (ST_CHECK | ST_NO_MOVE)) == ST_CHECK | ST_NO_MOVE


def _render_batch(lib, dev, games) -> List[Rendered]:
    G = len(games)
    off = np.zeros(G + 1, np.int32)
    parts, ids = [], []
    for i, g in enumerate(games):
        gid, positions, moves, _ = _fields(g)
        n = len(moves)
        if len(positions) < n + 1:
            raise ValueError(f"render_san: game {gid}: {len(positions)} positions for {n} moves")
        parts.append(_position_bytes(positions, n + 1))
        off[i + 1] = off[i] + n + 1
        ids.append(gid)
    N = int(off[-1])
    mv = np.zeros(N, np.int32)
    for i, g in enumerate(games):
        moves = _fields(g)[2]
        mv[off[i]:off[i + 1] - 1] = np.asarray(moves, dtype=np.int64).astype(np.int32)
    pos_t = torch.from_numpy(np.frombuffer(b"".join(parts), dtype=np.uint8).copy()).to(dev)
    off_t, mv_t = torch.from_numpy(off).to(dev), torch.from_numpy(mv).to(dev)
    san = torch.zeros(N * 8, dtype=torch.uint8, device=dev)
    state = torch.zeros(N, dtype=torch.uint8, device=dev)
    bad = torch.zeros(2 * G, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    rc = lib.bo_san_render(G, N, off_t.data_ptr(), pos_t.data_ptr(), mv_t.data_ptr(), san.data_ptr(), state.data_ptr(), bad.data_ptr(),
                           stream)
    if rc != 0:
        raise E.EngineError(f"bo_san_render: {lib.bo_last_error().decode()}")
    san_h, state_h, bad_h = san.cpu().numpy().reshape(N, 8), state.cpu().numpy(), bad.cpu().numpy().reshape(G, 2)
    for i in range(G):
        if bad_h[i, 0] >= 0:
            st = int(bad_h[i, 1])
            name = STATUS_NAMES[st] if 0 <= st < len(STATUS_NAMES) else str(st)
            raise ValueError(f"render_san: game {ids[i]} ply {int(bad_h[i, 0])}: {name}")
    return [Rendered(ids[i], san_h[off[i]:off[i + 1] - 1], state_h[off[i]:off[i + 1]]) for i in range(G)]


def render_san(games: Sequence, device="cuda:0", lib=None, max_positions: int = MAX_BATCH_POSITIONS) -> List[Rendered]:
    """SAN and position states of every game, on the device, at most max_positions positions per launch.  Raises ValueError naming the
    game id and ply of a move that is not legal ("illegal") or whose next position is not the game's ("mismatch")."""
    lib = lib or E.load_hip_library()
    dev = E.runtime_device(device)
    out: List[Rendered] = []
    batch, n_pos = [], 0
    for g in games:
        n = len(_fields(g)[2]) + 1
        if batch and n_pos + n > max_positions:
            out.extend(_render_batch(lib, dev, batch))
            batch, n_pos = [], 0
        batch.append(g)
        n_pos += n
    if batch:
        out.extend(_render_batch(lib, dev, batch))
    return out


def position_fen(position, lib=None) -> str:
    """FEN of a bo_position (the en-passant field as python-chess Board.fen() writes it)."""
    lib = lib or E.load_hip_library()
    buf = C.create_string_buffer(128)
    if lib.bo_position_fen(C.byref(position), buf, 128) != 0:
        raise E.EngineError(f"bo_position_fen: {lib.bo_last_error().decode()}")
    return buf.value.decode()


def movetext(r: Rendered, root_turn: int, root_fullmove: int, result: str, book_plies: int = 0, lib=None, comments=None,
             final_comment: Optional[str] = None) -> str:
    """comments: a text per ply (written as "{text}" after the move; "" none) -- bo_pgn_movetext_text; else bo_pgn_movetext."""
    lib = lib or E.load_hip_library()
    n = len(r.san)
    san = np.ascontiguousarray(r.san, dtype=np.uint8)
    state = np.ascontiguousarray(r.state, dtype=np.uint8)
    if comments is not None or final_comment:
        texts = [(comments[i] if comments is not None and i < len(comments) else "").encode() for i in range(n)]
        off = np.zeros(n + 1, np.int32)
        np.cumsum([len(t) for t in texts], out=off[1:])
        blob = b"".join(texts)
        cap = 24 * n + int(off[-1]) + 3 * n + len(final_comment or "") + 64
        buf = C.create_string_buffer(cap)
        ln = C.c_int64()
        rc = lib.bo_pgn_movetext_text(n, san.ctypes.data, state.ctypes.data, int(root_turn), int(root_fullmove), blob,
                                      off.ctypes.data_as(C.POINTER(C.c_int32)), (final_comment or "").encode(), result.encode(), buf, cap,
                                      C.byref(ln))
        if rc != 0:
            raise E.EngineError(f"bo_pgn_movetext_text: {lib.bo_last_error().decode()}")
        return buf.raw[:ln.value].decode()
    com = None
    if book_plies:
        com = np.zeros(max(n, 1), np.uint8)
        com[:min(book_plies, n)] = 1
    cap = 24 * n + 64
    buf = C.create_string_buffer(cap)
    ln = C.c_int64()
    rc = lib.bo_pgn_movetext(n, san.ctypes.data, state.ctypes.data, int(root_turn), int(root_fullmove),
                             com.ctypes.data if com is not None else None, result.encode(), buf, cap, C.byref(ln))
    if rc != 0:
        raise E.EngineError(f"bo_pgn_movetext: {lib.bo_last_error().decode()}")
    return buf.raw[:ln.value].decode()


def escape(v) -> str:
    return str(v).replace("\\", "\\\\").replace('"', '\\"')


def result_of(gid: int, positions, terminal: int, r: Rendered):
    """(Result, Termination) of a game."""
    if terminal == 1:
        if not r.mated():
            raise ValueError(f"write_pgn: game {gid} ply {len(r.san)}: terminal 1, but the final position is not checkmate")
        return ("0-1" if positions[len(r.san)].turn == 1 else "1-0"), "normal"
    if terminal == 2:
        return "1/2-1/2", "normal"
    if terminal == 3:  # the side to move in the final position resigned
        return ("0-1" if positions[len(r.san)].turn == 1 else "1-0"), "normal"
    return "*", "unterminated"


def _default_sims() -> int:
    from . import dropin

    dropin.install()
    import config

    return int(config.NUM_SIMULATIONS)


def today() -> str:
    return time.strftime("%Y.%m.%d", time.gmtime())


def write_pgn(fh, games: Sequence, tags=None, device="cuda:0", lib=None, book_plies: Optional[Sequence[int]] = None,
              sims: Optional[int] = None) -> int:
    """Writes `games` to the text file fh; returns the characters written.  tags: one dict for every game, or one dict per game;
    the Seven Tag Roster comes first (missing ones are "?", Date defaults to today's UTC date), then SetUp / FEN when the root is not
    the standard start, Termination, PlyCount, and any other tag given.  book_plies[i]: the first moves of game i that get a
    "{book}" comment.  sims: S of the eval comments of games with root values (default config.NUM_SIMULATIONS of the drop-in)."""
    lib = lib or E.load_hip_library()
    games = list(games)
    per_game = isinstance(tags, (list, tuple))
    if per_game and len(tags) != len(games):
        raise ValueError("write_pgn: one tags dict per game")
    rendered = render_san(games, device=device, lib=lib)
    date = today()
    written = 0
    for i, (g, r) in enumerate(zip(games, rendered)):
        gid, positions, moves, terminal = _fields(g)
        t: Dict[str, object] = dict((tags[i] if per_game else tags) or {})
        given = g.get("result") if isinstance(g, dict) else None  # (an annotated input game keeps its own result token: analyse.py)
        if given is not None:  # (a foreign game's 1-0 may be a resignation or a flag: only a game handed over as terminal 1 must end in mate)
            if terminal == 1 and not r.mated():
                raise ValueError(f"write_pgn: game {gid} ply {len(r.san)}: terminal 1, but the final position is not checkmate")
            result, termination = str(given), ("unterminated" if given == "*" else "normal")
        else:
            result, termination = result_of(gid, positions, terminal, r)
        head = {k: t.pop(k, "?") for k in SEVEN_TAGS}
        if head["Date"] == "?":
            head["Date"] = date
        head["Result"] = result
        root = positions[0]
        fen = position_fen(root, lib)
        if fen != START_FEN:
            head["SetUp"], head["FEN"] = "1", fen
        head["Termination"], head["PlyCount"] = termination, len(moves)
        head.update(t)
        text = "".join(f'[{k} "{escape(v)}"]\n' for k, v in head.items()) + "\n"
        rv = _root_values(g)
        if rv is not None or terminal == 3:
            if sims is None:
                sims = _default_sims()
            com = [eval_text(v, sims) if v is not None else "" for v in rv[:len(moves)]] if rv is not None else None  # (None: no comment)
            if com is not None and book_plies and book_plies[i]:
                com = ["book"] * min(book_plies[i], len(com)) + com[book_plies[i]:]
            fin = None
            if terminal == 3:
                # (a game the tablebases ended -- FinishedGame.adjudicated -- did not resign: the tables give its side to move as lost)
                fin = ("White" if positions[len(moves)].turn == 1 else "Black") + (" is lost by the tablebases" if getattr(g, "adjudicated", False) else " resigns")
            text += movetext(r, root.turn, root.fullmove_number, result, 0, lib, comments=com, final_comment=fin) + "\n"
        else:
            text += movetext(r, root.turn, root.fullmove_number, result, book_plies[i] if book_plies else 0, lib) + "\n"
        fh.write(text)
        written += len(text)
    return written


# ---- the converter: compact records -> PGN -------------------------------------------------------------------------------------------
def bog_paths(args: Sequence[str]) -> List[str]:
    """Files as given; a directory contributes its *.bog files in sorted order."""
    from .records import COMPACT_SUFFIX

    out = []
    for a in args:
        out.extend(sorted(glob.glob(os.path.join(a, "*" + COMPACT_SUFFIX))) if os.path.isdir(a) else [a])
    return out


def convert(paths: Sequence[str], fh, event="BetaOne self-play", player="BetaOne", date=None, device="cuda:0", lib=None,
            batch_plies: int = MAX_BATCH_POSITIONS, sims: Optional[int] = None) -> Dict:
    """Every game of the compact files `paths`, in (path, game_id) order, to fh; batches of about batch_plies plies."""
    from . import records

    lib = lib or E.load_hip_library()
    date = date or today()
    n_games = n_plies = n_chars = 0
    for path in bog_paths(paths):
        with open(path, "rb") as f:
            buf = f.read()
        idx = sorted(records.scan_games(buf), key=lambda e: e[0])
        k = 0
        while k < len(idx):
            j, plies = k, 0
            while j < len(idx) and (j == k or plies + idx[j][1] + 1 <= batch_plies):
                plies += idx[j][1] + 1
                j += 1
            games = records.unpack_games(b"".join(buf[o:o + s] for _, _, o, s in idx[k:j]))
            tags = [{"Event": event, "Date": date, "Round": g["game_id"], "White": player, "Black": player} for g in games]
            n_chars += write_pgn(fh, games, tags=tags, device=device, lib=lib, sims=sims)
            n_games += len(games)
            n_plies += sum(int(g["n_plies"]) for g in games)
            k = j
    return {"games": n_games, "plies": n_plies, "chars": n_chars}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(
        prog="python -m betaone_amd.pgn_write", description="Write self-play games (compact .bog records) as PGN; SAN rendered on the GPU.",
        epilog="Only compact records carry the moves: the reference's per-game pickles hold dense planes and no moves.  Write compact "
               "records with `python -m betaone_amd.selfplay_main --records compact` (or `both`).")
    ap.add_argument("paths", nargs="+", metavar="PATH", help="a .bog file, or a directory whose *.bog files are read in sorted order")
    ap.add_argument("-o", "--out", required=True, metavar="OUT.pgn")
    ap.add_argument("--event", default="BetaOne self-play")
    ap.add_argument("--player", default="BetaOne", help="the White and Black tags")
    ap.add_argument("--date", default=None, help="the Date tag (default: today, UTC), e.g. 2026.10.15")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--sims", type=int, default=None, help="S of the eval comments of BOG2 games (default: config.NUM_SIMULATIONS)")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    with open(args.out, "w", encoding="utf-8", newline="\n") as fh:
        st = convert(args.paths, fh, event=args.event, player=args.player, date=args.date, device=args.device, sims=args.sims)
    st["seconds"] = time.perf_counter() - t0
    st["bytes"] = os.path.getsize(args.out)
    print(json.dumps(st))
    return 0


if __name__ == "__main__":
    sys.exit(main())
