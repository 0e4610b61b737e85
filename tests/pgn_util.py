"""tests/pgn_util.py -- TEST HELPER: writes games as PGN text (SAN through the CPU oracle's rules, oracle/shim) for the pretraining
tests and scripts/pretrain_cost.py.  The product never writes PGN."""
from __future__ import annotations

import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle", "shim") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))

import chess  # noqa: E402  (oracle/shim)

LETTER = {2: "N", 3: "B", 4: "R", 5: "Q", 6: "K"}


def san(board, move) -> str:
    """Standard algebraic notation of a legal move, with the minimal disambiguation and the check / mate suffix."""
    pt = board.piece_type_at(move.from_square)
    ff, tf = move.from_square & 7, move.to_square & 7
    if pt == 6 and abs(tf - ff) == 2:
        s = "O-O" if tf > ff else "O-O-O"
    else:
        capture = board.piece_type_at(move.to_square) is not None or (pt == 1 and ff != tf)
        sq = chess.SQUARE_NAMES[move.to_square]
        if pt == 1:
            s = ("abcdefgh"[ff] + "x" if capture else "") + sq
            if move.promotion:
                s += "=" + LETTER[move.promotion]
        else:
            others = [m for m in board.legal_moves if m.to_square == move.to_square and m.from_square != move.from_square
                      and board.piece_type_at(m.from_square) == pt]
            dis = ""
            if others:
                if all((m.from_square & 7) != ff for m in others):
                    dis = "abcdefgh"[ff]
                elif all((m.from_square >> 3) != (move.from_square >> 3) for m in others):
                    dis = "12345678"[move.from_square >> 3]
                else:
                    dis = chess.SQUARE_NAMES[move.from_square]
            s = LETTER[pt] + dis + ("x" if capture else "") + sq
    board.push(move)
    suffix = "#" if board.is_checkmate() else "+" if board.is_check() else ""
    board.pop()
    return s + suffix


def random_eval_comment(rng: random.Random) -> str:
    r = rng.random()
    depth, secs = rng.randint(1, 30), f"{rng.randint(0, 9)}.{rng.randint(0, 999):03d}s"
    if r < 0.08:
        return f"{rng.choice('+-')}M{rng.randint(0, 12)}/{depth} {secs}"
    ev = f"{rng.choice('+-')}{rng.randint(0, 15)}.{rng.randint(0, 99):02d}/{depth} {secs}"
    return ev + (", adjudicated" if r > 0.97 else "")


def random_game(rng: random.Random, fen=None, max_plies=120, eval_p=0.8, book_p=0.05):
    """(moves as UCI, comments per move or None, SAN list, result): a random legal game from fen; castling, promotions and en passant are
    favoured when available so that every kind of move shows up."""
    b = chess.Board(fen) if fen else chess.Board()
    moves, sans, comments = [], [], []
    for _ in range(max_plies):
        legal = b.legal_moves
        if not legal or b.is_game_over(claim_draw=False):
            break
        special = [m for m in legal if m.promotion or (b.piece_type_at(m.from_square) == 6 and abs((m.to_square & 7) - (m.from_square & 7)) == 2)
                   or (b.piece_type_at(m.from_square) == 1 and m.to_square == b.ep_square)]
        m = rng.choice(special) if special and rng.random() < 0.7 else rng.choice(legal)
        sans.append(san(b, m))
        moves.append(m.uci())
        r = rng.random()
        comments.append(random_eval_comment(rng) if r < eval_p else ("book" if r < eval_p + book_p else None))
        b.push(m)
    return moves, comments, sans, b.result(claim_draw=False) if b.is_game_over() else "*"


def write_game(sans, comments, result="*", fen=None, headers=None, rng=None) -> str:
    """One game's PGN text."""
    out = []
    for k, v in (headers or {}).items():
        out.append(f'[{k} "{v}"]')
    if fen:
        out.append('[SetUp "1"]')
        out.append(f'[FEN "{fen}"]')
    out.append("")
    toks = []
    start_black = fen is not None and fen.split()[1] == "b"
    num = int(fen.split()[5]) if fen and len(fen.split()) > 5 else 1
    for i, s in enumerate(sans):
        black = (i % 2 == 1) != start_black
        if not black:
            toks.append(f"{num}.")
        elif i == 0:
            toks.append(f"{num}...")
        toks.append(s)
        if comments[i] is not None:
            toks.append("{" + comments[i] + "}")
        if black:
            num += 1
    toks.append(result)
    out.append(" ".join(toks))
    return "\n".join(out) + "\n\n"
