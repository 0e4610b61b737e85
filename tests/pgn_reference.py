"""tests/pgn_reference.py -- TEST YARDSTICK: the reference's PGNDataset.parse (train.py:81-143) restated on the oracle shim's Board,
dropin.utils.encode_board / RepetitionTracker / move_to_index, with the LIVE tracker (the positions of the game up to the encoded one).
It takes the games' moves and comments as known, so it needs no SAN parser; the eval rule is train.py's parse_pgn_eval / eval_to_value
restated with Python's re (no atomic group: the alternatives cannot overlap)."""
from __future__ import annotations

import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle", "shim") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))

import chess  # noqa: E402  (oracle/shim)

EVAL_RE = re.compile(r"^([+-])(?:M(\d+)|(\d+)\.(\d+))/\d+ \d+\.\d+s(?:,.*)?$")


def eval_target(comment):
    """float32 -value of a move's comment, or None (parse_pgn_eval + eval_to_value + the negation, train.py:32-78, 116-118)."""
    if not comment:
        return None
    m = EVAL_RE.search(comment)
    if not m:
        return None
    sign = -1 if m.group(1) == "-" else 1
    if m.group(2):
        value = 1.0 if sign * int(m.group(2)) > 0 else -1.0
    else:
        ev = sign * (int(m.group(3)) + float(f"0.{m.group(4)}"))
        try:
            value = max(-1.0, min(1.0, 2.0 / (1.0 + math.exp(-(ev / 2))) - 1.0))
        except OverflowError:
            return None
    return np.float32(-value)


def samples(fen, moves, comments):
    """[(planes [120,8,8] float32, action index, z float32)] of one game, in the order PGNDataset.parse yields them."""
    from betaone_amd import dropin

    dropin.install()
    import utils

    board = chess.Board(fen) if fen else chess.Board()
    history = [board.copy()]
    tracker = utils.RepetitionTracker()
    tracker.add_board(board)
    out, buffered = [], None
    for i, u in enumerate(moves):
        move = chess.Move.from_uci(u)
        t = eval_target(comments[i])
        if buffered is not None and t is not None:
            out.append((buffered[0], buffered[1], t))
        buffered = (utils.encode_board(board, history[-8:], tracker).numpy(), utils.move_to_index(move))
        board.push(move)
        tracker.add_board(board)
        history.append(board.copy())
    return out


def end_of_game_planes(fen, moves, k):
    """Ply k's planes with the END-of-game tracker (what the self-play records use): for the test that tells the two apart."""
    from betaone_amd import dropin

    dropin.install()
    import utils

    board = chess.Board(fen) if fen else chess.Board()
    boards = [board.copy()]
    for u in moves:
        board.push(chess.Move.from_uci(u))
        boards.append(board.copy())
    tracker = utils.RepetitionTracker()
    for b in boards:
        tracker.add_board(b)
    return utils.encode_board(boards[k], boards[max(0, k - 7):k + 1], tracker).numpy()
