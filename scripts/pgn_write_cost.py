"""scripts/pgn_write_cost.py -- what PGN export costs on the MI355X: end-to-end converter throughput (compact .bog records -> PGN, plies/s
and MB/s of PGN; in process into memory, and one run of the command line writing a file) and, under rocprofv3, the render kernel's time
per million plies.

    python scripts/pgn_write_cost.py --out profiles/pgn_write.json
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/pgn_write_cost.py --render-only --out OUT/r.json   # kernel time

The corpus is built from a seed: `--distinct` random legal games (castling, promotions, en passant favoured, from the start position and
[FEN] roots; tests/pgn_util.py's generator on the CPU oracle's rules) of up to `--plies` plies, repeated under new game ids up to
`--games` games, saved as compact records with records.save_games in files of 2 500 games.  The converter is pgn_write.convert, the
body of `python -m betaone_amd.pgn_write`."""
import argparse
import io
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pgn_util as U  # noqa: E402

from betaone_amd import pgn_write as W  # noqa: E402
from betaone_amd import records as R  # noqa: E402

FENS = [None, None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12", "4k3/8/8/8/8/8/8/4K2R b K - 7 33"]


class Fin:
    """The fields of a FinishedGame that records.pack_game reads."""

    def __init__(self, game_id, positions, moves, terminal):
        self.game_id, self.positions, self.moves, self.terminal = game_id, positions, moves, terminal
        self.outcome, self.first_ply = 0.0, 0
        self.pis = [(np.array([0], np.int32), np.array([1.0], np.float32))] * len(moves)


def corpus(seed, n_distinct, max_plies):
    import engine_cases as EC

    rng = random.Random(seed)
    out = []
    for i in range(n_distinct):
        fen = FENS[i % len(FENS)]
        mv, _, _, _ = U.random_game(rng, fen=fen, max_plies=max_plies)
        b = U.chess.Board(fen) if fen else U.chess.Board()
        pos, moves = [], []
        for u in mv + [None]:
            pos.append(EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1))
            if u:
                m = U.chess.Move.from_uci(u)
                moves.append(m.from_square | m.to_square << 6 | (m.promotion or 0) << 12)
                b.push(m)
        out.append((pos, moves, 1 if b.is_checkmate() else 2 if b.is_game_over(claim_draw=False) else 0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--games", type=int, default=10000)
    ap.add_argument("--distinct", type=int, default=1000)
    ap.add_argument("--plies", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--render-only", action="store_true", help="only render_san over the corpus (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t0 = time.perf_counter()
    base = corpus(args.seed, args.distinct, args.plies)
    fins = [Fin(i, *base[i % len(base)]) for i in range(args.games)]
    plies = sum(len(f.moves) for f in fins)
    res = {"games": args.games, "distinct": args.distinct, "plies": plies, "corpus_s": time.perf_counter() - t0}
    if args.render_only:
        W.render_san(fins[:64], device="cuda:0")  # (warm-up)
        t = time.perf_counter()
        W.render_san(fins, device="cuda:0")
        res["render_s"] = time.perf_counter() - t
    else:
        with tempfile.TemporaryDirectory() as d:
            for k in range(0, args.games, 2500):
                R.save_games(os.path.join(d, f"games_rank{k // 2500}.bog"), fins[k:k + 2500])
            W.convert([d], io.StringIO(), date="2026.01.01", device="cuda:0")  # (warm-up: library, allocator, page cache)
            runs = []
            for _ in range(args.repeats):
                f = io.StringIO()
                t = time.perf_counter()
                st = W.convert([d], f, date="2026.01.01", device="cuda:0")
                sec = time.perf_counter() - t
                mb = len(f.getvalue().encode()) / 1e6
                runs.append({"seconds": sec, "plies_per_s": st["plies"] / sec, "pgn_mb": mb, "pgn_mb_per_s": mb / sec})
            res["convert"] = runs
            # the command line as a user runs it: a fresh process, the PGN written to a file
            import subprocess

            out = os.path.join(d, "out.pgn")
            t = time.perf_counter()
            subprocess.run([sys.executable, "-m", "betaone_amd.pgn_write", d, "-o", out, "--date", "2026.01.01"], check=True, cwd=ROOT,
                           stdout=subprocess.DEVNULL)
            sec = time.perf_counter() - t
            mb = os.path.getsize(out) / 1e6
            res["cli"] = {"seconds": sec, "plies_per_s": plies / sec, "pgn_mb": mb, "pgn_mb_per_s": mb / sec,
                          "note": "python -m betaone_amd.pgn_write DIR -o FILE: process start, library load, reading, rendering, writing"}
            # where the time goes: SAN render (device + transfers) vs the whole write
            t = time.perf_counter()
            W.render_san(fins, device="cuda:0")
            res["render_san_s"] = time.perf_counter() - t
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
