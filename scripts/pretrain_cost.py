"""scripts/pretrain_cost.py -- what PGN pretraining costs on the MI355X: tokeniser MB/s, SAN replay positions/s, and pretraining samples/s
against train.py's from-buffer samples/s at the same net and batch.

    python scripts/pretrain_cost.py --out profiles/pretrain.json
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/pretrain_cost.py --replay-only --out OUT/r.json   # kernel time

The corpus is built from a seed: random legal games (castling, promotions, en passant favoured) from the start position and from
[FEN] roots, written as SAN through the CPU oracle's rules (tests/pgn_util.py), with synthetic fishtest-style eval comments on 80 % of
the moves.  Pretraining runs PgnIngest's reference order (6 workers) into train.train_steps; the from-buffer side is
scripts/train_cost.py's: a GpuReplayBuffer of 10x128 self-play records.  Both at batch 256 for the 10x128 and 20x256 nets, alternating
pretrain / from-buffer twice each."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

import pgn_util as U  # noqa: E402
import train_cost as TC  # noqa: E402

from betaone_amd import pgn as P  # noqa: E402
from betaone_amd.train import train_steps  # noqa: E402

FENS = [None, None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12", "r1bqkb1r/pppp1ppp/2n2n2/4p3/2B1P3/5N2/PPPP1PPP/RNBQK2R w KQkq - 4 4"]


def corpus(seed, n_games):
    rng = random.Random(seed)
    out = []
    for i in range(n_games):
        fen = FENS[i % len(FENS)]
        _, cm, sans, res = U.random_game(rng, fen=fen, max_plies=rng.randint(40, 160))
        out.append(U.write_game(sans, cm, res, fen=fen, headers={"Event": "fishtest-like", "Round": str(i)}))
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=800)
    ap.add_argument("--files", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--replay-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    text = corpus(0, a.games).encode()
    res = {"games": a.games, "corpus_bytes": len(text), "corpus_build_s": time.perf_counter() - t0}
    # tokeniser: the whole corpus, host
    lib = P.E.load_hip_library()
    t0 = time.perf_counter()
    for _ in range(3):
        pg = P.parse_text(text, lib)
    dt = (time.perf_counter() - t0) / 3
    res["tokenizer_mb_per_s"] = len(text) / 1e6 / dt
    res["tokens"] = pg.n_tokens
    # replay: one launch over every game (the kernel time comes from the rocprofv3 run)
    P.replay_games(pg, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = P.replay_games(pg, device="cuda:0")
    dt = time.perf_counter() - t0
    res["replay_call"] = {"positions": int(r["n_plies"].sum()), "seconds": dt, "positions_per_s": float(r["n_plies"].sum()) / dt,
                          "statuses": {P.STATUS_NAMES[s]: int(c) for s, c in zip(*np.unique(r["status"], return_counts=True))}}
    print(json.dumps(res), flush=True)
    if not a.replay_only:
        d = tempfile.mkdtemp()
        for i in range(a.files):
            with open(os.path.join(d, f"f{i:02d}.pgn"), "wb") as f:
                f.write(text)
        buf = TC.selfplay_buffer(256)
        res["nets"] = []
        for name in ("10x128", "20x256"):
            shape, B = TC.NETS[name], 256
            row = {"net": name, "batch": B, "pretrain": [], "from_buffer": []}
            for rep in range(2):
                net, opt, sched, scaler = TC.fresh(shape)
                ing = P.PgnIngest([d], device="cuda:0", window_plies=1 << 20)
                it = iter(ing.loader(B))
                train_steps(net, opt, sched, scaler, (next(it) for _ in range(a.warmup)), sparse=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train_steps(net, opt, sched, scaler, (next(it) for _ in range(a.steps)), sparse=True)
                dt = time.perf_counter() - t0
                row["pretrain"].append({"samples_per_s": a.steps * B / dt, "replay_s": ing.stats["replay_s"],
                                        "ingest_positions_per_s": ing.counts["plies"] / ing.stats["replay_s"]})
                row["from_buffer"].append(TC.throughput(buf, shape, B, True, a.steps, a.warmup))
                print(json.dumps(row), flush=True)
            pm = float(np.mean([x["samples_per_s"] for x in row["pretrain"]]))
            bm = float(np.mean([x["samples_per_s"] for x in row["from_buffer"]]))
            row["pretrain_over_from_buffer"] = pm / bm
            res["nets"].append(row)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
