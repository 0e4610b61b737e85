"""scripts/analyse_cost.py -- what analysing a PGN file costs on the MI355X, with and without the device set-up.

    python scripts/analyse_cost.py --path strings --out profiles/analyse_strings.json     # the ABI before bo_games_reset_dev (runs on any commit)
    python scripts/analyse_cost.py --path device  --out profiles/analyse_device.json      # betaone_amd.analyse
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/analyse_cost.py --path device --positions 4096 --out OUT/r.json

Both paths search the same roots -- every position before a move of a seeded corpus of random legal games (tests/pgn_util.py) -- with the
same net (--blocks x --filters float32, random init), `--slots` roots per batch, `--sims` simulations, Dirichlet noise off, through the
same Rollout evaluate stage and captured graph.  "strings": per batch bo_games_reset from the root FEN and the UCI moves so far,
bo_root_info, a host-made go mask, Rollout.search (begin, the iterations, a poll, bo_search_result).  "device": analyse_games."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pgn_util as U  # noqa: E402

FENS = [None, None, None, "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12", "4k3/8/8/8/8/8/8/4K2R b K - 7 33"]


def corpus(seed, positions, max_plies):
    rng = random.Random(seed)
    games, text, n = [], [], 0
    while n < positions:
        fen = FENS[len(games) % len(FENS)]
        mv, _, sans, res = U.random_game(rng, fen=fen, max_plies=max_plies, eval_p=0.0, book_p=0.0)
        games.append((fen, mv))
        text.append(U.write_game(sans, [None] * len(mv), res, fen=fen, headers={"Event": f"g{len(games)}"}))
        n += len(mv)
    return games, "".join(text)


def make_net(blocks, filters):
    import torch
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = blocks, 0, filters
    torch.manual_seed(0)
    return network.PolicyValueNet().to("cuda:0").eval()


def run_strings(games, net, slots, sims, batch):
    import torch
    from betaone_amd.nn_tune import best_inference_copy
    from betaone_amd.rollout import Rollout

    roots = [(f, mv[:k]) for f, mv in games for k in range(len(mv))]
    ro = Rollout(best_inference_copy(net, slots, torch.device("cuda:0")), slots, num_simulations=sims, mcts_batch_size=batch, dirichlet_alpha=0.0,
                 max_plies=max(len(mv) for _, mv in games) + 2, device="cuda:0")
    t_setup = t_search = 0.0
    searched = 0
    values = []
    t0 = time.perf_counter()
    for b0 in range(0, len(roots), slots):
        part = roots[b0:b0 + slots]
        n = len(part)
        t1 = time.perf_counter()
        ro.eng.reset(list(range(n)), [f for f, _ in part], [" ".join(m) or None for _, m in part], stream=ro._stream())
        nl, term, _ = ro.eng.root_info(ro._stream())
        go = np.zeros(slots, np.int32)
        go[:n] = term[:n] == 0
        t2 = time.perf_counter()
        res = ro.search(go, nl, term)
        t_search += time.perf_counter() - t2
        t_setup += t2 - t1
        searched += int(go.sum())
        values.append(res["best_move"][:n].copy())
    wall = time.perf_counter() - t0
    ro.close()
    return dict(path="strings", roots=len(roots), searched=searched, seconds=wall, setup_seconds=t_setup, search_seconds=t_search,
                positions_per_second=searched / wall, best_moves_crc=int(np.concatenate(values).astype(np.int64).sum()))


def run_device(text, net, slots, sims, batch):
    from betaone_amd import analyse as A

    t0 = time.perf_counter()
    r = A.analyse_games(text, net, sims=sims, slots=slots, mcts_batch_size=batch)
    rep = r["report"]
    allr = np.concatenate([g["plies"] for g in r["games"]])
    done = allr["phase"] == 2
    return dict(path="device", roots=rep["replayed_moves"], searched=rep["positions_analysed"], seconds=time.perf_counter() - t0,
                search_seconds=rep["search_seconds"], positions_per_second=rep["positions_per_second"], batches=rep["batches"],
                roots_searched_again=rep["roots_searched_again"],
                best_moves_crc=int(np.where(done, allr["best_move"], 0).astype(np.int64).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", choices=("strings", "device"), required=True)
    ap.add_argument("--positions", type=int, default=20480)
    ap.add_argument("--plies", type=int, default=120)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--mcts-batch", type=int, default=96)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    games, text = corpus(a.seed, a.positions, a.plies)
    net = make_net(a.blocks, a.filters)
    out = run_strings(games, net, a.slots, a.sims, a.mcts_batch) if a.path == "strings" else run_device(text, net, a.slots, a.sims, a.mcts_batch)
    out.update(settings=dict(positions=a.positions, slots=a.slots, sims=a.sims, mcts_batch=a.mcts_batch, blocks=a.blocks, filters=a.filters, seed=a.seed))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
