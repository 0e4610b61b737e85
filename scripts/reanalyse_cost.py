"""scripts/reanalyse_cost.py -- what reanalysing self-play records costs on the MI355X, against analysing the PGN export of the same games.

    python scripts/reanalyse_cost.py --out profiles/reanalyse_cost.json

Plays --games self-play games (noise off) with a random-init net, saves them as compact records and exports them with pgn_write; then
`betaone_amd.analyse` on the PGN and `betaone_amd.reanalyse` on the records search the same roots with the same net, --sims simulations
and --slots roots per batch, --runs times each, alternating.  Reported: roots per second of each run (the tools' own search time: set-up,
searches and read-out of every batch, without parsing, upload and writing), the spread of analyse's runs, bo_records_ring and upload
time per file, the per-batch copy."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--moves", type=int, default=40)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--mcts-batch", type=int, default=96)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from analyse_cost import make_net
    from betaone_amd import analyse as A
    from betaone_amd import pgn_write as W
    from betaone_amd import reanalyse as RA
    from betaone_amd import records as R
    from betaone_amd.nn_tune import best_inference_copy
    from betaone_amd.rollout import Rollout

    net = make_net(a.blocks, a.filters)
    dev = torch.device("cuda:0")
    search = dict(mcts_batch_size=a.mcts_batch, cpuct=1.0, widen_coeff=1.5, dirichlet_epsilon=0.25)
    tmp = tempfile.mkdtemp(prefix="reanalyse_cost_")
    d = os.path.join(tmp, "data", "iter_1")
    path = os.path.join(d, "games_rank0.bog")
    t0 = time.perf_counter()
    ro = Rollout(best_inference_copy(net, a.slots, dev), a.slots, num_simulations=a.sims, dirichlet_alpha=0.0, device="cuda:0", rng_mode="native",
                 max_game_moves=a.moves, record_values=True, **search)
    ro.start_games(list(range(a.slots)), list(range(a.slots)), [100 + g for g in range(a.slots)])
    nxt, fins = [a.slots], []

    def refill(slot):
        if nxt[0] >= a.games:
            return None
        nxt[0] += 1
        return nxt[0] - 1, 100 + nxt[0] - 1, None

    while len(fins) < a.games:
        ro.play_ply(on_finished=fins.append, refill=refill)
    ro.close()
    R.save_games(path, sorted(fins, key=lambda f: f.game_id))
    t_play = time.perf_counter() - t0
    pgn = os.path.join(tmp, "games.pgn")
    assert W.main([path, "-o", pgn, "--date", "2026.10.19", "--sims", str(a.sims)]) == 0
    runs = {"analyse": [], "reanalyse": []}
    last = None
    for i in range(a.runs):
        r = A.analyse_games([pgn], net, sims=a.sims, slots=a.slots, **search)["report"]
        runs["analyse"].append(dict(roots=r["positions_analysed"], search_seconds=r["search_seconds"], roots_per_second=r["positions_per_second"],
                                    seconds=r["seconds"], batches=r["batches"], retried=r["roots_searched_again"]))
        last = RA.reanalyse_records([d], net, os.path.join(tmp, f"out{i}"), sims=a.sims, slots=a.slots, **search)
        runs["reanalyse"].append(dict(roots=last["roots_searched"], search_seconds=last["search_seconds"], roots_per_second=last["roots_per_second"],
                                      seconds=last["seconds"], batches=last["batches"], retried=last["roots_retried"],
                                      upload_seconds=last["upload_seconds"], ring_seconds=last["ring_seconds"]))
    rate = lambda k: np.array([x["roots_per_second"] for x in runs[k]])
    out = dict(settings=vars(a), play_seconds=t_play, file_bytes=os.path.getsize(path), positions=int(sum(len(f.moves) + 1 for f in fins)),
               runs=runs, analyse_mean=float(rate("analyse").mean()), analyse_spread=float(rate("analyse").max() - rate("analyse").min()),
               reanalyse_mean=float(rate("reanalyse").mean()), reanalyse_spread=float(rate("reanalyse").max() - rate("reanalyse").min()),
               batch_copy_bytes=last["batch_copy_bytes"], search_result_block_bytes=a.slots * (4 + 2 * 256) * 4 + 16,
               identical_to_input=open(os.path.join(tmp, "out0", "iter_1", "games_rank0.bog"), "rb").read() == open(path, "rb").read(),
               mean_tv=last["mean_tv"], top1_agreement=last["top1_agreement"])
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
