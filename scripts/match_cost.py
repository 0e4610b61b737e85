"""scripts/match_cost.py -- ms per ply of a head-to-head match against self-play on the driver's configuration (profiles/match_two_net.md).

    python scripts/match_cost.py [--plies 120] [--modes selfplay,pair,merge,selfplay] [--out match_cost.json]

256 slots in 4 cohorts, 800 simulations per move, MCTS batch 96, net 10x128 (hash-initialised; B with other weights), temperature
(8, 1.0, 0.1), alpha 0, games from the start position, no refills.  Each mode: 10 untimed plies, then --plies timed
CohortRollout.play_ply calls.  Modes: selfplay (net A: FusedPolicyValueNet 'tower_split', step tail on), selfplay_b (net B alone), selfplay_notail (the same with
BETAONE_STEP_TAIL=0: the rows kernel kept, as a pair keeps it), pair (PairedNet, one launch for both nets), pair_same (PairedNet of A and
a copy of A: every row on one net's weights), merge (PairedNet route='merge').  Run under `rocprofv3 --kernel-trace --stats` for the
per-kernel split.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plies", type=int, default=120)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--modes", default="selfplay,pair,merge,selfplay")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from betaone_amd import dropin, match as M
    from betaone_amd.fused_net import FusedPolicyValueNet, PairedNet
    from betaone_amd.rollout import CohortRollout
    from betaone_amd.selfplay_main import game_seed
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 10, 0, 128
    dev = "cuda:0"
    a = hash_init_(network.PolicyValueNet(), gain=0.5).to(dev).eval()
    a2 = hash_init_(network.PolicyValueNet(), gain=0.5).to(dev).eval()
    b = hash_init_(network.PolicyValueNet(), gain=0.625).to(dev).eval()
    G, K, S = 256, 4, 800

    def run(model, pair):
        ro = CohortRollout(model, G, cohorts=K, num_simulations=S, dirichlet_alpha=0.0, temperature=(8, 1.0, 0.1), max_game_moves=100000,
                           rng_mode="native", device=dev)
        ids = list(range(G))
        seeds = [game_seed(0, i) for i in ids]
        if pair:
            sch = M.MatchScheduler([(None, "")], G, G, K)
            ro.start_games(ids, ids, seeds, [None] * G, None, [sch.admit(s, 0).net_of_white for s in ids])
        else:
            ro.start_games(ids, ids, seeds, [None] * G)
        for _ in range(args.warm):
            ro.play_ply()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.plies):
            ro.play_ply()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.plies * 1e3
        ro.drain()
        ro.close()
        return ms

    res = {}
    for mode in args.modes.split(","):
        if mode in ("selfplay", "selfplay_b"):
            ms = run(FusedPolicyValueNet(a if mode == "selfplay" else b, conv="tower_split").to(dev), False)
        elif mode == "selfplay_notail":
            os.environ["BETAONE_STEP_TAIL"] = "0"
            try:
                ms = run(FusedPolicyValueNet(a, conv="tower_split").to(dev), False)
            finally:
                del os.environ["BETAONE_STEP_TAIL"]
        elif mode in ("pair", "pair_same"):
            p = PairedNet(a, a2 if mode == "pair_same" else b, batch=G // K, device=dev)
            assert p.route == "pair:tower_split"
            ms = run(p, True)
        elif mode == "merge":
            p = PairedNet(a, b, batch=G // K, device=dev, route="merge")
            assert p.route == "pair:merge"
            ms = run(p, True)
        else:
            raise SystemExit(f"unknown mode {mode}")
        res.setdefault(mode + "_ms_per_ply", []).append(ms)
        print(f"[match_cost] {mode}: {ms:.3f} ms per play_ply", flush=True)
    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
