"""scripts/value_mix_cost.py -- what training on a mix of z and the root value costs on the MI355X (a sibling of scripts/train_cost.py).

    python scripts/value_mix_cost.py --out profiles/value_mix_cost.json
    python scripts/value_mix_cost.py --root OTHER_CHECKOUT --mixes 0 --out other.json      # another checkout of this repository

Records with root values come from a short CohortRollout self-play run (record_values=True) of the bench's 10x128 net.  For every
batch size the paths train `--steps` timed steps after `--warmup` under torch.autocast + GradScaler, `--repeats` times, taking turns
(mix 0, mix A, mix 0, ...): the spread between the repeats of one path is the noise the difference between two paths has to be read
against.  Mix 0 is train_steps without the argument -- the code path of a checkout that does not have it -- so the same file times
the parent commit when --root names a checkout of it (built, on the same machine, in the same session)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose betaone_amd is measured")
ap.add_argument("--mixes", default="0,0.5")
ap.add_argument("--batches", default="256,1024")
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--games", type=int, default=128)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))

from betaone_amd import dropin, records as R  # noqa: E402
from betaone_amd.train import train_steps  # noqa: E402

DEV = "cuda:0"
SHAPE = (8, 2, 128)


def make_net(seed=0):
    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = SHAPE
    try:
        torch.manual_seed(seed)
        return network.PolicyValueNet().to(DEV)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def selfplay_buffer(n_games):
    from betaone_amd.rollout import CohortRollout

    ro = CohortRollout(make_net().eval(), 64, cohorts=2, num_simulations=16, mcts_batch_size=8, max_game_moves=64, rng_mode="native",
                       device=DEV, record_values=True)
    ro.start_games(list(range(64)), list(range(64)), list(range(64)))
    nxt, fins = [64], []

    def refill(slot):
        if nxt[0] >= n_games:
            return None
        nxt[0] += 1
        return nxt[0] - 1, nxt[0] - 1, None

    while len(fins) < n_games:
        ro.play_ply(on_finished=fins.append, refill=refill)
    ro.close()
    buf = R.GpuReplayBuffer(200000, device=DEV, pi_width=2)
    buf.add(fins)
    return buf


def throughput(buf, B, mix):
    net = make_net(seed=1).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10000, eta_min=5e-7)
    scaler = torch.GradScaler("cuda")
    kw = {"value_mix": mix} if mix else {}
    lkw = {"with_q": True} if mix else {}
    train_steps(net, opt, sched, scaler, buf.loader(B, steps=a.warmup, seed=1, sparse=True, **lkw), **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = train_steps(net, opt, sched, scaler, buf.loader(B, steps=a.steps, seed=2, sparse=True, **lkw), **kw)
    dt = time.perf_counter() - t0  # (train_steps ends reading the losses: the device is done)
    return {"samples_per_s": a.steps * B / dt, "final_loss": r["losses"][-1][0]}


def main():
    assert torch.cuda.is_available(), "value_mix_cost.py measures the GPU"
    mixes = [float(m) for m in a.mixes.split(",")]
    t0 = time.perf_counter()
    buf = selfplay_buffer(a.games)
    out = {"root": os.path.abspath(a.root), "records": len(buf), "games": buf.n_games, "selfplay_s": round(time.perf_counter() - t0, 1),
           "records_with_values": getattr(buf, "n_with_values", None), "net": "10x128", "amp": True, "steps": a.steps,
           "device": torch.cuda.get_device_name(0), "runs": []}
    for B in (int(b) for b in a.batches.split(",")):
        res = {"batch": B, "samples_per_s": {str(m): [] for m in mixes}}
        for _ in range(a.repeats):
            for m in mixes:
                res["samples_per_s"][str(m)].append(round(throughput(buf, B, m)["samples_per_s"], 1))
        res["mean"] = {k: round(float(np.mean(v)), 1) for k, v in res["samples_per_s"].items()}
        res["spread"] = {k: round(float((max(v) - min(v)) / np.mean(v)), 4) for k, v in res["samples_per_s"].items()}
        out["runs"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    buf.close()


if __name__ == "__main__":
    main()
