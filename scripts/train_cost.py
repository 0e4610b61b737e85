"""scripts/train_cost.py -- what a training step costs on the MI355X, sparse-target loss kernels (csrc/bo_train.h) against the reference's
dense calculate_loss (--dense-loss), under torch.autocast + GradScaler as train.py:278 trains.

    python scripts/train_cost.py --out profiles/train_cost.json                      # steps/s, samples/s, per-phase event split
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python scripts/train_cost.py --profile-only --out OUT/p.json   # kernel split

Records come from a short CohortRollout self-play run of the 10x128 net.  For each net (10x128: 8 + 2 SE blocks x 128, the bench's;
20x256: 15 + 5 x 256, config's default) and batch (256, 1024) both loss paths train `--steps` timed steps after `--warmup`, alternating
sparse / dense twice.  A second pass times the phases of one step with device events (sample, forward, loss, backward, optimizer:
unscale + clip + step + update + scheduler).  Bytes the loss kernels move are computed from the shapes."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from betaone_amd import dropin, records as R  # noqa: E402
from betaone_amd.train import dense_policy_value_loss, sparse_policy_value_loss, train_steps  # noqa: E402

NETS = {"10x128": (8, 2, 128), "20x256": (15, 5, 256)}
DEV = "cuda:0"
HBM_BPS = 6.29e12  # MI355X_MICROARCH: measured float4 copy


def make_net(shape, seed=0):
    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = shape
    try:
        torch.manual_seed(seed)
        return network.PolicyValueNet().to(DEV)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def selfplay_buffer(n_games):
    from betaone_amd.rollout import CohortRollout

    ro = CohortRollout(make_net(NETS["10x128"]).eval(), 64, cohorts=2, num_simulations=16, mcts_batch_size=8, max_game_moves=64,
                       rng_mode="native", device=DEV)
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


def fresh(shape):
    net = make_net(shape, seed=1).train()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
    return net, opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=10000, eta_min=5e-7), torch.GradScaler("cuda")


def throughput(buf, shape, B, sparse, steps, warmup):
    net, opt, sched, scaler = fresh(shape)
    train_steps(net, opt, sched, scaler, buf.loader(B, steps=warmup, seed=1, sparse=sparse), sparse=sparse)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = train_steps(net, opt, sched, scaler, buf.loader(B, steps=steps, seed=2, sparse=sparse), sparse=sparse)
    dt = time.perf_counter() - t0
    return {"steps_per_s": steps / dt, "samples_per_s": steps * B / dt, "final_loss": r["losses"][-1][0]}


def phase_split(buf, shape, B, sparse, steps):
    """Device-event split of a step (the same step as train_steps), median over `steps` steps after 3 warm-up steps."""
    net, opt, sched, scaler = fresh(shape)
    rng = np.random.default_rng(3)
    names = ["sample", "forward", "loss", "backward", "optimizer"]
    rows = []
    for i in range(steps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        q = rng.integers(0, len(buf), size=B)
        ev[0].record()
        batch = buf.batch_sparse(q) if sparse else buf.batch(q)
        ev[1].record()
        opt.zero_grad()
        with torch.autocast("cuda"):
            logits, value = net(batch[0])
            ev[2].record()
            if sparse:
                loss = sparse_policy_value_loss(logits, value, batch[1], batch[2], batch[3])[0]
            else:
                loss = dense_policy_value_loss(logits, value, batch[1], batch[2])[0]
        ev[3].record()
        scaler.scale(loss).backward()
        ev[4].record()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=2.0)
        scaler.step(opt)
        scaler.update()
        sched.step()
        ev[5].record()
        torch.cuda.synchronize()
        if i >= 3:
            rows.append([ev[k].elapsed_time(ev[k + 1]) for k in range(5)])
    med = np.median(np.array(rows), axis=0)
    return {n: round(float(v), 4) for n, v in zip(names, med)} | {"step_ms": round(float(med.sum()), 4)}


def loss_bytes(B, W=2, dtype_bytes=2):
    """Bytes the loss kernels must move: forward reads logits + value + targets, writes row stats; backward reads the logits again
    and the targets, writes dlogits + dvalue."""
    tgt = B * (W * 8 + 4)
    fwd = B * 4672 * dtype_bytes + B * dtype_bytes + tgt + B * 16
    bwd = 2 * B * 4672 * dtype_bytes + 2 * B * dtype_bytes + tgt + B * 16
    return {"forward": fwd, "backward": bwd, "forward_us_at_hbm_peak": fwd / HBM_BPS * 1e6, "backward_us_at_hbm_peak": bwd / HBM_BPS * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--games", type=int, default=192)
    ap.add_argument("--profile-only", action="store_true", help="a few steps of each path at B=1024 on 10x128, for a kernel trace")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "train_cost.py measures the GPU"
    t0 = time.perf_counter()
    buf = selfplay_buffer(a.games)
    out = {"records": len(buf), "games": buf.n_games, "selfplay_s": round(time.perf_counter() - t0, 1), "amp": True,
           "device": torch.cuda.get_device_name(0), "runs": []}
    if a.profile_only:
        for sparse in (True, False):
            net, opt, sched, scaler = fresh(NETS["10x128"])
            train_steps(net, opt, sched, scaler, buf.loader(1024, steps=5, seed=1, sparse=sparse), sparse=sparse)
        torch.cuda.synchronize()
    else:
        for name, shape in NETS.items():
            for B in (256, 1024):
                res = {"net": name, "batch": B}
                for rep in range(2):  # alternate the two paths: the spread between repeats is the noise
                    for sparse in (True, False):
                        key = "sparse" if sparse else "dense"
                        res.setdefault(key, []).append(throughput(buf, shape, B, sparse, a.steps, a.warmup))
                for key in ("sparse", "dense"):
                    res[key + "_split_ms"] = phase_split(buf, shape, B, key == "sparse", 10)
                res["sparse_over_dense_samples_per_s"] = float(np.mean([r["samples_per_s"] for r in res["sparse"]]) /
                                                               np.mean([r["samples_per_s"] for r in res["dense"]]))
                res["loss_bytes_fp16"] = loss_bytes(B)
                out["runs"].append(res)
                print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    buf.close()


if __name__ == "__main__":
    main()
