"""betaone_amd/pretrain.py -- the pretraining stage: supervised training on PGN games before self-play.

The reference runs it first, when checkpoints/ holds neither best_model.pth nor pretrained.pth (main.py:129-139 -> run_pretraining,
train.py:356-396): PGNDataset over the fishtest games, AdamW, CosineAnnealingLR(T_max=PRETRAINING_T_MAX), GradScaler + autocast,
clipping at GRAD_CLIP_MAX, pretrained.pth every MID_EPOCH_CHECKPOINT steps while best_model.pth does not exist, and at the end.  Here the
games are tokenised by the library, replayed and encoded on the device (pgn.PgnIngest), and the steps are train.train_steps with the
sparse-target loss kernels.

    python -m betaone_amd.pretrain fishtest/ --save-dir checkpoints --out pretrain.json
    python -m betaone_amd.pretrain fishtest/ --count          # samples and ceil(samples / batch): PRETRAINING_T_MAX (countpgn.py)
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

from . import engine as E
from . import pgn as PG


def save_weights(model, path: str):
    """torch.save through a temporary file in the destination's directory and os.replace: path is the old file or the whole new one."""
    d = os.path.dirname(path) or "."
    os.makedirs(d, exist_ok=True)
    tmp = os.path.join(d, f".{os.path.basename(path)}.tmp{os.getpid()}")
    torch.save(model.state_dict(), tmp)
    os.replace(tmp, path)


def main(argv=None) -> int:
    from . import dropin
    from . import match as M
    from . import train as T

    dropin.install()
    import config

    ap = argparse.ArgumentParser(prog="python -m betaone_amd.pretrain", description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="*", help="PGN files (.pgn, .pgn.gz) or directories (default: config.PGN_DATA_DIR)")
    ap.add_argument("--save-dir", default=config.SAVE_DIR)
    ap.add_argument("--batch", type=int, default=config.BATCH_SIZE)
    ap.add_argument("--window-plies", type=int, default=1 << 22, help="position slots of the ring the games are replayed into")
    ap.add_argument("--order", choices=("reference", "shuffle"), default="reference")
    ap.add_argument("--workers", type=int, default=None, help="the DataLoader's num_workers the reference order reproduces (config.NUM_WORKERS)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--init", default=None, help="starting weights (state_dict); the net takes its shape from their keys")
    ap.add_argument("--count", action="store_true", help="only ingest: print the samples and ceil(samples / batch)")
    ap.add_argument("--max-games", type=int, default=None, help="games read per file (PGNDataset's max_games)")
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--t-max", type=int, default=None, help="CosineAnnealingLR T_max (default config.PRETRAINING_T_MAX)")
    ap.add_argument("--log-every", type=int, default=100, help="steps per loss interval (and per train_steps call)")
    ap.add_argument("--no-amp", action="store_true")
    ap.add_argument("--out", default=None, help="JSON: games per status, plies, samples, steps, interval losses, lr, samples/s, ingest rate")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    log = lambda s: print(f"[pretrain] {s}", flush=True)  # noqa: E731

    dev = E.runtime_device(a.device)
    paths = PG.pgn_paths(a.paths or [config.PGN_DATA_DIR])
    if not paths:
        log("no PGN files")
        return 1
    ing = PG.PgnIngest(paths, device=dev, window_plies=a.window_plies, order=a.order, workers=a.workers, seed=a.seed, max_games=a.max_games)
    log(f"{len(paths)} PGN files, order {a.order}" + (f", {ing.workers} workers" if a.order == "reference" else ""))

    def summary(extra):
        s = {"files": len(paths), "order": a.order, "batch": a.batch, "counts": dict(ing.counts),
             "tokenizer_mb_per_s": ing.stats["bytes"] / 1e6 / ing.stats["parse_s"] if ing.stats["parse_s"] > 0 else None,
             "ingest_positions_per_s": ing.counts["plies"] / ing.stats["replay_s"] if ing.stats["replay_s"] > 0 else None}
        s.update(extra)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(s, f, indent=1)
        return s

    if a.count:
        n = ing.count()
        log(f"{n} samples, {math.ceil(n / a.batch)} steps at batch {a.batch}; games {ing.counts}")
        print(json.dumps({"samples": n, "steps": math.ceil(n / a.batch)}))
        summary({"samples": n, "steps": math.ceil(n / a.batch)})
        return 0

    torch.manual_seed(a.seed)
    if a.init:
        model = M.build_net(M.load_state_dict(a.init), dev)
    else:
        import network

        model = network.PolicyValueNet().to(dev)
    model.train()
    optimizer = torch.optim.AdamW(model.parameters(), lr=config.LEARNING_RATE, weight_decay=config.WEIGHT_DECAY)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=a.t_max or config.PRETRAINING_T_MAX, eta_min=config.LR_MIN)
    amp = not a.no_amp
    scaler = torch.GradScaler(dev.type, enabled=amp)
    best_path = os.path.join(a.save_dir, "best_model.pth")
    pre_path = os.path.join(a.save_dir, "pretrained.pth")
    mid = int(config.MID_EPOCH_CHECKPOINT)
    writes = []

    it = iter(ing.loader(a.batch, sparse=True, max_steps=a.max_steps))
    state = {"i": 0, "done": False}

    def window(n):
        for _ in range(n):
            b = next(it, None)
            if b is None:
                state["done"] = True
                return
            yield b
            # (resumed after the step of batch i) train.py:325-335 with global_step = i - 1
            i = state["i"]
            if (i - 1) % mid == 0 and not os.path.exists(best_path):
                save_weights(model, pre_path)
                writes.append(i)
            state["i"] = i + 1

    intervals = []
    steps = samples = 0
    per = max(1, a.log_every)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    while not state["done"]:
        lr = optimizer.param_groups[0]["lr"]
        r = T.train_steps(model, optimizer, scheduler, scaler, window(per), sparse=True, amp=amp)
        if r["steps"] == 0:
            break
        steps += r["steps"]
        samples += r["samples"]
        intervals.append({"first_step": steps - r["steps"], "steps": r["steps"], "loss": r["loss"][0], "policy_loss": r["loss"][1],
                          "value_loss": r["loss"][2], "lr": lr, "clipped": r["clipped"]})
        log(f"step {steps}: loss {r['loss'][0]:.4f} policy {r['loss'][1]:.4f} value {r['loss'][2]:.4f} lr {lr:.3g}")
    dt = time.perf_counter() - t0
    save_weights(model, pre_path)
    log(f"{steps} steps, {samples} samples in {dt:.1f} s ({samples / dt if dt > 0 else 0:.0f} samples/s); weights {pre_path}")
    summary({"steps": steps, "samples": samples, "seconds": dt, "samples_per_s": samples / dt if dt > 0 else None,
             "steps_per_s": steps / dt if dt > 0 else None, "amp": amp, "lr_final": optimizer.param_groups[0]["lr"], "intervals": intervals,
             "checkpoint_writes_after_batch": writes, "weights": pre_path})
    ing.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
