"""betaone_amd/train.py -- the training stage of the AlphaZero loop: compact self-play records -> GpuReplayBuffer -> a new net.

The reference trains in train.py (/root/reference/train.py:252-345 train_network, 386-481 run_training_iteration, main.py:96-127 resume):
dense pickles read into one Python list, a DataLoader, F.cross_entropy against a dense [B,4672] target, and three .item() per step.
Here the records stay in HBM (records.GpuReplayBuffer), a batch keeps pi as the records hold it (at most pi_width entries per ply) and
the loss is a pair of HIP kernels that read that sparse target (csrc/bo_train.h): the dense row is never built.  The tower's forward and
backward passes are PyTorch's (MIOpen); only the loss and its gradient are hand-written.

    loss, p_loss, v_loss = sparse_policy_value_loss(logits, value, pi_idx, pi_val, z)     # train.calculate_loss, sparse target
    loss, p_loss, v_mix, v_z, v_q = sparse_policy_value_loss_mix(logits, value, pi_idx, pi_val, z, q, mix)   # value target (1-mix) z + mix q

    python -m betaone_amd.train --iteration 3 --data-dir data --save-dir checkpoints --candidate cand.pth
    python -m betaone_amd.train --value-mix 0.5 ...     # records of selfplay_main --record-values, or of a run with resignation
    python -m betaone_amd.train --holdout-fraction 0.05 ...   # 5 % of the games never train; validated after every epoch (validate.py)
    python -m betaone_amd.train --merge-duplicates input ...  # records with equal inputs train on their group's mean pi, z and q (csrc/bo_merge.h)
    python -m betaone_amd.match checkpoints/best_model.pth cand.pth --promote checkpoints/best_model.pth
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import re
import sys
import time
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import engine as E
from . import records as R

DTYPE_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}  # BO_DTYPE_* of include/betaone_engine.h
ROW_STATS = 4
ROW_STATS_MIX = 6


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def _check(lib, rc: int):
    if rc != 0:
        raise E.EngineError(f"training loss: {lib.bo_last_error().decode()}")


def _and(names) -> str:
    return names[0] if len(names) == 1 else ", ".join(names[:-1]) + " and " + names[-1]


def check_batch(who, logits, value, pi_idx, pi_val, z, extras=(), device=None, device_name="one device"):
    """The input check of the loss and of validate.MetricsAccumulator.add: logits [n,4672] and value (n elements) in one of DTYPE_CODES
    each, pi_idx [n,W] int32, pi_val [n,W] and z (n elements) float32; extras: (name, tensor or None, dtype, elements or None for n) per
    optional input; everything on `device` (default: the logits').  ValueError / TypeError with `who` in front.  Returns (logits, value,
    pi_idx, pi_val, z, *the extras' tensors), contiguous."""
    n, W = pi_idx.shape
    named = [("logits", logits), ("value", value), ("pi_idx", pi_idx), ("pi_val", pi_val), ("z", z)] + [(k, t) for k, t, _, _ in extras if t is not None]
    if (logits.dim() != 2 or logits.shape != (n, E.NUM_ACTIONS) or value.numel() != n or pi_val.shape != (n, W) or z.numel() != n
            or any(t is not None and t.numel() != (n if count is None else count) for _, t, _, count in extras)):
        raise ValueError(f"{who}: shapes " + " ".join(f"{k} {tuple(t.shape)}" for k, t in named))
    if logits.dtype not in DTYPE_CODES or value.dtype not in DTYPE_CODES:
        raise TypeError(f"{who}: logits {logits.dtype} / value {value.dtype}: float32, float16 or bfloat16")
    want = [("pi_idx", pi_idx, torch.int32), ("pi_val", pi_val, torch.float32), ("z", z, torch.float32)] + [e[:3] for e in extras if e[1] is not None]
    if any(t.dtype != dt for _, t, dt in want):
        raise TypeError(f"{who}: {_and([k for k, _, dt in want if dt == torch.int32])} int32, "
                        f"{_and([k for k, _, dt in want if dt == torch.float32])} float32")
    dev = logits.device if device is None else device
    if any(t.device != dev for _, t in named):
        raise ValueError(f"{who}: all inputs on {device_name}")
    return tuple(t.contiguous() for t in (logits, value, pi_idx, pi_val, z)) + tuple(None if t is None else t.contiguous() for _, t, _, _ in extras)


def batch_args(logits, value, pi_idx, pi_val, z):
    """The arguments every bo_train_* entry point starts with (engine._TRAIN_BATCH), of checked tensors."""
    n, W = pi_idx.shape
    return (n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.data_ptr(), DTYPE_CODES[value.dtype], pi_idx.data_ptr(), pi_val.data_ptr(),
            z.data_ptr())


class _SparseLoss(torch.autograd.Function):
    """Without a mix: loss3 = [total, policy, value] of bo_train_loss_forward, row statistics [n,4].  With q and mix: loss5 of
    bo_train_loss_forward_mix, row statistics [n,6]; both are read on the device.  The backward is the matching bo_train_loss_backward
    with the gradient of the first three losses read from the device (a GradScaler scale reaches the kernel without a host round
    trip; loss5's two diagnostics carry none)."""

    @staticmethod
    def forward(ctx, logits, value, pi_idx, pi_val, z, q, mix):
        lib = E.load_hip_library()
        mixed = mix is not None
        extras = (("q", q, torch.float32, None), ("mix", mix, torch.float32, 1)) if mixed else ()
        batch = check_batch("sparse loss", logits, value, pi_idx, pi_val, z, extras)
        n = pi_idx.shape[0]
        row_stats = torch.empty((n, ROW_STATS_MIX if mixed else ROW_STATS), dtype=torch.float32, device=logits.device)
        loss = torch.empty(5 if mixed else 3, dtype=torch.float32, device=logits.device)
        fn = lib.bo_train_loss_forward_mix if mixed else lib.bo_train_loss_forward
        _check(lib, fn(*batch_args(*batch[:5]), *(t.data_ptr() for t in batch[5:]), row_stats.data_ptr(), loss.data_ptr(), _stream(logits)))
        ctx.save_for_backward(row_stats, *batch)
        ctx.value_shape = batch[1].shape
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = E.load_hip_library()
        row_stats, *batch = ctx.saved_tensors
        g3 = g[:3].to(torch.float32).contiguous()
        dlogits, dvalue = torch.empty_like(batch[0]), torch.empty_like(batch[1])
        fn = lib.bo_train_loss_backward_mix if len(batch) > 5 else lib.bo_train_loss_backward
        _check(lib, fn(*batch_args(*batch[:5]), *(t.data_ptr() for t in batch[5:]), row_stats.data_ptr(), g3.data_ptr(), dlogits.data_ptr(),
                       dvalue.data_ptr(), _stream(batch[0])))
        return dlogits, dvalue.view(ctx.value_shape), None, None, None, None, None


def sparse_policy_value_loss(logits, value, pi_idx, pi_val, z):
    """(total, policy, value) of train.calculate_loss (train.py:222-249) with the target as [B,W] indices (-1 = unused) and values:
    policy = mean_b -sum_e pi_val[b,e] * log_softmax(logits[b])[pi_idx[b,e]], value = mean_b (value[b] - z[b])^2, total = their sum.
    logits [B,4672] and value [B,1] (or [B]) in float32, float16 or bfloat16 -- the net's outputs, under torch.autocast too; the three
    losses are float32 tensors on the logits' device.  Computed on the current stream by two HIP kernels (csrc/bo_train.h)."""
    loss3 = _SparseLoss.apply(logits, value, pi_idx, pi_val, z.reshape(-1), None, None)
    return loss3[0], loss3[1], loss3[2]


def sparse_policy_value_loss_mix(logits, value, pi_idx, pi_val, z, q, mix):
    """(total, policy, value_mix, value_vs_z, value_vs_q): sparse_policy_value_loss with the value head regressed on
    t = (1 - mix) z + mix q, q [B,1] (or [B]) the records' root values (GpuReplayBuffer.batch_sparse_q; both z and q are from the side
    to move's point of view).  value_mix = mean (value - t)^2 and total = policy + value_mix; value_vs_z and value_vs_q are the means
    against z and q alone, detached diagnostics.  mix: a Python float, or a one-element float32 tensor on the logits' device that the
    kernels read when they run (change it in place under a captured step).  mix == 0 is sparse_policy_value_loss bit for bit; a mix
    outside [0, 1] is not clamped, every loss is NaN."""
    if not isinstance(mix, torch.Tensor):
        mix = torch.tensor([float(mix)], dtype=torch.float32, device=logits.device)
    loss5 = _SparseLoss.apply(logits, value, pi_idx, pi_val, z.reshape(-1), q.reshape(-1), mix.reshape(-1))
    return loss5[0], loss5[1], loss5[2], loss5[3].detach(), loss5[4].detach()


def dense_policy_value_loss(logits, value, target_policy, target_value):
    """The reference's calculate_loss on a dense target (train.py:222-249): the A/B baseline of --dense-loss and the tests' yardstick."""
    value_loss = F.mse_loss(value, target_value)
    policy_loss = F.cross_entropy(logits, target_policy)
    return value_loss + policy_loss, policy_loss, value_loss


def train_steps(model, optimizer, scheduler, scaler, loader, *, sparse: bool = True, amp: bool = True, grad_clip: Optional[float] = None,
                log_every: int = 0, log=None, value_mix=0.0) -> Dict:
    """One pass of train_network's loop (train.py:271-295) over `loader`'s batches: zero_grad, forward (under torch.autocast when amp),
    scaler.scale(loss).backward(), unscale_, clip_grad_norm_(max_norm=GRAD_CLIP_MAX), scaler.step, scaler.update, scheduler.step.
    sparse: batches are (states, pi_idx, pi_val, z) and the loss is sparse_policy_value_loss; otherwise (states, pi, z) and
    dense_policy_value_loss.  The running losses stay on the device: the host reads them every `log_every` steps (0: never) and at the
    end.  Returns {"steps", "samples", "loss": [total, policy, value] means, "losses": [steps][3] per step, "clipped": steps whose
    gradient norm exceeded grad_clip}.
    value_mix: a float other than 0, or a one-element float32 device tensor WHATEVER it holds (its value is the device's business: a
    schedule may change it between steps) -> batches are batch_sparse_q's five-tuples (loader(..., with_q=True)) and the loss is
    sparse_policy_value_loss_mix; "loss"[2] / "losses"[:, 2] are then value_mix and the result gains "value_vs_z" / "value_vs_q" (means)
    and "diagnostics" [steps][2].  At 0 nothing changes: four-tuples and sparse_policy_value_loss."""
    mixed = isinstance(value_mix, torch.Tensor) or float(value_mix) != 0.0
    if mixed and not sparse:
        raise ValueError("train_steps: value_mix needs the sparse loss")
    if mixed and not isinstance(value_mix, torch.Tensor):  # one upload, not one per step
        value_mix = torch.tensor([float(value_mix)], dtype=torch.float32, device=next(model.parameters()).device)
    diag: List[torch.Tensor] = []
    if grad_clip is None:
        from . import dropin

        dropin.install()
        import config

        grad_clip = config.GRAD_CLIP_MAX
    model.train()
    per_step: List[torch.Tensor] = []
    clipped: List[torch.Tensor] = []
    samples = 0
    for batch in loader:
        states = batch[0]
        dev = states.device
        optimizer.zero_grad()
        if mixed and len(batch) < 5:
            raise ValueError(f"train_steps: value_mix is set (a tensor counts whatever it holds) but the loader yields {len(batch)}-tuples: "
                             f"it needs batch_sparse_q's (states, pi_idx, pi_val, z, q) -- loader(..., sparse=True, with_q=True)")
        with torch.autocast(dev.type, enabled=amp):
            logits, value = model(states)
            if mixed:
                loss, p_loss, v_loss, v_z, v_q = sparse_policy_value_loss_mix(logits, value, batch[1], batch[2], batch[3], batch[4], value_mix)
                diag.append(torch.stack([v_z, v_q]))
            elif sparse:
                loss, p_loss, v_loss = sparse_policy_value_loss(logits, value, batch[1], batch[2], batch[3])
            else:
                loss, p_loss, v_loss = dense_policy_value_loss(logits, value, batch[1], batch[2])
        scaler.scale(loss).backward()
        scaler.unscale_(optimizer)
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=grad_clip)
        scaler.step(optimizer)
        scaler.update()
        scheduler.step()
        per_step.append(torch.stack([loss.detach(), p_loss.detach(), v_loss.detach()]).float())
        clipped.append(norm.detach() > grad_clip)
        samples += int(states.shape[0])
        if log is not None and log_every and len(per_step) % log_every == 0:
            m = torch.stack(per_step[-log_every:]).mean(0).tolist()
            log(f"step {len(per_step)}: loss {m[0]:.4f} policy {m[1]:.4f} value {m[2]:.4f} lr {optimizer.param_groups[0]['lr']:.3g}")
    if not per_step:
        return {"steps": 0, "samples": 0, "loss": [0.0, 0.0, 0.0], "losses": [], "clipped": 0}
    losses = torch.stack(per_step)
    host = losses.cpu()
    out = {"steps": len(per_step), "samples": samples, "loss": host.double().mean(0).tolist(), "losses": host.tolist(),
           "clipped": int(torch.stack(clipped).sum().item())}
    if mixed:
        d = torch.stack(diag).cpu()
        out.update(value_vs_z=float(d[:, 0].double().mean()), value_vs_q=float(d[:, 1].double().mean()), diagnostics=d.tolist())
    return out


# ---- the command line: one training iteration of main.py's loop ---------------------------------------------------------------

def iteration_files(data_dir: str, iteration: int, past: int = 5):
    """{iteration: [compact files]} for load_recent_data's window (train.py:187-193: iterations max(0, I - past) .. I), and the
    iterations of the window that hold only the reference's pickles."""
    found, pickles_only = {}, []
    for it in range(max(0, iteration - past), iteration + 1):
        d = os.path.join(data_dir, f"iter_{it}")
        files = sorted(glob.glob(os.path.join(d, f"games_rank*{R.COMPACT_SUFFIX}")))
        if files:
            found[it] = files
        elif glob.glob(os.path.join(d, "game_*.pkl")):
            pickles_only.append(it)
    return found, pickles_only


def load_window_games(files: Dict[int, List[str]]) -> List[dict]:
    """The games of the window that have plies, oldest iteration first, each with its "iteration" (validate.holdout_games keys the
    split on it and the game's id)."""
    games = []
    for it in sorted(files):
        for f in files[it]:
            for g in R.load_games(f):
                if int(g["n_plies"]) > 0:
                    g["iteration"] = it
                    games.append(g)
    return games


def load_buffer(files: Dict[int, List[str]], device, games: Optional[List[dict]] = None) -> R.GpuReplayBuffer:
    """A replay buffer sized for all the games of the window (nothing is evicted: record k of the buffer is record k of the games in
    load_window_games' order)."""
    if games is None:
        games = load_window_games(files)
    if not games:
        raise SystemExit("train: the compact files of the window hold no plies")
    width = max(2, max(len(ix) for g in games for ix, _ in g["pis"]))
    plies = sum(int(g["n_plies"]) + 1 for g in games)
    buf = R.GpuReplayBuffer(capacity_plies=plies + 64, device=device, pi_width=width)
    lost = buf.add(games)
    if lost:
        raise SystemExit(f"train: {lost} records did not fit the replay buffer")
    return buf


def checkpoint_iteration(path: str) -> int:
    return int(re.search(r"checkpoint_iter_(\d+)\.pth$", path).group(1))


def latest_checkpoint(save_dir: str) -> Optional[str]:
    files = glob.glob(os.path.join(save_dir, "checkpoint_iter_*.pth"))
    return max(files, key=checkpoint_iteration) if files else None


def save_checkpoint(path: str, model, optimizer, scheduler, iteration: int):
    """train.save_checkpoint's layout (train.py:484-520), loadable by train.load_checkpoint."""
    torch.save({"iteration": iteration, "model_state_dict": model.state_dict(), "optimizer_state_dict": optimizer.state_dict(),
                "scheduler_state_dict": scheduler.state_dict()}, path)


def main(argv=None) -> int:
    from . import dropin
    from . import match as M

    dropin.install()
    import config

    ap = argparse.ArgumentParser(prog="python -m betaone_amd.train", description=__doc__.split("\n\n")[0])
    ap.add_argument("--iteration", type=int, default=None, help="the iteration to train (default: the one after the newest checkpoint)")
    ap.add_argument("--data-dir", default=config.DATA_DIR)
    ap.add_argument("--save-dir", default=config.SAVE_DIR)
    ap.add_argument("--past", type=int, default=5, help="iterations before --iteration whose records are read too (load_recent_data)")
    ap.add_argument("--epochs", type=int, default=config.EPOCHS_PER_ITERATION)
    ap.add_argument("--batch", type=int, default=config.BATCH_SIZE)
    ap.add_argument("--steps-per-epoch", type=int, default=None, help="batches drawn with replacement per epoch (default: one shuffled pass)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--init", default=None, help="initial weights (state_dict); the net takes its shape from their keys")
    ap.add_argument("--candidate", default=None, help="write the new weights here and leave best_model.pth alone")
    ap.add_argument("--out", default=None, help="JSON with per-epoch losses, learning rate, steps/s and samples/s")
    ap.add_argument("--dense-loss", action="store_true", help="the reference's calculate_loss on dense batches (A/B comparisons)")
    ap.add_argument("--value-mix", type=float, default=0.0, metavar="A",
                    help="regress the value head on (1 - A) z + A q, q the records' root values (selfplay_main --record-values or a resign "
                         "threshold); 0 = the game's outcome alone, as the reference trains")
    ap.add_argument("--merge-duplicates", choices=sorted(R.MERGE_KEYS), default=None, metavar="KEY",
                    help="average the targets of training records that recur: 'input' merges records whose 120 planes are equal, 'position' "
                         "those whose current board is (GpuReplayBuffer.merge_duplicates); held-out games never contribute")
    ap.add_argument("--merge-sample", choices=("records", "groups"), default="records",
                    help="with --merge-duplicates: 'records' draws as ever and replaces each record's targets by its group's; 'groups' draws "
                         "one record per group, so every distinct input counts once per epoch")
    ap.add_argument("--augment", choices=("none",) + tuple(sorted(R.AUGMENT_CODES)), default="none",
                    help="hand every training sample out under a random board symmetry (csrc/bo_sym.h): 'colour' = as it is or with the "
                         "colours swapped, 'mirror' = as it is or with the files mirrored (records with a castling right stay as they are), "
                         "'both' = one of the four; held-out validation stays untransformed")
    ap.add_argument("--holdout-fraction", type=float, default=0.0, metavar="F",
                    help="keep this share of the games (whole games, chosen by a hash of iteration, game id and --holdout-seed) out of "
                         "training and evaluate them after every epoch (betaone_amd.validate); 0 = train on everything")
    ap.add_argument("--holdout-seed", type=int, default=0)
    ap.add_argument("--no-amp", action="store_true", help="float32 forward (the reference trains under torch.autocast)")
    ap.add_argument("--log-every", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.value_mix != 0.0 and a.dense_loss:
        ap.error("--value-mix needs the sparse loss: not with --dense-loss")
    if a.merge_duplicates and a.dense_loss:
        ap.error("--merge-duplicates needs the sparse loss: not with --dense-loss")
    if not 0.0 <= a.value_mix <= 1.0:
        ap.error(f"--value-mix {a.value_mix}: a mix in [0, 1]")
    if not 0.0 <= a.holdout_fraction < 1.0:
        ap.error(f"--holdout-fraction {a.holdout_fraction}: a share in [0, 1)")
    log = lambda s: print(f"[train] {s}", flush=True)  # noqa: E731

    dev = E.runtime_device(a.device)
    torch.manual_seed(a.seed)
    best_path = os.path.join(a.save_dir, "best_model.pth")
    # weights: --init, else best_model.pth, else a fresh net of config's shape (main.py:96-127 resumes from best + newest checkpoint)
    if a.init:
        model = M.build_net(M.load_state_dict(a.init), dev)
    elif os.path.exists(best_path):
        model = M.build_net(M.load_state_dict(best_path), dev)
    else:
        import network

        model = network.PolicyValueNet().to(dev)
    model.train()
    optimizer = torch.optim.AdamW(model.parameters(), lr=config.LEARNING_RATE, weight_decay=config.WEIGHT_DECAY)
    total_steps = config.NUM_ITERATIONS * config.EPOCHS_PER_ITERATION * math.ceil(config.GAME_BUFFER_SIZE / config.BATCH_SIZE)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=total_steps, eta_min=config.LR_MIN)
    start_iter = 0
    ck = latest_checkpoint(a.save_dir)
    if ck:
        state = torch.load(ck, map_location=dev)
        model.load_state_dict(state["model_state_dict"])
        optimizer.load_state_dict(state["optimizer_state_dict"])
        scheduler.load_state_dict(state["scheduler_state_dict"])
        start_iter = int(state["iteration"]) + 1
        log(f"resumed from {ck}: iteration {start_iter}")
    iteration = start_iter if a.iteration is None else a.iteration

    files, pickles_only = iteration_files(a.data_dir, iteration, a.past)
    for it in pickles_only:
        log(f"iteration {it} has only pickles (game_*.pkl, written with --records pickle): its positions cannot be recovered from the "
            f"planes; re-run its self-play with --records compact or both to train on it")
    if not files:
        log(f"no compact records for iterations {max(0, iteration - a.past)}..{iteration} under {a.data_dir}")
        return 1
    train_index = held_index = None
    games = None
    if a.holdout_fraction > 0.0:
        from . import validate as V

        games = load_window_games(files)
        train_index, held_index = V.holdout_games(games, a.holdout_fraction, a.holdout_seed)
        if held_index.size == 0 or train_index.size == 0:
            raise SystemExit(f"train: --holdout-fraction {a.holdout_fraction} (seed {a.holdout_seed}) holds out "
                             f"{V.held_out_game_count(games, a.holdout_fraction, a.holdout_seed)} of the {len(games)} games: "
                             f"{'nothing to validate on' if held_index.size == 0 else 'nothing left to train on'}")
    buf = load_buffer(files, dev, games=games)
    if held_index is not None:
        log(f"held out: {held_index.size} records of {V.held_out_game_count(games, a.holdout_fraction, a.holdout_seed)} games "
            f"(fraction {a.holdout_fraction}, seed {a.holdout_seed}); {train_index.size} records train")
    log(f"iteration {iteration}: {len(buf)} records of {buf.n_games} games from iterations {sorted(files)} (pi_width {buf.pi_width})")
    with_values = buf.n_with_values
    if a.value_mix > 0.0 and with_values == 0:
        n_rec = len(buf)
        buf.close()
        raise SystemExit(f"train: --value-mix {a.value_mix}: none of the {n_rec} records carries a root value: "
                         f"run selfplay_main with --record-values or a resign threshold")
    if a.value_mix > 0.0:
        log(f"value target (1 - {a.value_mix}) z + {a.value_mix} q: {with_values} of {len(buf)} records carry a root value (the rest train on z)")

    merged = merge_report = None
    draw_index = train_index
    if a.merge_duplicates:  # over the training records only: a held-out game's targets never reach a training target
        merged = buf.merge_duplicates(index=train_index, key=a.merge_duplicates)
        merge_report = dict(merged.report(), sample=a.merge_sample)
        if a.merge_sample == "groups":
            draw_index = merged.representatives
        merge_report["records_per_epoch"] = int(len(buf) if draw_index is None else draw_index.size)
        log(f"merged targets ({a.merge_duplicates}): {merged.n_groups} groups of {merged.n_records} records, "
            f"{100.0 * merge_report['duplicate_share']:.1f}% of them in groups larger than one, largest {merged.largest_group}, "
            f"pi width {merged.width}; sampling {a.merge_sample}: {merge_report['records_per_epoch']} per epoch")

    amp = not a.no_amp
    scaler = torch.GradScaler(dev.type, enabled=amp)
    epochs = []
    augment = None if a.augment == "none" else a.augment
    applied_codes = np.zeros(4, dtype=np.int64)   # samples trained under each applied symmetry code
    if augment:
        log(f"augment {augment}: every sample under one of the codes {list(R.AUGMENT_CODES[augment])} (bit 0 colour flip, bit 1 file mirror)")
    for ep in range(a.epochs):
        loader = buf.loader(a.batch, steps=a.steps_per_epoch, seed=a.seed * 1000003 + iteration * 1009 + ep, sparse=not a.dense_loss,
                            with_q=a.value_mix > 0.0, index=draw_index, merged=merged, augment=augment)
        lr = optimizer.param_groups[0]["lr"]
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = train_steps(model, optimizer, scheduler, scaler, loader, sparse=not a.dense_loss, amp=amp, log_every=a.log_every, log=log,
                        value_mix=a.value_mix)
        dt = time.perf_counter() - t0  # (train_steps ends reading the losses: the device is done)
        applied_codes += loader.applied_counts if augment else np.array([r["samples"], 0, 0, 0], dtype=np.int64)
        epochs.append({"epoch": ep, "steps": r["steps"], "samples": r["samples"], "loss": r["loss"][0], "policy_loss": r["loss"][1],
                       "value_loss": r["loss"][2], "lr": lr, "clipped": r["clipped"], "seconds": dt,
                       "steps_per_s": r["steps"] / dt if dt > 0 else None, "samples_per_s": r["samples"] / dt if dt > 0 else None,
                       # (at mix 0 the value loss IS the loss against z, and nothing is compared with q)
                       "value_vs_z": r.get("value_vs_z", r["loss"][2]), "value_vs_q": r.get("value_vs_q"), "records_with_values": with_values})
        val = ""
        if held_index is not None:  # (after the clock: the epoch's steps/s stay those of training)
            rep = V.evaluate(model, buf, held_index, batch=a.batch, amp=amp, with_q=with_values > 0)
            epochs[-1]["validation"] = rep["overall"]
            o = rep["overall"]
            fmt = lambda x: "-" if x is None else f"{x:.4f}"  # noqa: E731
            val = f"; val policy {fmt(o['policy_ce'])} top1 {fmt(o['policy_top1'])} value {fmt(o['value_mse_z'])}"
        log(f"epoch {ep + 1}/{a.epochs}: loss {r['loss'][0]:.4f} policy {r['loss'][1]:.4f} value {r['loss'][2]:.4f} "
            f"({r['steps']} steps, {r['samples'] / dt if dt > 0 else 0:.0f} samples/s){val}")
    if merged is not None:
        merged.close()
    buf.close()

    os.makedirs(a.save_dir, exist_ok=True)
    ck_path = os.path.join(a.save_dir, f"checkpoint_iter_{iteration}.pth")
    save_checkpoint(ck_path, model, optimizer, scheduler, iteration)
    weights = a.candidate or best_path
    if os.path.dirname(weights):
        os.makedirs(os.path.dirname(weights), exist_ok=True)
    torch.save(model.state_dict(), weights)
    log(f"checkpoint {ck_path}; weights {weights}")
    if a.out:
        summary = {"iteration": iteration, "records": sum(e["samples"] for e in epochs[:1]), "loss": "dense" if a.dense_loss else "sparse",
                   "amp": amp, "batch": a.batch, "value_mix": a.value_mix, "epochs": epochs, "checkpoint": ck_path, "weights": weights,
                   "augment": a.augment, "applied_codes": {str(t): int(c) for t, c in enumerate(applied_codes)}}
        if held_index is not None:
            summary.update(holdout_fraction=a.holdout_fraction, holdout_seed=a.holdout_seed, held_out_records=int(held_index.size))
        if merge_report is not None:
            summary["merge"] = merge_report
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
