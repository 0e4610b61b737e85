"""scripts/validate_cost.py -- what held-out validation costs on the MI355X (profiles/validate.md).

    python scripts/validate_cost.py kernels [--loss-lib OTHER/libbetaone_hip.so]
        bo_train_metrics (csrc/bo_metrics.h) next to bo_train_loss_forward at n = 256 and 4096, fp16 and float32 logits, W = 2: device
        events around back-to-back calls that rotate over input copies larger than the caches together, three windows of >= 0.2 s
        each, the median.  --loss-lib times the loss forward of another build of the library (the parent commit's) in the same run.
    python scripts/validate_cost.py epoch
        one validation pass over a held-out set as a share of an epoch: train_steps and validate.evaluate on the bench's 10x128 net at
        batch 256 under autocast, the same number of batches each; the share for a holdout fraction F is F t_eval / ((1 - F) t_train).
One JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from betaone_amd import engine as E  # noqa: E402

A = 4672
DEV = "cuda:0"
CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
LOSS_ARGS = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 6


def _inputs(n, W, dtype, copies, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for _ in range(copies):
        logits = (torch.randn((n, A), generator=g, device=DEV) * 3.0).to(dtype)
        value = torch.tanh(torch.randn((n,), generator=g, device=DEV)).to(dtype)
        idx = torch.argsort(torch.rand((n, A), generator=g, device=DEV), dim=1)[:, :W].int().contiguous()
        val = torch.rand((n, W), generator=g, device=DEV) + 0.05
        val = (val / val.sum(1, keepdim=True)).contiguous()
        z = torch.randint(-1, 2, (n,), generator=g, device=DEV).float()
        out.append((logits, value, idx, val, z))
    return out


def _time(call, inputs, min_seconds=0.2, windows=3):
    """Median microseconds per call over `windows` windows of back-to-back calls, each at least min_seconds long."""
    for t in inputs:
        call(t)
    torch.cuda.synchronize()
    reps = 64
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            call(inputs[k % len(inputs)])
        b.record()
        torch.cuda.synchronize()
        if a.elapsed_time(b) >= 1e3 * min_seconds:
            break
        reps *= 2
    us = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            call(inputs[k % len(inputs)])
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b) / reps)
    return statistics.median(us), min(us), max(us), reps


def kernels(args):
    lib = E.load_hip_library()
    other = None
    if args.loss_lib:
        other = C.CDLL(args.loss_lib)
        other.bo_train_loss_forward.restype, other.bo_train_loss_forward.argtypes = C.c_int, LOSS_ARGS
    stream = torch.cuda.current_stream().cuda_stream
    W = 2
    for n in (256, 4096):
        for dtype in (torch.float16, torch.float32):
            copies = max(2, int(1.5 * 2 ** 30 / (n * A * dtype.itemsize)))  # 1.5 GiB of logits: no cache holds a copy until its turn comes again
            copies = min(copies, 256)
            inputs = _inputs(n, W, dtype, copies)
            rows = torch.empty((n, E.METRIC_ROW_COLS), device=DEV)
            accum = torch.zeros((1, E.METRIC_COLS), dtype=torch.float64, device=DEV)
            stats, loss3 = torch.empty((n, 4), device=DEV), torch.empty(3, device=DEV)

            def metrics(t):
                rc = lib.bo_train_metrics(n, W, t[0].data_ptr(), CODES[dtype], t[1].data_ptr(), CODES[dtype], t[2].data_ptr(), t[3].data_ptr(),
                                          t[4].data_ptr(), None, None, 1, rows.data_ptr(), accum.data_ptr(), stream)
                assert rc == 0

            def loss_of(which):
                def call(t):
                    rc = which.bo_train_loss_forward(n, W, t[0].data_ptr(), CODES[dtype], t[1].data_ptr(), CODES[dtype], t[2].data_ptr(),
                                                     t[3].data_ptr(), t[4].data_ptr(), stats.data_ptr(), loss3.data_ptr(), stream)
                    assert rc == 0
                return call

            todo = [("bo_train_metrics", metrics), ("bo_train_loss_forward", loss_of(lib))]
            if other is not None:
                todo.append(("bo_train_loss_forward (--loss-lib)", loss_of(other)))
            res = {}
            for rnd in range(2):  # alternate the candidates twice; keep both rounds
                for name, call in todo:
                    res.setdefault(name, []).append(_time(call, inputs))
            for name, runs in res.items():
                print(json.dumps({"what": name, "n": n, "W": W, "dtype": str(dtype).split(".")[-1], "input_copies": copies,
                                  "us_per_call_median": [round(r[0], 2) for r in runs], "us_min": round(min(r[1] for r in runs), 2),
                                  "us_max": round(max(r[2] for r in runs), 2), "calls_per_window": runs[0][3],
                                  "logits_GB_per_s": round(n * A * dtype.itemsize / (1e3 * min(r[0] for r in runs)), 1)}), flush=True)
            del inputs


def epoch(args):
    from betaone_amd import dropin
    from betaone_amd import records as R
    from betaone_amd import train as T
    from betaone_amd import validate as V
    from betaone_amd.rollout import Rollout

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 8, 2, 128
    try:
        torch.manual_seed(0)
        net = network.PolicyValueNet().to(DEV)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    ro = Rollout(net.eval(), 16, num_simulations=16, mcts_batch_size=8, device=DEV, rng_mode="native", max_game_moves=32)
    ro.start_games(list(range(16)), list(range(16)), list(range(16)))
    fins = []
    while any(g is not None for g in ro.games):
        ro.play_ply(on_finished=fins.append)
    ro.close()
    buf = R.GpuReplayBuffer(65536, device=DEV, pi_width=2)
    buf.add(fins)
    batch, steps = 256, args.steps
    index = np.resize(np.arange(len(buf)), batch * steps)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=100000, eta_min=5e-7)
    scaler = torch.GradScaler("cuda", enabled=True)
    out = {"train": [], "evaluate": []}
    for rnd in range(3):  # the first round warms both up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.train_steps(net, opt, sched, scaler, buf.loader(batch, steps=steps, seed=rnd, sparse=True), amp=True, grad_clip=1.0)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        V.evaluate(net, buf, index, batch=batch, amp=True, buckets="phase")
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rnd:
            out["train"].append((t1 - t0) / steps)
            out["evaluate"].append((t2 - t1) / steps)
    tr, ev = min(out["train"]), min(out["evaluate"])
    print(json.dumps({"what": "epoch share", "net": "10x128", "batch": batch, "batches": steps, "records_resident": len(buf),
                      "train_ms_per_batch": [round(1e3 * x, 3) for x in out["train"]], "evaluate_ms_per_batch": [round(1e3 * x, 3) for x in out["evaluate"]],
                      "evaluate_over_train": round(ev / tr, 4),
                      "share_of_epoch": {str(f): round(f * ev / ((1 - f) * tr), 5) for f in (0.02, 0.05, 0.1)}}), flush=True)
    buf.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--loss-lib", default=None)
    e = sub.add_parser("epoch")
    e.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validate_cost: needs an MI355X (no CPU path: a timing taken elsewhere says nothing)")
    {"kernels": kernels, "epoch": epoch}[a.mode](a)
