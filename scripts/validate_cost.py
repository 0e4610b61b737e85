"""scripts/validate_cost.py -- what held-out validation costs on the MI355X (profiles/validate.md).

    python scripts/validate_cost.py kernels [--loss-lib OTHER/libbetaone_hip.so]
        bo_train_metrics (csrc/bo_metrics.h) next to the loss entry points (forward and backward, and their _mix forms at mixes 0 and
        0.5) at n = 256 and 4096, fp16 and float32 logits, W = 2: device events around back-to-back calls that rotate over input copies
        larger than the caches together, three windows of >= 0.2 s each.  --loss-lib times the same calls of another build of the
        library (the parent commit's) in the same run, the two taking turns, and adds a verdict per entry point: this build's median
        against the other's slowest window, and whether the other's own spread is smaller than the difference.
    python scripts/validate_cost.py parity --loss-lib OTHER.so [--device cpu]
        both builds on the cases of tests/loss_cases.py and tests/metrics_cases.py, every dtype pair, all five entry points: every
        output compared as bytes; prints the number of comparisons and of mismatches.  --device cpu: the wave emulator's build
        (tests/wave_emulator) against another emulator build, e.g. the one a worktree of the parent commit makes with its build.sh.
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
        q = torch.tanh(0.8 * torch.randn((n,), generator=g, device=DEV))
        out.append((logits, value, idx, val, z, q))
    return out


def _time(call, copies, min_seconds=0.2, windows=3):
    """Microseconds per call in each of `windows` windows of back-to-back calls call(k), k rotating over the input copies, each window
    at least min_seconds long; and the calls per window."""
    for k in range(copies):
        call(k)
    torch.cuda.synchronize()
    reps = 64
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(reps):
            call(k % copies)
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
            call(k % copies)
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b) / reps)
    return us, reps


ENTRIES = (("bo_train_metrics", None), ("bo_train_loss_forward", None), ("bo_train_loss_backward", None), ("bo_train_loss_forward_mix", 0.0),
           ("bo_train_loss_forward_mix", 0.5), ("bo_train_loss_backward_mix", 0.0), ("bo_train_loss_backward_mix", 0.5))


def kernels(args):
    from betaone_amd import train as T

    libs = [("", E.load_hip_library())]
    if args.loss_lib:
        libs.append((" (--loss-lib)", E.bind(C.CDLL(args.loss_lib))))
    stream = torch.cuda.current_stream().cuda_stream
    W = 2
    for n in (256, 4096):
        for dtype in (torch.float16, torch.float32):
            copies = max(2, int(1.5 * 2 ** 30 / (n * A * dtype.itemsize)))  # 1.5 GiB of logits: no cache holds a copy until its turn comes again
            copies = min(copies, 256)
            inputs = _inputs(n, W, dtype, copies)
            rows = torch.empty((n, E.METRIC_ROW_COLS), device=DEV)
            accum = torch.zeros((1, E.METRIC_COLS), dtype=torch.float64, device=DEV)
            loss, g3 = torch.empty(5, device=DEV), torch.tensor([1.0, 0.0, 0.0], device=DEV)
            dlogits, dvalue = torch.empty((n, A), dtype=dtype, device=DEV), torch.empty(n, dtype=dtype, device=DEV)
            mixes = {m: torch.tensor([m], device=DEV) for m in (0.0, 0.5)}
            # a copy's row statistics per kind of forward (the builds write the same bits): a backward reads what a forward left
            stats = {m: torch.zeros((copies, n, T.ROW_STATS_MIX), device=DEV) for m in (None, 0.0, 0.5)}

            def caller(lib, entry, mix):
                fn = getattr(lib, entry)
                sets = []
                for k, t in enumerate(inputs):   # the arguments once per copy: the timed loop is the calls alone
                    head = T.batch_args(*t[:5])
                    if entry == "bo_train_metrics":
                        sets.append(head + (None, None, 1, rows.data_ptr(), accum.data_ptr(), stream))
                        continue
                    head += (t[5].data_ptr(), mixes[mix].data_ptr(), stats[mix][k].data_ptr()) if mix is not None else (stats[mix][k].data_ptr(),)
                    sets.append(head + ((loss.data_ptr(), stream) if "forward" in entry else
                                        (g3.data_ptr(), dlogits.data_ptr(), dvalue.data_ptr(), stream)))

                def call(k):
                    assert fn(*sets[k]) == 0

                return call

            todo = [((entry, mix, tag), caller(lib, entry, mix)) for entry, mix in ENTRIES for tag, lib in libs]   # forwards before backwards
            res = {}
            for rnd in range(2):  # the candidates take turns, twice; both rounds are kept
                for key, call in todo:
                    res.setdefault(key, []).append(_time(call, copies))
            for (entry, mix, tag), runs in res.items():
                wins = [u for r in runs for u in r[0]]
                print(json.dumps({"what": entry + ("" if mix is None else f" mix {mix}") + tag, "n": n, "W": W, "dtype": str(dtype).split(".")[-1],
                                  "input_copies": copies, "us_per_call_median": [round(statistics.median(r[0]), 2) for r in runs],
                                  "windows_us": [round(u, 3) for u in wins], "us_min": round(min(wins), 2), "us_max": round(max(wins), 2),
                                  "calls_per_window": runs[0][1],
                                  "logits_GB_per_s": round(n * A * dtype.itemsize / (1e3 * min(statistics.median(r[0]) for r in runs)), 1)}), flush=True)
            if len(libs) > 1:   # this build against the other's own spread in this run
                for entry, mix in ENTRIES:
                    mine = [u for r in res[(entry, mix, libs[0][0])] for u in r[0]]
                    theirs = [u for r in res[(entry, mix, libs[1][0])] for u in r[0]]
                    diff, spread = statistics.median(mine) - statistics.median(theirs), max(theirs) - min(theirs)
                    print(json.dumps({"what": "verdict " + entry + ("" if mix is None else f" mix {mix}"), "n": n, "dtype": str(dtype).split(".")[-1],
                                      "median_us": round(statistics.median(mine), 3), "other_median_us": round(statistics.median(theirs), 3),
                                      "other_slowest_window_us": round(max(theirs), 3), "other_spread_us": round(spread, 3),
                                      "no_slower_than_the_other_s_slowest_window": statistics.median(mine) <= max(theirs),
                                      "difference_resolved": abs(diff) > spread}), flush=True)
            del inputs


# ---- parity: two builds of the library on the same inputs, byte for byte --------------------------------------------------------------

PARITY_MIXES = (0.0, 0.25, 1.0, 1.5, float("nan"))


def _outputs(lib, dev, stream, logits, value, idx, val, z, q, bucket, n_buckets, w3):
    """Every output of the five entry points of `lib` on one batch: {name: tensor}.  Without a q the mix entry points get z (what a
    record without a root value has) and the metrics none."""
    from betaone_amd import train as T

    n = idx.shape[0]
    batch = T.batch_args(logits, value, idx, val, z)
    g3 = torch.tensor(w3, dtype=torch.float32, device=dev)
    out = {}

    def ok(rc):
        assert rc == 0, lib.bo_last_error().decode()

    def loss_buffers(cols, losses):
        return (torch.zeros((n, cols), device=dev), torch.zeros(losses, device=dev), torch.zeros_like(logits), torch.zeros_like(value))

    st, loss, dx, dv = loss_buffers(T.ROW_STATS, 3)
    ok(lib.bo_train_loss_forward(*batch, st.data_ptr(), loss.data_ptr(), stream))
    ok(lib.bo_train_loss_backward(*batch, st.data_ptr(), g3.data_ptr(), dx.data_ptr(), dv.data_ptr(), stream))
    out.update({"row_stats": st, "loss3": loss, "dlogits": dx, "dvalue": dv})
    qq = z if q is None else q
    for mix in PARITY_MIXES:
        m = torch.tensor([mix], dtype=torch.float32, device=dev)
        st, loss, dx, dv = loss_buffers(T.ROW_STATS_MIX, 5)
        ok(lib.bo_train_loss_forward_mix(*batch, qq.data_ptr(), m.data_ptr(), st.data_ptr(), loss.data_ptr(), stream))
        ok(lib.bo_train_loss_backward_mix(*batch, qq.data_ptr(), m.data_ptr(), st.data_ptr(), g3.data_ptr(), dx.data_ptr(), dv.data_ptr(), stream))
        out.update({f"row_stats mix {mix}": st, f"loss5 mix {mix}": loss, f"dlogits mix {mix}": dx, f"dvalue mix {mix}": dv})
    rows = torch.zeros((n, E.METRIC_ROW_COLS), device=dev)
    accum = torch.zeros((n_buckets, E.METRIC_COLS), dtype=torch.float64, device=dev)
    ok(lib.bo_train_metrics(*batch, None if q is None else q.data_ptr(), None if bucket is None else bucket.data_ptr(), n_buckets,
                            rows.data_ptr(), accum.data_ptr(), stream))
    out.update({"rows": rows, "accum": accum})
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    return out


def parity(args):
    """Both libraries on every case of tests/loss_cases.py (finite and non-finite) and of tests/metrics_cases.py (with its drop-out
    cases), every dtype pair the backend has, all five entry points, the mixes of PARITY_MIXES: every output tensor compared as bytes."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import loss_cases as LC
    import metrics_cases as MC
    import value_mix_cases as VM

    dev = args.device
    if torch.device(dev).type == "cuda":
        this, stream = E.load_hip_library(), torch.cuda.current_stream().cuda_stream
        pairs = LC.PAIRS
    else:  # the wave emulator's build of the same sources (tests/wave_emulator): it has no _Float16
        import engine_harness as H

        this, stream = H.emu_lib(), 0
        pairs = tuple(p for p in LC.PAIRS if torch.float16 not in p)
    other = E.bind(C.CDLL(os.path.abspath(args.loss_lib)))
    assert this._handle != other._handle, "--loss-lib is the library under test"
    batches = [(c.name, c.logits, c.value, c.idx, c.val, c.z, VM.root_values_for(c), None, 1, c.w3) for c in LC.cases() + tuple(LC.nonfinite_cases())]
    batches += [(c.name, c.logits, c.value, c.idx, c.val, c.z, c.q, c.bucket, c.n_buckets, LC.W3[2]) for c in MC.cases() + tuple(MC.dropout_cases())]
    tensors = elements = bad_tensors = bad_bytes = 0
    for name, logits, value, idx, val, z, q, bucket, n_buckets, w3 in batches:
        for pair in pairs:
            t = [logits.to(pair[0]), value.to(pair[1]).reshape(-1), idx, val, z.reshape(-1), None if q is None else q.reshape(-1), bucket]
            t = [None if a is None else a.contiguous().to(dev) for a in t]
            a, b = (_outputs(lib, dev, stream, *t, n_buckets, w3) for lib in (this, other))
            for key in a:
                diff = int((a[key].view(torch.uint8) != b[key].view(torch.uint8)).sum())
                tensors, elements = tensors + 1, elements + a[key].numel()
                if diff:
                    bad_tensors, bad_bytes = bad_tensors + 1, bad_bytes + diff
                    print(json.dumps({"what": "mismatch", "case": name, "pair": [LC.short(pair[0]), LC.short(pair[1])], "output": key,
                                      "bytes": diff}), flush=True)
    print(json.dumps({"what": "parity", "device": dev, "other": args.loss_lib, "cases": len(batches), "dtype_pairs": len(pairs),
                      "mixes": [str(m) for m in PARITY_MIXES], "comparisons": tensors, "elements": elements, "mismatches": bad_tensors,
                      "mismatching_bytes": bad_bytes}), flush=True)
    return 1 if bad_tensors else 0


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
    p = sub.add_parser("parity")
    p.add_argument("--loss-lib", required=True)
    p.add_argument("--device", default=DEV)
    a = ap.parse_args()
    if a.mode == "parity":
        sys.exit(parity(a))
    if not torch.cuda.is_available():
        raise SystemExit("validate_cost: needs an MI355X (no CPU path: a timing taken elsewhere says nothing)")
    {"kernels": kernels, "epoch": epoch}[a.mode](a)
