"""scripts/symmetry_cost.py -- what a board symmetry costs in the replay samplers on the MI355X, and how consistently a net treats a
position and its twin.

    python scripts/symmetry_cost.py --out profiles/symmetry_cost.json [--parent-lib PATH/libbetaone_hip.so] [--checkpoint W.pth]

Plays --games self-play games with a random-init net (the corpus recipe of scripts/merge_cost.py) and adds them to a GpuReplayBuffer.
Each of the four samplers is then called at --batch records per call (the training batch size) in five variants: today's entry point,
and the _sym entry point with codes all 0, all 1, all 3 and random.  With --parent-lib the same games are also added to a buffer of a
library built from the parent commit, and its samplers are a sixth variant ("parent") and, where that library exports the _sym entry
points, a seventh ("parent sym random": the random codes through the parent's).  After --warmup rounds the variants are called in turn,
in a new random order every round, --reps rounds; every call is timed by device events around it and by the host clock (the call ends
in a stream synchronise).  The same record indices are used by every variant of a round.  Reported: median, minimum, maximum and the
quartiles per variant, and the ratio of medians to the baseline (the parent's sampler where there is one, else today's entry point);
with a parent, also whether this tree's median is inside the parent's own spread (no higher than the parent's third quartile), "plain"
against "parent" and "sym random" against "parent sym random".  The outputs of all eight entry points are compared byte for byte with
the parent's on 4096 random records.
Then validate.symmetry_consistency for a random-init net and, with --checkpoint, for those weights."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

SAMPLERS = ("batch", "batch_sparse", "batch_sparse_q", "batch_merged")


def parent_buffer(path, games, width, device):
    """A GpuReplayBuffer on another build of the library (the parent commit's), bound by hand: every bo_replay_* entry point that
    library exports, the _sym ones included where it has them (buf.has_sym)."""
    from betaone_amd import engine as E
    from betaone_amd import records as R

    lib = C.CDLL(path)
    for name, (res, args) in E._SYMBOLS.items():
        if name.startswith(("bo_replay_", "bo_last_error")) and hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    buf = object.__new__(R.GpuReplayBuffer)
    buf.lib, buf.device, buf.pi_width, buf.n_evicted = lib, device, width, 0
    h = C.c_void_p()
    slots = sum(int(g["n_plies"]) + 1 for g in games) + 64
    buf._check(lib.bo_replay_create(slots, width, device.index or 0, C.byref(h)))
    buf.h = h
    buf.has_sym = all(hasattr(lib, f"bo_replay_sample{k}_sym") for k in ("", "_sparse", "_sparse_q", "_merged"))
    assert buf.add(games) == 0
    return buf


def stat(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), q1=float(np.percentile(v, 25)), q3=float(np.percentile(v, 75)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=32)
    ap.add_argument("--mcts-batch", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--batch", type=int, nargs="+", default=(256, 4096))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--train-epochs", type=int, default=0, help="also train the random-init net on the corpus this many epochs, once with "
                    "--augment none and once with --augment both, and report the consistency of both results")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from analyse_cost import make_net
    from betaone_amd import match as M
    from betaone_amd import records as R
    from betaone_amd import validate as V
    from betaone_amd.nn_tune import best_inference_copy
    from betaone_amd.rollout import Rollout

    dev = torch.device("cuda:0")
    net = make_net(a.blocks, a.filters)
    t0 = time.perf_counter()
    ro = Rollout(best_inference_copy(net, a.slots, dev), a.slots, num_simulations=a.sims, mcts_batch_size=a.mcts_batch, device="cuda:0",
                 rng_mode="native", max_game_moves=a.moves, record_values=True)
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
    games = R.unpack_games(b"".join(R.pack_game(f) for f in sorted(fins, key=lambda f: f.game_id)))
    width = max(2, max(len(ix) for g in games for ix, _ in g["pis"]))
    buf = R.GpuReplayBuffer(sum(int(g["n_plies"]) + 1 for g in games) + 64, device="cuda:0", pi_width=width)
    assert buf.add(games) == 0
    n = len(buf)
    free = V.without_castling_rights(games)
    print(f"[symmetry_cost] {a.games} games in {time.perf_counter() - t0:.1f} s: {n} records, pi_width {width}, "
          f"{int(free.sum())} without castling rights", flush=True)
    merged = buf.merge_duplicates()
    old = old_merged = None
    if a.parent_lib:
        old = parent_buffer(a.parent_lib, games, width, buf.device)
        old_merged = old.merge_duplicates()
        assert len(old) == n and old_merged.width == merged.width
    out = dict(settings=vars(a), records=n, pi_width=width, merged_width=merged.width, records_without_castling_rights=int(free.sum()), samplers={})

    rng = np.random.default_rng(0)
    for batch in a.batch:
        codes = {"sym all 0": np.zeros(batch, np.int32), "sym all 1": np.ones(batch, np.int32), "sym all 3": np.full(batch, 3, np.int32),
                 "sym random": rng.integers(0, 4, size=batch).astype(np.int32)}
        for name in SAMPLERS:
            def call(b, m, idx, sym=None, name=name):
                kw = {} if sym is None else {"sym": sym}
                return b.batch_merged(m, idx, **kw) if name == "batch_merged" else getattr(b, name)(idx, **kw)

            variants = {"plain": lambda idx: call(buf, merged, idx)}
            for label, c in codes.items():
                variants[label] = lambda idx, c=c: call(buf, merged, idx, c)
            if old is not None:
                variants["parent"] = lambda idx: call(old, old_merged, idx)
                if old.has_sym:
                    variants["parent sym random"] = lambda idx, c=codes["sym random"]: call(old, old_merged, idx, c)
            labels = list(variants)
            dev_ms, host_ms = {k: [] for k in labels}, {k: [] for k in labels}
            for r in range(a.warmup + a.reps):
                idx = rng.integers(0, n, size=batch)
                for k in rng.permutation(len(labels)):
                    label = labels[k]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    res = variants[label](idx)
                    e1.record()
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if r >= a.warmup:
                        dev_ms[label].append(e0.elapsed_time(e1))
                        host_ms[label].append(dt * 1e3)
                    del res
            base = "parent" if old is not None else "plain"
            row = {k: dict(device_ms=stat(dev_ms[k]), host_ms=stat(host_ms[k]), ratio_to_baseline=float(np.median(dev_ms[k]) / np.median(dev_ms[base])))
                   for k in labels}
            out["samplers"][f"{name} @ {batch}"] = dict(baseline=base, variants=row)
            for mine, theirs in (("plain", "parent"), ("sym random", "parent sym random")):
                if theirs in row:   # this tree's median against the parent's own spread
                    row[mine]["parent_variant"] = theirs
                    row[mine]["median_within_parent_q3"] = bool(row[mine]["device_ms"]["median"] <= row[theirs]["device_ms"]["q3"])
            print(f"[symmetry_cost] {name} @ {batch}: " + "; ".join(
                f"{k} {row[k]['device_ms']['median'] * 1e3:.1f} us ({row[k]['device_ms']['min'] * 1e3:.1f} .. {row[k]['device_ms']['max'] * 1e3:.1f}; "
                f"x{row[k]['ratio_to_baseline']:.3f})" for k in labels), flush=True)
    # the outputs: code 0 is today's entry point, and every entry point (the _sym ones with random codes) is the parent's, byte for byte
    idx, mixed = rng.integers(0, n, size=4096), rng.integers(0, 4, size=4096).astype(np.int32)
    same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))  # noqa: E731  (applied, where only one has it, is left out)
    out["entry_points_equal_to_parent"] = []
    for name in SAMPLERS:
        f = lambda b, m, **kw: b.batch_merged(m, idx, **kw) if name == "batch_merged" else getattr(b, name)(idx, **kw)  # noqa: E731
        plain, zero = f(buf, merged), f(buf, merged, sym=np.zeros(4096, np.int32))
        assert same(plain, zero), name
        if old is not None:
            assert same(plain, f(old, old_merged)), name
            out["entry_points_equal_to_parent"].append(name)
            if old.has_sym:
                assert same(f(buf, merged, sym=mixed), f(old, old_merged, sym=mixed)), f"{name}, sym"
                out["entry_points_equal_to_parent"].append(f"{name}, sym")
    out["outputs_equal"] = True

    # consistency: how differently a net scores a position and its twin
    sample = rng.choice(n, size=min(n, 32768), replace=False)
    nets = {"random init": make_net(a.blocks, a.filters).train(False)}
    if a.checkpoint:
        nets[os.path.basename(a.checkpoint)] = M.build_net(M.load_state_dict(a.checkpoint), dev)
    if a.train_epochs:
        import tempfile

        from betaone_amd import train as T

        tmp = tempfile.mkdtemp()
        data, init = os.path.join(tmp, "data"), os.path.join(tmp, "init.pth")
        R.save_games(R.compact_path(data, 0), [R.pack_game(f) for f in sorted(fins, key=lambda f: f.game_id)], append=False)
        torch.save(make_net(a.blocks, a.filters).state_dict(), init)
        out["training"] = {}
        for mode in ("none", "both"):
            w, js = os.path.join(tmp, f"{mode}.pth"), os.path.join(tmp, f"{mode}.json")
            assert T.main(["--data-dir", data, "--save-dir", os.path.join(tmp, f"ck_{mode}"), "--init", init, "--epochs", str(a.train_epochs),
                           "--batch", "256", "--iteration", "0", "--candidate", w, "--augment", mode, "--holdout-fraction", "0.05", "--out", js]) == 0
            r = json.load(open(js))
            out["training"][mode] = dict(applied_codes=r["applied_codes"], epochs=[dict(loss=e["loss"], samples_per_s=e["samples_per_s"],
                                         val_policy_ce=e["validation"]["policy_ce"], val_value_mse_z=e["validation"]["value_mse_z"]) for e in r["epochs"]])
            nets[f"{a.train_epochs} epochs on the corpus, --augment {mode}"] = M.build_net(M.load_state_dict(w), dev)
    out["consistency"] = {}
    for label, model in nets.items():
        rows = [V.symmetry_consistency(model, buf, sample[free[sample]] if t & 2 else sample, t, 1024, False) for t in (1, 2, 3)]
        out["consistency"][label] = rows
        print(f"[symmetry_cost] {label}\n{V.format_consistency(rows)}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
