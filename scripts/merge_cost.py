"""scripts/merge_cost.py -- what merging the targets of duplicate positions costs on the MI355X, and what it finds.

    python scripts/merge_cost.py --out profiles/merge_cost.json

Plays --games self-play games (Dirichlet noise and temperature on: the games differ) with a random-init net -- the corpus recipe of
scripts/book_cost.py -- and adds them to a GpuReplayBuffer.  GpuReplayBuffer.merge_duplicates is called --reps times after two warm-up
calls; the library times bo_k_replay_group and the two launches of bo_k_replay_merge with device events of their own, apart from each
other.  The largest group is merged once more alone (index = its members) for its share of the merge time.  The NumPy restatement
groups the same records on the host the way the tests do -- the state rows of buf.batch by their bytes (hashed per row, so the 16 GB
of planes pass through in chunks) -- and averages with np.add.at in float64; it must give the same partition and the same values within
one float32 ulp.  Then batch_merged against batch_sparse_q at two batch sizes, and from the host's float64 means the variance of the
per-record z and pi around their group means: the quantity the feature removes."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)


def numpy_groups(buf, chunk=4096):
    """Representative (lowest record index) of every record's group: equal state rows, by a 16-byte hash of the row's bytes."""
    n = len(buf)
    h = np.empty((n, 2), dtype=np.uint64)
    for a in range(0, n, chunk):
        s = buf.batch(np.arange(a, min(n, a + chunk)))[0].cpu().numpy().reshape(-1, 120 * 64)
        for i, row in enumerate(s):
            h[a + i] = np.frombuffer(hashlib.blake2b(row.tobytes(), digest_size=16).digest(), dtype=np.uint64)
    _, first, inv = np.unique(h.view(np.dtype((np.void, 16))).reshape(-1), return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


def numpy_means(rep, pi_idx, pi_val, z, q):
    """Per group (ascending representative): count, float64 means of z and q, and the mean pi as {(group, action): value} arrays."""
    reps, gid, cnt = np.unique(rep, return_inverse=True, return_counts=True)
    gid = gid.reshape(-1)
    G = reps.size
    zs, qs = np.zeros(G), np.zeros(G)
    np.add.at(zs, gid, z.astype(np.float64))
    np.add.at(qs, gid, q.astype(np.float64))
    used = pi_idx >= 0
    cell = (gid[:, None] * 4672 + pi_idx)[used]
    cells, ci = np.unique(cell, return_inverse=True)
    sums = np.zeros(cells.size)
    np.add.at(sums, ci.reshape(-1), pi_val[used].astype(np.float64))
    return reps, gid, cnt, zs / cnt, qs / cnt, cells, sums / cnt[cells // 4672]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=16384)
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=32)
    ap.add_argument("--mcts-batch", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=(256, 4096))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from analyse_cost import make_net
    from betaone_amd import records as R
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
    t_play = time.perf_counter() - t0
    width = max(2, max(len(ix) for g in games for ix, _ in g["pis"]))
    buf = R.GpuReplayBuffer(sum(int(g["n_plies"]) + 1 for g in games) + 64, device="cuda:0", pi_width=width)
    assert buf.add(games) == 0
    n = len(buf)
    print(f"[merge_cost] {a.games} games played in {t_play:.1f} s: {n} records, pi_width {width}", flush=True)
    out = dict(settings=vars(a), play_seconds=t_play, records=n, pi_width=width, keys={})

    everything = np.arange(n)
    for key in ("input", "position"):
        g_ms, m_ms, wall = [], [], []
        for r in range(a.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = buf.merge_duplicates(key=key)
            dt = time.perf_counter() - t0
            if r >= 2:
                g_ms.append(m.group_ms)
                m_ms.append(m.merge_ms)
                wall.append(dt)
            if r < a.reps + 1:
                m.close()
        rep = m.report()
        big = int(m.representatives[int(np.argmax(m.counts))])
        members = everything[m.representative_of(everything) == big]
        alone = []
        for _ in range(5):
            one = buf.merge_duplicates(index=members, key=key)
            assert one.n_groups == 1
            alone.append(one.merge_ms)
            one.close()
        stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))  # noqa: E731
        out["keys"][key] = dict(report=rep, table_slots=m.table_slots, group_ms=stat(g_ms), merge_ms=stat(m_ms), create_wall_s=stat(wall),
                                largest_group_alone_merge_ms=stat(alone), largest_group_share=float(np.median(alone) / np.median(m_ms)))
        print(f"[merge_cost] {key}: {json.dumps(out['keys'][key])}", flush=True)
        if key == "input":
            merged = m
        else:
            m.close()

    # the restatement, and the variance the means remove
    cols = [[], [], [], []]
    for lo in range(0, n, 65536):
        for c, t in zip(cols, buf.batch_sparse_q(everything[lo:lo + 65536])[1:]):
            c.append(t.cpu().numpy())
    pi_idx, pi_val, z, q = (np.concatenate(c) for c in cols)
    z, q = z.reshape(-1), q.reshape(-1)
    t0 = time.perf_counter()
    rep_np = numpy_groups(buf)
    t_group = time.perf_counter() - t0
    t0 = time.perf_counter()
    reps, gid, cnt, zm, qm, cells, pm = numpy_means(rep_np, pi_idx, pi_val, z, q)
    t_mean = time.perf_counter() - t0
    assert np.array_equal(rep_np, merged.representative_of(everything)) and np.array_equal(reps, merged.representatives)
    worst = 0.0
    for lo in range(0, reps.size, 65536):
        _, gi, gv, gz, gq = (t.cpu().numpy() for t in buf.batch_merged(merged, reps[lo:lo + 65536]))
        for got, want in ((gz.reshape(-1), zm[lo:lo + 65536]), (gq.reshape(-1), qm[lo:lo + 65536])):
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))))
        used = gi >= 0
        cell = ((np.arange(lo, lo + gi.shape[0])[:, None]) * 4672 + gi)[used]
        at = np.searchsorted(cells, cell)
        assert np.array_equal(cells[at], cell) and int(used.sum()) == int(((cells // 4672 >= lo) & (cells // 4672 < lo + gi.shape[0])).sum())
        want = pm[at]
        worst = max(worst, float(np.max(np.abs(gv[used].astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64))))
    assert worst <= 1.0, worst
    multi = cnt[gid] > 1
    used = pi_idx >= 0
    ss_rec = float((pi_val.astype(np.float64) ** 2 * used).sum())
    ss_grp = float((pm ** 2 * cnt[cells // 4672]).sum())
    out["numpy"] = dict(group_seconds=t_group, mean_seconds=t_mean, equal_partition=True, worst_error_ulp=worst)
    out["variance"] = dict(z_all=float(np.mean((z - zm[gid]) ** 2)), z_in_groups=float(np.mean((z[multi] - zm[gid][multi]) ** 2)),
                           q_all=float(np.mean((q - qm[gid]) ** 2)), pi_all=(ss_rec - ss_grp) / n, z_total=float(np.var(z.astype(np.float64))),
                           records_in_groups=int(multi.sum()))
    print(f"[merge_cost] numpy {json.dumps(out['numpy'])} variance {json.dumps(out['variance'])}", flush=True)

    # the sampler
    rng = np.random.default_rng(0)
    out["sampler"] = {}
    for B in a.batches:
        res = {}
        for name, make in (("batch_sparse_q", buf.batch_sparse_q), ("batch_merged", lambda ix: buf.batch_merged(merged, ix))):
            us = []
            for r in range(a.reps + 2):
                ix = rng.integers(0, n, size=B)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                make(ix)
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    us.append((e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6))
            us = np.array(us)
            res[name] = dict(device_us_median=float(np.median(us[:, 0])), device_us_min=float(us[:, 0].min()), device_us_max=float(us[:, 0].max()),
                             wall_us_median=float(np.median(us[:, 1])), wall_us_min=float(us[:, 1].min()), wall_us_max=float(us[:, 1].max()))
        out["sampler"][str(B)] = dict(res, width=merged.width)
        print(f"[merge_cost] batch {B}: {json.dumps(out['sampler'][str(B)])}", flush=True)
    merged.close()
    buf.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
