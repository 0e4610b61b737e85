"""scripts/book_cost.py -- what grouping a corpus into an opening book costs on the MI355X.

    python scripts/book_cost.py --out profiles/book_cost.json

Plays --games self-play games (Dirichlet noise and temperature on: the games differ) with a random-init net, saves them as compact
records and exports them with pgn_write.  On the PGN's ring two work lists are timed: a DEEP window (most groups are one game) and a
HOT window that starts at ply 0 (nearly every game adds to the same few slots), each with and without the per-wave combining of
csrc/bo_book.h.  A call is timed with device events around the launch alone (the columns are reset outside the events), --reps times
after two warm-up calls.  The NumPy restatement below groups the same items on the host (np.unique over the 68 key bytes) and must
give the same table.  Last, the command end to end, --runs times, with its own split into parse, replay, insert, select and write."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)

F_KEY_MASK = 0x7F001F


def numpy_table(ring, it):
    """The table of bo_book_insert from the ring bytes on the host: {first: (n, w, d, l, n_eval, min_ply, sum_eval)}."""
    from betaone_amd import analyse as A

    e = it["entry"]
    d = ring.reshape(-1).view(A.DPOS_DTYPE)[e]
    key = np.zeros(len(e), np.dtype([("bb", "<u8", (8,)), ("f", "<u4")]))
    key["bb"], key["f"] = d["bb"], d["flags"] & F_KEY_MASK
    _, kid = np.unique(key.view(np.dtype((np.void, key.dtype.itemsize))), return_inverse=True)
    kid = kid.reshape(-1)
    # once per game: the first item of every (game, key) pair -- the items are game-major, ply-minor
    pair = it["game"] * (int(kid.max()) + 1) + kid
    _, keep = np.unique(pair, return_index=True)
    kid, e, ply, res, ev, white = kid[keep], e[keep], it["ply"][keep], it["result"][keep], it["eval"][keep], (d["flags"][keep] & 1) != 0
    G = int(kid.max()) + 1
    has = ~np.isnan(ev)
    q = np.rint(np.clip(np.where(has, ev, 0), -1, 1).astype(np.float32) * np.float32(2 ** 20)).astype(np.int64)
    q = np.where(white, q, -q) * has
    cols = [np.bincount(kid, minlength=G)] + [np.bincount(kid, weights=(res == r), minlength=G).astype(np.int64) for r in (1, 2, 3)]
    cols.append(np.bincount(kid, weights=has, minlength=G).astype(np.int64))
    mp, first, s = np.full(G, 2 ** 31 - 1, np.int64), np.full(G, 2 ** 63 - 1, np.int64), np.zeros(G, np.int64)
    np.minimum.at(mp, kid, ply)
    np.minimum.at(first, kid, e)
    np.add.at(s, kid, q)
    return {int(first[g]): (int(cols[0][g]), int(cols[1][g]), int(cols[2][g]), int(cols[3][g]), int(cols[4][g]), int(mp[g]), int(s[g])) for g in range(G)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=16384)
    ap.add_argument("--moves", type=int, default=32)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=32)
    ap.add_argument("--mcts-batch", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--deep", type=int, nargs=2, default=(16, 27))
    ap.add_argument("--hot", type=int, nargs=2, default=(0, 11))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from analyse_cost import make_net
    from betaone_amd import book as B
    from betaone_amd import pgn_write as W
    from betaone_amd import records as R
    from betaone_amd.nn_tune import best_inference_copy
    from betaone_amd.rollout import Rollout

    dev = torch.device("cuda:0")
    net = make_net(a.blocks, a.filters)
    tmp = tempfile.mkdtemp(prefix="book_cost_")
    bog = os.path.join(tmp, "data", "iter_1", "games_rank0.bog")
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
    R.save_games(bog, sorted(fins, key=lambda f: f.game_id))
    t_play = time.perf_counter() - t0
    pgn = os.path.join(tmp, "games.pgn")
    assert W.main([bog, "-o", pgn, "--date", "2026.10.19", "--sims", str(a.sims)]) == 0
    print(f"[book_cost] {a.games} games played in {t_play:.1f} s, PGN {os.path.getsize(pgn)} B", flush=True)

    c = B.Corpus([pgn], "cuda:0")
    lib = c.lib
    ring = c.pos.cpu().numpy().reshape(-1, 80)
    out = dict(settings=vars(a), play_seconds=t_play, games=int(c.n_games), positions=int(c.capacity), pgn_bytes=os.path.getsize(pgn), windows={})
    for name, (lo, hi) in (("deep", a.deep), ("hot", a.hot)):
        it = c.items(lo, hi)
        n = len(it["entry"])
        d = {k: torch.from_numpy(np.ascontiguousarray(it[k])).to(dev) for k in ("entry", "ply", "result", "back")}
        ev = c.ev[d["entry"]]
        it["eval"] = ev.cpu().numpy()
        T = B.next_pow2(2 * n)
        gid, res = torch.zeros(n, dtype=torch.int32, device=dev), {}
        tables = {}
        for label, flags in (("combine", 0), ("no_combine", B.NO_COMBINE)):
            us = []
            for r in range(a.reps + 2):
                cols = {nm: torch.full((T,), fill, dtype=dt, device=dev) for nm, dt, fill in B.COLUMNS}
                status = torch.zeros(2, dtype=torch.int32, device=dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                rc = lib.bo_book_insert(c.pos.data_ptr(), c.capacity, n, d["entry"].data_ptr(), d["ply"].data_ptr(), d["result"].data_ptr(), ev.data_ptr(),
                                        d["back"].data_ptr(), T, *[cols[nm].data_ptr() for nm, _, _ in B.COLUMNS], gid.data_ptr(), status.data_ptr(), flags,
                                        torch.cuda.current_stream().cuda_stream)
                e1.record()
                torch.cuda.synchronize()
                assert rc == 0 and status.cpu().tolist() == [0, 0]
                if r >= 2:
                    us.append(e0.elapsed_time(e1) * 1e3)
            us = np.array(us)
            occ = torch.nonzero(cols["owner"] >= 0).flatten()
            h = {nm: cols[nm][occ].cpu().numpy() for nm, _, _ in B.COLUMNS}
            tables[label] = {int(h["first"][i]): tuple(int(h[k][i]) for k in ("n", "w", "d", "l", "n_eval", "min_ply", "sum_eval")) for i in range(len(occ))}
            res[label] = dict(us_median=float(np.median(us)), us_min=float(us.min()), us_max=float(us.max()), items_per_second=float(n / (np.median(us) * 1e-6)))
        t_np = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = numpy_table(ring, it)
            t_np.append(time.perf_counter() - t0)
        assert tables["combine"] == tables["no_combine"] == want
        sizes = np.array([v[0] for v in want.values()])
        out["windows"][name] = dict(window=[lo, hi], items=n, table_slots=T, groups=len(want), singleton_share=float((sizes == 1).mean()),
                                    largest_group=int(sizes.max()), insert=res, numpy_seconds=t_np, equal_to_numpy=True)
        print(f"[book_cost] {name}: {json.dumps(out['windows'][name])}", flush=True)
    del c
    runs = []
    for i in range(a.runs):
        t0 = time.perf_counter()
        rep = B.build_book([pgn], os.path.join(tmp, f"book{i}.txt"), min_ply=8, max_ply=16, min_games=10, max_bias=0.1, json_path=os.path.join(tmp, f"book{i}.json"))
        runs.append(dict(seconds=rep["seconds"], total=time.perf_counter() - t0, items=rep["items"], groups=rep["groups"], qualifying=rep["qualifying"],
                         kept=rep["kept"]))
    out["command"] = runs
    out["books_identical"] = all(open(os.path.join(tmp, f"book{i}.txt")).read() == open(os.path.join(tmp, "book0.txt")).read() for i in range(a.runs))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
