"""tests/evaluate_batches.py -- TEST HELPER for tests/test_evaluate_batches_gpu.py: the persistent tower kernels' grid geometry (which
batches make a workgroup loop, and how often), distinct encoded positions from seeded random games, the rows to sample on each pass,
and the float64 reference of a net.  Its own CPU test: tests/test_evaluate_batches_cpu.py.

Grid geometry (csrc/bo_engine.cpp, tower_forward_impl): every tower kernel is persistent -- the grid is capped and a workgroup loops
over boards.  `tower_split`, `tower_wg`, `tower` at 128 filters: one board per workgroup, min(B, n_cu) workgroups; `tower` at 64
filters: two workgroups per CU, min(B, 2 n_cu); `tower_f16`: two boards per workgroup, min((B + 1) / 2, n_cu) workgroups
(bo_tower_h.h / bo_tower_h16.h: `pb += gridDim.x`).  The per-layer `mfma` route is given n_cu slots like the one-board routes."""
from __future__ import annotations

import random

import numpy as np

HEADS_F16_ABOVE = 1024  # fused_net.FusedPolicyValueNet.forward: behind the fp16 tower, bo_nn_heads up to 1024 rows, bo_nn_heads_f16 beyond


def slots(conv: str, filters: int, n_cu: int) -> int:
    """Workgroup slots of one pass over the grid: boards, or board PAIRS for conv='tower_f16'."""
    if conv == "tower" and filters == 64:
        return 2 * n_cu
    return n_cu


def boards_per_pass(conv: str, filters: int, n_cu: int) -> int:
    return 2 * slots(conv, filters, n_cu) if conv == "tower_f16" else slots(conv, filters, n_cu)


def passes(batch: int, per_pass: int) -> int:
    return -(-batch // per_pass)


def batch_list(conv: str, filters: int, n_cu: int) -> list:
    """Batches (boards) around and beyond the grid: S - 1, S, S + 1, 2S + 1, 3S + 37 slots for slot count S; for the fp16 tower the
    same counts of pairs, plus two odd batches whose lone tail board sits in a workgroup on a later pass (S + 1 and 3S + 37 pairs)."""
    s = slots(conv, filters, n_cu)
    counts = [s - 1, s, s + 1, 2 * s + 1, 3 * s + 37]
    if conv != "tower_f16":
        return counts
    return sorted({2 * p for p in counts} | {2 * (s + 1) - 1, 2 * (3 * s + 37) - 1})


def largest_batch(conv: str, filters: int, n_cu: int) -> int:
    """The largest multi-pass batch of batch_list (odd for the fp16 tower: its tail board is alone in its pair)."""
    bl = batch_list(conv, filters, n_cu)
    if conv == "tower_f16":
        return max(b for b in bl if b % 2)
    return max(bl)


def sub_batch(batch: int, conv: str):
    """Rows [1, batch) -- every board moves to another slot, and for the fp16 tower to another partner -- or None where that would
    put the fp16 tower's heads on the other side of their switch (the logits would come from the other heads kernel)."""
    if conv == "tower_f16" and (batch - 1 <= HEADS_F16_ABOVE) != (batch <= HEADS_F16_ABOVE):
        return None
    return slice(1, batch) if batch > 1 else None


def sample_rows(batch: int, conv: str, filters: int, n_cu: int, n_max: int = 64) -> list:
    """Rows to compare with the float64 net: the first and last row of every pass; for the fp16 tower at odd batches the lone tail
    board and the boards its workgroup held on earlier passes; then a strided sample up to n_max rows."""
    per = boards_per_pass(conv, filters, n_cu)
    rows = set()
    for k in range(passes(batch, per)):
        rows.add(k * per)
        rows.add(min((k + 1) * per, batch) - 1)
    if conv == "tower_f16" and batch % 2:
        tail = batch - 1
        wg = (tail // 2) % slots(conv, filters, n_cu)
        for pb in range(wg, tail // 2 + 1, slots(conv, filters, n_cu)):
            rows.update(r for r in (2 * pb, 2 * pb + 1) if r < batch)
    rows = sorted(rows)
    assert len(rows) <= n_max, (batch, len(rows))
    left = n_max - len(rows)
    if left > 0:
        step = max(1, batch // left)
        for r in range(step // 2, batch, step):
            if len(rows) >= n_max:
                break
            if r not in rows:
                rows.append(r)
    return sorted(set(rows))[:n_max]


def pass_of(row: int, conv: str, filters: int, n_cu: int) -> int:
    return row // boards_per_pass(conv, filters, n_cu)


def random_positions(n: int, seed: int = 0, max_plies: int = 80) -> np.ndarray:
    """n encoded positions [n, 120, 8, 8] float32, every ply of seeded random games (tests/pgn_util.random_game), through
    oracle.encode_board with the game's history and a repetition tracker fed ply by ply (the history and repetition planes are filled)."""
    import pgn_util
    from oracle import oracle as O

    rng = random.Random(seed)
    out, seen = [], set()
    while len(out) < n:
        moves = pgn_util.random_game(rng, max_plies=max_plies)[0]
        b = O.Board(O.STARTING_FEN)
        trk = O.PyTracker()
        trk.add_board(b)
        for m in moves:
            b.push(m)
            trk.add_board(b)
            planes = O.encode_board(b.positions(), trk)
            key = planes.tobytes()
            if key not in seen:
                seen.add(key)
                out.append(planes)
            if len(out) == n:
                break
    return np.stack(out)


def make_rows(bases, n: int, seed: int = 0):
    """n input rows (torch, on the bases' device): base position i % len(bases) times a per-row factor in [0.5, 1) that no other row
    has (a seeded permutation of n levels), so no two rows are equal and neighbouring rows are not near copies of each other."""
    import torch

    g = torch.Generator().manual_seed(seed)
    f = 0.5 + 0.5 * torch.randperm(n, generator=g).double() / n
    idx = torch.arange(n) % bases.shape[0]
    return (bases[idx.to(bases.device)] * f.float().to(bases.device)[:, None, None, None]).contiguous()


def assert_rows_distinct(x, chunk: int = 4096):
    """Rows of x pairwise distinct: their (sum, dot product with a fixed random vector) keys, in float64, are (distinct keys imply
    distinct rows)."""
    import torch

    n = x.shape[0]
    flat = x.reshape(n, -1)
    r = torch.randn(flat.shape[1], generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(x.device)
    keys = []
    for i in range(0, n, chunk):
        blk = flat[i:i + chunk].double()
        keys.append(torch.stack([blk.sum(1), blk @ r], 1))
    keys = torch.cat(keys)
    assert torch.unique(keys, dim=0).shape[0] == n, "input rows are not pairwise distinct"


def reference64(net, x):
    """(logits, value) of the same net in float64 on the CPU (eval mode, unfused BatchNorm) for the rows x."""
    import copy

    import torch

    ref = copy.deepcopy(net).to("cpu").double().eval()
    with torch.no_grad():
        l, v = ref(x.detach().to("cpu").double())
    return l, v.reshape(-1, 1)


def row_errors(logits, value, l64, v64):
    """Per-row max |difference| over the logits and the value, in float64 on the CPU."""
    dl = (logits.detach().to("cpu").double() - l64).abs().amax(1)
    dv = (value.detach().to("cpu").double().reshape(-1, 1) - v64).abs().amax(1)
    return (dl.maximum(dv)).numpy()
