"""betaone_amd/validate.py -- held-out validation: what a net does on games it was not trained on, measured on the GPU.

The training stage reports the loss on the batches it has just fitted; the only other signal for a candidate is a full match.  This
module gives the cheap answer in between.  A deterministic split keeps whole games out of training (holdout_games; train
--holdout-fraction), and one pass over their records reports how often the policy's best move is the search's best move (top-1 / 3 / 5,
mean rank), the cross entropy and KL against the search's pi, the entropies and probability masses, and the value head's error, sign
accuracy and calibration -- overall and per bucket (game phase by the number of men, or the value's bin for a reliability table).

The per-row work and the sums are two HIP kernels (csrc/bo_metrics.h, bo_train_metrics): a record per row from one read of its 4672
logits, then the rows of every bucket added in float64 into an accumulator that stays on the device.  A pass makes one device -> host
copy, at its end.

    acc = MetricsAccumulator(n_buckets=3, device="cuda:0")
    acc.add(logits, value, pi_idx, pi_val, z, bucket=phase_bucket(states))         # per batch; nothing comes back
    report = acc.result()                                                           # {"overall": {...}, "buckets": [{...}, ...]}

    python -m betaone_amd.train --holdout-fraction 0.05 ...                         # "validation" per epoch in --out
    python -m betaone_amd.validate --model cand.pth --compare best.pth data/iter_7 data/iter_8 --holdout-fraction 0.05 --buckets phase
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as E
from . import records as R
from .train import batch_args, check_batch

CURRENT_PIECE_PLANES = slice(98, 110)  # utils.encode_board: 8 history blocks of 12 piece + 2 repetition planes, the current position last
CALIBRATION_BINS = 10
_M64 = (1 << 64) - 1


# ---- the split -----------------------------------------------------------------------------------------------------------------

def splitmix64(x: int) -> int:
    """One step of splitmix64 (Steele, Lea, Flood 2014): the output for the state x + the golden-ratio increment."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def holdout_hash(iteration: int, game_id: int, seed: int) -> int:
    """64 bits from (iteration, game_id, seed) alone: three chained splitmix64 steps."""
    h = splitmix64(int(seed) & _M64)
    h = splitmix64(h ^ (int(iteration) & _M64))
    return splitmix64(h ^ (int(game_id) & _M64))


def is_held_out(iteration: int, game_id: int, fraction: float, seed: int) -> bool:
    return holdout_hash(iteration, game_id, seed) < int(float(fraction) * 2.0 ** 64)


def holdout_games(games: Sequence[dict], fraction: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(train_index, held_index): the record indices, in a GpuReplayBuffer that got `games` in this order, of the games that train and of
    the games that are held out.  A game (a dict of records.load_games with its "iteration" beside "game_id") is held out iff
    holdout_hash(iteration, game_id, seed) < fraction * 2^64: that depends on nothing else, so a game stays on its side whatever the
    order of the files, whichever other games are there, and when the window of iterations moves.  Games without plies have no
    records, as in the buffer."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"holdout_games: fraction {fraction} is not in [0, 1]")
    train, held, at = [], [], 0
    for g in games:
        n = int(g["n_plies"])
        if n <= 0:
            continue
        (held if is_held_out(int(g.get("iteration", 0)), int(g["game_id"]), fraction, seed) else train).append(np.arange(at, at + n, dtype=np.int64))
        at += n
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)  # noqa: E731
    return cat(train), cat(held)


def held_out_game_count(games: Sequence[dict], fraction: float, seed: int) -> int:
    return sum(1 for g in games if int(g["n_plies"]) > 0 and is_held_out(int(g.get("iteration", 0)), int(g["game_id"]), fraction, seed))


# ---- the accumulator -------------------------------------------------------------------------------------------------------------

def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0


def _mean(total: float, count: float) -> Optional[float]:
    return float(total) / float(count) if count > 0 else None


def summarise(a: np.ndarray, with_q: bool) -> Dict:
    """The report of one row of bo_train_metrics' accumulator (float64 [BO_METRIC_COLS])."""
    M = E.METRIC
    n, pol, dec = float(a[M["N_ROWS"]]), float(a[M["N_POLICY_ROWS"]]), float(a[M["N_DECISIVE"]])
    ce, te = _mean(a[M["SUM_CE"]], pol), _mean(a[M["SUM_TARGET_ENTROPY"]], pol)
    return {
        "records": int(n), "bad_rows": int(a[M["N_BAD"]]), "policy_records": int(pol), "decisive_records": int(dec),
        "policy_top1": _mean(a[M["SUM_TOP1"]], pol), "policy_top3": _mean(a[M["SUM_TOP3"]], pol), "policy_top5": _mean(a[M["SUM_TOP5"]], pol),
        "mean_rank": _mean(a[M["SUM_RANK"]], pol), "argmax_in_support": _mean(a[M["SUM_ARGMAX_IN_SUPPORT"]], pol),
        "policy_ce": ce, "policy_kl": None if ce is None else ce - te, "net_entropy": _mean(a[M["SUM_NET_ENTROPY"]], pol),
        "p_top": _mean(a[M["SUM_P_TOP"]], pol), "p_support": _mean(a[M["SUM_P_SUPPORT"]], pol),
        "value_mse_z": _mean(a[M["SUM_SE_Z"]], n), "value_mse_q": _mean(a[M["SUM_SE_Q"]], n) if with_q else None,
        "value_sign_accuracy": _mean(a[M["SUM_SIGN_OK"]], dec), "mean_abs_value": _mean(a[M["SUM_ABS_V"]], n),
        "mean_value": _mean(a[M["SUM_V"]], n), "mean_outcome": _mean(a[M["SUM_Z"]], n),
    }


class MetricsAccumulator:
    """The float64 accumulator [n_buckets][BO_METRIC_COLS] of bo_train_metrics, on the device.  add() enqueues the two kernels on the
    current stream and returns nothing; result() is the pass's only device -> host copy."""

    def __init__(self, n_buckets: int = 1, device="cuda:0"):
        if int(n_buckets) < 1:
            raise ValueError("MetricsAccumulator: n_buckets >= 1")
        self.lib = E.load_hip_library()
        self.device = E.runtime_device(device)
        self.n_buckets = int(n_buckets)
        self.accum = torch.zeros((self.n_buckets, E.METRIC_COLS), dtype=torch.float64, device=self.device)
        self.with_q = False
        self.rows: Optional[torch.Tensor] = None  # the last batch's per-row records [n, BO_METRIC_ROW_COLS]

    def reset(self):
        self.accum.zero_()
        self.with_q = False

    def add(self, logits, value, pi_idx, pi_val, z, q=None, bucket=None):
        """One batch: logits [n,4672] and value [n] or [n,1] (float32, float16 or bfloat16, each its own), pi_idx [n,W] int32,
        pi_val [n,W], z [n] or [n,1] and q (optional) float32, bucket (optional) [n] int32 -- all on the accumulator's device."""
        *batch, q, bucket = check_batch("metrics", logits, value, pi_idx, pi_val, z, (("q", q, torch.float32, None), ("bucket", bucket, torch.int32, None)),
                                        device=self.accum.device, device_name="the accumulator's device")
        rows = torch.empty((pi_idx.shape[0], E.METRIC_ROW_COLS), dtype=torch.float32, device=self.accum.device)
        rc = self.lib.bo_train_metrics(*batch_args(*batch), q.data_ptr() if q is not None else None,
                                       bucket.data_ptr() if bucket is not None else None, self.n_buckets, rows.data_ptr(),
                                       self.accum.data_ptr(), _stream(logits))
        if rc != 0:
            raise E.EngineError(f"metrics: {self.lib.bo_last_error().decode()}")
        self.with_q = self.with_q or q is not None
        self.rows = rows

    def sums(self) -> np.ndarray:
        """The accumulator on the host, float64 [n_buckets][BO_METRIC_COLS] (synchronises)."""
        return self.accum.cpu().numpy()

    def result(self) -> Dict:
        a = self.sums()
        return {"overall": summarise(a.sum(0), self.with_q), "buckets": [summarise(a[k], self.with_q) for k in range(self.n_buckets)]}


# ---- bucket keys (torch on the batch that is on the device already) -----------------------------------------------------------------

def phase_bucket(states: torch.Tensor, edges: Sequence[int] = (10, 20)) -> torch.Tensor:
    """The game's phase by the number of men on the board: bucket k = the number of edges below the count, so (10, 20) gives
    <= 10 / 11-20 / 21-32.  The men are the sum of the current position's 12 piece planes."""
    men = states[:, CURRENT_PIECE_PLANES].sum(dim=(1, 2, 3))
    e = torch.tensor([float(x) for x in edges], dtype=men.dtype, device=men.device)
    return (men[:, None] > e[None, :]).sum(1).to(torch.int32)


def calibration_bucket(value: torch.Tensor) -> torch.Tensor:
    """The value's bin of ten over [-1, 1]: min(9, floor((v + 1) 5)).  Per bin, mean_value against mean_outcome is the reliability
    table."""
    v = torch.nan_to_num(value.detach().reshape(-1).float(), nan=0.0)
    return torch.clamp(torch.floor((v + 1.0) * 5.0), 0, CALIBRATION_BINS - 1).to(torch.int32)


def bucket_labels(buckets: Optional[str], edges: Sequence[int] = (10, 20)) -> List[str]:
    if buckets is None:
        return ["all"]
    if buckets == "phase":
        e = [int(x) for x in edges]
        return [f"<={e[0]} men"] + [f"{a + 1}-{b} men" for a, b in zip(e[:-1], e[1:])] + [f">{e[-1]} men"]
    if buckets == "calibration":
        return [f"v in [{-1 + 0.2 * k:+.1f}, {-1 + 0.2 * (k + 1):+.1f}{']' if k == CALIBRATION_BINS - 1 else ')'}" for k in range(CALIBRATION_BINS)]
    raise ValueError(f"buckets {buckets!r}: phase or calibration")


def evaluate(model, buf: R.GpuReplayBuffer, record_index, *, batch: int, amp: bool, buckets: Optional[str] = None, with_q: bool = False,
             edges: Sequence[int] = (10, 20), sym: Optional[int] = None) -> Dict:
    """One validation pass of `model` over the records `record_index` of `buf`, in index order, `batch` at a time (the last batch may be
    short): model.eval() under torch.no_grad() (and torch.autocast when amp), the metrics of every batch added on the device, one copy
    at the end.  buckets: None, "phase" (edges: the men counts that end a bucket) or "calibration".  The model's train / eval mode is
    restored.  Returns MetricsAccumulator.result() with "labels".
    sym (a transform code 1..3 of csrc/bo_sym.h; None: as the records are): every record is sampled under that board symmetry -- the net
    sees the twin position and is scored against the twin's targets, so the tables of two passes compare side by side.  A record with a
    castling right drops the mirror bit; the result gains "sym" and "applied_codes" (records per applied code)."""
    labels = bucket_labels(buckets, edges)
    index = np.ascontiguousarray(record_index, dtype=np.int64).reshape(-1)
    if index.size == 0:
        raise ValueError("evaluate: no records")
    acc = MetricsAccumulator(len(labels), buf.device)
    was_training = model.training
    model.eval()
    codes = torch.zeros(4, dtype=torch.int64, device=buf.device)
    try:
        with torch.no_grad():
            for i in range(0, index.size, int(batch)):
                part = index[i:i + int(batch)]
                if sym is None:
                    b = (buf.batch_sparse_q if with_q else buf.batch_sparse)(part)
                else:
                    b = (buf.batch_sparse_q if with_q else buf.batch_sparse)(part, sym=np.full(part.size, int(sym), dtype=np.int32))
                    codes += torch.bincount(b[-1].long(), minlength=4)[:4]
                states = b[0]
                with torch.autocast(states.device.type, enabled=amp):
                    logits, value = model(states)
                key = phase_bucket(states, edges) if buckets == "phase" else calibration_bucket(value) if buckets == "calibration" else None
                acc.add(logits, value, b[1], b[2], b[3], q=b[4] if with_q else None, bucket=key)
    finally:
        model.train(was_training)
    out = acc.result()
    out["labels"] = labels
    if sym is not None:
        out["sym"] = int(sym)
        out["applied_codes"] = {str(t): int(c) for t, c in enumerate(codes.cpu().tolist())}
    return out


def without_castling_rights(games: Sequence[dict]) -> np.ndarray:
    """Per record of the games in order (the buffer's record index space): True where the position has no castling right left, so the
    file mirror applies to it."""
    return np.array([int(g["positions"][i].castling) == 0 for g in games for i in range(int(g["n_plies"]))], dtype=bool)


def symmetry_consistency(model, buf: R.GpuReplayBuffer, record_index, t: int, batch: int, amp: bool) -> Dict:
    """How differently `model` scores a position x and its twin T x under the transform code t (csrc/bo_sym.h), over the records
    `record_index`: per record the net is run on the plain sample and on the transformed one, the twin's logits are gathered back into
    the original move indexing (symmetry.unmap_logits), and
        kl               mean KL(p(x) || p(T x) mapped back), both softmaxes and the sum in float64
        top1_agreement   the share of records whose best move is the same move
        value_abs_diff   mean |v(x) - v(T x)| (the value is the side to move's: a symmetric net gives 0)
    are taken over the records the code was applied to in full (a record with a castling right drops the mirror bit and is left out);
    "records" counts them.  An equivariant net gives 0, 1, 0."""
    from . import symmetry as S

    t = int(t)
    if t not in (1, 2, 3):
        raise ValueError(f"symmetry_consistency: transform code {t}: 1..3")
    index = np.ascontiguousarray(record_index, dtype=np.int64).reshape(-1)
    if index.size == 0:
        raise ValueError("symmetry_consistency: no records")
    sums = torch.zeros(4, dtype=torch.float64, device=buf.device)   # records, kl, agreements, |dv|
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i in range(0, index.size, int(batch)):
                part = index[i:i + int(batch)]
                x = buf.batch_sparse(part)[0]
                tx, _, _, _, applied = buf.batch_sparse(part, sym=np.full(part.size, t, dtype=np.int32))
                with torch.autocast(x.device.type, enabled=amp):
                    logits, value = model(x)
                    logits_t, value_t = model(tx)
                full = (applied == t).double()
                lp = torch.log_softmax(logits.double(), dim=1)
                back = S.unmap_logits(logits_t.double(), applied)
                lq = torch.log_softmax(back, dim=1)
                kl = (lp.exp() * (lp - lq)).sum(1)
                same = (logits.double().argmax(1) == back.argmax(1)).double()
                dv = (value.double().reshape(-1) - value_t.double().reshape(-1)).abs()
                sums += torch.stack([full.sum(), (kl * full).sum(), (same * full).sum(), (dv * full).sum()])
    finally:
        model.train(was_training)
    n, kl, same, dv = sums.cpu().tolist()
    return {"sym": t, "records": int(n), "kl": _mean(kl, n), "top1_agreement": _mean(same, n), "value_abs_diff": _mean(dv, n)}


SYMMETRY_NAMES = {1: "colour flip", 2: "file mirror", 3: "colour flip + file mirror"}


def format_consistency(rows: Sequence[Dict]) -> str:
    fmt = lambda x, f: "-" if x is None else format(x, f)  # noqa: E731
    lines = [f"{'consistency':<26} {'records':>9} {'kl':>12} {'top1 same':>10} {'|dv|':>10}"]
    for r in rows:
        lines.append(f"{SYMMETRY_NAMES[r['sym']]:<26} {r['records']:>9d} {fmt(r['kl'], '.6f'):>12} {fmt(r['top1_agreement'], '.4f'):>10} "
                     f"{fmt(r['value_abs_diff'], '.6f'):>10}")
    return "\n".join(lines)


# ---- the command ---------------------------------------------------------------------------------------------------------------

_COLUMNS = (("records", "records", "d"), ("policy_top1", "top1", ".4f"), ("policy_top3", "top3", ".4f"), ("policy_top5", "top5", ".4f"),
            ("mean_rank", "rank", ".2f"), ("policy_ce", "ce", ".4f"), ("policy_kl", "kl", ".4f"), ("net_entropy", "H(net)", ".4f"),
            ("p_top", "p_top", ".4f"), ("p_support", "p_supp", ".4f"), ("value_mse_z", "mse_z", ".4f"), ("value_sign_accuracy", "sign", ".4f"),
            ("mean_value", "mean_v", "+.4f"), ("mean_outcome", "mean_z", "+.4f"))


def format_table(report: Dict, signed: bool = False) -> str:
    """The report as text: one line per bucket (when there are several) and one for all records."""
    rows = ([(lab, r) for lab, r in zip(report["labels"], report["buckets"])] if len(report["buckets"]) > 1 else []) + [("all", report["overall"])]
    width = max(len(lab) for lab, _ in rows)
    lines = [" " * width + "".join(f" {head:>9}" for _, head, _ in _COLUMNS)]
    for lab, r in rows:
        cells = []
        for key, _, fmt in _COLUMNS:
            v = r.get(key)
            if signed and v is not None and not fmt.startswith("+") and key != "records":
                fmt = "+" + fmt
            cells.append(f" {'-':>9}" if v is None else f" {format(v, fmt):>9}")
        lines.append(f"{lab:<{width}}" + "".join(cells))
    return "\n".join(lines)


def difference(a: Dict, b: Dict) -> Dict:
    """b - a, key by key, over two reports of the same records (None where either side has no value; records stay a's)."""
    def one(x, y):
        return {k: (x[k] if k in ("records", "bad_rows", "policy_records", "decisive_records") else
                    None if x[k] is None or y[k] is None else y[k] - x[k]) for k in x}

    return {"overall": one(a["overall"], b["overall"]), "buckets": [one(x, y) for x, y in zip(a["buckets"], b["buckets"])], "labels": a["labels"]}


def iteration_dirs(paths: Sequence[str]) -> Dict[int, List[str]]:
    """{iteration: [compact files]} of DATA_DIR/iter_N directories."""
    found: Dict[int, List[str]] = {}
    for p in paths:
        m = re.search(r"iter_(\d+)$", os.path.normpath(p))
        if not m:
            raise SystemExit(f"validate: {p}: not a DATA_DIR/iter_N directory")
        files = sorted(glob.glob(os.path.join(p, f"games_rank*{R.COMPACT_SUFFIX}")))
        if not files:
            raise SystemExit(f"validate: {p} holds no compact records (games_rank*{R.COMPACT_SUFFIX})")
        found.setdefault(int(m.group(1)), []).extend(files)
    return found


def main(argv=None) -> int:
    from . import match as M
    from . import train as T

    ap = argparse.ArgumentParser(prog="python -m betaone_amd.validate", description=__doc__.split("\n\n")[0])
    ap.add_argument("dirs", nargs="+", metavar="DATA_DIR/iter_N", help="directories with compact records")
    ap.add_argument("--model", required=True, help="weights (state_dict); the net takes its shape from their keys, as with train --init")
    ap.add_argument("--compare", default=None, help="a second net, evaluated on the same records; the differences (compare - model) are printed")
    ap.add_argument("--holdout-fraction", type=float, default=None, metavar="F", help="evaluate the games that train --holdout-fraction F held out")
    ap.add_argument("--seed", type=int, default=0, help="the split's seed: train's --holdout-seed")
    ap.add_argument("--all", action="store_true", help="evaluate every record of the directories")
    ap.add_argument("--buckets", choices=("phase", "calibration"), default=None)
    ap.add_argument("--bucket-edges", default="10,20", help="phase: the men counts that end a bucket (default 10,20: <=10 / 11-20 / 21-32)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-amp", action="store_true", help="float32 forward")
    ap.add_argument("--with-q", action="store_true", help="also the value's error against the records' root values")
    ap.add_argument("--symmetry", choices=("colour", "mirror", "both"), default=None,
                    help="score the records once more under board symmetries (the colour flip, the file mirror, or each of the two and "
                         "their product) and print how consistently the net treats a position and its twin; the mirror runs over the "
                         "records without castling rights")
    ap.add_argument("--out", default=None, help="the report as JSON")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.all == (a.holdout_fraction is not None):
        ap.error("one of --all and --holdout-fraction F")
    edges = [int(x) for x in a.bucket_edges.split(",") if x.strip()]
    if not edges or sorted(set(edges)) != edges:
        ap.error(f"--bucket-edges {a.bucket_edges}: increasing men counts")
    log = lambda s: print(f"[validate] {s}", flush=True)  # noqa: E731

    dev = E.runtime_device(a.device)
    files = iteration_dirs(a.dirs)
    games = T.load_window_games(files)
    if a.all:
        index = np.arange(sum(int(g["n_plies"]) for g in games), dtype=np.int64)
        held_games = len(games)
    else:
        _, index = holdout_games(games, a.holdout_fraction, a.seed)
        held_games = held_out_game_count(games, a.holdout_fraction, a.seed)
        if index.size == 0:
            raise SystemExit(f"validate: --holdout-fraction {a.holdout_fraction} (seed {a.seed}) holds out none of the {len(games)} games")
    buf = T.load_buffer(files, dev, games=games)
    log(f"{index.size} records of {held_games} games (of {len(buf)} records, {len(games)} games, iterations {sorted(files)})")
    reports = {}
    for name, path in (("model", a.model), ("compare", a.compare)):
        if path is None:
            continue
        net = M.build_net(M.load_state_dict(path), dev)
        reports[name] = evaluate(net, buf, index, batch=a.batch, amp=not a.no_amp, buckets=a.buckets, with_q=a.with_q, edges=edges)
        log(f"{name}: {path}")
        print(format_table(reports[name]), flush=True)
        if a.symmetry:
            from . import symmetry as S

            free = without_castling_rights(games)
            sym_rep = {"passes": [], "consistency": []}
            for t in S.CODES[a.symmetry]:
                part = index[free[index]] if t & S.MIRROR else index
                if part.size == 0:
                    log(f"{name}: {SYMMETRY_NAMES[t]}: none of the {index.size} records is without castling rights")
                    continue
                rep = evaluate(net, buf, part, batch=a.batch, amp=not a.no_amp, buckets=a.buckets, with_q=a.with_q, edges=edges, sym=t)
                log(f"{name} under the {SYMMETRY_NAMES[t]}: {part.size} of {index.size} records")
                print(format_table(rep), flush=True)
                sym_rep["passes"].append(dict(rep, name=SYMMETRY_NAMES[t], records_scored=int(part.size)))
                sym_rep["consistency"].append(symmetry_consistency(net, buf, part, t, a.batch, not a.no_amp))
            if sym_rep["consistency"]:
                print(format_consistency(sym_rep["consistency"]), flush=True)
            reports[name]["symmetry"] = sym_rep
    buf.close()
    out = {"records": int(index.size), "games": held_games, "iterations": sorted(files), "holdout_fraction": a.holdout_fraction,
           "seed": a.seed, "buckets": a.buckets, "bucket_edges": edges, "batch": a.batch, "amp": not a.no_amp, "model_path": a.model,
           "compare_path": a.compare, **reports}
    if a.compare:
        out["difference"] = difference(reports["model"], reports["compare"])
        log("compare - model")
        print(format_table(out["difference"], signed=True), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
