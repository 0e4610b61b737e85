"""tests/metrics_cases.py -- TEST HELPER for tests/test_validate_emu.py (wave emulator) and tests/test_validate_gpu.py (MI355X): the
validation metrics kernels of csrc/bo_metrics.h (bo_train_metrics) against a float64 reference, in the manner of tests/loss_cases.py.

reference64   every column of the per-row record and of the per-bucket sums in float64 (numpy), written out from the definitions in the
              header of bo_metrics.h; no call into the library.  Inputs are the STORED values: fp16 / bf16 logits and values are
              widened exactly.
envelope      what a float32 implementation may differ from it by, per row and column, derived from the formats (below), not measured.
cases         a seeded list over n in {1, 64, 65, 130} x W in {1, 2, 64, 65} with n_buckets in {1, 3, 65}; dropout_cases: a NaN, a
              +inf, a -inf logit and a NaN value in one row of a batch of 7.
check_*       the conditions; raw_metrics drives the library (torch tensors on "cpu" under the emulator, on "cuda:0" on the GPU).

Rows of a case follow seven patterns in turn (the case's number shifts the turn, so the cases with n = 1 differ): random entries (in
every other such row the top entry gets the logit maximum); entries
and the logit maximum on the corners of the lane / register layout (actions 0, 63, 64, 4607, 4608, 4671); two equal pi_val maxima (the
lowest action is i*, whichever slot it is in); logits equal to x[i*] on both sides of i* and some above it; a row of equal logits
(rank == i*); a repeated logit maximum (argmax is the lowest action); a row with nothing but invalid entries (-1, 4672, INT_MIN).  No
row has an action twice.

The envelope.  With mx = max_a x_a, ls = log sum_a exp(x_a - mx), d_a = (x_a - mx) - ls, p_a = exp(d_a), eps = 2^-23, the valid entries
e with t_e and i_e, S = sum_e t_e, and c = 0 for the kernels (loss_cases.TORCH_SUM_C for PyTorch's float32 path: its sum of the 4672
exponentials, see loss_cases):
  f_a = 4 + c + |x_a - mx| + |ls|    the relative error of p_a in eps, loss_cases' first factor: the half-ulp roundings of x - mx and of
                                     - ls scale the exponential, a few ulp for expf and logf, c for the row sum behind ls
  p_top           eps f_i* p_i* + 2^-126
  p_support       eps sum_e f_ie p_ie + eps/2 (ceil(W / 64) + 6) p_support + 2^-126: a lane adds ceil(W / 64) terms, the butterfly six
                  levels, every term >= 0
  ce              loss_cases' row term: eps (4 ce + (4 + c) S) + 2^-126 (the kernel's ce has to equal the loss kernel's bit for bit
                  anyway)
  target_entropy  eps (4 + (ceil(W / 64) + 6) / 2) sum_e |t_e log t_e| + 2^-126: logf to a few ulp and the product, relative to each
                  term, and the summation relative to the sum of the magnitudes
  net_entropy     eps sum_a p_a f_a (|d_a| + 1) + eps/2 (73 + 6) sum_a p_a |d_a| + 2^-126: a term p_a d_a has the relative error of
                  p_a, and d_a the absolute error of its two roundings and of ls, which f_a bounds as well; then 73 additions in a
                  lane and six butterfly levels, relative to the sum of the magnitudes (every term has one sign)
  se_z, se_q      eps 4 (v - t)^2 + 2^-126 (loss_cases' value term);  abs_v, z, v and every count: exact
  sums            the sum of the rows' allowances plus 2^-50 sum |row value|: the reduce adds float32 values in float64
A kernel output passes within loss_cases.FACTOR (4) envelopes; PyTorch's float32 computation of the same columns has to pass within ONE
(tests/test_validate_emu.py), which keeps the envelope honest."""
from __future__ import annotations

import functools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

import loss_cases as LC

A = LC.A
EPS, TINY = LC.EPS, LC.TINY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_NAMES = ("BAD", "HAS_POLICY", "DECISIVE", "RANK", "TOP1", "TOP3", "TOP5", "ARGMAX_IN_SUPPORT", "CE", "TARGET_ENTROPY", "NET_ENTROPY", "P_TOP",
             "P_SUPPORT", "SE_Z", "SE_Q", "ABS_V", "SIGN_OK", "Z", "V")
ROW = {name: k for k, name in enumerate(ROW_NAMES)}
ROW_COLS, COLS = len(ROW_NAMES), len(ROW_NAMES) + 1   # accum: N_ROWS, then the sum of every row column
EXACT = ("BAD", "HAS_POLICY", "DECISIVE", "RANK", "TOP1", "TOP3", "TOP5", "ARGMAX_IN_SUPPORT", "ABS_V", "SIGN_OK", "Z", "V")
FLOAT = ("CE", "TARGET_ENTROPY", "NET_ENTROPY", "P_TOP", "P_SUPPORT", "SE_Z", "SE_Q")
COUNT_SUMS = ("BAD", "HAS_POLICY", "DECISIVE", "RANK", "TOP1", "TOP3", "TOP5", "ARGMAX_IN_SUPPORT", "SIGN_OK")
INVALID = (-1, A, -2 ** 31)
INT_MAX = 2 ** 31 - 1


def header_enums():
    """(row names, accum names) of include/betaone_engine.h's BO_METRIC_ROW_* / BO_METRIC_* enums, in order."""
    text = open(os.path.join(ROOT, "include", "betaone_engine.h")).read()
    rows = re.search(r"enum \{\s*BO_METRIC_ROW_BAD = 0,(.*?)\};", text, re.S).group(0)
    acc = re.search(r"enum \{\s*BO_METRIC_N_ROWS = 0,(.*?)\};", text, re.S).group(0)
    return ([n[len("BO_METRIC_ROW_"):] for n in re.findall(r"BO_METRIC_ROW_\w+", rows)], [n[len("BO_METRIC_"):] for n in re.findall(r"BO_METRIC_\w+", acc)])


# ---- the float64 reference and its envelope ------------------------------------------------------------------------------------

def reference64(logits, value, idx, val, z, q=None, bucket=None, n_buckets=1, c=0.0):
    """rows [n, ROW_COLS] and accum [n_buckets, COLS] in float64, and their allowances env_rows / env_accum (module docstring)."""
    x = logits.detach().cpu().double().numpy()
    v = value.detach().cpu().double().numpy().reshape(-1)
    zz = z.detach().cpu().double().numpy().reshape(-1)
    qq = None if q is None else q.detach().cpu().double().numpy().reshape(-1)
    ix = idx.cpu().numpy().astype(np.int64)
    tv = val.cpu().double().numpy()
    n, W = ix.shape
    R, Eenv = np.zeros((n, ROW_COLS)), np.zeros((n, ROW_COLS))
    chunks = math.ceil(W / 64)
    for b in range(n):
        bad = (not np.isfinite(x[b]).all()) or np.isnan(v[b])
        R[b, ROW["BAD"]] = float(bad)
        if bad:
            continue
        ok = (ix[b] >= 0) & (ix[b] < A)
        ie, te = ix[b][ok], tv[b][ok]
        R[b, ROW["DECISIVE"]] = float(zz[b] != 0)
        R[b, ROW["SE_Z"]] = (v[b] - zz[b]) ** 2
        R[b, ROW["SE_Q"]] = 0.0 if qq is None else (v[b] - qq[b]) ** 2
        R[b, ROW["ABS_V"]] = abs(v[b])
        R[b, ROW["SIGN_OK"]] = float(zz[b] != 0 and v[b] * zz[b] > 0)
        R[b, ROW["Z"]], R[b, ROW["V"]] = zz[b], v[b]
        Eenv[b, ROW["SE_Z"]] = EPS * 4 * R[b, ROW["SE_Z"]] + TINY
        Eenv[b, ROW["SE_Q"]] = EPS * 4 * R[b, ROW["SE_Q"]] + TINY
        if ie.size == 0:
            continue
        mx = x[b].max()
        xm = x[b] - mx
        ls = math.log(np.exp(xm).sum())
        d = xm - ls
        p = np.exp(d)
        f = 4.0 + c + np.abs(xm) + abs(ls)
        best = te.max()
        istar = int(ie[te == best].min())          # ties: the lowest action
        xs = x[b, istar]
        rank = int((x[b] > xs).sum() + ((x[b] == xs) & (np.arange(A) < istar)).sum())
        ce = float(-(te * d[ie]).sum())
        pos = te > 0
        tlogt = te[pos] * np.log(te[pos])
        R[b, ROW["HAS_POLICY"]] = 1.0
        R[b, ROW["RANK"]] = rank
        R[b, ROW["TOP1"]], R[b, ROW["TOP3"]], R[b, ROW["TOP5"]] = float(rank < 1), float(rank < 3), float(rank < 5)
        R[b, ROW["ARGMAX_IN_SUPPORT"]] = float(int(np.argmax(x[b])) in set(ie.tolist()))
        R[b, ROW["CE"]] = ce
        R[b, ROW["TARGET_ENTROPY"]] = float(-tlogt.sum())
        R[b, ROW["NET_ENTROPY"]] = float(-(p[p > 0] * d[p > 0]).sum())
        R[b, ROW["P_TOP"]] = p[istar]
        R[b, ROW["P_SUPPORT"]] = float(p[ie].sum())
        Eenv[b, ROW["CE"]] = EPS * (4 * abs(ce) + (4 + c) * float(te.sum())) + TINY
        Eenv[b, ROW["TARGET_ENTROPY"]] = EPS * (4 + (chunks + 6) / 2) * float(np.abs(tlogt).sum()) + TINY
        Eenv[b, ROW["NET_ENTROPY"]] = EPS * float((p * f * (np.abs(d) + 1)).sum()) + 0.5 * EPS * (73 + 6) * float((p * np.abs(d)).sum()) + TINY
        Eenv[b, ROW["P_TOP"]] = EPS * f[istar] * p[istar] + TINY
        Eenv[b, ROW["P_SUPPORT"]] = EPS * float((f[ie] * p[ie]).sum()) + 0.5 * EPS * (chunks + 6) * float(p[ie].sum()) + TINY
    bk = np.zeros(n, dtype=np.int64) if bucket is None else bucket.cpu().numpy().astype(np.int64)
    acc, eacc = np.zeros((n_buckets, COLS)), np.zeros((n_buckets, COLS))
    for k in range(n_buckets):
        sel = bk == k
        acc[k, 0] = float((1.0 - R[sel, 0]).sum())
        acc[k, 1:] = R[sel].sum(0)
        eacc[k, 1:] = Eenv[sel].sum(0) + 2.0 ** -50 * np.abs(R[sel]).sum(0)
    return SimpleNamespace(rows=R, env_rows=Eenv, accum=acc, env_accum=eacc)


def torch32_rows(logits, value, idx, val, z, q=None):
    """PyTorch's own float32 computation of the float columns on the CPU (log_softmax, exp, sums), rows [n, ROW_COLS] float32; the exact
    columns are not its business and stay 0.  Rows that are bad or have no valid entry stay 0 in the policy columns."""
    x = logits.detach().cpu().float()
    v, zz = value.detach().cpu().float().reshape(-1), z.detach().cpu().float().reshape(-1)
    n = x.shape[0]
    out = torch.zeros((n, ROW_COLS), dtype=torch.float32)
    logp = torch.log_softmax(x, 1)
    p = torch.exp(logp)
    ne = -torch.where(p > 0, p * logp, torch.zeros(())).sum(1)
    ok = LC.valid(idx.cpu())
    ii = torch.where(ok, idx.cpu(), torch.zeros_like(idx.cpu())).long()
    t = torch.where(ok, val.cpu().float(), torch.zeros(()))
    ce = -(t * torch.gather(logp, 1, ii)).sum(1)
    ps = torch.where(ok, torch.gather(p, 1, ii), torch.zeros(())).sum(1)
    te = -torch.where(t > 0, t * torch.log(torch.where(t > 0, t, torch.ones(()))), torch.zeros(())).sum(1)
    for b in range(n):
        if not bool(torch.isfinite(x[b]).all()) or bool(torch.isnan(v[b])):
            continue
        out[b, ROW["SE_Z"]] = (v[b] - zz[b]) ** 2
        if q is not None:
            out[b, ROW["SE_Q"]] = (v[b] - q.detach().cpu().float().reshape(-1)[b]) ** 2
        if not bool(ok[b].any()):
            continue
        ie, tb = idx[b][ok[b]].long(), val[b][ok[b]]
        istar = int(ie[tb == tb.max()].min())
        out[b, ROW["CE"]], out[b, ROW["TARGET_ENTROPY"]], out[b, ROW["NET_ENTROPY"]] = ce[b], te[b], ne[b]
        out[b, ROW["P_TOP"]], out[b, ROW["P_SUPPORT"]] = p[b, istar], ps[b]
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def _distinct(g, m, keep=()):
    """m distinct actions that avoid `keep`."""
    pool = torch.randperm(A, generator=g)
    pool = pool[~torch.isin(pool, torch.tensor(list(keep), dtype=torch.long))] if keep else pool
    return pool[:m]


def make_case(name, n, W, seed, n_buckets=1, with_q=True, with_bucket=True, shift=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, A), generator=g) * 3.0
    value = torch.tanh(torch.randn((n, 1), generator=g))
    z = torch.randint(-1, 2, (n, 1), generator=g).float()
    for b, (v_, z_) in enumerate(((1.0, 1.0), (-1.0, 1.0), (0.0, -1.0), (0.5, 0.0))):
        if b < n:
            value[b, 0], z[b, 0] = v_, z_
    q = torch.tanh(torch.randn((n, 1), generator=g)) if with_q else None
    idx = torch.full((n, W), -1, dtype=torch.int32)
    val = torch.zeros((n, W))
    pattern = []
    edges = list(LC.EDGE_ACTIONS)
    for b in range(n):
        kind = (b + shift) % 7
        pattern.append(kind)
        m = int(torch.randint(1, W + 1, (1,), generator=g))
        acts = _distinct(g, m)
        vals = torch.rand(m, generator=g) + 0.05
        pos = torch.randperm(W, generator=g)[:m]   # entries anywhere in the row, gaps of -1 between them
        if kind == 0 and (b // 7) % 2 == 0:     # the net agrees with the search: the top entry is the logit maximum
            x[b, int(acts[int(vals.argmax())])] = x[b].max() + 1.0
        elif kind == 1:      # entries on the corners of the layout, the top entry and the logit maximum on two of them
            k = min(m, len(edges))
            rot = [edges[(b + e) % len(edges)] for e in range(k)]
            acts = torch.cat([torch.tensor(rot, dtype=torch.long), _distinct(g, m - k, keep=edges)])
            vals[0] = 2.0
            x[b, edges[(b + 3) % len(edges)]] = x[b].max() + 1.0
        elif kind == 2 and m >= 2:    # two equal pi_val maxima: the LOWER action is i*; put it in the later slot
            vals[0] = vals[1] = 2.0
            lo, hi = sorted((int(acts[0]), int(acts[1])))
            acts[0], acts[1] = hi, lo
            pos = torch.sort(pos)[0]
        elif kind == 3:    # logits equal to x[i*] below and above i*, and a few larger ones
            vals[0] = 2.0
            i0 = int(acts[0])
            x[b, i0] = 1.5
            others = _distinct(g, 9, keep=acts.tolist())
            x[b, others[:6]] = 1.5
            x[b, others[6:]] = 2.5
            for a in (i0 - 1, i0 + 1, i0 - 64, i0 + 64):
                if 0 <= a < A and a not in acts.tolist():
                    x[b, a] = 1.5
        elif kind == 4:    # every logit equal: rank == i*
            x[b] = 0.25
        elif kind == 5:    # the maximum three times: argmax is the lowest action; a target entry on the highest of them
            top = torch.sort(_distinct(g, 3, keep=acts.tolist()))[0]
            x[b, top] = x[b].max() + 2.0
            acts[0] = top[2]
        elif kind == 6:    # nothing but invalid entries
            acts = torch.tensor([INVALID[(b + e) % len(INVALID)] for e in range(m)], dtype=torch.long)
        vals = vals / vals.sum() * (0.97 if b % 2 else 1.0)
        idx[b, pos] = acts.int()
        val[b, pos] = vals.float()
    bucket = None
    if with_bucket:
        bucket = torch.randint(0, n_buckets, (n,), generator=g).int()
        if n > 2:
            bucket[n // 2], bucket[n - 1] = -1, n_buckets     # out of range: counted nowhere
    return SimpleNamespace(name=name, n=n, W=W, n_buckets=n_buckets, logits=x, value=value, idx=idx, val=val, z=z, q=q, bucket=bucket, pattern=pattern)


NS, WS, NBS = (1, 64, 65, 130), (1, 2, 64, 65), (1, 3, 65)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (n, W) in enumerate((n, W) for n in NS for W in WS):
        nb = NBS[(k + k // 4) % 3]
        out.append(make_case(f"n{n}_W{W}_nb{nb}", n, W, 5000 + k, n_buckets=nb, with_q=k % 2 == 0, with_bucket=not (nb == 1 and k % 3 == 0), shift=k))
    return tuple(out)


def pairs_case():
    """The shape that runs all nine (logits, value) dtype pairs."""
    return next(c for c in cases() if c.name.startswith("n65_W2_"))


def dropout_cases(row=2):
    """A NaN, a +inf and a -inf logit, and a NaN value, in row `row` of a batch of 7 (W = 4)."""
    out = []
    for k, label in enumerate(("nan_logit", "posinf_logit", "neginf_logit", "nan_value")):
        c = make_case(label, 7, 4, 6000 + k, n_buckets=1, with_q=True, with_bucket=False, shift=0)
        if label == "nan_value":
            c.value[row, 0] = float("nan")
        else:
            c.logits[row, 1234] = {"nan_logit": float("nan"), "posinf_logit": float("inf"), "neginf_logit": float("-inf")}[label]
        c.row = row
        out.append(c)
    return out


def cast(case, pair, device="cpu", rows=None):
    """(logits, value, idx, val, z, q, bucket) on `device`, logits / value stored as the dtype pair; rows: these rows only."""
    t = [case.logits.to(pair[0]), case.value.to(pair[1]), case.idx, case.val, case.z, case.q, case.bucket]
    if rows is not None:
        t = [None if a is None else a[rows] for a in t]
    return tuple(None if a is None else a.contiguous().to(device) for a in t)


# ---- driving the library -------------------------------------------------------------------------------------------------------

def guarded64(rows, cols, device, guard=4):
    """float64 [rows + guard, cols]: zeros, then guard rows of loss_cases.NAN32 in both halves of every word."""
    t = torch.empty((rows + guard, cols), dtype=torch.float64, device=device)
    t.view(torch.int32).fill_(LC.NAN32)
    t[:rows] = 0.0
    return t


def guard64_intact(t, rows) -> bool:
    return bool((t[rows:].view(torch.int32) == LC.NAN32).all())


def raw_metrics(logits, value, idx, val, z, q, bucket, n_buckets, accum=None, guard=8):
    """bo_train_metrics called directly with rows allocated `guard` rows longer than the batch, pre-filled with the NaN payload, and
    accum (a fresh guarded one unless given) -- returns (rows, accum) with their guard rows."""
    from betaone_amd import engine as E
    from betaone_amd.train import DTYPE_CODES

    lib = E.load_hip_library()
    dev = logits.device
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    n, W = idx.shape
    rows = LC.guarded(n, ROW_COLS, torch.float32, dev, guard)
    if accum is None:
        accum = guarded64(n_buckets, COLS, dev)
    rc = lib.bo_train_metrics(n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.reshape(-1).data_ptr(), DTYPE_CODES[value.dtype],
                              idx.data_ptr(), val.data_ptr(), z.reshape(-1).data_ptr(), q.reshape(-1).data_ptr() if q is not None else None,
                              bucket.data_ptr() if bucket is not None else None, n_buckets, rows.data_ptr(), accum.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return rows, accum


def loss_row_policy(logits, value, idx, val, z):
    """row_stats[:, 2] of bo_train_loss_forward on the same inputs."""
    from betaone_amd import engine as E
    from betaone_amd.train import DTYPE_CODES

    lib = E.load_hip_library()
    dev = logits.device
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    n, W = idx.shape
    st, l3 = torch.empty((n, LC.ROW_STATS), dtype=torch.float32, device=dev), torch.empty(3, dtype=torch.float32, device=dev)
    rc = lib.bo_train_loss_forward(n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.reshape(-1).data_ptr(), DTYPE_CODES[value.dtype],
                                   idx.data_ptr(), val.data_ptr(), z.reshape(-1).data_ptr(), st.data_ptr(), l3.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return st[:, 2].contiguous()


# ---- the conditions ------------------------------------------------------------------------------------------------------------

def check_rows(got, ref, what, factor=LC.FACTOR, exact=True):
    """rows [n, ROW_COLS] (float64 numpy) against a reference64 result: the exact columns equal, the float columns within `factor`
    envelopes.  Returns {column: worst error / envelope}."""
    worst = {}
    if exact:
        for name in EXACT:
            k = ROW[name]
            assert np.array_equal(got[:, k], ref.rows[:, k]), (f"{what}: column {name} differs in rows "
                                                               f"{np.nonzero(got[:, k] != ref.rows[:, k])[0][:8].tolist()}: "
                                                               f"{got[got[:, k] != ref.rows[:, k], k][:8]} != {ref.rows[got[:, k] != ref.rows[:, k], k][:8]}")
    for name in FLOAT:
        k = ROW[name]
        err, env = np.abs(got[:, k] - ref.rows[:, k]), ref.env_rows[:, k]
        zero = env == 0                           # rows that are bad / without policy: the column is 0 exactly
        assert np.array_equal(got[zero, k], ref.rows[zero, k]), f"{what}: column {name} is not 0 in a row that drops out"
        ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, env))
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        assert not (ratio > factor).any() and not np.isnan(got[:, k]).any(), (f"{what}: column {name} at {worst[name]:.3g} envelopes in row "
                                                                               f"{int(ratio.argmax())} ({got[int(ratio.argmax()), k]!r} "
                                                                               f"against {ref.rows[int(ratio.argmax()), k]!r})")
    return worst


def check_accum(got, ref, what, factor=LC.FACTOR):
    """accum [n_buckets, COLS] (float64 numpy): N_ROWS and the sums of the count columns exact, the float sums within the envelope."""
    assert np.array_equal(got[:, 0], ref.accum[:, 0]), f"{what}: N_ROWS {got[:, 0]} != {ref.accum[:, 0]}"
    for name in COUNT_SUMS:
        k = ROW[name] + 1
        assert np.array_equal(got[:, k], ref.accum[:, k]), f"{what}: the sum of {name} {got[:, k]} != {ref.accum[:, k]}"
    worst = 0.0
    for name in FLOAT + ("ABS_V", "Z", "V"):
        k = ROW[name] + 1
        err = np.abs(got[:, k] - ref.accum[:, k])
        allow = factor * ref.env_accum[:, k]
        assert (err <= allow).all(), f"{what}: the sum of {name} off by {err.max():.3g} (allowed {allow[err.argmax()]:.3g})"
        worst = max(worst, float((err / np.where(allow > 0, allow, 1.0)).max()))
    return worst


def golden_counts(accum):
    """The count columns of accum [n_buckets, COLS] as {name: [per bucket]} of ints (what tests/golden/validate_counts.json stores)."""
    out = {"N_ROWS": [int(v) for v in accum[:, 0]]}
    for name in COUNT_SUMS:
        out[name] = [int(v) for v in accum[:, ROW[name] + 1]]
        assert all(float(v) == float(int(v)) for v in accum[:, ROW[name] + 1])
    return out


def check_case(case, pair, device):
    """One case and dtype pair through bo_train_metrics: guards, every row written, the exact and the float columns, ce against the
    loss kernel bit for bit, the sums, and a second pass from a zeroed accumulator bit for bit."""
    t = cast(case, pair, device)
    what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])}"
    rows, accum = raw_metrics(*t, case.n_buckets)
    n = case.n
    assert LC.guard_intact(rows, n), f"{what}: rows written past row {n}"
    assert guard64_intact(accum, case.n_buckets), f"{what}: accum written past bucket {case.n_buckets}"
    assert not bool((rows[:n].view(torch.int32) == LC.NAN32).any()), f"{what}: rows has unwritten elements"
    ref = reference64(*t, n_buckets=case.n_buckets)
    got = rows[:n].cpu().double().numpy()
    worst = check_rows(got, ref, what)
    ce_loss = loss_row_policy(*t[:5])
    assert LC.same_bits(rows[:n, ROW["CE"]].contiguous(), ce_loss), f"{what}: ce differs from bo_train_loss_forward's row policy term"
    worst["sums"] = check_accum(accum[:case.n_buckets].cpu().numpy(), ref, what)
    rows2, accum2 = raw_metrics(*t, case.n_buckets)
    assert LC.same_bits(rows[:n], rows2[:n]) and bool(torch.equal(accum.view(torch.int32), accum2.view(torch.int32))), f"{what}: a second pass differs"
    return worst


def check_dropout(case, pair, device):
    """The bad row counts in N_BAD only, its record is 0 but for BAD, and the sums of the other six rows are those of the batch
    without it, bit for bit."""
    what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])}"
    t = cast(case, pair, device)
    rows, accum = raw_metrics(*t, 1)
    others = [b for b in range(case.n) if b != case.row]
    rows6, accum6 = raw_metrics(*cast(case, pair, device, rows=others), 1)
    r = rows[case.row].cpu().numpy()
    assert r[ROW["BAD"]] == 1.0 and not r[1:].any() and not np.signbit(r[1:]).any(), f"{what}: the bad row's record is {r}"
    a, a6 = accum[0].cpu().numpy(), accum6[0].cpu().numpy()
    assert a[ROW["BAD"] + 1] == 1.0 and a6[ROW["BAD"] + 1] == 0.0 and a[0] == 6.0 and a6[0] == 6.0, what
    keep = [k for k in range(COLS) if k != ROW["BAD"] + 1]
    assert np.array_equal(a[keep].view(np.uint64), a6[keep].view(np.uint64)), f"{what}: the other rows' sums changed: {a[keep] - a6[keep]}"
    assert LC.same_bits(rows[others].contiguous(), rows6[:6].contiguous()), f"{what}: the other rows' records changed"
    ref = reference64(*t)
    check_rows(rows[:case.n].cpu().double().numpy(), ref, what)
    check_accum(accum[:1].cpu().numpy(), ref, what)


def check_halves(case, pair, device):
    """MetricsAccumulator: two add() calls on the halves of a batch against one on the whole -- the counts exactly, the float sums
    within the envelope; result() of a bucket without rows has records 0 and None means."""
    from betaone_amd.validate import MetricsAccumulator

    what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} halves"
    t = cast(case, pair, device)
    whole, parts = MetricsAccumulator(case.n_buckets, device), MetricsAccumulator(case.n_buckets, device)
    whole.add(*t[:5], q=t[5], bucket=t[6])
    h = case.n // 2
    for rows in (slice(0, h), slice(h, case.n)):
        parts.add(*(a[rows] for a in t[:5]), q=None if t[5] is None else t[5][rows], bucket=None if t[6] is None else t[6][rows])
    a, b = whole.sums(), parts.sums()
    ref = reference64(*t, n_buckets=case.n_buckets)
    check_accum(a, ref, what + " (one call)")
    check_accum(b, ref, what + " (two calls)")
    for name in ("N_ROWS",) + COUNT_SUMS:
        k = 0 if name == "N_ROWS" else ROW[name] + 1
        assert np.array_equal(a[:, k], b[:, k]), f"{what}: {name} depends on the split"
    rep = parts.result()
    assert rep["overall"]["records"] == int(ref.accum[:, 0].sum())
    for k, bk in enumerate(rep["buckets"]):
        assert bk["records"] == int(ref.accum[k, 0])
        if bk["records"] == 0:
            assert bk["value_mse_z"] is None and bk["mean_abs_value"] is None
        if ref.accum[k, ROW["HAS_POLICY"] + 1] == 0:
            assert bk["policy_top1"] is None and bk["policy_ce"] is None and bk["policy_kl"] is None and bk["mean_rank"] is None
        if ref.accum[k, ROW["DECISIVE"] + 1] == 0:
            assert bk["value_sign_accuracy"] is None
    return rep
