"""tests/loss_cases.py -- TEST HELPER for tests/test_loss_cases_cpu.py (wave emulator) and tests/test_train_gpu.py (MI355X): the
sparse-target loss kernels of csrc/bo_train.h against a float64 reference at the shapes, dtypes and values where a kernel goes wrong.

reference64   the three losses and both gradients in float64 on the CPU, written out from the formulas in the header of bo_train.h
              (no autograd, no call into the library).  Inputs are the STORED values: fp16 / bf16 logits are widened exactly.
envelope      what a float32 implementation may differ from it by, per element, derived from the formats (below), not measured.
cases         a seeded list of finite cases; nonfinite_cases: a NaN / +inf / -inf logit in one row of a batch of 7.
check_*       the conditions; run_loss / raw_forward_backward drive the library (torch tensors on "cpu" under the emulator, on
              "cuda:0" on the GPU); check_wide_replay is the sampler test's body for both.

No row has an action twice: the header of bo_train.h does not define what duplicate indices mean (the forward would add both, the
backward keep the last), and the replay buffer never stores them.

The envelope.  With mx_b = max_a x[b,a], ls_b = log sum_a exp(x[b,a] - mx_b), p = exp(x - mx - ls), S_b = sum of the row's valid target
entries, t the dense target, g_p = w3[0] + w3[1], g_v = w3[0] + w3[2], eps = 2^-23, and c = 0 for the kernels:
  dlogits[b,a]  eps (4 + c + |x - mx_b| + |ls_b|) (S_b p[b,a] + t[b,a]) |g_p| / B + 2^-126
      first factor: float32 rounding of the exponent's argument (x - mx, then - ls: half an ulp of each magnitude, which is the relative
      error of the exponential) plus a few ulp for expf, logf, the row sum S and the products; second factor: the magnitudes of the two
      terms, so cancellation at a target entry is allowed for; 2^-126 admits float32 underflow (denormals, flushed or not).  At a
      -inf logit the exponential is exactly 0 and |x - mx| counts as 0.
      c is for PyTorch's float32 path alone (TORCH_SUM_C = 13.95).  With c = 0 that path leaves ONE envelope: in
      B4097_W64_randn3_invalid, row 1005 has a logit with p = 0.854 (x = mx, ls = 0.158), float64 gives dlogits 1.5628239625e-4 there
      and PyTorch float32 1.5628256369e-4, 1.07e-6 relative = 9.0 eps against a first factor of 4.16.  The cause is its sum of the 4672
      exponentials: a relative error of the sum is an absolute error of ls and so a relative error of every p of the row.  PyTorch's
      vectorised sum runs chains of 4672 / 8 (or / 16) additions; each rounds by at most half an ulp of a partial sum that is at most
      the total (a large term early in a chain makes every later addition round at the total's size), and with these errors
      independent and uniform a chain of m additions has a standard deviation of eps sqrt(m / 12): 6.98 eps at m = 584.  c is two of
      them.  The kernels' chain is 73 additions in a lane and 6 butterfly levels (1.3 eps by the same count), so they get no such
      term: they are held to the formula with c = 0, in which the same element may be 4 x 4.16 eps off.
  dvalue[b]     eps 4 |2/B (v_b - z_b) g_v| + 2^-126
  row terms     policy_b = sum_e t_be (mx_b + ls_b - x[b,i_be]): eps (4 policy_b + (4 + c) S_b) + 2^-126; value_b = (v_b - z_b)^2:
      eps 4 value_b + 2^-126.  Every summand of policy_b is t (|x_i - mx| + ls) with both parts >= 0, so the roundings of x_i - mx, of
      - ls and of the product are relative to the term itself (3 half-ulps).  The one error that is not is that of ls: the absolute
      error (4 + c) eps of the logarithm of the float32 sum, times S_b in the term.  A purely relative bound is therefore wrong where a
      target sits on a dominant logit: with one logit 60 above the rest the true term is ls = 4671 e^-60 ~ 4e-23, and float32
      (PyTorch's as well as the kernel's) has sum = 1 and ls = 0 exactly.
  losses        the mean of the row allowances, plus eps/2 (ceil(log2 B) + 2) mean_b |term_b| for the summation (a pairwise sum of B
      terms has ceil(log2 B) roundings on each path, relative to the sum of the magnitudes, which is the sum itself as no term is
      negative; + 2 for the division by B and one spare), and for the total the two allowances plus eps/2 |total| for its own addition.
      The kernel's own order (lane s adds rows s, s + 64, ..., then a 6-level butterfly) is longer at B = 4097 (70 roundings on a path,
      13 here); its error grows like the root of that count, and the factor below covers it.
A float32 output of a kernel passes within 4 envelopes -- the margin for the device's expf / logf (a couple of ulp each) and its other
summation order; PyTorch's own float32 path has to pass within ONE envelope with its c (tests/test_loss_cases_cpu.py), which keeps the
envelope honest.
A 16-bit output passes within one ulp of its type of round(reference), or within 4 envelopes where that is larger, and is inf exactly
where round(reference) is -- except within 4 envelopes of the overflow threshold, where either answer passes; those elements are
counted and have to be fewer than 0.1 % of the case's."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

A = 4672
EPS = 2.0 ** -23
TINY = 2.0 ** -126
TORCH_SUM_C = 2.0 * math.sqrt(A / 8 / 12.0)   # PyTorch's float32 sum of a row's exponentials, in eps (module docstring): 13.95
FACTOR = 4.0            # envelopes a kernel's float32 output may be off by
NEAR_SHARE = 1e-3       # share of a case's elements that may sit at the overflow threshold of a 16-bit output
EDGE_ACTIONS = (0, 63, 64, 4607, 4608, 4671)              # corners of the lane / register layout (action = lane + 64 * register)
INVALID = (4672, 2 ** 31 - 1, -2 ** 31, -2)               # not -1 and not an action: bo_loss_valid ignores them
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
PAIRS = tuple((a, b) for a in DTYPES for b in DTYPES)     # (logits, value)
NAN32 = 0x7FC0DEAD      # the guard patterns of tests/test_evaluate_batches_gpu.py: quiet NaNs with a payload no kernel writes
NAN16 = 0x7E5B
ROW_STATS = 4


def short(dtype) -> str:
    return {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]


def valid(idx):
    return (idx >= 0) & (idx < A)


def dense_target(idx, val, dtype=torch.float32):
    """[B, 4672] target of the valid entries (what PyTorch's F.cross_entropy takes)."""
    ok = valid(idx)
    d = torch.zeros((idx.shape[0], A + 1), dtype=dtype, device=idx.device)
    d.scatter_(1, torch.where(ok, idx, torch.full_like(idx, A)).long(), torch.where(ok, val, torch.zeros_like(val)).to(dtype))
    return d[:, :A].contiguous()


# ---- the float64 reference and its envelope ------------------------------------------------------------------------------------

def reference64(logits, value, idx, val, z, w3):
    """loss3 = [total, policy, value], dlogits [B, 4672] and dvalue [B] of bo_train.h's formulas in float64 on the CPU, for the stored
    inputs and the gradient w3 of loss3 (float32 values, as the kernel reads them).  A row with a non-finite logit has a NaN policy
    term, as the header states.  Also the per-row terms and the intermediates envelope() needs."""
    v, zz = value.detach().cpu().double().reshape(-1), z.detach().cpu().double().reshape(-1)
    x = logits.detach().cpu().double()
    idx = idx.cpu().long()
    B = x.shape[0]
    ok = valid(idx)
    tv = torch.where(ok, val.cpu().double(), torch.zeros((), dtype=torch.float64))
    t = torch.zeros((B, A + 1), dtype=torch.float64).scatter_(1, torch.where(ok, idx, torch.full_like(idx, A)), tv)[:, :A]
    S = tv.sum(1)
    mx = x.amax(1, keepdim=True)
    xm = x - mx
    ls = torch.log(torch.exp(xm).sum(1, keepdim=True))
    logp = xm - ls
    p = torch.exp(logp)
    picked = torch.gather(logp, 1, torch.where(ok, idx, torch.zeros_like(idx)))
    row_policy = -torch.where(ok, tv * picked, torch.zeros((), dtype=torch.float64)).sum(1)
    row_policy[~torch.isfinite(x).all(1)] = float("nan")
    row_value = (v - zz) ** 2
    w = torch.tensor(w3, dtype=torch.float32).double()
    gp, gv = float(w[0] + w[1]), float(w[0] + w[2])
    pol, vl = row_policy.sum() / B, row_value.sum() / B
    return SimpleNamespace(B=B, loss3=torch.stack([pol + vl, pol, vl]), dlogits=gp / B * (p * S[:, None] - t),
                           dvalue=2.0 / B * (v - zz) * gv, row_policy=row_policy, row_value=row_value,
                           xm=xm, ls=ls, p=p, S=S, t=t, gp=gp, gv=gv)


def envelope(ref, c=0.0):
    """The float32 allowances of the module docstring for a reference64 result: dlogits [B, 4672], dvalue [B], loss3 [3] and the
    per-row terms.  c: the extra allowance for the float32 sum of a row's exponentials, in eps -- 0 for the kernels, TORCH_SUM_C for
    PyTorch's float32 path.  Rows with a NaN or +inf logit have NaN allowances (the non-finite cases do not compare them)."""
    B = ref.B
    first = 4.0 + c + torch.where(torch.isinf(ref.xm) & (ref.xm < 0), torch.zeros((), dtype=torch.float64), ref.xm.abs()) + ref.ls.abs()
    dlogits = EPS * first * (ref.S[:, None] * ref.p + ref.t) * abs(ref.gp) / B + TINY
    dvalue = EPS * 4.0 * ref.dvalue.abs() + TINY
    row_policy = EPS * (4.0 * ref.row_policy.abs() + (4.0 + c) * ref.S) + TINY
    row_value = EPS * 4.0 * ref.row_value + TINY
    depth = math.ceil(math.log2(B)) + 2
    pol = row_policy.mean() + 0.5 * EPS * depth * ref.row_policy.abs().mean()
    vl = row_value.mean() + 0.5 * EPS * depth * ref.row_value.mean()
    tot = pol + vl + 0.5 * EPS * ref.loss3[0].abs()
    return SimpleNamespace(dlogits=dlogits, dvalue=dvalue, loss3=torch.stack([tot, pol, vl]), row_policy=row_policy, row_value=row_value)


def autograd64(logits, value, idx, val, z, w3):
    """The same quantities from torch.autograd of F.cross_entropy + F.mse_loss in float64: reference64's own check."""
    x, v = logits.double().clone().requires_grad_(), value.double().reshape(-1).clone().requires_grad_()
    pol, vl = F.cross_entropy(x, dense_target(idx, val, torch.float64)), F.mse_loss(v, z.double().reshape(-1))
    tot = pol + vl
    w = torch.tensor(w3, dtype=torch.float32).double()
    (w[0] * tot + w[1] * pol + w[2] * vl).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


def torch32(logits, value, idx, val, z, w3):
    """PyTorch's float32 path on the inputs' device for the stored inputs widened to float32."""
    x, v = logits.float().clone().requires_grad_(), value.float().reshape(-1).clone().requires_grad_()
    pol, vl = F.cross_entropy(x, dense_target(idx, val)), F.mse_loss(v, z.reshape(-1))
    tot = pol + vl
    (w3[0] * tot + w3[1] * pol + w3[2] * vl).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


# ---- the conditions ------------------------------------------------------------------------------------------------------------

_FMT = {torch.float16: (10, -14, 65520.0, 65504.0),                                   # mantissa bits, least exponent, overflow threshold
        torch.bfloat16: (7, -126, (2.0 - 2.0 ** -8) * 2.0 ** 127, (2.0 - 2.0 ** -7) * 2.0 ** 127)}  # (round to nearest), largest finite


def check_output(got, ref, env, what, rows=None):
    """One output tensor against its float64 reference and envelope (CPU float64 tensors; moved to got's device).  float32: every
    element within FACTOR envelopes.  fp16 / bf16: the module docstring's rule.  Returns (worst error / envelope for float32, worst
    error / allowance for 16 bits; number of elements at the overflow threshold).  rows: compare these rows only."""
    dev = got.device
    g = got.detach().double().reshape(ref.shape)
    ref, env = ref.to(dev), env.to(dev)
    if rows is not None:
        g, ref, env = g[rows], ref[rows], env[rows]
    if got.dtype == torch.float32:
        err = (g - ref).abs()
        bad = ~(err <= FACTOR * env)
        worst = float((err / env).max()) if err.numel() else 0.0
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond {FACTOR} envelopes, worst error / envelope "
                                     f"{worst:.3g} at {_where(bad, err / env)}")
        return worst, 0
    mant, emin, thr, top = _FMT[got.dtype]
    r = ref.to(got.dtype).double()
    sign = torch.where(ref < 0, -1.0, 1.0).to(dev).double()
    near = ((ref.abs() - thr).abs() <= FACTOR * env)
    rf = torch.where(torch.isfinite(r), r, sign * top)
    expo = torch.where(rf == 0, torch.full_like(rf, emin), (torch.frexp(rf.abs())[1] - 1).double())  # (frexp(0) has exponent 0)
    ulp = torch.exp2(expo.clamp(min=emin) - mant)
    tol = torch.maximum(ulp, FACTOR * env)
    err = (g - rf).abs()
    fits = torch.isfinite(g) & (err <= tol)
    ok = torch.where(near, fits | (g == sign * float("inf")), torch.where(torch.isfinite(r), fits, g == r))
    worst = float((err / tol)[torch.isfinite(g) & torch.isfinite(r)].max()) if bool((torch.isfinite(g) & torch.isfinite(r)).any()) else 0.0
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} elements beyond one ulp / {FACTOR} envelopes or with a misplaced "
                            f"inf, worst error / allowance {worst:.3g} at {_where(~ok, err / tol)}")
    return worst, int(near.sum())


def _where(bad, ratio):
    r = torch.where(bad, torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")), torch.zeros_like(ratio))
    i = int(r.reshape(-1).argmax())
    return tuple(int(k) for k in np.unravel_index(i, tuple(ratio.shape))) if ratio.dim() else ()


def check_against_reference(out, ref, env, what):
    """(loss3, dlogits, dvalue) of a run against reference64 / envelope.  Returns {"loss", "dlogits", "dvalue": worst ratios, "near"}."""
    loss3, gx, gv = out
    assert loss3.dtype == torch.float32
    worst_l, _ = check_output(loss3, ref.loss3, env.loss3, what + " loss3")
    worst_x, near_x = check_output(gx, ref.dlogits, env.dlogits, what + " dlogits")
    worst_v, near_v = check_output(gv, ref.dvalue, env.dvalue, what + " dvalue")
    near = near_x + near_v
    assert near < NEAR_SHARE * (ref.dlogits.numel() + ref.dvalue.numel()), f"{what}: {near} elements at the overflow threshold"
    return {"loss": worst_l, "dlogits": worst_x, "dvalue": worst_v, "near": near}


# ---- the cases -----------------------------------------------------------------------------------------------------------------

# (B, W, logits, placement, index into W3, entries of 1e-30): every B with one small and one large W, every W with a small (<= 65)
# and a large (>= 127) B; every kind of logits, every placement and every w3 at least once
GRID = ((1, 1, "randn3", "prefix", 0, False), (1, 130, "randn001", "scattered", 1, True), (2, 2, "flat", "full", 2, False),
        (2, 65, "dom60", "empty_rows", 0, True), (63, 32, "dom90", "edges", 2, False), (63, 64, "neg80", "invalid", 5, True),
        (64, 1, "pos80", "prefix", 6, False), (64, 130, "f16max", "scattered", 0, True), (65, 2, "dom60_first", "full", 1, False),
        (65, 63, "dom90_last", "empty_rows", 2, True), (127, 32, "randn3", "edges", 3, False), (127, 63, "randn001", "invalid", 1, True),
        (128, 2, "flat", "prefix", 4, False), (128, 130, "dom60", "scattered", 6, True), (1000, 1, "dom90", "full", 0, False),
        (1000, 65, "neg80", "empty_rows", 1, True), (4097, 2, "pos80", "edges", 2, False), (4097, 64, "randn3", "invalid", 1, True))
LOGITS = ("randn3", "randn001", "flat", "dom60", "dom90", "neg80", "pos80", "f16max", "dom60_first", "dom90_last")
PLACEMENTS = ("prefix", "scattered", "full", "empty_rows", "edges", "invalid")
W3 = ((1.0, 0.0, 0.0), (0.75, 0.0, 0.0), (0.37, 1.5, -2.25), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (2.0 ** 10, 0.0, 0.0), (2.0 ** 16, 0.0, 0.0))
ROW_SUMS = (1.0, 0.97, 1e-3)


def _logits(kind, B, g):
    x = torch.randn((B, A), generator=g) * (0.01 if kind == "randn001" else 1.0 if kind in ("neg80", "pos80") else 3.0)
    if kind == "flat":                       # flat rows among random ones
        x[0] = 1.25
        x[B - 1] = -7.5
    elif kind in ("neg80", "pos80"):
        x += 80.0 if kind == "pos80" else -80.0
    elif kind.startswith("dom"):             # one logit 60 / 90 above the row's largest: most of the row underflows in float32
        up = 60.0 if kind.startswith("dom60") else 90.0
        at = torch.randint(0, A, (B,), generator=g)
        if kind.endswith("_first"):
            at[:] = 0                        # lane 0, register 0
        elif kind.endswith("_last"):
            at[:] = A - 1                    # lane 63, register 72
        x[torch.arange(B), at] = x.amax(1) + up
    elif kind == "f16max":                   # the ends of the fp16 range in one row
        x[0, torch.randperm(A, generator=g)[:8]] = torch.tensor([65504.0] * 3 + [-65504.0] * 5)
    return x


def _targets(placement, B, W, g, tiny):
    idx = torch.full((B, W), -1, dtype=torch.int32)
    val = torch.zeros((B, W))
    for b in range(B):
        if placement == "full":
            m = W
        elif placement == "empty_rows" and b in ((0, B // 2, B - 1) if B > 2 else (0,)):
            m = 0                            # an empty row first, in the middle and last
        elif placement == "all_empty":
            m = 0
        else:
            m = int(torch.randint(1, W + 1, (1,), generator=g))
        actions = torch.randperm(A, generator=g)[:m + len(EDGE_ACTIONS)]
        if placement == "edges":             # the corners of the lane / register layout first, rotated by the row
            k = min(m, len(EDGE_ACTIONS))
            edge = torch.tensor([EDGE_ACTIONS[(b + e) % len(EDGE_ACTIONS)] for e in range(k)], dtype=torch.long)
            rest = actions[~torch.isin(actions, torch.tensor(EDGE_ACTIONS))][:m - k]
            actions = torch.cat([edge, rest])
        actions = actions[:m]
        pos = torch.arange(m) if placement in ("prefix", "full", "empty_rows", "edges") else torch.randperm(W, generator=g)[:m]
        v = torch.rand(m, generator=g) + 0.05
        if tiny and m > 1:
            v[0] = 1e-30 * float(v[1:].sum())    # an entry of about 1e-30 after the normalisation
        v = v / v.sum().clamp_min(1e-30) * ROW_SUMS[b % len(ROW_SUMS)]
        idx[b, pos] = actions.int()
        val[b, pos] = v.float()
    if placement == "invalid":               # indices that are neither -1 nor an action, with values, in the slots left over
        k = torch.arange(B)[:, None] + torch.arange(W)[None, :]
        free = (idx < 0) & (k % 5 != 0)
        idx[free] = torch.tensor(INVALID, dtype=torch.int64)[k % len(INVALID)].int()[free]
        val[free] = (0.25 + 0.5 * torch.rand((B, W), generator=g))[free]
    return idx, val


def make_case(name, B, W, seed, logits="randn3", placement="prefix", w3=(1.0, 0.0, 0.0), tiny=False):
    """A case in float32 (cast logits / value to a dtype pair with cast()).  Values: +1 and -1 exactly and one near 0 among tanh(randn);
    z in {-1, 0, 1} with z[0] = value[0], so that a dvalue is exactly 0."""
    g = torch.Generator().manual_seed(seed)
    x = _logits(logits, B, g)
    value = torch.tanh(torch.randn((B, 1), generator=g))
    z = torch.randint(-1, 2, (B, 1), generator=g).float()
    for b, (v_, z_) in enumerate(((1.0, 1.0), (-1.0, 1.0), (1e-4, 0.0), (1.0, -1.0))):
        if b < B:
            value[b, 0], z[b, 0] = v_, z_
    idx, val = _targets(placement, B, W, g, tiny)
    return SimpleNamespace(name=name, B=B, W=W, logits=x, value=value, idx=idx, val=val, z=z, w3=tuple(float(w) for w in w3),
                           kind=logits, placement=placement)


@functools.lru_cache(maxsize=None)
def cases():
    """The finite cases: GRID (row sums 1 / 0.97 / 1e-3 alternate by row in every case), then combinations it does not have."""
    out = [make_case(f"B{B}_W{W}_{kind}_{place}", B, W, 1000 + k, kind, place, W3[w], tiny)
           for k, (B, W, kind, place, w, tiny) in enumerate(GRID)]
    out.append(make_case("all_rows_empty", 5, 3, 2001, "randn3", "all_empty", W3[2]))
    out.append(make_case("edges_on_dominant_first", 7, 8, 2002, "dom60_first", "edges", W3[1]))    # a target on the dominant logit
    out.append(make_case("edges_on_dominant_last", 65, 130, 2003, "dom90_last", "edges", W3[2]))
    out.append(make_case("edges_f16max", 6, 6, 2004, "f16max", "edges", W3[0]))
    out.append(make_case("invalid_wide", 63, 130, 2005, "randn3", "invalid", W3[1], tiny=True))
    out.append(make_case("empty_rows_wide", 127, 65, 2006, "randn001", "empty_rows", W3[2]))
    out.append(make_case("scale_2p16_dominant", 64, 2, 2007, "dom60", "prefix", W3[6]))
    # a GradScaler scale that overflows fp16 at the target entries: g_p / B = 2^19, so every target entry above 1/8 is beyond 65504
    out.append(make_case("overflow_fp16", 65, 2, 2008, "randn3", "prefix", (2.0 ** 19 * 65, 0.0, 0.0)))
    out.append(make_case("overflow_fp16_wide", 127, 65, 2009, "randn3", "scattered", (2.0 ** 19 * 127, 0.0, 0.0)))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def nonfinite_cases(row=2):
    """A NaN, a +inf and a -inf logit, each at a target and at a non-target action of row `row` of a batch of 7 (W = 4, prefix)."""
    out = []
    for k, (label, bad) in enumerate((("nan", float("nan")), ("posinf", float("inf")), ("neginf", float("-inf")))):
        for at_target in (True, False):
            c = make_case(f"{label}_{'target' if at_target else 'other'}", 7, 4, 3000 + k, "randn3", "full", W3[2])
            a = int(c.idx[row, 1]) if at_target else int(torch.nonzero(~torch.isin(torch.arange(A), c.idx[row].long()))[17])
            c.logits[row, a] = bad
            c.bad, c.row, c.action, c.at_target = label, row, a, at_target
            out.append(c)
    return out


def cast(case, pair, device="cpu"):
    """The case's tensors on `device` with logits / value stored as the dtype pair: (logits, value, idx, val, z)."""
    return (case.logits.to(pair[0]).to(device), case.value.to(pair[1]).to(device), case.idx.to(device), case.val.to(device),
            case.z.to(device))


# ---- driving the library -------------------------------------------------------------------------------------------------------

def run_loss(logits, value, idx, val, z, w3):
    """(loss3, dlogits, dvalue) of train.sparse_policy_value_loss and its backward for the gradient w3 of [total, policy, value]."""
    from betaone_amd.train import sparse_policy_value_loss

    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    tot, pol, vl = sparse_policy_value_loss(x, v, idx, val, z)
    (w3[0] * tot + w3[1] * pol + w3[2] * vl).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad.reshape(-1)


def same_bits(a, b) -> bool:
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def guarded(rows, cols, dtype, device, guard=64):
    """[rows + guard, cols] filled with the NaN payload pattern of its width."""
    t = torch.empty((rows + guard, cols), dtype=dtype, device=device)
    if dtype == torch.float32:
        t.view(torch.int32).fill_(NAN32)
    else:
        t.view(torch.int16).fill_(NAN16)
    return t


def guard_intact(t, rows) -> bool:
    bits = t[rows:].view(torch.int32) if t.dtype == torch.float32 else t[rows:].view(torch.int16)
    return bool((bits == (NAN32 if t.dtype == torch.float32 else NAN16)).all())


def raw_forward_backward(logits, value, idx, val, z, w3, guard=64):
    """bo_train_loss_forward / bo_train_loss_backward called directly, with row_stats, dlogits and dvalue allocated `guard` rows longer
    than the batch and pre-filled with the NaN payload.  Returns (row_stats, loss3, dlogits, dvalue), the three with their guard rows."""
    from betaone_amd import engine as E
    from betaone_amd.train import DTYPE_CODES

    lib = E.load_hip_library()
    dev = logits.device
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    n, W = idx.shape
    logits, value, z = logits.contiguous(), value.contiguous().reshape(-1), z.contiguous().reshape(-1)
    row_stats = guarded(n, ROW_STATS, torch.float32, dev, guard)
    dlogits, dvalue = guarded(n, A, logits.dtype, dev, guard), guarded(n, 1, value.dtype, dev, guard)
    loss3 = torch.empty(3, dtype=torch.float32, device=dev)
    g3 = torch.tensor(w3, dtype=torch.float32, device=dev)
    rc = lib.bo_train_loss_forward(n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.data_ptr(), DTYPE_CODES[value.dtype],
                                   idx.data_ptr(), val.data_ptr(), z.data_ptr(), row_stats.data_ptr(), loss3.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    rc = lib.bo_train_loss_backward(n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.data_ptr(), DTYPE_CODES[value.dtype],
                                    idx.data_ptr(), val.data_ptr(), z.data_ptr(), row_stats.data_ptr(), g3.data_ptr(), dlogits.data_ptr(),
                                    dvalue.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return row_stats, loss3, dlogits, dvalue


def check_guard_rows(case, pair, device):
    """The raw calls on buffers with 64 guard rows: the guard holds its pattern, every row below B is written (no payload left), and
    the results are those of the reference."""
    t = cast(case, pair, device)
    row_stats, loss3, dlogits, dvalue = raw_forward_backward(*t, case.w3)
    B = case.B
    what = f"{case.name} {short(pair[0])}/{short(pair[1])} guard rows"
    for name, buf in (("row_stats", row_stats), ("dlogits", dlogits), ("dvalue", dvalue)):
        assert guard_intact(buf, B), f"{what}: {name} written past row {B}"
        bits = buf[:B].view(torch.int32) if buf.dtype == torch.float32 else buf[:B].view(torch.int16)
        assert not bool((bits == (NAN32 if buf.dtype == torch.float32 else NAN16)).any()), f"{what}: {name} has unwritten elements"
    ref = reference64(*t, case.w3)
    env = envelope(ref)
    check_output(row_stats[:B, 2], ref.row_policy, env.row_policy, what + " row policy terms")
    check_output(row_stats[:B, 3], ref.row_value, env.row_value, what + " row value terms")
    return check_against_reference((loss3, dlogits[:B], dvalue[:B].reshape(-1)), ref, env, what)


def check_row_independence(case, pair, device, seed=0):
    """The rows in a permuted order: the same row_stats and dlogits / dvalue rows bit for bit (w3 reaches every row as g / B, and B is
    the same); the three reduced losses within their bound."""
    t = cast(case, pair, device)
    perm = torch.randperm(case.B, generator=torch.Generator().manual_seed(seed)).to(device)
    assert case.B < 2 or not bool(torch.equal(perm, torch.arange(case.B, device=device)))
    rs0, l0, dx0, dv0 = raw_forward_backward(*t, case.w3, guard=0)
    rs1, l1, dx1, dv1 = raw_forward_backward(*(a[perm].contiguous() for a in t), case.w3, guard=0)
    what = f"{case.name} {short(pair[0])}/{short(pair[1])} permuted rows"
    assert same_bits(rs0[perm], rs1), what + ": row_stats differ"
    assert same_bits(dx0[perm], dx1), what + ": dlogits rows differ"
    assert same_bits(dv0[perm], dv1), what + ": dvalue rows differ"
    ref = reference64(*t, case.w3)
    env = envelope(ref)
    for l in (l0, l1):
        check_output(l, ref.loss3, env.loss3, what + " loss3")


def check_nonfinite(case, pair, device):
    """What the header of bo_train.h states for a row with a non-finite logit (see nonfinite_cases)."""
    t = cast(case, pair, device)
    loss3, gx, gv = run_loss(*t, case.w3)
    ref = reference64(*t, case.w3)
    env = envelope(ref)
    what = f"{case.name} {short(pair[0])}/{short(pair[1])}"
    assert bool(torch.isnan(loss3[:2]).all()), f"{what}: total / policy {loss3.tolist()} are not NaN"
    assert bool(torch.isfinite(loss3[2])), what
    check_output(loss3[2], ref.loss3[2], env.loss3[2], what + " value loss")
    check_output(gv, ref.dvalue, env.dvalue, what + " dvalue")
    others = [b for b in range(case.B) if b != case.row]
    assert bool(torch.isfinite(gx[others]).all()), what
    check_output(gx, ref.dlogits, env.dlogits, what + " dlogits of the other rows", rows=others)
    if case.bad == "neginf":   # the softmax without that action: 0 there, minus the target entry if it is one
        assert bool(torch.isfinite(gx[case.row]).all()), what
        assert bool(torch.isfinite(ref.dlogits[case.row]).all())
        check_output(gx, ref.dlogits, env.dlogits, what + " dlogits of the row", rows=[case.row])
    else:                      # NaN or +inf: the max is NaN / inf, the softmax and the whole row's gradient NaN
        assert bool(torch.isnan(gx[case.row]).all()), f"{what}: the row's gradient is not all NaN"
        assert bool(torch.isnan(ref.dlogits[case.row]).all())


def check_refusals(device):
    """What the five bo_train_* entry points refuse, and in which words (the texts are written out here, not taken from the library's
    source: "<entry>: bad arguments" and "<entry>: unsupported dtype").  With n = 2, W = 2 and float32 buffers that a call could run on:
    every pointer that must not be null, null in turn; n = 0, W = 0, W = BO_RES_CAP + 1 and, for the metrics, n_buckets = 0 give
    -1 (BO_E_ARG) and "<entry>: bad arguments"; the dtype code 7 for the logits or for the value gives -3 (BO_E_CONFIG) and
    "<entry>: unsupported dtype"; a null pointer together with the code 7 gives -1.  q and bucket of bo_train_metrics and every stream
    may be null (no root values, one bucket, the default stream): they are no refusals.  The unchanged arguments are accepted first
    (0), so each refusal is the changed argument's.  Returns the number of refusals seen."""
    from betaone_amd import engine as E

    lib = E.load_hip_library()
    n = W = 2

    def buf(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=device)

    logits, value, idx, val, z = buf(n, A), buf(n), buf(n, W, dtype=torch.int32), buf(n, W), buf(n)
    q, mix, g3, stats, loss, dlogits, dvalue = buf(n), buf(1), buf(3), buf(n, 6), buf(5), buf(n, A), buf(n)
    rows, accum, bucket = buf(n, E.METRIC_ROW_COLS), buf(1, E.METRIC_COLS, dtype=torch.float64), buf(n, dtype=torch.int32)
    p = torch.Tensor.data_ptr
    batch = [n, W, p(logits), 0, p(value), 0, p(idx), p(val), p(z)]   # arguments 0..8 of every entry point; 2, 4, 6, 7, 8 are pointers
    entries = {   # the arguments from 9 on, and which of them are pointers that must not be null
        "bo_train_loss_forward": ([p(stats), p(loss), None], (9, 10)),
        "bo_train_loss_backward": ([p(stats), p(g3), p(dlogits), p(dvalue), None], (9, 10, 11, 12)),
        "bo_train_loss_forward_mix": ([p(q), p(mix), p(stats), p(loss), None], (9, 10, 11, 12)),
        "bo_train_loss_backward_mix": ([p(q), p(mix), p(stats), p(g3), p(dlogits), p(dvalue), None], (9, 10, 11, 12, 13, 14)),
        "bo_train_metrics": ([p(q), p(bucket), 1, p(rows), p(accum), None], (12, 13)),
    }
    seen = 0
    for entry, (rest, own) in entries.items():
        fn, good = getattr(lib, entry), batch + rest

        def refused(code, text, **changed):
            args = list(good)
            for k, v in changed.items():
                args[int(k[1:])] = v
            rc = fn(*args)
            assert rc == code and lib.bo_last_error().decode() == f"{entry}: {text}", (entry, changed, rc, lib.bo_last_error())
            return 1

        assert fn(*good) == 0, (entry, lib.bo_last_error())
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        for k in (2, 4, 6, 7, 8) + own:
            seen += refused(-1, "bad arguments", **{f"a{k}": None})
            seen += refused(-1, "bad arguments", **{f"a{k}": None}, a3=7)
        seen += refused(-1, "bad arguments", a0=0) + refused(-1, "bad arguments", a1=0) + refused(-1, "bad arguments", a1=res_cap() + 1)
        if entry == "bo_train_metrics":
            seen += refused(-1, "bad arguments", a11=0) + refused(-1, "bad arguments", a11=0, a5=7)
        seen += refused(-3, "unsupported dtype", a3=7) + refused(-3, "unsupported dtype", a5=7)
        seen += refused(-1, "bad arguments", a0=0, a3=7, a5=7)
    return seen


# ---- the replay samplers at wide rows ------------------------------------------------------------------------------------------

def res_cap() -> int:
    """BO_RES_CAP of csrc/bo_tree.h: the widest pi a replay buffer accepts."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "betaone_amd", "csrc", "bo_tree.h")
    return int(re.search(r"^#define\s+BO_RES_CAP\s+(\d+)", open(path).read(), re.M).group(1))


def synthetic_pis(games, W, seed):
    """The games (rollout.FinishedGame objects or dicts) as dicts whose pis are seeded synthetic ones of 0..W entries: distinct
    actions, float32 values normalised to 1; every fifth ply has none, the first ply of every game has W."""
    from betaone_amd import records as R

    rng = np.random.default_rng(seed)
    out, k = [], 0
    for f in games:
        g = dict(f) if isinstance(f, dict) else R.unpack_games(R.pack_game(f))[0]
        pis = []
        for ply in range(int(g["n_plies"])):
            m = W if ply == 0 else 0 if k % 5 == 4 else int(rng.integers(0, W + 1))
            k += 1
            ix = rng.choice(A, size=m, replace=False).astype(np.int32)
            v = (rng.random(m) + 0.05).astype(np.float32)
            pis.append((ix, (v / max(float(v.sum()), 1e-30)).astype(np.float32)))
        g["pis"] = pis
        out.append(g)
    return out


def check_wide_replay(games, W, device, seed=0):
    """GpuReplayBuffer(pi_width=W) over the games with synthetic pis: batch_sparse equals the stored records entry for entry with
    (-1, 0) in the unused slots, its scatter equals batch bit for bit with equal planes and z, and one sparse loss forward and
    backward on that batch is within the envelope of reference64.  Returns the loss check's worst ratios."""
    from betaone_amd import records as R

    games = [g for g in synthetic_pis(games, W, seed) if int(g["n_plies"]) > 0]
    buf = R.GpuReplayBuffer(4096, device=device, pi_width=W)
    try:
        assert buf.add(games) == 0
        stored = [pi for g in games for pi in g["pis"]]
        n = len(buf)
        assert n == len(stored)
        q = np.arange(n)
        s0, p0, z0 = buf.batch(q)
        s1, i1, v1, z1 = buf.batch_sparse(q)
        assert i1.dtype == torch.int32 and i1.shape == (n, W) and v1.shape == (n, W) and z1.shape == (n, 1)
        want_i, want_v = np.full((n, W), -1, dtype=np.int32), np.zeros((n, W), dtype=np.float32)
        for r, (ix, v) in enumerate(stored):
            want_i[r, :len(ix)], want_v[r, :len(ix)] = ix, v
        assert np.array_equal(i1.cpu().numpy(), want_i), f"W={W}: batch_sparse indices differ from the records"
        assert np.array_equal(v1.cpu().numpy().view(np.uint32), want_v.view(np.uint32)), f"W={W}: batch_sparse values differ from the records"
        counts = (i1 >= 0).sum(1)
        assert int(counts.min()) == 0 and int(counts.max()) == W
        assert same_bits(s0, s1) and same_bits(z0, z1)
        assert same_bits(dense_target(i1, v1), p0), f"W={W}: the scatter of batch_sparse differs from batch"
        g = torch.Generator().manual_seed(seed + W)
        logits = (torch.randn((n, A), generator=g) * 3.0).to(device)
        value = torch.tanh(torch.randn((n, 1), generator=g)).to(device)
        w3 = W3[2]
        out = run_loss(logits, value, i1, v1, z1, w3)
        ref = reference64(logits, value, i1, v1, z1, w3)
        return check_against_reference(out, ref, envelope(ref), f"replay batch W={W}")
    finally:
        buf.close()
