"""tests/value_mix_cases.py -- TEST HELPER for tests/test_value_mix_emu.py (wave emulator) and tests/test_value_mix_gpu.py (MI355X): the
value head trained on a mix of the game's outcome z and the search's root value q, t = (1 - a) z + a q, from the replay record to the
`train` command.  The bodies run on "cpu" under the emulator and on "cuda:0" on the GPU.

fake_games        games of random legal moves (the CPU oracle's rules, oracle/shim) with made-up outcomes, pis and root values that
                  can be recognised: no search is played for them.
check_sampler     GpuReplayBuffer.batch_sparse_q against the stored records, across ring wrap-around and eviction.
reference64_mix   loss5 = [policy + value_mix, policy, value_mix, value_vs_z, value_vs_q] and both gradients in float64, written out
                  from the formulas (the policy side is tests/loss_cases.py's reference64, which has no value mix in it).
check_loss_case   the kernels against it on the cases of tests/loss_cases.py.
check_mix0 / check_invalid_mix / check_perspective / check_command / check_training   the other conditions.

The bounds are the ones the project uses for these kernels and no others: every loss within 1e-6 relative of float64 and float32
gradients within 1e-6 absolute (tests/test_train_gpu.py, tests/test_train_emu.py), fp16 / bf16 gradients within one ulp of the rounded
reference with inf in the same places (check_output of tests/loss_cases.py; for dlogits, whose formula the mix does not touch, with
that module's envelope at the overflow threshold; for dvalue with no envelope at all).

The gradient of [total, policy, value_mix].  tests/loss_cases.py gives every case a w3, some of them GradScaler scales of 2^10, 2^16
and 2^19 B.  An absolute bound of 1e-6 on a float32 gradient presupposes gradients of order 1 -- the tests it comes from use 0.75 and
(0.37, 1.5, -2.25): at a scale of 2^16 the spacing of float32 numbers at the gradient's size is itself 1e-3.  So a float32 output is
checked against 1e-6 with the case's w3 where its largest weight is at most 2.25 and with (1, 0, 0) otherwise; the scales are kept for
the dtype pairs whose two gradients are both 16-bit, where the bound is relative (an ulp) and the scale decides where inf has to appear.
A pair that had its scale replaced runs a second time AT the case's scale, under the relative conditions alone: a float32 output
within FACTOR envelopes of the reference (tests/loss_cases.py's envelope for dlogits, dvalue_envelope below for dvalue), a 16-bit
output by the one-ulp rule.  So every instance sees every scale.

dvalue_envelope.  tests/loss_cases.py allows dvalue eps 4 |dvalue|: relative to the result, which is right for v - z (z is given) and
wrong for v - t, where t is computed and v - t may cancel.  In float32 t = (1 - a) z + a q is four operations -- 1 - a, two products,
one sum -- each rounding by at most eps/2 of its result, so |t - t_exact| <= eps/2 (2 |(1 - a) z| + |a q| + |t|) <= eps 2 T with
T = |(1 - a) z| + |a q|; that error reaches dvalue times |2/B g_v|.  The subtraction, the two products and g_v = w3[0] + w3[2] are
relative to the result, inside the 4 eps |dvalue| of that module.  Allowance: eps (4 |dvalue| + 2 |2/B g_v| T) + 2^-126.

q for a loss case: tanh(0.8 randn), with the first rows set against tests/loss_cases.py's (value, z) = (1, 1), (-1, 1), (1e-4, 0),
(1, -1): q = z (the fallback of a record without a value: t = z whatever the mix), q = value, q = 0 and q = -z."""
from __future__ import annotations

import json
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_cases as LC

MIXES = (0.25, 0.5, 1.0)
INVALID_MIXES = (1.5, -0.1, float("nan"))
UNIT_W3 = (1.0, 0.0, 0.0)
MAX_UNIT_WEIGHT = 2.25
MESSAGE = "run selfplay_main with --record-values or a resign threshold"
F32 = torch.float32


# ---- fake games ----------------------------------------------------------------------------------------------------------------

def _recognisable_q(gid, n, positions, white_won):
    """One float32 per ply, exactly representable and different for every (game, ply).  The game white won gets values that SAY so
    from the side to move's point of view: positive with white to move, negative with black to move -- the sign of its z."""
    if white_won:
        return np.array([(0.5 + i / 256.0) * (1.0 if positions[i].turn == 1 else -1.0) for i in range(n)], dtype=np.float32)
    return np.array([((gid * 37 + i * 11) % 199 - 99) / 128.0 for i in range(n)], dtype=np.float32)


def fake_games(n_games=8, seed=5, values=lambda gid: gid % 4 != 3, min_plies=9, max_plies=28, const_q=None):
    """unpack_games dicts of n_games random legal games.  Game g: outcome (+1, -1, 0)[g % 3] -- game 0 is won by white, so its records
    with black to move have z = -1, and the drawn games have z = +0.0 and -0.0; a pi of 1 or 2 distinct actions per ply; root values
    (BOG2) where values(g), none (BOG1) elsewhere.  const_q: one root value for every ply of a game, const_q(g), instead."""
    import engine_cases as EC
    import pgn_util as U
    from betaone_amd import records as R

    rng = random.Random(seed)
    nrng = np.random.default_rng(seed)
    blobs = []
    for gid in range(n_games):
        while True:
            ucis = U.random_game(rng, max_plies=rng.randint(min_plies, max_plies), eval_p=0.0, book_p=0.0)[0]
            if len(ucis) >= min_plies:
                break
        b = U.chess.Board()
        pos = [EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1)]
        moves = []
        for u in ucis:
            m = U.chess.Move.from_uci(u)
            moves.append(m.from_square | m.to_square << 6 | (m.promotion or 0) << 12)
            b.push(m)
            pos.append(EC.to_bo_position(b._p, b.ep_square if b.has_legal_en_passant() else -1))
        n = len(moves)
        pis = []
        for _ in range(n):
            k = int(nrng.integers(1, 3))
            v = (nrng.random(k) + 0.05).astype(np.float32)
            pis.append((nrng.choice(LC.A, size=k, replace=False).astype(np.int32), (v / v.sum()).astype(np.float32)))
        outcome = (1.0, -1.0, 0.0)[gid % 3]
        fin = SimpleNamespace(game_id=gid, pis=pis, positions=pos, moves=moves, terminal=1 if outcome else 2, outcome=outcome)
        if values(gid):
            fin.root_values = (np.full(n, const_q(gid), dtype=np.float32) if const_q is not None
                               else _recognisable_q(gid, n, pos, white_won=gid == 0))
        blobs.append(R.pack_game(fin))
    games = R.unpack_games(b"".join(blobs))
    assert len(games) == n_games and [g["root_values"] is not None for g in games] == [bool(values(g)) for g in range(n_games)]
    return games


def stored(games):
    """(z, q, has value) per record of the games in order, as the buffer has to hold them: z by self_play.py:202, q the root value
    or z itself."""
    z, q, has = [], [], []
    for g in games:
        out = np.float32(g["outcome"])
        zz = np.array([out if g["positions"][i].turn == 1 else -out for i in range(int(g["n_plies"]))], dtype=np.float32)
        z.append(zz)
        q.append(zz if g["root_values"] is None else np.asarray(g["root_values"], dtype=np.float32))
        has.append(np.full(len(zz), g["root_values"] is not None))
    return np.concatenate(z), np.concatenate(q), np.concatenate(has)


def _u32(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).reshape(-1).view(np.uint32)


def _check_resident(buf, resident, rng, what):
    z, q, has = stored(resident)
    n = len(buf)
    assert n == len(z) and buf.n_games == len(resident), what
    assert buf.n_with_values == int(has.sum()), f"{what}: n_with_values {buf.n_with_values}, host count {int(has.sum())}"
    order = rng.permutation(n)
    s1, i1, v1, z1, q1 = buf.batch_sparse_q(order)
    s0, i0, v0, z0 = buf.batch_sparse(order)
    assert q1.shape == (n, 1) and q1.dtype == torch.float32
    assert LC.same_bits(s0, s1) and torch.equal(i0, i1) and LC.same_bits(v0, v1) and LC.same_bits(z0, z1), f"{what}: not batch_sparse's batch"
    assert np.array_equal(_u32(z1), z[order].view(np.uint32)), f"{what}: z"
    assert np.array_equal(_u32(q1), q[order].view(np.uint32)), f"{what}: q differs from the records"
    no = ~has[order]
    assert np.array_equal(_u32(q1)[no], _u32(z1)[no]), f"{what}: a record without a value has q != z"
    return z, q, has


def check_sampler(device, seed=0):
    """Everything item 1 of the issue asks of the sampler.  Returns the number of records evicted in the wrap-around part."""
    import ctypes as C

    from betaone_amd import records as R

    games = fake_games()
    rng = np.random.default_rng(seed)
    buf = R.GpuReplayBuffer(4096, device=device, pi_width=2)
    try:
        assert buf.n_with_values == 0
        assert buf.add(games) == 0
        z, q, has = _check_resident(buf, games, rng, "all games resident")
        assert has.any() and not has.all() and bool((z[has] != q[has]).all())
        z0 = stored(games[:1])[0]
        assert games[0]["outcome"] == 1.0 and set(z0.tolist()) == {1.0, -1.0}            # white won: z = -1 with black to move
        neg0 = np.float32(-0.0).view(np.uint32)
        assert (z.view(np.uint32) == neg0).any() and ((z == 0) & (z.view(np.uint32) != neg0)).any()   # both zeros are in the records
        # the loader hands out the same batches with q as without
        for four, five in zip(buf.loader(16, steps=3, seed=5, sparse=True), buf.loader(16, steps=3, seed=5, sparse=True, with_q=True)):
            assert len(five) == 5 and all(LC.same_bits(a.float(), b.float()) for a, b in zip(four, five[:4]))
        with pytest.raises(ValueError):
            buf.loader(16, sparse=False, with_q=True)
        # bad arguments: the codes bo_replay_sample_sparse gives
        lib, n = buf.lib, len(buf)
        s, i, v, zz, qq = buf.batch_sparse_q(np.arange(4))
        idx = lambda a: np.asarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        good = (s.data_ptr(), i.data_ptr(), v.data_ptr(), zz.data_ptr())
        BO_E_ARG = -1
        assert lib.bo_replay_sample_sparse(buf.h, 4, idx([0, 1, 2, n]), *good, None) == BO_E_ARG
        assert lib.bo_replay_sample_sparse_q(buf.h, 4, idx([0, 1, 2, n]), *good, qq.data_ptr(), None) == BO_E_ARG
        assert b"out of range" in lib.bo_last_error()
        assert lib.bo_replay_sample_sparse_q(buf.h, 4, idx([0, 1, 2, -1]), *good, qq.data_ptr(), None) == BO_E_ARG
        assert lib.bo_replay_sample_sparse_q(buf.h, 4, idx([0, 1, 2, 3]), *good, None, None) == BO_E_ARG       # NULL q_dev
        assert lib.bo_replay_sample_sparse_q(buf.h, 4, idx([0, 1, 2, 3]), good[0], good[1], good[2], None, qq.data_ptr(), None) == BO_E_ARG
        assert lib.bo_replay_sample_sparse_q(buf.h, 0, idx([0]), *good, qq.data_ptr(), None) == BO_E_ARG
        assert lib.bo_replay_sample_sparse_q(None, 4, idx([0, 1, 2, 3]), *good, qq.data_ptr(), None) == BO_E_ARG
        out = C.c_int64(7)
        assert lib.bo_replay_values(None, C.byref(out)) == BO_E_ARG and lib.bo_replay_values(buf.h, None) == BO_E_ARG
        with pytest.raises(ValueError):   # root values of the wrong length
            buf.add([dict(games[0], root_values=np.zeros(3, np.float32))])
    finally:
        buf.close()
    # a ring of about three games: every add past that evicts, and the ring comes round several times
    slots = sum(int(g["n_plies"]) + 1 for g in games[:3]) + 4
    small = R.GpuReplayBuffer(slots - 2, device=device, pi_width=2)   # (the constructor adds max(2, n // 64) slots of its own)
    try:
        added, used = [], 0
        for rnd in range(3):
            for g in games:
                small.add([dict(g, game_id=100 * rnd + g["game_id"])])
                added.append(g)
                used += int(g["n_plies"]) + 1
                resident = added[-small.n_games:]          # games leave oldest first
                _check_resident(small, resident, rng, f"round {rnd}, game {g['game_id']}")
        assert small.n_evicted > 0 and used > 3 * slots and small.n_games < len(games)
        return small.n_evicted
    finally:
        small.close()


# ---- the float64 reference -------------------------------------------------------------------------------------------------------

def root_values_for(case, seed=77):
    g = torch.Generator().manual_seed(seed + case.B * 131 + case.W)
    q = torch.tanh(0.8 * torch.randn((case.B, 1), generator=g))
    z, v = case.z, case.value
    for b, val in enumerate((z[0, 0] if case.B > 0 else 0, v[1, 0] if case.B > 1 else 0, 0.0, -z[3, 0] if case.B > 3 else 0)):
        if b < case.B:
            q[b, 0] = float(val)
    return q


def reference64_mix(base, value, z, q, mix):
    """loss5, dlogits, dvalue in float64 for the stored inputs: base = LC.reference64(...) of the same case (policy term, dlogits and
    the weights w3 -- none of them knows the mix), and here t = (1 - a) z + a q with a the float32 the kernel reads,
    value_mix = mean (v - t)^2, value_vs_z = mean (v - z)^2, value_vs_q = mean (v - q)^2, dvalue = 2/B (v - t) g_v."""
    v, zz, qq = (t.detach().cpu().double().reshape(-1) for t in (value, z, q))
    a = float(np.float32(mix))
    t = (1.0 - a) * zz + a * qq
    B = base.B
    pol = base.loss3[1]
    vm, vz, vq = ((v - t) ** 2).sum() / B, ((v - zz) ** 2).sum() / B, ((v - qq) ** 2).sum() / B
    return SimpleNamespace(loss5=torch.stack([pol + vm, pol, vm, vz, vq]), dlogits=base.dlogits, dvalue=2.0 / B * (v - t) * base.gv, t=t,
                           T=((1.0 - a) * zz).abs() + (a * qq).abs(), scale=abs(2.0 / B * base.gv))


def dvalue_envelope(ref):
    """The float32 allowance for dvalue under a mix (module docstring), per row."""
    return LC.EPS * (4.0 * ref.dvalue.abs() + 2.0 * ref.scale * ref.T) + LC.TINY


def run_loss_mix(logits, value, idx, val, z, q, mix, w3):
    """(loss5, dlogits, dvalue) of train.sparse_policy_value_loss_mix and its backward for the gradient w3 of [total, policy, value_mix]."""
    from betaone_amd.train import sparse_policy_value_loss_mix

    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    out = sparse_policy_value_loss_mix(x, v, idx, val, z, q, mix)
    assert not out[3].requires_grad and not out[4].requires_grad
    (w3[0] * out[0] + w3[1] * out[1] + w3[2] * out[2]).backward()
    return torch.stack([o.detach() for o in out]), x.grad, v.grad.reshape(-1)


def weights_for(case, pair):
    if max(abs(w) for w in case.w3) <= MAX_UNIT_WEIGHT or F32 not in pair:
        return case.w3
    return UNIT_W3


def check_losses(loss5, ref5, what):
    got, ref = loss5.detach().cpu().double(), ref5.double()
    rel = ((got - ref).abs() / ref.abs()).nan_to_num(nan=0.0)   # (0 / 0: both are exactly 0)
    print(f"FIGURE {what} loss5 relative errors {[f'{r:.2e}' for r in rel.tolist()]}")
    assert loss5.dtype == torch.float32 and tuple(loss5.shape) == (5,)
    assert bool(((got - ref).abs() <= 1e-6 * ref.abs()).all()), f"{what}: loss5 {got.tolist()} against {ref.tolist()}: relative {rel.tolist()}"


def check_gradient(got, ref, env, what):
    """float32: 1e-6 absolute (and, where tests/loss_cases.py has an envelope for the formula, inside it element by element, the small
    elements too).  16-bit: one ulp of the rounded reference, inf in the same places (LC.check_output; env: the allowance at the
    overflow threshold, or None for none at all).  Returns the number of elements at the overflow threshold."""
    if got.dtype == F32:
        err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
        print(f"FIGURE {what} float32 worst absolute error {float(err.max()):.3e}")
        assert bool((err <= 1e-6).all()), f"{what}: {int((err > 1e-6).sum())} elements beyond 1e-6, worst {float(err.max()):.3e}"
        if env is not None:
            LC.check_output(got, ref, env, what)
        return 0
    worst, near = LC.check_output(got, ref, env if env is not None else torch.zeros_like(ref), what)
    print(f"FIGURE {what} {LC.short(got.dtype)} worst error / allowance {worst:.3f}, {near} elements at the overflow threshold")
    return near


def check_loss_case(case, pair, device, mixes=MIXES, again=False):
    """One case of tests/loss_cases.py on one dtype pair: every mix against reference64_mix, all five losses and both gradients;
    again: a second call on the same inputs gives the same bits."""
    t = LC.cast(case, pair, device)
    q = root_values_for(case).to(device)
    w3 = weights_for(case, pair)
    base = LC.reference64(*t, w3)
    env = LC.envelope(base)
    for mix in mixes:
        what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} mix {mix}"
        out = run_loss_mix(*t, q, mix, w3)
        assert out[1].dtype == pair[0] and out[2].dtype == pair[1]
        ref = reference64_mix(base, t[1], t[4], q, mix)
        check_losses(out[0], ref.loss5, what)
        near = check_gradient(out[1], ref.dlogits, env.dlogits, what + " dlogits") + check_gradient(out[2], ref.dvalue, None, what + " dvalue")
        assert near < LC.NEAR_SHARE * (ref.dlogits.numel() + ref.dvalue.numel()), f"{what}: {near} elements at the overflow threshold"
        if again:
            twice = run_loss_mix(*t, q, mix, w3)
            assert all(LC.same_bits(a, b) for a, b in zip(out, twice)), what + ": a second call differs"
    if w3 == case.w3:
        return
    base = LC.reference64(*t, case.w3)   # the pair again at the case's own scale: the relative conditions (module docstring)
    env = LC.envelope(base)
    for mix in mixes:
        what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} mix {mix} at scale {max(abs(w) for w in case.w3):g}"
        out = run_loss_mix(*t, q, mix, case.w3)
        ref = reference64_mix(base, t[1], t[4], q, mix)
        wx, near_x = LC.check_output(out[1], ref.dlogits, env.dlogits, what + " dlogits")
        wv, near_v = LC.check_output(out[2], ref.dvalue, dvalue_envelope(ref) if out[2].dtype == F32 else torch.zeros_like(ref.dvalue),
                                     what + " dvalue")
        print(f"FIGURE {what} worst error / allowance dlogits {wx:.3f} dvalue {wv:.3f}")
        assert near_x + near_v < LC.NEAR_SHARE * (ref.dlogits.numel() + ref.dvalue.numel()), f"{what}: elements at the overflow threshold"


# ---- the raw calls on guarded buffers ------------------------------------------------------------------------------------------------

ROW_STATS_MIX = 6
GUARD_CASES = (("B1_W1_randn3_prefix", (0.5,)), ("B65_W2_dom60_first_full", (0.5, 0.0)), ("B65_W63_dom90_last_empty_rows", (0.5,)))


def raw_forward_backward_mix(logits, value, idx, val, z, q, mix, w3, guard=64):
    """bo_train_loss_forward_mix / bo_train_loss_backward_mix called directly, with row_stats [n + guard, 6], dlogits and dvalue
    allocated `guard` rows longer than the batch and pre-filled with the NaN payload (LC.raw_forward_backward for the mix entry
    points).  Returns (row_stats, loss5, dlogits, dvalue), the three with their guard rows."""
    from betaone_amd import engine as E
    from betaone_amd.train import DTYPE_CODES

    lib = E.load_hip_library()
    dev = logits.device
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    n, W = idx.shape
    logits, value, z, q = logits.contiguous(), value.contiguous().reshape(-1), z.contiguous().reshape(-1), q.contiguous().reshape(-1)
    row_stats = LC.guarded(n, ROW_STATS_MIX, F32, dev, guard)
    dlogits, dvalue = LC.guarded(n, LC.A, logits.dtype, dev, guard), LC.guarded(n, 1, value.dtype, dev, guard)
    loss5 = torch.empty(5, dtype=F32, device=dev)
    g3, m = torch.tensor(w3, dtype=F32, device=dev), torch.tensor([mix], dtype=F32, device=dev)
    args = (n, W, logits.data_ptr(), DTYPE_CODES[logits.dtype], value.data_ptr(), DTYPE_CODES[value.dtype], idx.data_ptr(), val.data_ptr(),
            z.data_ptr(), q.data_ptr(), m.data_ptr(), row_stats.data_ptr())
    rc = lib.bo_train_loss_forward_mix(*args, loss5.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    rc = lib.bo_train_loss_backward_mix(*args, g3.data_ptr(), dlogits.data_ptr(), dvalue.data_ptr(), stream)
    assert rc == 0, lib.bo_last_error().decode()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return row_stats, loss5, dlogits, dvalue


def check_guard_rows_mix(case, pair, device, mix):
    """LC.check_guard_rows for the mix entry points: the guard rows keep their pattern, no payload is left below row B in any of the
    six columns of row_stats (a stride of 4 leaves some and runs short; a stride of 6 in the plain kernels would write past them) nor in
    dlogits and dvalue, and the results are reference64_mix's.  The row terms: the policy term within LC's envelope; the three value
    terms d^2 with d = v - t, v - z, v - q within FACTOR allowances of eps (4 d^2 + 4 |d| T) + 2^-126 -- 4 eps d^2 is LC's allowance for
    (v - z)^2, and the target's own error of 2 eps T (dvalue_envelope, module docstring; T = 0 for a target that is given) reaches d^2
    times 2 |d|.  The losses and the gradients by the conditions of check_loss_case; the three cases' w3 have no scale."""
    t = LC.cast(case, pair, device)
    q = root_values_for(case).to(device)
    assert weights_for(case, pair) == case.w3
    row_stats, loss5, dlogits, dvalue = raw_forward_backward_mix(*t, q, mix, case.w3)
    B = case.B
    what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} mix {mix} guard rows"
    assert tuple(row_stats.shape) == (B + 64, ROW_STATS_MIX)
    for name, buf in (("row_stats", row_stats), ("dlogits", dlogits), ("dvalue", dvalue)):
        assert LC.guard_intact(buf, B), f"{what}: {name} written past row {B}"
        bits = buf[:B].view(torch.int32) if buf.dtype == F32 else buf[:B].view(torch.int16)
        left = bits == (LC.NAN32 if buf.dtype == F32 else LC.NAN16)
        assert not bool(left.any()), f"{what}: {name} has unwritten elements in columns {sorted(set(torch.nonzero(left)[:, 1].tolist()))[:8]}"
    base = LC.reference64(*t, case.w3)
    env = LC.envelope(base)
    ref = reference64_mix(base, t[1], t[4], q, mix)
    LC.check_output(row_stats[:B, 2], base.row_policy, env.row_policy, what + " row policy terms")
    v, zz, qq = (x.detach().cpu().double().reshape(-1) for x in (t[1], t[4], q))
    for col, target, T in ((3, ref.t, ref.T), (4, zz, 0.0), (5, qq, 0.0)):
        d = v - target
        LC.check_output(row_stats[:B, col], d * d, LC.EPS * (4.0 * d * d + 4.0 * d.abs() * T) + LC.TINY, f"{what} row value terms, column {col}")
    check_losses(loss5, ref.loss5, what)
    near = (check_gradient(dlogits[:B], ref.dlogits, env.dlogits, what + " dlogits")
            + check_gradient(dvalue[:B].reshape(-1), ref.dvalue, None, what + " dvalue"))
    assert near < LC.NEAR_SHARE * (ref.dlogits.numel() + ref.dvalue.numel()), f"{what}: {near} elements at the overflow threshold"


# ---- mix 0, invalid mixes, the point of view ---------------------------------------------------------------------------------------

def hard_inputs(case, device, pair):
    """The case with z = -0.0 in some rows (one of them under value = -0.0, where t = +0.0 would flip the sign of dvalue) and
    q = NaN in every third row."""
    c = SimpleNamespace(**vars(case))
    c.z, c.value = case.z.clone(), case.value.clone()
    B = case.B
    for b in range(0, B, 4):
        c.z[b, 0] = -0.0
    c.value[0, 0] = -0.0
    if B > 4:
        c.value[4, 0] = 0.0
    q = root_values_for(case)
    q[::3] = float("nan")
    return LC.cast(c, pair, device), q.to(device)


def check_mix0(case, pair, device):
    """Mix 0 against the existing entry points, bit for bit: loss5[0:3], dlogits, dvalue.  A NaN q reaches value_vs_q and nothing
    else; value_vs_z is the value loss.  The mix as a Python float, as -0.0 and as a device tensor."""
    t, q = hard_inputs(case, device, pair)
    what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} mix 0"
    assert bool((t[4].view(torch.int32) == -2 ** 31).any()) and bool(torch.isnan(q).any())
    old = LC.run_loss(*t, case.w3)
    for mix in (0.0, -0.0, torch.zeros(1, device=device)):
        new = run_loss_mix(*t, q, mix, case.w3)
        assert LC.same_bits(new[0][:3], old[0]), f"{what}: loss5[0:3] {new[0][:3].tolist()} against {old[0].tolist()}"
        assert LC.same_bits(new[1], old[1]), what + ": dlogits differ"
        assert LC.same_bits(new[2], old[2]), what + ": dvalue differs"
        assert LC.same_bits(new[0][3:4], old[0][2:3]), what + ": value_vs_z is not the value loss"
        assert bool(torch.isnan(new[0][4])), what + ": value_vs_q of a NaN q"
    finite_q = torch.nan_to_num(q, nan=0.25)
    new = run_loss_mix(*t, finite_q, 0.0, case.w3)
    assert LC.same_bits(new[0][:3], old[0]) and LC.same_bits(new[2], old[2]) and bool(torch.isfinite(new[0][4])), what
    return old, new


def check_invalid_mix(case, pair, device):
    """Mixes 1.5, -0.1 and NaN: every loss NaN, dvalue NaN, dlogits the valid call's (nothing is clamped: a clamp would give the
    losses of mix 1 or 0)."""
    t = LC.cast(case, pair, device)
    q = root_values_for(case).to(device)
    good = run_loss_mix(*t, q, 1.0, case.w3)
    assert bool(torch.isfinite(good[0]).all())
    for mix in INVALID_MIXES:
        for m in (mix, torch.tensor([mix], dtype=F32, device=device)):
            out = run_loss_mix(*t, q, m, case.w3)
            what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])} mix {mix}"
            assert bool(torch.isnan(out[0]).all()), f"{what}: losses {out[0].tolist()}"
            assert bool(torch.isnan(out[2].float()).all()), what + ": dvalue"
            assert LC.same_bits(out[1], good[1]), what + ": dlogits"


def check_perspective(device):
    """z and q of a record are both from the point of view of the side to move at the record's position, and the target mixes them
    as they are.  In the game white won, with root values that say so, z and q have the same sign in every record, black to move
    included; a value head that outputs 0.5 z + 0.5 q computed here from the records, with no flip anywhere, has value_mix exactly 0 and
    a zero dvalue at mix 0.5 (every term is exact in float32), and would not with a flipped q."""
    from betaone_amd import records as R

    games = fake_games(2)
    buf = R.GpuReplayBuffer(1024, device=device, pi_width=2)
    try:
        buf.add(games)
        n0 = int(games[0]["n_plies"])
        s, i, v, z, q = buf.batch_sparse_q(np.arange(n0))
        turn = np.array([games[0]["positions"][k].turn for k in range(n0)])
        zz, qq = z.cpu().numpy().reshape(-1), q.cpu().numpy().reshape(-1)
        assert set(turn.tolist()) == {0, 1}
        assert bool((zz[turn == 1] == 1.0).all()) and bool((zz[turn == 0] == -1.0).all())
        assert bool((qq[turn == 1] > 0).all()) and bool((qq[turn == 0] < 0).all())
        g = torch.Generator().manual_seed(3)
        logits = (torch.randn((n0, LC.A), generator=g) * 3.0).to(device)
        for flip, zero in ((1.0, True), (-1.0, False)):
            value = (0.5 * z + 0.5 * flip * q).clone()
            loss5, _, dv = run_loss_mix(logits, value, i, v, z, q, 0.5, UNIT_W3)
            assert (float(loss5[2]) == 0.0 and float(dv.abs().max()) == 0.0) == zero, (flip, float(loss5[2]))
            assert float(loss5[3]) > 0.0 and float(loss5[4]) > 0.0
    finally:
        buf.close()


# ---- the command and a training run -----------------------------------------------------------------------------------------------

def tiny_init(path):
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 0, 16
    try:
        torch.manual_seed(0)
        torch.save(network.PolicyValueNet().state_dict(), path)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def _repack(games):
    from betaone_amd import records as R

    return [R.pack_game(SimpleNamespace(game_id=g["game_id"], pis=g["pis"], positions=list(g["positions"]), moves=list(g["moves"]),
                                        terminal=g["terminal"], outcome=g["outcome"],
                                        **({} if g["root_values"] is None else {"root_values": g["root_values"]}))) for g in games]


def check_command(device, tmp_path, extra=()):
    """python -m betaone_amd.train --value-mix: a checkpoint that loads and the new JSON fields on BOG2 games; the refusal on BOG1-only
    data, with nothing written; the refusal together with --dense-loss."""
    from betaone_amd import match as M
    from betaone_amd import records as R
    from betaone_amd import train as T

    with_values = fake_games(6, values=lambda g: g != 5)
    n_valued = sum(int(g["n_plies"]) for g in with_values if g["root_values"] is not None)
    data, save = str(tmp_path / "data"), str(tmp_path / "ck")
    R.save_games(R.compact_path(data, 0), _repack(with_values), append=False)
    init, cand, out = str(tmp_path / "init.pth"), str(tmp_path / "cand.pth"), str(tmp_path / "train.json")
    tiny_init(init)
    common = ["--data-dir", data, "--init", init, "--epochs", "2", "--batch", "16", "--steps-per-epoch", "3", "--device", device, *extra]
    assert T.main(common + ["--save-dir", save, "--iteration", "0", "--value-mix", "0.5", "--candidate", cand, "--out", out]) == 0
    M.build_net(M.load_state_dict(cand))
    ck = torch.load(os.path.join(save, "checkpoint_iter_0.pth"), map_location="cpu")
    M.build_net(ck["model_state_dict"])
    assert not os.path.exists(os.path.join(save, "best_model.pth"))
    summary = json.load(open(out))
    assert summary["value_mix"] == 0.5 and len(summary["epochs"]) == 2
    for e in summary["epochs"]:
        assert e["records_with_values"] == n_valued and e["steps"] == 3
        assert np.isfinite(e["value_vs_z"]) and np.isfinite(e["value_vs_q"]) and e["value_vs_z"] > 0 and e["value_vs_q"] > 0
        assert e["value_vs_z"] != e["value_vs_q"] and np.isfinite(e["value_loss"])
    # BOG1 only
    data1, save1 = str(tmp_path / "data1"), str(tmp_path / "ck1")
    R.save_games(R.compact_path(data1, 0), _repack(fake_games(4, values=lambda g: False)), append=False)
    cand1, out1 = str(tmp_path / "cand1.pth"), str(tmp_path / "train1.json")
    common1 = ["--data-dir", data1, "--save-dir", save1, "--init", init, "--epochs", "1", "--batch", "16", "--steps-per-epoch", "2",
               "--device", device, "--iteration", "0", "--candidate", cand1, "--out", out1, *extra]
    with pytest.raises(SystemExit) as ex:
        T.main(common1 + ["--value-mix", "0.5"])
    assert MESSAGE in str(ex.value.code)
    assert not os.path.exists(save1) and not os.path.exists(cand1) and not os.path.exists(out1)
    with pytest.raises(SystemExit) as ex:   # the argument parser
        T.main(common + ["--save-dir", save1, "--iteration", "0", "--value-mix", "0.5", "--dense-loss"])
    assert ex.value.code == 2 and not os.path.exists(save1)
    # the default trains those games as before, and says what it did
    assert T.main(common1) == 0
    e = json.load(open(out1))["epochs"][0]
    assert e["records_with_values"] == 0 and e["value_vs_q"] is None and e["value_vs_z"] == e["value_loss"]


def check_training(device, tmp_path, steps=100):
    """Games whose root value is one constant per game that differs from z; `steps` steps (the count of test_training_lowers_the_loss
    in tests/test_train_emu.py) on one fixed batch at mix 1: value_vs_q ends below its first-step value."""
    from betaone_amd import match as M
    from betaone_amd import records as R
    from betaone_amd import train as T

    games = fake_games(6, values=lambda g: True, const_q=lambda g: (0.375, -0.625, 0.25, -0.125, 0.5, -0.75)[g])
    z, q, _ = stored(games)
    assert bool((z != q).all())
    torch.manual_seed(1)
    buf = R.GpuReplayBuffer(4096, device=device, pi_width=2)
    try:
        buf.add(games)
        fixed = buf.batch_sparse_q(np.arange(32))
        tiny_init(str(tmp_path / "i.pth"))
        model = M.build_net(M.load_state_dict(str(tmp_path / "i.pth")), device)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000, eta_min=5e-7)
        scaler = torch.GradScaler(torch.device(device).type, enabled=False)
        r = T.train_steps(model, opt, sched, scaler, [fixed] * steps, amp=False, value_mix=1.0)
        d = r["diagnostics"]
        assert r["steps"] == steps and len(d) == steps
        print(f"FIGURE value_vs_q first {d[0][1]:.4f} last {d[-1][1]:.4f}; value_vs_z first {d[0][0]:.4f} last {d[-1][0]:.4f}")
        assert d[-1][1] < d[0][1], (d[0], d[-1])
        assert [x[2] for x in r["losses"]] == [x[1] for x in d]       # at mix 1 the value loss IS value_vs_q
        # mix 0 takes four-tuples through sparse_policy_value_loss, as before
        r0 = T.train_steps(model, opt, sched, scaler, [fixed[:4]] * 2, amp=False, value_mix=0.0)
        assert r0["steps"] == 2 and "diagnostics" not in r0
        # a mix with four-tuples is refused in words, a tensor holding 0 included (its value is read on the device, not here)
        for mix in (0.5, torch.zeros(1, device=device)):
            with pytest.raises(ValueError, match="with_q=True"):
                T.train_steps(model, opt, sched, scaler, [fixed[:4]], amp=False, value_mix=mix)
    finally:
        buf.close()
