"""CPU tests of tests/loss_cases.py and, through it, of the sparse-target loss kernels (csrc/bo_train.h) and the sparse replay sampler
(csrc/bo_replay.h) under the wave emulator: the float64 reference against float64 autograd, PyTorch's float32 path inside ONE envelope,
every case of the list against the reference (the emulator build has no _Float16: dtype pairs with fp16 are skipped, and exactly
those), bit-reproducibility, the non-finite rows, guard rows, row independence and the samplers at wide rows.  The GPU runs the same
bodies on every dtype pair (tests/test_train_gpu.py)."""
import pytest
import torch

import engine_harness as H
import loss_cases as LC
from fake_model import FakeNet

CASES = LC.cases()
NONFINITE = LC.nonfinite_cases()
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BIG_PAIRS = {1000: ((BF16, F32),), 4097: ((F32, F32),)}  # (the emulator runs one wave at a time)


def _by_name(name):
    return next(c for c in CASES if c.name == name)


def test_the_list_has_what_it_promises():
    assert {c.B for c in CASES} >= {1, 2, 63, 64, 65, 127, 128, 1000, 4097}
    assert {c.W for c in CASES} >= {1, 2, 32, 63, 64, 65, 130}
    for B in (1, 2, 63, 64, 65, 127, 128, 1000, 4097):
        ws = {c.W for c in CASES if c.B == B}
        assert min(ws) <= 32 and max(ws) >= 63, B
    for W in (1, 2, 32, 63, 64, 65, 130):
        bs = {c.B for c in CASES if c.W == W}
        assert min(bs) <= 65 and max(bs) >= 127, W
    assert {c.kind for c in CASES} == set(LC.LOGITS) and {c.placement for c in CASES} == set(LC.PLACEMENTS) | {"all_empty"}
    assert {c.w3 for c in CASES} >= set(LC.W3)
    hit, invalid = set(), set()
    for c in CASES:
        ok = LC.valid(c.idx)
        for b in range(min(c.B, 200)):  # no action twice in a row
            row = c.idx[b][ok[b]]
            assert row.unique().numel() == row.numel(), (c.name, b)
        hit |= set(c.idx[ok].unique().tolist()) & set(LC.EDGE_ACTIONS)
        invalid |= set(c.idx[~ok].unique().tolist())
        assert bool((c.val[ok] >= 0).all())
    assert hit == set(LC.EDGE_ACTIONS) and invalid == set(LC.INVALID) | {-1}
    scattered = _by_name("B64_W130_f16max_scattered")
    assert bool(((scattered.idx[:, :-1] < 0) & (scattered.idx[:, 1:] >= 0)).any())  # gaps of -1 before valid entries
    assert bool(LC.valid(_by_name("B2_W2_flat_full").idx).all()) and not bool(LC.valid(_by_name("all_rows_empty").idx).any())
    e = _by_name("B65_W63_dom90_last_empty_rows")
    assert [int(LC.valid(e.idx[b]).sum()) for b in (0, 32, 64)] == [0, 0, 0] and int(LC.valid(e.idx[1]).sum()) > 0
    tiny = _by_name("invalid_wide")
    assert 0 < float(tiny.val[tiny.val > 0].min()) < 1e-29
    sums = torch.where(LC.valid(tiny.idx), tiny.val, torch.zeros(())).sum(1)
    assert all(abs(float(sums[b]) / s - 1) < 1e-5 for b, s in enumerate(LC.ROW_SUMS))
    d = _by_name("edges_on_dominant_first")  # the dominant logit on lane 0 / register 0, and a target on it
    assert bool((d.logits.argmax(1) == 0).all()) and bool((d.idx == 0).any())
    assert bool((_by_name("edges_on_dominant_last").logits.argmax(1) == LC.A - 1).all())
    f = _by_name("edges_f16max")
    assert float(f.logits[0].max()) == 65504.0 and float(f.logits[0].min()) == -65504.0 and bool(torch.isfinite(f.logits.half()).all())
    for c in CASES:
        assert [float(c.value[b]) for b in range(min(c.B, 2))] == [1.0, -1.0][:min(c.B, 2)] and set(c.z.reshape(-1).tolist()) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference64_against_float64_autograd_and_torch_float32_inside_one_envelope(case):
    """reference64 to 1e-12 of torch.autograd of F.cross_entropy + F.mse_loss in float64 (relative to the magnitudes of the terms: the
    two ways cancel differently at a target entry), and PyTorch's float32 path within ONE envelope of it (with the allowance for
    its sum of the exponentials, LC.TORCH_SUM_C), element by element -- for the float32 inputs and, up to B = 65, for the fp16 and
    bf16 ones widened."""
    for dt in LC.DTYPES if case.B <= 65 else (F32,):
        t = LC.cast(case, (dt, dt))
        ref = LC.reference64(*t, case.w3)
        env = LC.envelope(ref, LC.TORCH_SUM_C)
        l64, gx64, gv64 = LC.autograd64(*t, case.w3)
        B = case.B
        assert bool(((ref.loss3 - l64).abs() <= 1e-12 * l64.abs()).all()), (ref.loss3, l64)
        assert bool(((ref.dlogits - gx64).abs() <= 1e-12 * (ref.S[:, None] * ref.p + ref.t) * abs(ref.gp) / B).all())
        assert bool(((ref.dvalue - gv64).abs() <= 1e-12 * gv64.abs()).all())
        l32, gx32, gv32 = LC.torch32(*t, case.w3)
        for name, got, want, allow in (("loss3", l32, ref.loss3, env.loss3), ("dlogits", gx32, ref.dlogits, env.dlogits),
                                       ("dvalue", gv32, ref.dvalue, env.dvalue)):
            ratio = (got.double() - want).abs() / allow
            assert bool((ratio <= 1.0).all()), f"{case.name} {LC.short(dt)} {name}: PyTorch float32 at {float(ratio.max()):.3g} envelopes"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=LC.short)
def test_the_rounded_reference_passes_the_16_bit_rule(dtype):
    """The float64 reference rounded to the output type meets the 16-bit condition in every case (so the w3 scales leave fewer than
    0.1 % of the elements at the overflow threshold), the overflow cases have inf and finite elements in fp16, and an element several ulp
    off, a lost inf and a spurious inf are each refused."""
    for case in CASES:
        if case.B > 128:
            continue
        t = LC.cast(case, (dtype, dtype))
        ref = LC.reference64(*t, case.w3)
        env = LC.envelope(ref)
        got = (ref.loss3.float(), ref.dlogits.to(dtype), ref.dvalue.to(dtype))
        LC.check_against_reference(got, ref, env, case.name)
        if case.name.startswith("overflow_fp16"):
            assert dtype != F16 or (bool(torch.isinf(got[1]).any()) and bool(torch.isfinite(got[1]).any()))
            assert dtype != BF16 or bool(torch.isfinite(got[1]).all())
    case = _by_name("overflow_fp16")
    t = LC.cast(case, (dtype, dtype))
    ref = LC.reference64(*t, case.w3)
    env = LC.envelope(ref)
    good = ref.dlogits.to(dtype)
    wrongs = [(1, 5, float(good[1, 5]) * 1.05), (1, 5, float("inf"))]  # a non-target entry: several ulp off, a spurious inf
    if dtype == F16:
        b, a = (int(k) for k in torch.nonzero(torch.isinf(good))[0])
        wrongs.append((b, a, -65504.0))  # a lost inf
    for b, a, wrong in wrongs:
        bad = good.clone()
        bad[b, a] = wrong
        assert not LC.same_bits(bad, good)
        with pytest.raises(AssertionError):
            LC.check_output(bad, ref.dlogits, env.dlogits, "a wrong element")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=LC.short)
def test_the_16_bit_rule_holds_where_the_rounded_reference_is_zero(dtype):
    """Where round(reference) is 0 the ulp is the type's smallest denormal (2^-24, 2^-133), not that of a normal number: small values
    planted there are refused -- in a row under a dominant logit, in an empty row, and with a zero weight."""
    rows = (("B65_W63_dom90_last_empty_rows", 0), ("all_rows_empty", 2))
    if dtype == F16:  # (e^-60 / B is a normal number in bf16)
        rows += (("B65_W2_dom60_first_full", 7),)
    for name, b in rows:
        case = _by_name(name)
        t = LC.cast(case, (dtype, dtype))
        ref = LC.reference64(*t, case.w3)
        env = LC.envelope(ref)
        good = ref.dlogits.to(dtype)
        zero = torch.nonzero(good[b] == 0).reshape(-1)
        assert zero.numel() > 1000, name
        LC.check_output(good, ref.dlogits, env.dlogits, name)
        for wrong in (4e-4, -3e-3, 1e-6, 2.0 ** -20):
            bad = good.clone()
            bad[b, zero[17]] = wrong
            assert float(bad[b, zero[17]]) != 0
            with pytest.raises(AssertionError):
                LC.check_output(bad, ref.dlogits, env.dlogits, "a small value where the reference rounds to 0")
        bad = good.clone()
        bad[b, zero] = 4e-4
        with pytest.raises(AssertionError):
            LC.check_output(bad, ref.dlogits, env.dlogits, "small values in every element that rounds to 0")


def test_check_output_refuses_float32_errors():
    case = _by_name("B65_W2_dom60_first_full")
    t = LC.cast(case, (F32, F32))
    ref = LC.reference64(*t, case.w3)
    env = LC.envelope(ref)
    good = ref.dlogits.float()
    assert LC.check_output(good, ref.dlogits, env.dlogits, "rounded reference")[0] <= 1.0
    for b, a, wrong in ((7, 4671, 0.0), (7, 100, 1e-30), (0, 0, float("nan")), (64, 0, float(good[64, 0]) * (1 + 2e-4))):
        bad = good.clone()
        bad[b, a] = wrong
        with pytest.raises(AssertionError):
            LC.check_output(bad, ref.dlogits, env.dlogits, "a wrong element")


def _emu_pairs(case):
    return LC.PAIRS if case.B <= 128 else BIG_PAIRS[case.B]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_under_the_emulator(case):
    """sparse_policy_value_loss and its backward against reference64 with the module's conditions, and a second call
    bit for bit (the first dtype pair, up to B = 1000)."""
    skipped, worst = [], {}
    with H.emulator_backend():
        for pair in _emu_pairs(case):
            if F16 in pair:
                skipped.append(pair)
                continue
            t = LC.cast(case, pair)
            out = LC.run_loss(*t, case.w3)
            assert out[1].dtype == pair[0] and out[2].dtype == pair[1]
            ref = LC.reference64(*t, case.w3)
            r = LC.check_against_reference(out, ref, LC.envelope(ref), f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])}")
            worst[f"{LC.short(pair[0])}/{LC.short(pair[1])}"] = r
            if case.B > 1000 or pair != _emu_pairs(case)[0]:
                continue
            again = LC.run_loss(*t, case.w3)
            assert all(LC.same_bits(a, b) for a, b in zip(out, again)), f"{case.name}: a second call differs"
    assert skipped == [p for p in _emu_pairs(case) if F16 in p] and len(skipped) == (5 if case.B <= 128 else 0)
    print(f"RATIO emu {case.name} " + " ".join(f"{k} loss {r['loss']:.3f} dlogits {r['dlogits']:.3f} dvalue {r['dvalue']:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("case", NONFINITE, ids=lambda c: c.name)
def test_non_finite_rows_under_the_emulator(case):
    """Also PyTorch's float32 path on the dense target, which the header of bo_train.h names as the model: NaN total and policy (but
    +inf where the -inf logit is under a target entry: the kernel's NaN is the header's word, and kept), the whole row's gradient NaN
    for a NaN or +inf logit, and for a -inf logit the finite gradient of the reference, inside one envelope."""
    t = LC.cast(case, (F32, F32))
    l32, gx32, _ = LC.torch32(*t, case.w3)
    if case.bad == "neginf" and case.at_target:
        assert l32[:2].tolist() == [float("inf")] * 2
    else:
        assert bool(torch.isnan(l32[:2]).all())
    assert bool(torch.isfinite(l32[2]))
    if case.bad == "neginf":
        ref = LC.reference64(*t, case.w3)
        assert bool(((gx32.double() - ref.dlogits).abs() <= LC.envelope(ref, LC.TORCH_SUM_C).dlogits).all())
        assert float(ref.dlogits[case.row, case.action]) == (-ref.gp / 7 * float(case.val[case.row, 1]) if case.at_target else 0.0)
    else:
        assert bool(torch.isnan(gx32[case.row]).all())
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, BF16)):
            LC.check_nonfinite(case, pair, "cpu")


def test_guard_rows_and_row_independence_under_the_emulator():
    with H.emulator_backend():
        for name in ("B65_W2_dom60_first_full", "B65_W63_dom90_last_empty_rows", "invalid_wide"):
            for pair in ((F32, F32), (BF16, F32)):
                LC.check_guard_rows(_by_name(name), pair, "cpu")
                LC.check_row_independence(_by_name(name), pair, "cpu")


def test_the_entry_points_refuse_bad_arguments_in_their_words_under_the_emulator():
    with H.emulator_backend():
        assert LC.check_refusals("cpu") > 0


@pytest.fixture(scope="module")
def fake_games():
    """Finished self-play games of FakeNet on the emulator, as in tests/test_train_emu.py."""
    from betaone_amd.rollout import Rollout

    with H.emulator_backend():
        ro = Rollout(FakeNet(scale=2.0, salt=7), 4, num_simulations=24, mcts_batch_size=8, device="cpu", use_graph=False, rng_mode="native",
                     policy_kind="logits", max_game_moves=12)
        ro.start_games(list(range(4)), list(range(4)), [900 + g for g in range(4)])
        fins = []
        for _ in range(40):
            ro.play_ply(on_finished=fins.append)
            if len(fins) >= 4:
                break
        ro.close()
    assert len(fins) >= 3
    return fins


def test_res_cap_is_read_from_the_header():
    assert LC.res_cap() >= 130 and f"#define BO_RES_CAP {LC.res_cap()}\n" in open(H.ROOT + "/betaone_amd/csrc/bo_tree.h").read()


@pytest.mark.parametrize("W", [1, 64, 65, LC.res_cap()])
def test_replay_samplers_at_wide_rows_under_the_emulator(fake_games, W):
    with H.emulator_backend():
        r = LC.check_wide_replay(fake_games, W, "cpu", seed=11)
    print(f"RATIO emu replay W={W} f32/f32 loss {r['loss']:.3f} dlogits {r['dlogits']:.3f} dvalue {r['dvalue']:.3f}")
