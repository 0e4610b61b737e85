"""GPU tests on the MI355X of the value head trained on a mix of the game's outcome and the search's root value: the bodies of
tests/value_mix_cases.py through libbetaone_hip.so -- the sampler with root values, the mixed loss kernels against float64 on every
case of tests/loss_cases.py and every dtype pair (fp16 included), mix 0 against the existing entry points bit for bit, invalid mixes,
and `python -m betaone_amd.train --value-mix` under autocast."""
import pytest
import torch

import loss_cases as LC
import value_mix_cases as VM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = LC.cases()
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def _by_name(name):
    return next(c for c in CASES if c.name == name)


def test_sampler_returns_the_stored_root_values_across_wrap_around():
    assert VM.check_sampler(DEV) > 0


def test_z_and_q_share_the_side_to_move_s_point_of_view():
    VM.check_perspective(DEV)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_mixed_loss_against_float64(case):
    """Mixes 0.25, 0.5 and 1 on every case and dtype pair: all five losses and both gradients; a second call bit for bit."""
    for pair in LC.PAIRS:
        VM.check_loss_case(case, pair, DEV, again=True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_mix_0_is_the_existing_loss_bit_for_bit(case):
    for pair in ((F32, F32), (F16, F16), (BF16, F32), (F16, BF16)):
        VM.check_mix0(case, pair, DEV)


@pytest.mark.parametrize("case", LC.nonfinite_cases(), ids=lambda c: c.name)
def test_mix_0_with_non_finite_logits(case):
    for pair in ((F32, F32), (F16, F16), (BF16, F32)):
        VM.check_mix0(case, pair, DEV)


@pytest.mark.parametrize("name", ["B63_W32_dom90_edges", "B4097_W2_pos80_edges"])
def test_invalid_mixes_give_nan_losses(name):
    for pair in ((F32, F32), (F16, F16), (BF16, F32)):
        VM.check_invalid_mix(_by_name(name), pair, DEV)


@pytest.mark.parametrize("name,mixes", VM.GUARD_CASES, ids=[c[0] for c in VM.GUARD_CASES])
def test_mix_kernels_write_no_row_past_the_batch(name, mixes):
    for pair in LC.PAIRS if len(mixes) > 1 else ((F16, F16),):   # (every dtype pair on the case that also runs mix 0)
        for mix in mixes:
            VM.check_guard_rows_mix(_by_name(name), pair, DEV, mix)


def test_the_mix_is_read_on_the_device_when_the_kernels_run():
    """One device tensor, changed in place between calls (what a schedule does under a captured step): each call sees its value."""
    case = _by_name("B65_W2_dom60_first_full")
    t = LC.cast(case, (F32, F32), DEV)
    q = VM.root_values_for(case).to(DEV)
    mix = torch.zeros(1, device=DEV)
    for a in (0.25, 1.0, 0.5):
        mix.fill_(a)
        got = VM.run_loss_mix(*t, q, mix, case.w3)
        want = VM.run_loss_mix(*t, q, a, case.w3)
        assert all(LC.same_bits(x, y) for x, y in zip(got, want)), a


def test_train_command_with_a_value_mix(tmp_path):
    VM.check_command(DEV, tmp_path)


def test_training_at_mix_1_moves_the_value_head_towards_q(tmp_path):
    VM.check_training(DEV, tmp_path)
