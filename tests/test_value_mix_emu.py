"""CPU tests (wave emulator) of the value head trained on a mix of the game's outcome and the search's root value: the replay buffer's
root values and bo_replay_sample_sparse_q, the loss kernels bo_train_loss_forward_mix / _backward_mix against float64, mix 0 against
the existing entry points bit for bit, invalid mixes, and `python -m betaone_amd.train --value-mix`.  The bodies are
tests/value_mix_cases.py's; the emulator's host compiler has no _Float16, so the float32 and bf16 instances run here and the GPU runs
every dtype pair (tests/test_value_mix_gpu.py)."""
import pytest
import torch

import engine_harness as H
import loss_cases as LC
import value_mix_cases as VM

CASES = LC.cases()
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
PAIRS = tuple(p for p in LC.PAIRS if F16 not in p)
BIG_PAIRS = {1000: ((BF16, F32),), 4097: ((F32, F32),)}  # (the emulator runs one wave at a time)


def _by_name(name):
    return next(c for c in CASES if c.name == name)


def test_sampler_returns_the_stored_root_values_across_wrap_around():
    with H.emulator_backend():
        assert VM.check_sampler("cpu") > 0


def test_z_and_q_share_the_side_to_move_s_point_of_view():
    with H.emulator_backend():
        VM.check_perspective("cpu")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_mixed_loss_against_float64(case):
    """Mixes 0.25, 0.5 and 1 on every case: all five losses and both gradients; a second call bit for bit on the first pair."""
    pairs = PAIRS if case.B <= 128 else BIG_PAIRS[case.B]
    with H.emulator_backend():
        for k, pair in enumerate(pairs):
            VM.check_loss_case(case, pair, "cpu", again=k == 0 and case.B <= 1000)


@pytest.mark.parametrize("name", ["B1_W1_randn3_prefix", "B2_W2_flat_full", "B65_W63_dom90_last_empty_rows", "B128_W2_flat_prefix",
                                  "invalid_wide", "scale_2p16_dominant"])
def test_mix_0_is_the_existing_loss_bit_for_bit(name):
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, BF16), (BF16, F32)):
            VM.check_mix0(_by_name(name), pair, "cpu")


@pytest.mark.parametrize("case", LC.nonfinite_cases(), ids=lambda c: c.name)
def test_mix_0_with_non_finite_logits(case):
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, BF16)):
            VM.check_mix0(case, pair, "cpu")


def test_invalid_mixes_give_nan_losses():
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, F32)):
            VM.check_invalid_mix(_by_name("B63_W32_dom90_edges"), pair, "cpu")


@pytest.mark.parametrize("name,mixes", VM.GUARD_CASES, ids=[c[0] for c in VM.GUARD_CASES])
def test_mix_kernels_write_no_row_past_the_batch(name, mixes):
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, F32)):
            for mix in mixes:
                VM.check_guard_rows_mix(_by_name(name), pair, "cpu", mix)


def test_bad_arguments_are_refused():
    from betaone_amd.train import sparse_policy_value_loss_mix

    with H.emulator_backend():
        case = _by_name("B2_W2_flat_full")
        logits, value, idx, val, z = LC.cast(case, (F32, F32))
        q = VM.root_values_for(case)
        with pytest.raises(ValueError):
            sparse_policy_value_loss_mix(logits, value, idx, val, z, q[:1], 0.5)
        with pytest.raises(ValueError):
            sparse_policy_value_loss_mix(logits, value, idx, val, z, q, torch.zeros(2))
        with pytest.raises(TypeError):
            sparse_policy_value_loss_mix(logits, value, idx, val, z, q.double(), 0.5)
        from betaone_amd import engine as E

        lib = E.load_hip_library()
        st, l5, m = torch.empty(12), torch.empty(5), torch.zeros(1)
        args = (2, 2, logits.data_ptr(), 0, value.data_ptr(), 0, idx.data_ptr(), val.data_ptr(), z.data_ptr())
        assert lib.bo_train_loss_forward_mix(*args, None, m.data_ptr(), st.data_ptr(), l5.data_ptr(), None) == -1
        assert lib.bo_train_loss_forward_mix(*args, q.data_ptr(), None, st.data_ptr(), l5.data_ptr(), None) == -1
        assert lib.bo_train_loss_forward_mix(2, 2, logits.data_ptr(), 7, *args[4:], q.data_ptr(), m.data_ptr(), st.data_ptr(), l5.data_ptr(), None) == -3
        assert lib.bo_train_loss_backward_mix(*args, q.data_ptr(), None, st.data_ptr(), l5.data_ptr(), logits.data_ptr(), value.data_ptr(), None) == -1


def test_train_command_with_a_value_mix(tmp_path):
    with H.emulator_backend():
        VM.check_command("cpu", tmp_path, extra=("--no-amp",))


def test_training_at_mix_1_moves_the_value_head_towards_q(tmp_path):
    with H.emulator_backend():
        VM.check_training("cpu", tmp_path)
