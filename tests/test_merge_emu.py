"""CPU tests (wave emulator) of the replay buffer's merged targets: bo_k_replay_group, bo_k_replay_merge and bo_k_replay_encode_merged
through GpuReplayBuffer.merge_duplicates / batch_merged / loader(merged=...) and `python -m betaone_amd.train --merge-duplicates`.
The bodies are tests/merge_cases.py's; the contention case runs 96 copies here and 2 048 on the GPU (tests/test_merge_gpu.py)."""
import engine_harness as H
import merge_cases as MC


def test_the_partition_is_the_planes_partition_and_the_means_are_exact():
    with H.emulator_backend():
        by_input, by_position = MC.check_families("cpu")
        assert by_input > by_position > 100


def test_no_duplicates_no_difference():
    with H.emulator_backend():
        MC.check_no_duplicates("cpu")


def test_index_and_hold_out():
    with H.emulator_backend():
        MC.check_holdout("cpu")


def test_probing_one_position_under_many_histories():
    with H.emulator_backend():
        assert MC.check_probing("cpu") >= 64


def test_contention_on_twelve_groups():
    with H.emulator_backend():
        assert MC.check_contention("cpu", copies=96) == 12 * 96


def test_a_merge_follows_the_ring_and_goes_stale_with_it():
    with H.emulator_backend():
        assert MC.check_wrap_around("cpu") > 0


def test_refusals():
    with H.emulator_backend():
        MC.check_refusals("cpu")


def test_a_union_above_the_cap_is_refused_by_name():
    with H.emulator_backend():
        MC.check_wide_union("cpu")


def test_train_command_with_merged_targets(tmp_path):
    with H.emulator_backend():
        MC.check_command("cpu", tmp_path, extra=("--no-amp",))


def test_train_command_without_duplicates_writes_the_same_weights(tmp_path):
    with H.emulator_backend():
        MC.check_command_without_duplicates("cpu", tmp_path, extra=("--no-amp",))
