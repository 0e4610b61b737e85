"""GPU tests on the MI355X of the replay buffer's merged targets: the bodies of tests/merge_cases.py through libbetaone_hip.so -- the
partition against the planes' bytes, the means against exact fractions, the sampler against batch_sparse_q, probing and table sizes,
2 048 copies of one game on twelve groups, the ring's life cycle, refusals, and `python -m betaone_amd.train --merge-duplicates`."""
import pytest

import merge_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_the_partition_is_the_planes_partition_and_the_means_are_exact():
    by_input, by_position = MC.check_families(DEV)
    assert by_input > by_position > 100


def test_no_duplicates_no_difference():
    MC.check_no_duplicates(DEV)


def test_index_and_hold_out():
    MC.check_holdout(DEV)


def test_probing_one_position_under_many_histories():
    assert MC.check_probing(DEV) >= 64


def test_contention_two_thousand_copies_on_twelve_groups():
    assert MC.check_contention(DEV, copies=2048) == 12 * 2048


def test_a_merge_follows_the_ring_and_goes_stale_with_it():
    assert MC.check_wrap_around(DEV) > 0


def test_refusals():
    MC.check_refusals(DEV)


def test_a_union_above_the_cap_is_refused_by_name():
    MC.check_wide_union(DEV)


def test_train_command_with_merged_targets(tmp_path):
    MC.check_command(DEV, tmp_path)


def test_train_command_without_duplicates_writes_the_same_weights(tmp_path):
    MC.check_command_without_duplicates(DEV, tmp_path)
