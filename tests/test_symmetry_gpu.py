"""GPU tests on the MI355X of the board symmetries in the replay samplers: the bodies of tests/symmetry_cases.py through
libbetaone_hip.so -- every record of a dozen games under the colour flip, the file mirror and both against the transformed game played
out by the CPU chess rules, for all four samplers; the loader's second generator; merged targets; refusals; the two commands; and the
consistency figures of two nets with a known answer."""
import pytest

import symmetry_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_colour_flip_is_the_flipped_game():
    assert SC.check_colour(DEV) > 200


def test_file_mirror_is_the_mirrored_game_where_no_castling_right_is_left():
    assert SC.check_mirror(DEV) > 100


def test_both_at_once():
    SC.check_both(DEV)


def test_nothing_changes_when_off():
    SC.check_off(DEV)


def test_merged_targets_are_transformed_on_the_way_out():
    assert SC.check_merged(DEV) > 60


def test_refusals_and_odd_batch_sizes():
    SC.check_refusals(DEV)


def test_one_staging_block_under_calls_of_every_shape():
    SC.check_staging(DEV)


def test_train_command_with_augment(tmp_path):
    SC.check_train_command(DEV, tmp_path)


def test_validate_command_with_symmetry(tmp_path):
    SC.check_validate_command(DEV, tmp_path)


def test_consistency_of_nets_with_a_known_answer():
    SC.check_consistency(DEV)
