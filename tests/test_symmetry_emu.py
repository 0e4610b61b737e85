"""CPU tests (wave emulator) of the board symmetries in the replay samplers: csrc/bo_sym.h and the _sym variants of the four samplers
through GpuReplayBuffer.batch*(sym=...), loader(augment=...), `python -m betaone_amd.train --augment`, `python -m betaone_amd.validate
--symmetry` and validate.symmetry_consistency.  The bodies are tests/symmetry_cases.py's; the oracle is the transformed game played
out by the CPU chess rules."""
import engine_harness as H
import symmetry_cases as SC


def test_the_corpus_has_every_property_and_the_table_is_the_codec():
    SC.check_corpus()
    SC.check_tables()


def test_colour_flip_is_the_flipped_game():
    with H.emulator_backend():
        assert SC.check_colour("cpu") > 200


def test_file_mirror_is_the_mirrored_game_where_no_castling_right_is_left():
    with H.emulator_backend():
        assert SC.check_mirror("cpu") > 100


def test_both_at_once():
    with H.emulator_backend():
        SC.check_both("cpu")


def test_nothing_changes_when_off():
    with H.emulator_backend():
        SC.check_off("cpu")


def test_merged_targets_are_transformed_on_the_way_out():
    with H.emulator_backend():
        assert SC.check_merged("cpu") > 60


def test_refusals_and_odd_batch_sizes():
    with H.emulator_backend():
        SC.check_refusals("cpu")


def test_one_staging_block_under_calls_of_every_shape():
    with H.emulator_backend():
        SC.check_staging("cpu")


def test_train_command_with_augment(tmp_path):
    with H.emulator_backend():
        SC.check_train_command("cpu", tmp_path, extra=("--no-amp",))


def test_validate_command_with_symmetry(tmp_path):
    with H.emulator_backend():
        SC.check_validate_command("cpu", tmp_path, extra=("--no-amp",))


def test_consistency_of_nets_with_a_known_answer():
    with H.emulator_backend():
        SC.check_consistency("cpu")
