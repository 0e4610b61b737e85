"""GPU tests (MI355X) of the endgame tablebases inside the search and at the root, with the real KQK / KRK / KPK tables built on the
device: the bodies of tb_search_cases.py (shared with the wave-emulator tests), adjudication on the host-made turn and on the device
turn with a captured graph and two cohorts."""
import pytest

import tb_search_cases as C

pytestmark = pytest.mark.gpu


def test_tree_invariants_node_by_node():
    C.check_tree_invariants("hip")


def test_off_means_off():
    C.check_off_means_off("hip")


def test_oracle_parity_with_tables_attached_and_both_flags_on():
    C.check_oracle_parity_with_tables_attached("hip")


def test_adjudication_equals_rescore_on_the_host_made_turn(tmp_path):
    C.check_adjudication_equals_rescore("hip", tmp_path, cohorts=1, device_turn=False, max_game_moves=12)


def test_adjudication_equals_rescore_on_the_device_turn_with_graphs_and_two_cohorts(tmp_path):
    C.check_adjudication_equals_rescore("hip", tmp_path, cohorts=2, device_turn=True, max_game_moves=12)


def test_both_flags_together():
    C.check_both_flags("hip")


def test_refusals():
    C.check_refusals("hip")


def test_match_scores_an_adjudicated_game_as_a_loss_for_the_side_to_move():
    C.check_match_scores_an_adjudicated_game("hip")
