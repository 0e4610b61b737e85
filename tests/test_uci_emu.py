"""CPU tests of the interactive front end on the FAST search mode under the wave emulator: bo_search_info, bo_search_stop on fast-mode
engines (csrc/bo_info.h) and the UCI protocol of betaone_amd/uci.py -- the bodies of tests/uci_cases.py."""
import pytest

import uci_cases as UC

B = "emu"


@pytest.mark.parametrize("fen,moves,sims,L", UC.INFO_CASES, ids=UC.INFO_IDS)
def test_info_record_equals_a_host_walk_over_the_tree(fen, moves, sims, L):
    UC.check_info_after_search(B, fen, moves, sims, L, every_step=(sims, L) == (64, 8))


def test_info_on_mated_unexpanded_and_barely_visited_roots():
    UC.check_info_edge_roots(B)


def test_info_cuts_a_deep_main_line_at_the_pv_cap():
    UC.check_info_deep_line(B)


def test_info_orders_tied_visit_counts_by_legal_move_order():
    UC.check_info_tied_counts(B)


def test_info_refuses_reference_semantics_engines():
    UC.check_info_refuses_reference_engines(B)


def test_info_is_read_only():
    UC.check_info_is_read_only(B)


@pytest.mark.parametrize("fen,moves,sims,L,k", UC.STOP_CASES, ids=UC.STOP_IDS)
def test_stopped_fast_search_equals_a_search_of_the_simulations_done(fen, moves, sims, L, k):
    UC.check_stop_after_k_steps(B, fen, moves, sims, L, k)


def test_stop_while_only_the_roots_row_is_outstanding():
    UC.check_stop_before_the_root_is_expanded(B)


def test_stop_drops_shared_rows_and_known_terminal_simulations_in_flight():
    UC.check_stop_with_shared_rows_and_known_terminals_in_flight(B)


def test_stop_leaves_idle_and_unmasked_slots_alone():
    UC.check_stop_idle_and_masked_slots(B)


def test_stop_on_reference_semantics_engines_still_equals_the_oracle():
    UC.check_reference_semantics_stop_unchanged(B)


def test_uci_handshake():
    UC.check_uci_handshake(B)


def test_uci_go_nodes_prints_info_and_a_legal_reproducible_bestmove():
    UC.check_uci_go_nodes(B)


def test_uci_multipv_three_lines_in_visit_order():
    UC.check_uci_multipv(B)


def test_uci_go_infinite_answers_once_and_only_after_stop():
    UC.check_uci_infinite_and_stop(B)


def test_uci_position_extension_reuses_the_tree_and_ucinewgame_drops_it():
    UC.check_uci_tree_reuse(B)


def test_uci_illegal_moves_keep_the_legal_prefix_and_a_mated_root_answers_0000():
    UC.check_uci_illegal_move_and_mated_root(B)


def test_clock_rule_on_a_table_of_go_lines():
    UC.check_clock_table()
