"""CPU tests of the tree step on degenerate evaluation rows, under the wave emulator (bodies: tests/degenerate_eval_cases.py)."""
import pytest

import degenerate_eval_cases as DC


@pytest.fixture(scope="module")
def backend():
    return "emu"


@pytest.mark.parametrize("name", DC.DEGENERATE_SEARCH_NAMES)
def test_degenerate_search_matches_reference_trace(backend, name):
    DC.check_degenerate_golden_search(backend, name)


@pytest.mark.parametrize("family,widen,alpha,pos", DC.SWEEP, ids=DC.SWEEP_IDS)
def test_degenerate_family_matches_oracle(backend, family, widen, alpha, pos):
    DC.check_family_vs_oracle(backend, family, widen, alpha, pos)


def test_the_degenerate_inputs_hold_zero_and_denormal_priors():
    DC.check_edge_conditions()


@pytest.mark.parametrize("family", ["peak", "v_pm1"])
def test_degenerate_family_games_match_oracle(backend, family):
    DC.check_family_games(backend, family)


@pytest.mark.parametrize("widen", DC.WIDENS)
@pytest.mark.parametrize("kind,poison,when", DC.POISON_CASES, ids=DC.POISON_IDS)
def test_non_finite_row_flags_the_game_and_keeps_the_tree_sound(backend, kind, poison, when, widen):
    DC.check_poisoned_search(backend, kind, poison, when, widen)


@pytest.mark.parametrize("widen", DC.WIDENS)
def test_nan_at_an_illegal_index_of_a_leaf_row_is_never_read(backend, widen):
    DC.check_illegal_index_nan_is_not_read(backend, widen)


@pytest.mark.parametrize("kind,poison,when", DC.POISON_CASES, ids=DC.POISON_IDS)
def test_non_finite_row_in_fast_mode(backend, kind, poison, when):
    DC.check_poisoned_search(backend, kind, poison, when, 1.5, fast_L=4)


def test_nan_at_an_illegal_index_in_fast_mode(backend):
    DC.check_illegal_index_nan_is_not_read(backend, 1.5, fast_L=4)


def test_rollout_with_a_net_that_returns_nan_rows_is_flagged(backend):
    DC.check_rollout_with_nan_net(backend)
