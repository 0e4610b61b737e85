"""GPU tests (-m gpu, MI355X) of the FAST search mode on ties, uniform and zero priors, counts beyond the kernel's tables, full in-flight
counters, the path cap and tree reuse: the bodies of tests/fast_degenerate_cases.py on the product library."""
import pytest

import fast_degenerate_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from betaone_amd import engine as E

    E.load_hip_library()  # fails loudly if the HIP library is missing
    return "hip"


@pytest.mark.parametrize("policy,pos,L,sims,opts", FC.TIE_SINGLE_CASES, ids=FC.TIE_SINGLE_IDS)
def test_ties_and_uniform_priors_match_restatement(backend, policy, pos, L, sims, opts):
    FC.check_tie_single(backend, policy, pos, L, sims, opts)


@pytest.mark.parametrize("policy,L,sims,opts", FC.TIE_MULTI_CASES, ids=FC.TIE_MULTI_IDS)
def test_ties_and_uniform_priors_with_a_different_position_in_every_slot(backend, policy, L, sims, opts):
    FC.check_tie_multi(backend, policy, L, sims, opts)


@pytest.mark.parametrize("L,opts", FC.BY_HAND, ids=FC.BY_HAND_IDS)
def test_uniform_priors_visit_the_first_ten_root_children_once_each(backend, L, opts):
    FC.check_by_hand(backend, L, opts)


@pytest.mark.parametrize("sims,opts", FC.RCP_CASES, ids=FC.rcp_ids(FC.RCP_CASES))
def test_counts_beyond_the_reciprocal_table_match_restatement(backend, sims, opts):
    FC.check_rcp_table(backend, sims, opts)


@pytest.mark.parametrize("pos,sims,L,opts", FC.PACKED_CASES, ids=FC.PACKED_IDS)
def test_full_in_flight_counters_match_restatement(backend, pos, sims, L, opts):
    FC.check_packed_counts(backend, pos, sims, L, opts)


@pytest.mark.parametrize("L,opts", FC.SQRT_CASES, ids=FC.SQRT_IDS)
def test_visits_beyond_the_square_root_table_match_restatement(backend, L, opts):
    """4300 simulations of a king-and-rook ending: the root and its best child pass 4096 visits (sqrtf instead of the table) while
    children pass 254 (1.0f / n instead of the table): bit-equal only with correctly rounded division and square root."""
    FC.check_sqrt_table(backend, L, opts)


@pytest.mark.parametrize("opts", FC.CAP_VARIANTS, ids=FC.vid)
def test_a_descent_64_nodes_deep_is_a_draw_and_flags_the_game(backend, opts):
    FC.check_path_cap(backend, opts)


@pytest.mark.parametrize("policy,value,opts", FC.REUSE_CASES, ids=FC.REUSE_IDS)
def test_tree_reuse_on_zero_and_uniform_priors_matches_restatement(backend, policy, value, opts):
    FC.check_reuse(backend, policy, value, opts)
