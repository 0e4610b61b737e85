"""GPU tests (-m gpu, MI355X) of the tree step on degenerate evaluation rows: the bodies of tests/degenerate_eval_cases.py on the product
library, the step kernel's own softmax on sharp and on masked logits, and a Rollout whose net returns NaN rows."""
import numpy as np
import pytest

import degenerate_eval_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from betaone_amd import engine as E

    E.load_hip_library()  # fails loudly if the HIP library is missing
    return "hip"


@pytest.mark.parametrize("name", DC.DEGENERATE_SEARCH_NAMES)
def test_degenerate_search_matches_reference_trace(backend, name):
    DC.check_degenerate_golden_search(backend, name)


@pytest.mark.parametrize("family,widen,alpha,pos", DC.SWEEP, ids=DC.SWEEP_IDS)
def test_degenerate_family_matches_oracle(backend, family, widen, alpha, pos):
    """(peak keeps denormal priors in the tree: a build that flushes them to zero fails here on prior bits)"""
    DC.check_family_vs_oracle(backend, family, widen, alpha, pos)


@pytest.mark.parametrize("family", ["peak", "v_pm1"])
def test_degenerate_family_games_match_oracle(backend, family):
    DC.check_family_games(backend, family)


def test_step_heads_sees_the_bits_of_the_rows_kernel_on_sharp_logits(backend):
    """The three launch forms of test_engine_gpu.test_step_heads_sees_the_bits_of_the_rows_kernel with a policy head whose logits spread
    over more than 200: exp underflows to denormals and to zero, and the step kernel's softmax must still give bo_k_heads_rows' bits."""
    import test_engine_gpu as TG

    plies = TG.step_heads_three_launch_forms(sims=96, plies=2, wp_scale=4.0, min_nodes=10, min_spread=200.0)
    priors = [np.array([v[2]], np.uint32).view(np.float32)[0] for trees in plies for t in trees for k, v in t.items() if k]
    assert any(p == 0 for p in priors), "no node holds a zero prior: the logits are not sharp enough"


def test_in_kernel_softmax_close_to_torch_on_masked_logits(backend):
    """-inf at every odd action: a masked move is no fault (status 0), its prior is 0, and the other priors stay within 1e-5 relative of
    torch.softmax with equal visit counts."""
    import test_engine_gpu as TG

    from oracle import oracle as O

    masked = [O.move_to_index(m) % 2 == 1 for m in O.Board().legal_moves()]
    assert any(masked) and not all(masked)  # the mask does cut into the root's legal moves, and leaves some
    TG.in_kernel_softmax_vs_torch(masked=True)


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
    """The product path: a Rollout (captured step, engine softmax, the default step tail setting) on the GPU library."""
    DC.check_rollout_with_nan_net(backend)
