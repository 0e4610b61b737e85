"""CPU tests of the FAST search mode on ties, uniform and zero priors, counts beyond the kernel's tables, full in-flight counters and
tree reuse, under the wave emulator (bodies: tests/fast_degenerate_cases.py).  The 4300-simulation square-root case and the path-cap
case run here on one kernel of each body only, every other variant on the GPU (tests/test_fast_degenerate_gpu.py;
profiles/fast_degenerate_rows.md has the times)."""
import numpy as np
import pytest

import fast_degenerate_cases as FC
from fake_model import FAMILIES, fake_logits_values, family_eval


@pytest.fixture(scope="module")
def backend():
    return "emu"


def test_combined_families_leave_the_existing_evaluators_bits_unchanged():
    """A policy family with a value family gives that policy's logits and that value family's values; every earlier call form
    returns what it returned (the combined form is checked against the single-family calls, which no caller's bits may leave)."""
    planes = np.zeros((3, 120, 8, 8), np.float32)
    planes[1, 5, 2, 3] = 1.0
    planes[2, 99, 7, 7] = 1.0
    base_l, base_v = fake_logits_values(planes, 6.0, 31)
    assert np.array_equal(fake_logits_values(planes, 6.0, 31, None)[0], base_l)
    for pol in FC.TIE_POLICIES:
        pl, pv = fake_logits_values(planes, salt=31, family=pol)
        assert np.array_equal(pv.view(np.uint32), base_v.view(np.uint32))
        for val in ("v_pm1", "v_zero"):
            cl, cv = fake_logits_values(planes, salt=31, family=pol, value=val)
            assert np.array_equal(cl, pl) and np.array_equal(cv.view(np.uint32), fake_logits_values(planes, salt=31, family=val)[1].view(np.uint32))
        cl, cv = fake_logits_values(planes, salt=31, family=pol, value="v_m1")
        assert np.array_equal(cl, pl) and np.all(cv == -1.0)
    assert np.array_equal(fake_logits_values(planes, salt=31, family="peak", peak_scale=400.0)[0], fake_logits_values(planes, salt=31, family="peak")[0])
    assert np.array_equal(fake_logits_values(planes, 800.0, 31)[0], fake_logits_values(planes, salt=31, family="peak", peak_scale=800.0)[0])
    for fam in FAMILIES:
        a, b = family_eval(fam, 31)(planes), family_eval(fam, 31, value=None)(planes)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("policy,pos,L,sims,opts", FC.TIE_SINGLE_CASES, ids=FC.TIE_SINGLE_IDS)
def test_ties_and_uniform_priors_match_restatement(backend, policy, pos, L, sims, opts):
    FC.check_tie_single(backend, policy, pos, L, sims, opts)


@pytest.mark.parametrize("policy,L,sims,opts", FC.TIE_MULTI_CASES, ids=FC.TIE_MULTI_IDS)
def test_ties_and_uniform_priors_with_a_different_position_in_every_slot(backend, policy, L, sims, opts):
    FC.check_tie_multi(backend, policy, L, sims, opts)


@pytest.mark.parametrize("L,opts", FC.BY_HAND, ids=FC.BY_HAND_IDS)
def test_uniform_priors_visit_the_first_ten_root_children_once_each(backend, L, opts):
    FC.check_by_hand(backend, L, opts)


@pytest.mark.parametrize("sims,opts", FC.RCP_CASES_EMU, ids=FC.rcp_ids(FC.RCP_CASES_EMU))
def test_counts_beyond_the_reciprocal_table_match_restatement(backend, sims, opts):
    FC.check_rcp_table(backend, sims, opts)


@pytest.mark.parametrize("pos,sims,L,opts", FC.PACKED_CASES, ids=FC.PACKED_IDS)
def test_full_in_flight_counters_match_restatement(backend, pos, sims, L, opts):
    FC.check_packed_counts(backend, pos, sims, L, opts)


@pytest.mark.parametrize("policy,value,opts", FC.REUSE_CASES, ids=FC.REUSE_IDS)
def test_tree_reuse_on_zero_and_uniform_priors_matches_restatement(backend, policy, value, opts):
    FC.check_reuse(backend, policy, value, opts)


@pytest.mark.parametrize("L,opts", FC.SQRT_CASES_EMU, ids=FC.SQRT_IDS_EMU)
def test_visits_beyond_the_square_root_table_match_restatement(backend, L, opts):
    FC.check_sqrt_table(backend, L, opts)


@pytest.mark.parametrize("opts", FC.CAP_VARIANTS_EMU, ids=FC.vid)
def test_a_descent_64_nodes_deep_is_a_draw_and_flags_the_game(backend, opts):
    FC.check_path_cap(backend, opts)


def test_the_restatement_cuts_a_descent_short_at_64_nodes():
    """The restatement's own rule: visits cut short at 64 nodes, each a terminal simulation backed up as a draw over nodes that were
    visited, every simulation delivered."""
    ref = FC.cap_reference()
    sims = FC.CAP[4]
    assert sum(v for _m, v in ref.visits) == sims and ref.n_term_sims >= ref.overflows
    assert max(k.count("/") + 1 for k, v in ref.canon.items() if k and v[0] > 0) == 63  # the deepest visited node: 64 nodes with the root
