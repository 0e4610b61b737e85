"""GPU tests (-m gpu, MI355X) of the interactive front end on the FAST search mode: bo_search_info, bo_search_stop on fast-mode engines
(csrc/bo_info.h) and the UCI protocol of betaone_amd/uci.py on the product library -- the bodies of tests/uci_cases.py -- and one
`python -m betaone_amd.uci` child process."""
import os
import subprocess
import sys

import pytest

import uci_cases as UC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from betaone_amd import engine as E

    E.load_hip_library()  # fails loudly if the HIP library is missing
    return "hip"


@pytest.mark.parametrize("fen,moves,sims,L", UC.INFO_CASES, ids=UC.INFO_IDS)
def test_info_record_equals_a_host_walk_over_the_tree(backend, fen, moves, sims, L):
    UC.check_info_after_search(backend, fen, moves, sims, L, every_step=(sims, L) == (64, 8))


def test_info_on_mated_unexpanded_and_barely_visited_roots(backend):
    UC.check_info_edge_roots(backend)


def test_info_cuts_a_deep_main_line_at_the_pv_cap(backend):
    UC.check_info_deep_line(backend)


def test_info_orders_tied_visit_counts_by_legal_move_order(backend):
    UC.check_info_tied_counts(backend)


def test_info_refuses_reference_semantics_engines(backend):
    UC.check_info_refuses_reference_engines(backend)


def test_info_is_read_only(backend):
    UC.check_info_is_read_only(backend)


@pytest.mark.parametrize("fen,moves,sims,L,k", UC.STOP_CASES, ids=UC.STOP_IDS)
def test_stopped_fast_search_equals_a_search_of_the_simulations_done(backend, fen, moves, sims, L, k):
    UC.check_stop_after_k_steps(backend, fen, moves, sims, L, k)


def test_stop_while_only_the_roots_row_is_outstanding(backend):
    UC.check_stop_before_the_root_is_expanded(backend)


def test_stop_drops_shared_rows_and_known_terminal_simulations_in_flight(backend):
    UC.check_stop_with_shared_rows_and_known_terminals_in_flight(backend)


def test_stop_leaves_idle_and_unmasked_slots_alone(backend):
    UC.check_stop_idle_and_masked_slots(backend)


def test_stop_on_reference_semantics_engines_still_equals_the_oracle(backend):
    UC.check_reference_semantics_stop_unchanged(backend)


def test_uci_handshake(backend):
    UC.check_uci_handshake(backend)


def test_uci_go_nodes_prints_info_and_a_legal_reproducible_bestmove(backend):
    UC.check_uci_go_nodes(backend)


def test_uci_multipv_three_lines_in_visit_order(backend):
    UC.check_uci_multipv(backend)


def test_uci_go_infinite_answers_once_and_only_after_stop(backend):
    UC.check_uci_infinite_and_stop(backend)


def test_uci_position_extension_reuses_the_tree_and_ucinewgame_drops_it(backend):
    UC.check_uci_tree_reuse(backend)


def test_uci_illegal_moves_keep_the_legal_prefix_and_a_mated_root_answers_0000(backend):
    UC.check_uci_illegal_move_and_mated_root(backend)


def test_uci_module_as_a_child_process_plays_a_five_line_session(backend, tmp_path):
    import torch

    path = str(tmp_path / "net.pth")
    torch.save({k: v.cpu() for k, v in UC.make_net(backend).state_dict().items()}, path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    session = "uci\nisready\nposition startpos moves e2e4\ngo nodes 64\nquit\n"
    p = subprocess.run([sys.executable, "-m", "betaone_amd.uci", "--model", path], input=session, capture_output=True, text=True, cwd=root,
                       timeout=300)
    out = p.stdout.splitlines()
    assert p.returncode == 0, p.stderr[-2000:]
    assert "uciok" in out and "readyok" in out and sum(ln.startswith("bestmove") for ln in out) == 1
    assert out[-1].split()[1] in UC._legal(UC.START, ["e2e4"])
    assert any(ln.startswith("info depth") for ln in out)
