"""CPU tests (wave emulator) of the endgame tablebases inside the search and at the root: bo_engine_tablebases, the probing step
kernel (step_body<true>), adjudication in root_prepare, Rollout's tablebases / tb_search / tb_adjudicate and the match scoring.  No
table pass can run on the emulator, so KQK and KRK are synthetic tables uploaded through bo_tb_upload (tb_search_cases.synthetic_set);
the bodies are shared with the MI355X tests (test_tb_search_gpu.py)."""
import tb_search_cases as C


def test_tree_invariants_node_by_node():
    C.check_tree_invariants("emu")


def test_off_means_off():
    C.check_off_means_off("emu")


def test_oracle_parity_with_tables_attached_and_both_flags_on():
    C.check_oracle_parity_with_tables_attached("emu")


def test_adjudication_equals_rescore_on_the_host_made_turn(tmp_path):
    C.check_adjudication_equals_rescore("emu", tmp_path, cohorts=1, device_turn=False, max_game_moves=5)


def test_adjudication_equals_rescore_on_the_device_turn(tmp_path):
    C.check_adjudication_equals_rescore("emu", tmp_path, cohorts=1, device_turn=True, max_game_moves=5)


def test_both_flags_together():
    C.check_both_flags("emu")


def test_refusals():
    C.check_refusals("emu")


def test_command_line_refusals(tmp_path):
    C.check_command_line_refusals(tmp_path)


def test_match_scores_an_adjudicated_game_as_a_loss_for_the_side_to_move():
    C.check_match_scores_an_adjudicated_game("emu")
