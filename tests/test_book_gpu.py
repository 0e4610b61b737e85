"""GPU tests of the opening-book path on an MI355X: the bodies of tests/book_cases.py on the product library -- bo_book_insert against
the NumPy / dict restatement (PGN corpus, one khash word for many positions, table sizes and overflow, the order of the work list,
refusals), a contention case in which 24 576 items from 2 048 games fall on 12 slots, records made by the emulator, and the command."""
import pytest

import book_cases as BC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("book_gpu")


def test_pgn_corpus_against_the_restatement(tmp):
    assert BC.check_pgn_corpus("gpu", tmp) > 100


def test_one_khash_word_many_positions():
    BC.check_shared_khash("gpu")


def test_table_sizes_and_overflow(tmp):
    assert BC.check_table_sizes("gpu", tmp) > 0


def test_order_of_the_work_list(tmp):
    BC.check_order_independence("gpu", tmp)


def test_two_thousand_games_on_one_line(tmp):
    assert BC.check_contention("gpu", tmp) == 12 * 2048


def test_refusals_and_edges():
    BC.check_refusals("gpu")


def test_records_made_by_the_emulator(tmp):
    BC.check_records("gpu", tmp)


def test_the_command_line(tmp, capsys):
    BC.check_command_line("gpu", tmp)
    capsys.readouterr()


@pytest.mark.parametrize("kw", [dict(min_games=2, max_bias=0.5), dict(min_games=2, max_bias=0.5, allow_nested=True, max_n=5, max_eval=0.5)])
def test_selection_equals_its_restatement(tmp, kw):
    BC.check_selection("gpu", tmp, **kw)
