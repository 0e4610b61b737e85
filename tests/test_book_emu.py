"""CPU tests (wave emulator) of the opening-book path: bo_book_insert (csrc/bo_book.h) against the NumPy / dict restatement of
tests/book_cases.py -- a PGN corpus with a transposition, a castling-rights pair, an en-passant pair and a repetition; positions that
share one khash word; table sizes and overflow; the order of the work list; refusals -- self-play records as BOG1 and BOG2, and
betaone_amd.book end to end: the command line, its selection against a plain-Python restatement, match.parse_openings and
MatchScheduler on its output."""
import io
import json

import numpy as np
import pytest

import book_cases as BC
import engine_harness as H

from betaone_amd import book as B
from betaone_amd import records as R


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("book")


def test_pgn_corpus_against_the_restatement(tmp):
    assert BC.check_pgn_corpus("emu", tmp) > 100


def test_one_khash_word_many_positions():
    BC.check_shared_khash("emu")


def test_table_sizes_and_overflow(tmp):
    assert BC.check_table_sizes("emu", tmp) > 0


def test_order_of_the_work_list(tmp):
    BC.check_order_independence("emu", tmp)


def test_refusals_and_edges():
    BC.check_refusals("emu")


# ---- records ---------------------------------------------------------------------------------------------------------------------------
def test_records_as_bog1_and_bog2(tmp):
    """(5) emulator self-play games, without and with root values; some get a terminal code written into their header so that every
    result occurs.  Counts, results, sum_eval, min_ply and first against a restatement over records.load_games."""
    BC.check_records("emu", tmp)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_the_command_line(tmp, capsys):
    BC.check_command_line("emu", tmp)
    capsys.readouterr()


@pytest.mark.parametrize("kw", [dict(min_games=2, max_bias=0.5), dict(min_games=3, max_bias=0.2), dict(min_games=2, max_bias=0.5, max_eval=0.3),
                                dict(min_games=2, max_bias=0.5, allow_nested=True), dict(min_games=2, max_bias=0.5, max_n=2),
                                dict(min_games=2, max_bias=0.5, allow_nested=True, max_n=5, max_eval=0.5)])
def test_selection_equals_its_restatement(tmp, kw):
    BC.check_selection("emu", tmp, **kw)


def test_an_empty_selection_is_a_message(tmp, capsys):
    _, _, _, _, path = BC.pgn_corpus("emu", tmp)
    out = tmp / "empty.txt"
    with H.emulator_backend():
        rc = B.main([str(path), "-o", str(out), "--min-games", "1000", "--device", "cpu"], out=io.StringIO())
        assert B.main([str(tmp / "missing.pgn"), "-o", str(out), "--device", "cpu"], out=io.StringIO()) == 2
    err = capsys.readouterr().err
    assert rc == 1 and out.read_text() == "" and "no position qualifies" in err and "no such file" in err


def test_record_result_follows_pgn_write():
    """Terminals 1 and 3 are a loss for the side to move at the end, 2 a draw, anything else unknown (pgn_write.result_of)."""
    assert [B.record_result(t, 1) for t in (0, 1, 2, 3, 4, -1)] == [0, 3, 2, 3, 0, 0]
    assert [B.record_result(t, 0) for t in (0, 1, 2, 3)] == [0, 1, 2, 1]
