"""The anchor's quiescence search (bo_anchor_q, csrc/bo_anchor.h) on the MI355X: the bodies of anchor_q_cases.py over middlegame trees
-- Kiwipete at one and two full-width plies, the perft suite's roots as one batch, the 218-move position, whose tactical moves lie in
all four 64-move words of its list -- against the definitional search over the oracle's rules.  The reference is computed once per
root, depth and quiescence and shared by every test of the module.  Kiwipete stays at three quiescence plies or fewer: the reference
grows about six times per ply there."""
import pytest

import anchor_cases as AC
import anchor_q_cases as QC
import mate_cases as MC

pytestmark = pytest.mark.gpu
B = "hip"
MATE = QC.MATE
SMALL = (MC.KRK, MC.MATED, MC.STALE_TRAP, MC.STALEMATED, QC.POISONED, MC.PROMO_KEYS, QC.BACK_RANK, QC.EP_BELOW, QC.PROMO_BELOW)
KIWIPETE_CASES = [(1, 1), (1, 2), (1, 3), (2, 1)]
NAMED_Q = [1, 2, 3, 4, 5, 8]


@pytest.mark.parametrize("depth,q", KIWIPETE_CASES)
def test_values_of_kiwipete(depth, q):
    r = QC.check_values(B, (QC.KIWIPETE,), depth, q)[0]
    assert r.status == "ok" and (r.nodes == 1 + 48) == ((depth, q) == (1, 1))


def test_the_value_of_kiwipete_swings_with_the_parity_of_the_quiescence():
    a, b, c = (QC.run(B, (QC.KIWIPETE,), 1, q)[0].score for q in (1, 2, 3))
    assert a < b > c  # (the side that captures last looks better: expected of a depth-limited quiescence, see the profile)


def test_values_of_the_perft_suite():
    res = QC.check_values(B, QC.SUITE, 1, 2)
    assert res[0].nodes > 1024  # (the levels together cross a scan tile)


@pytest.mark.parametrize("q", [2, 3])
def test_values_of_the_218_move_position(q):
    r = QC.check_values(B, (QC.MANY_MOVES,), 1, q)[0]
    assert r.n_moves == 218


@pytest.mark.parametrize("q", NAMED_Q)
def test_values_of_the_named_positions(q):
    res = QC.check_values(B, QC.NAMED, 1, q)
    assert all(r.status == "ok" for r in res)


def test_values_with_terminal_roots_and_two_full_levels():
    res = QC.check_values(B, SMALL + QC.SUITE[2:5], 2, 2)
    assert [r.status for r in res].count("ok") == len(res) - 2


def test_the_reference_meets_every_kind_of_node():
    QC.check_classes([(QC.KIWIPETE, d, q) for d, q in KIWIPETE_CASES] + [(f, 1, 2) for f in QC.SUITE] + [(QC.MANY_MOVES, 1, 3)]
                     + [(f, 1, q) for f in QC.NAMED for q in NAMED_Q])


def test_what_quiescence_is_for():
    QC.check_purpose(B)


def test_quiesce_0_is_bo_anchor():
    QC.check_q0(B, QC.SUITE + SMALL + (QC.MANY_MOVES,))


@pytest.mark.parametrize("depth,q", [(2, 1), (1, 3)])
def test_chunking_does_not_change_the_results(depth, q):
    """(2, 1): level D = 2 has 2 039 entries, filled by the full-width expand in chunks; (1, 3): level 3 has some 3 000, filled by the
    tactical expand in chunks, and the backups of two quiescence levels run chunk by chunk."""
    want = QC.ref_root(QC.KIWIPETE, depth, q)
    assert want.entries - 1 - 48 > 2 * 300
    QC.check_chunking(B, (QC.KIWIPETE,), depth, q, (256, 300))
    QC.check_values(B, (QC.KIWIPETE,), depth, q, capacity=256)


def test_chunking_of_a_batch():
    fens = QC.SUITE + (QC.MANY_MOVES,)
    assert sum(QC.ref_root(f, 1, 2).n_moves for f in fens) > 300  # level D = 1
    QC.check_chunking(B, fens, 1, 2, (256, 300))
    QC.check_values(B, fens, 1, 2, capacity=300)


def test_batch_invariance_and_input_forms():
    QC.check_batch_invariance(B, QC.SUITE + SMALL + (QC.MANY_MOVES,), 1, 2)


def test_game_loop():
    openings = [(None, "e2e4 e7e5 g1f3"), (QC.POISONED, "")]
    played, fins, text = QC.play(B, openings, 4, 4, sims=16, depth=1, q=2, max_game_moves=10)
    plies = QC.check_games(4, 1, 2, played, fins, text)
    print(f"{plies} anchor plies")


def test_command_line(tmp_path):
    QC.check_cli_best(B, QC.POISONED, 1, 1)
    QC.check_cli_match(B, tmp_path, 1, 2)
