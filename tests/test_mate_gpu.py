"""Forced mates (betaone_amd/mate.py, csrc/bo_mate.h) on the MI355X: the bodies of mate_cases.py over the full sets -- the KRK and KQK
positions at N = 3, about 1 500 middlegame roots each two plies below the smothered-mate position and perft position 5 at N = 2,
9 467 roots three plies below perft position 4 at N = 1 -- against the definitional minimax over the oracle's rules.  The reference
is computed once per root and shared by every test of the module."""
import pytest

import mate_cases as MC

pytestmark = pytest.mark.gpu
B = "hip"
CAPACITIES = (256, 300)
ROOTS = dict(krk=(MC.KRK, 2), kqk=(MC.KQK, 2), smothered=(MC.SMOTHERED, 2), pos5=(MC.POS5, 2), pos4=(MC.POS4, 3))


def S(name):
    """The set's roots: every position some plies below its root position (computed once, when a test first asks)."""
    return MC.below(*ROOTS[name])


@pytest.mark.parametrize("fen,n,dtm", [(MC.KRK, 3, 3), (MC.SMOTHERED, 2, 3), (MC.EP_MATE, 1, 1), (MC.EP_GONE, 2, 0), (MC.STALE_TRAP, 3, 3),
                                       (MC.PROMO_KEYS, 1, 1), (MC.KPK_5, 3, 5), (MC.START, 2, 0)])
def test_values_of_the_named_positions(fen, n, dtm):
    r = MC.check_values(B, (fen,), n)[0]
    assert r.dtm == dtm  # (what the position is there for: the reference must see it too)
    if fen == MC.EP_MATE:
        assert r.keys == ["f5g6"]
    if fen == MC.STALE_TRAP:
        assert r.keys == ["f7f8r"]
    if fen == MC.PROMO_KEYS:
        assert len(r.keys) > 1 and all(len(k) == 5 for k in r.keys)


def test_statuses_of_roots_without_moves():
    res = MC.check_values(B, (MC.MATED, MC.STALEMATED, MC.PROMO_KEYS), 2)
    assert [r.status for r in res] == ["checkmated", "stalemated", "ok"]


@pytest.mark.parametrize("name,n,want", [("krk", 3, (1, 3, 5, 0)), ("kqk", 3, (1, 3, 5, 0)), ("smothered", 2, (1, 3, 0)), ("pos5", 2, (1, 3, 0)),
                                         ("pos4", 1, (1, 0))])
def test_values_of_the_sets(name, n, want):
    fens = S(name)
    cl = MC.classes(fens, n)
    assert all(cl.get(d) for d in want), cl
    MC.check_values(B, fens, n)


@pytest.mark.parametrize("name,n", [("krk", 3), ("kqk", 3), ("smothered root", 2), ("pos5", 2)])
def test_chunking_does_not_change_the_results(name, n):
    fens = (MC.SMOTHERED,) if name == "smothered root" else S(name)
    assert name != "pos5" or len(fens) > 1024  # (the root level crosses a scan tile)
    MC.check_chunking(B, fens, n, CAPACITIES, CAPACITIES)


def test_batch_invariance_and_position_input():
    MC.check_batch_invariance(B, S("krk"), 3)
    MC.check_batch_invariance(B, S("kqk"), 3)
    for fens, n in ((S("smothered"), 2), (S("pos4"), 1)):
        assert [MC.facts(r) for r in MC.run(B, fens, n, as_positions=True)] == [MC.facts(r) for r in MC.run(B, fens, n)]


def test_iterative_deepening_stops_at_the_budget():
    MC.check_budget(B, S("krk"), 3)


@pytest.mark.parametrize("name,n", [("krk", 3), ("kqk", 3), ("smothered", 2)])
def test_principal_variations(name, n):
    MC.check_pv(B, S(name), n)


def test_principal_variations_do_not_depend_on_the_capacity():
    for fens, n in ((S("krk"), 3), ((MC.SMOTHERED,), 2)):
        assert [MC.facts(r) for r in MC.run(B, fens, n, pv=True, capacity=256)] == [MC.facts(r) for r in MC.run(B, fens, n, pv=True)]


def test_command_line_epd(tmp_path):
    MC.check_epd(B, tmp_path)


def test_command_line_audit(tmp_path):
    MC.check_audit(B, tmp_path)


def test_command_line_prints_the_mate_and_its_line():
    rc, text = MC.cli(B, [MC.SMOTHERED, "--moves", "2", "--pv"])
    print(text)
    lines = text.splitlines()
    assert rc == 0 and lines[0] == "Mate in 2 (3 plies): d5f6 (unique)" and lines[1] == "pv d5f6 g7f6 c4f7"
