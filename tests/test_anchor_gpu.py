"""The anchor opponent (betaone_amd/anchor.py, csrc/bo_anchor.h) on the MI355X: the bodies of anchor_cases.py over middlegame trees
-- Kiwipete to depth 3 (castling, promotions and checks in one tree; its level 2 crosses a scan tile and splits at the small
capacities), the perft suite's roots as one batch -- against the definitional negamax over the oracle's rules.  The reference is
computed once per root and depth and shared by every test of the module."""
import pytest

import anchor_cases as AC
import mate_cases as MC

pytestmark = pytest.mark.gpu
B = "hip"
SUITE = tuple(p[0] for p in AC.PERFT)
KRK_ROOTS = AC.krk_roots()
BATCH = SUITE + tuple(sorted(MC.below(MC.SMOTHERED, 1)))


def test_static_evaluation():
    AC.check_ev(B, AC.ev_fens() + list(MC.below(AC.KIWIPETE, 2)))


@pytest.mark.parametrize("fen,depth", AC.NAMED + [(AC.KIWIPETE, 2), (MC.START, 3), (MC.SMOTHERED, 2)])
def test_values_of_the_named_positions(fen, depth):
    r = AC.check_named(B, fen, depth)
    assert r.status == "ok" and (r.nodes == 49) == (fen == AC.KIWIPETE)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_values_at_every_depth(depth):
    fens = (MC.KRK, MC.KQK, AC.KPK, MC.KPK_5, MC.STALE_TRAP, MC.MATED, MC.STALEMATED, AC.INNER_TERMINALS, AC.PERFT[2][0], AC.MATED_IN_2,
            AC.POISONED, MC.EP_MATE, MC.PROMO_KEYS)
    res = AC.check_values(B, fens, depth)
    assert [r.status for r in res].count("ok") == len(fens) - 2


def test_values_of_a_middlegame_batch():
    res = AC.check_values(B, BATCH, 2)
    assert len(res) > 40 and res[0].nodes > 1024  # (level 1 crosses a scan tile)


def test_values_of_kiwipete_at_depth_3():
    r = AC.check_values(B, (AC.KIWIPETE,), 3)[0]
    assert r.nodes == 1 + 48 + 2039


@pytest.mark.parametrize("name,depth", [("kiwipete", 3), ("krk", 2), ("batch", 2)])
def test_chunking_does_not_change_the_results(name, depth):
    fens = {"kiwipete": (AC.KIWIPETE,), "krk": KRK_ROOTS, "batch": BATCH}[name]
    assert sum(AC.ref_root(f, depth).entries for f in fens) > 2 * 300
    AC.check_chunking(B, fens, depth, (256, 300))
    AC.check_values(B, fens, depth, capacity=256)


def test_batch_invariance_and_input_forms():
    AC.check_batch_invariance(B, SUITE + (MC.KRK, MC.MATED, MC.STALE_TRAP, MC.STALEMATED, AC.POISONED, MC.PROMO_KEYS, AC.MANY_MOVES), 2)


@pytest.fixture(scope="module")
def match():
    openings = [(None, "e2e4 e7e5 g1f3"), (AC.MATE_IN_1_OPENING, "")]
    return (openings, 4, 2) + AC.play(B, openings, 4, 4, sims=16, depth=2, max_game_moves=12)


def test_game_loop(match):
    openings, n_games, depth, played, fins, st, text = match
    AC.check_games(openings, n_games, depth, played, fins, st, text)
    won = [g for g in played["games"] if g["opening"] == 1 and g["white"] == "A"]
    assert len(won) == 1 and (won[0]["moves"], won[0]["termination"], won[0]["result_b"]) == (["a1a8"], "checkmate", 0.0)
    long = [g for g in played["games"] if g["opening"] == 0]
    assert len(long) == 2 and all(3 < g["plies"] <= 12 and g["prefix"] == "e2e4 e7e5 g1f3" for g in long)


def test_command_line_best(tmp_path):
    AC.check_cli_best(B, tmp_path)


def test_command_line_match(tmp_path):
    AC.check_cli_match(B, tmp_path)
