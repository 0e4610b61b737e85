"""The anchor opponent (betaone_amd/anchor.py, csrc/bo_anchor.h) under the wave emulator, and the refusals on the CPU.  The bodies
are anchor_cases.py's; the emulator runs one lane at a time, so the trees here are those of few-men positions (and the 218-move
position, whose replies are few).  Middlegame trees run on the MI355X (test_anchor_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import anchor_cases as AC
import mate_cases as MC
from betaone_amd import anchor as A
from betaone_amd import build, engine as E

B = "emu"
MATE = AC.MATE
KRK_ROOTS = AC.krk_roots()


def test_static_evaluation():
    AC.check_ev(B, AC.ev_fens())


def test_static_evaluation_of_records_that_are_no_positions():
    import engine_harness as H

    arr = MC.to_bo_positions([MC.KRK] * 3)
    arr[1].bb[5] = 0   # no kings
    arr[2].turn = 7    # a field out of range
    with H.emulator_backend():
        got = A.evaluate(arr, device="cpu")
        assert A.evaluate(arr[:0], device="cpu").tolist() == []
    assert got.tolist() == [AC.ev_bo(arr[0]), A.NONE, A.NONE]


@pytest.mark.parametrize("fen,depth", AC.NAMED)
def test_values_of_the_named_positions(fen, depth):
    AC.check_named(B, fen, depth)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_values_at_every_depth(depth):
    res = AC.check_values(B, (MC.KRK, MC.KQK, AC.KPK, MC.KPK_5, MC.STALE_TRAP, MC.MATED, MC.STALEMATED, AC.INNER_TERMINALS), depth)
    assert [r.status for r in res].count("ok") == 6 and res[5].status == "checkmated" and res[6].status == "stalemated"
    assert all((r.score, r.best, r.n_best, r.n_moves) == (0, None, 0, 0) for r in res[5:7])


@pytest.mark.parametrize("capacity", [256, 300])
def test_chunking_does_not_change_the_results(capacity):
    fens = KRK_ROOTS[:24]
    assert sum(AC.ref_root(f, 2).n_moves for f in fens) > 300  # level D - 1 does not fit either capacity
    AC.check_chunking(B, fens, 2, (capacity,))


def test_chunking_with_backups_through_two_levels():
    fens = MC.below(MC.KRK, 1)[:6] + (AC.INNER_TERMINALS,)  # (the lone king moves on level 2: many entries with few children each)
    assert sum(AC.ref_root(f, 3).entries - 1 - AC.ref_root(f, 3).n_moves for f in fens) > 256  # level 2
    AC.check_chunking(B, fens, 3, (256,))
    AC.check_values(B, fens, 3, capacity=256)


def test_batch_invariance_and_input_forms():
    AC.check_batch_invariance(B, (MC.KRK, MC.MATED, MC.STALE_TRAP, MC.STALEMATED, AC.POISONED, MC.PROMO_KEYS), 2)


def test_positions_that_are_none_get_their_status():
    import engine_harness as H

    arr = MC.to_bo_positions([MC.PROMO_KEYS] * 4 + ["k7/1Q6/1K6/8/8/8/8/8 w - - 0 1"])
    arr[1].bb[5] = 0               # no kings
    arr[2].bb[6] |= arr[2].bb[7]   # a man of both colours
    arr[3].ep_square = 99          # a field out of range
    with H.emulator_backend():     # (the last one: white to move while black is in check -- the device sees that)
        res = A.search(arr, 1, scores=True, device="cpu")
    assert [r.status for r in res] == ["ok"] + ["not a position"] * 4
    assert res[0].score == MATE - 1 and all((r.score, r.best, r.n_moves, r.scores) == (0, None, 0, []) for r in res[1:])
    assert res[0].nodes == 1  # (not searched: only the first root is an entry)


def test_bad_arguments_are_refused_before_any_device_call():
    """On the product library with no device here: each case returns its code with a message, in the documented order."""
    lib = E.bind(C.CDLL(build.build()))
    lib.bo_last_error.restype = C.c_char_p
    fens = (C.c_char_p * 1)(MC.KRK.encode())
    pos = MC.to_bo_positions([MC.KRK])
    res = (A.BoAnchorResult * 1)()

    def call(n_roots=1, f=fens, p=None, depth=2, capacity=256, flags=0, results=C.addressof(res)):
        return lib.bo_anchor(0, n_roots, f, C.addressof(p) if p is not None else None, depth, capacity, flags, results, None, None, None, None)

    cases = [
        (dict(p=pos), -1),                           # both root sources
        (dict(f=None), -1),                          # neither
        (dict(n_roots=(1 << 20) + 1), -1),
        (dict(depth=0), -1), (dict(depth=A.MAX_DEPTH + 1), -1),
        (dict(capacity=255), -3), (dict(capacity=(1 << 26) + 1), -3),
        (dict(flags=1), -1),                         # unknown flag bits
        (dict(results=None), -1),
        (dict(p=pos, depth=0, capacity=1), -1),      # (the order: the root sources come first ...
        (dict(depth=0, capacity=1), -1),             #  ... then the depth, before the capacity)
        (dict(capacity=1, flags=2), -3),             # (the capacity before the flags)
    ]
    for i, (kw, code) in enumerate(cases):
        rc = call(**kw)
        assert rc == code and lib.bo_last_error(), (i, rc, code, lib.bo_last_error())
    bad = (C.c_char_p * 1)(b"8/8/8/8/8/8/8/K7 w - - 0 1")  # one king: BO_E_FEN, parsed on the host
    assert call(f=bad) == -4 and b"root 0" in lib.bo_last_error()
    assert call(n_roots=0) == 0
    assert lib.bo_anchor_eval(0, 1, None, None, None) == -1 and lib.bo_anchor_eval(0, -1, None, None, None) == -1
    assert lib.bo_anchor_eval(0, 0, None, None, None) == 0
    for kw in (dict(depth=A.MAX_DEPTH + 1), dict(depth=-1), dict(depth=2, margin=-1), dict(depth=2, fast=True)):
        with pytest.raises(ValueError):  # (before an engine is made)
            A.AnchorRollout(None, 2, **kw)


def test_pick():
    r = AC.run(B, AC.POISONED, 2)  # 18 moves with distinct-ish scores
    assert A.pick(r) == r.best_word and A.pick(r, 0) == r.best_word
    with pytest.raises(ValueError):
        A.pick(r, 15)  # a margin needs a generator
    margin = 40
    cand = A.candidates(r, margin)
    assert 1 < len(cand) < r.n_moves and all(r.scores[i] >= r.score - margin for i in cand)
    assert [i for i in range(r.n_moves) if i not in cand and r.scores[i] >= r.score - margin] == []
    seq = [A.pick(r, margin, rng) for rng in [np.random.RandomState(5)] for _ in range(64)]
    assert seq == [A.pick(r, margin, rng) for rng in [np.random.RandomState(5)] for _ in range(64)]  # reproducible from the seed
    want = np.random.RandomState(5)
    assert seq == [r.move_words[cand[int(want.randint(len(cand)))]] for _ in range(64)]
    assert set(seq) == {r.move_words[i] for i in cand}  # (64 draws over a handful of moves reach each)
    # margin 0 with a generator: uniform among the moves that tie for the best
    two = AC.run(B, MC.KRK, 3)
    assert two.n_best == 2 and {A.pick(two, 0, rng) for rng in [np.random.RandomState(1)] for _ in range(32)} == \
        {w for w, v in zip(two.move_words, two.scores) if v == two.score}
    # a found mate ignores the margin
    assert A.candidates(two, 30000) == [i for i, v in enumerate(two.scores) if v == two.score]
    trap = AC.run(B, MC.STALE_TRAP, 3)
    assert {A.pick(trap, 30000, rng) for rng in [np.random.RandomState(2)] for _ in range(16)} == {trap.best_word}
    # ... and a lost position does not
    lost = AC.run(B, AC.MATED_IN_2, 1)
    assert lost.score < MATE - 1 and len(A.candidates(lost, 30000)) == lost.n_moves
    # depth 0: uniform over the legal moves, as a seeded sequence
    rnd = A.random_result(r.move_words)
    g, h = np.random.RandomState(11), np.random.RandomState(11)
    assert [A.pick(rnd, 0, g) for _ in range(40)] == [r.move_words[int(h.randint(r.n_moves))] for _ in range(40)]
    with pytest.raises(ValueError):
        A.pick(rnd)
    with pytest.raises(ValueError):
        A.pick(AC.run(B, MC.MATED, 1))


@pytest.fixture(scope="module")
def krk_match():
    openings = [(MC.KRK, "")]
    return (openings, 2, 2) + AC.play(B, openings, 2, 2, sims=8, depth=2, max_game_moves=8)


def test_game_loop(krk_match):
    openings, n_games, depth, played, fins, st, text = krk_match
    AC.check_games(openings, n_games, depth, played, fins, st, text)
    assert all(g["plies"] == 8 or g["termination"] != "move_limit" for g in played["games"])


def test_game_loop_mate_in_one():
    openings = [(AC.MATE_IN_1_OPENING, "")]
    played, fins, st, text = AC.play(B, openings, 2, 2, sims=8, depth=2, max_game_moves=4)
    AC.check_games(openings, 2, 2, played, fins, st, text)
    won = [g for g in played["games"] if g["white"] == "A"]
    assert len(won) == 1 and (won[0]["moves"], won[0]["termination"], won[0]["result_b"]) == (["a1a8"], "checkmate", 0.0)
    assert fins[won[0]["game_id"]].terminal == 1 and "1-0" in text


def test_game_loop_with_a_random_mover_and_a_margin():
    """Depth 0 and a margin draw from the anchor's own seeded stream: the same match twice is the same match."""
    openings = [(MC.KRK, "")]
    for depth, margin in ((0, 0), (1, 25)):
        a = AC.play(B, openings, 2, 2, sims=8, depth=depth, max_game_moves=6, margin=margin)[0]["games"]
        b = AC.play(B, openings, 2, 2, sims=8, depth=depth, max_game_moves=6, margin=margin)[0]["games"]
        assert [g["moves"] for g in a] == [g["moves"] for g in b] and all(len(g["moves"]) for g in a)


def test_command_line_best(tmp_path):
    AC.check_cli_best(B, tmp_path)


def test_command_line_match(tmp_path):
    AC.check_cli_match(B, tmp_path)
