"""The anchor's quiescence search (bo_anchor_q, csrc/bo_anchor.h) under the wave emulator, and the refusals on the CPU.  The bodies are
anchor_q_cases.py's; the emulator runs one lane at a time, so the trees here are those of the named positions and Kiwipete at (1, 1).
Middlegame trees, deeper quiescence and the games run on the MI355X (test_anchor_q_gpu.py)."""
import ctypes as C

import pytest

import anchor_cases as AC
import anchor_q_cases as QC
import mate_cases as MC
from betaone_amd import anchor as A
from betaone_amd import build, engine as E

B = "emu"
MATE = QC.MATE
SMALL = (MC.KRK, MC.MATED, MC.STALE_TRAP, MC.STALEMATED, QC.POISONED, MC.PROMO_KEYS, QC.BACK_RANK, QC.EP_BELOW, QC.PROMO_BELOW)


@pytest.mark.parametrize("q", [1, 2])
def test_values_of_the_named_positions(q):
    res = QC.check_values(B, QC.NAMED, 1, q)
    assert all(r.status == "ok" for r in res)


def test_values_of_kiwipete():
    r = QC.check_values(B, (QC.KIWIPETE,), 1, 1)[0]
    assert r.nodes == 1 + 48  # (levels 0 and 1; the tactical children the leaf level makes are not entries)


def test_values_of_the_218_move_position_through_the_tactical_expand():
    """At (1, 3) level 2 holds white entries with some 200 moves of which a few capture: the expand kernel ranks them across the
    four 64-move words."""
    r = QC.check_values(B, (QC.MANY_MOVES,), 1, 3)[0]
    assert r.n_moves == 218


def test_values_with_terminal_roots_and_two_full_levels():
    res = QC.check_values(B, SMALL, 2, 2)
    assert [r.status for r in res].count("ok") == len(SMALL) - 2


def test_the_reference_meets_every_kind_of_node():
    QC.check_classes([(f, 1, q) for f in QC.NAMED for q in (1, 2)] + [(f, 2, 2) for f in SMALL] + [(QC.MANY_MOVES, 1, 3)])


def test_what_quiescence_is_for():
    QC.check_purpose(B)


def test_quiesce_0_is_bo_anchor():
    QC.check_q0(B, (MC.KRK, AC.KPK, MC.KPK_5, MC.STALE_TRAP, MC.MATED, MC.STALEMATED))


@pytest.mark.parametrize("capacity", [256, 300])
def test_chunking_does_not_change_the_results(capacity):
    """Levels 0 and 1 full width, level 2 the first quiescence level, level 3 its tactical children."""
    fens = (QC.BACK_RANK,)
    below = QC.ref_root(QC.BACK_RANK, 2, 2).entries - QC.ref_root(QC.BACK_RANK, 2, 1).entries  # level 3
    assert QC.ref_root(QC.BACK_RANK, 2, 1).entries - QC.ref_root(QC.BACK_RANK, 1, 1).entries > 300  # level D = 2 fits neither capacity ...
    assert below > 300  # ... nor does level 3, which the tactical expand kernel fills
    QC.check_chunking(B, fens, 2, 2, (capacity,))
    QC.check_values(B, fens, 2, 2, capacity=capacity)


def test_chunking_with_backups_through_two_quiescence_levels():
    fens = (QC.BACK_RANK,)  # (at (2, 3) level 3 is an inner quiescence level: its entries are counted, expanded and backed up in chunks)
    assert QC.ref_root(QC.BACK_RANK, 2, 2).entries - QC.ref_root(QC.BACK_RANK, 2, 1).entries > 2 * 256  # level 3
    assert QC.ref_root(QC.BACK_RANK, 2, 3).entries > QC.ref_root(QC.BACK_RANK, 2, 2).entries          # level 4 is not empty
    QC.check_chunking(B, fens, 2, 3, (256,))
    QC.check_values(B, fens, 2, 3, capacity=256)


def test_batch_invariance_and_input_forms():
    QC.check_batch_invariance(B, SMALL, 1, 2)


def test_bad_arguments_are_refused_before_any_device_call():
    """On the product library with no device here: each case returns its code with a message, in the documented order."""
    lib = E.bind(C.CDLL(build.build()))
    lib.bo_last_error.restype = C.c_char_p
    fens = (C.c_char_p * 1)(MC.KRK.encode())
    pos = MC.to_bo_positions([MC.KRK])
    res = (A.BoAnchorResult * 1)()

    def call(n_roots=1, f=fens, p=None, depth=2, quiesce=2, capacity=256, flags=0, results=C.addressof(res)):
        return lib.bo_anchor_q(0, n_roots, f, C.addressof(p) if p is not None else None, depth, quiesce, capacity, flags, results, None, None, None, None)

    cases = [
        (dict(p=pos), -1), (dict(f=None), -1), (dict(n_roots=(1 << 20) + 1), -1),   # the root sources
        (dict(depth=0), -1), (dict(depth=A.MAX_DEPTH + 1), -1),
        (dict(quiesce=-1), -1), (dict(quiesce=A.MAX_QUIESCE + 1), -1),
        (dict(depth=0, quiesce=0), -1),              # (depth 0 is no search, with or without quiescence)
        (dict(capacity=255), -3), (dict(capacity=(1 << 26) + 1), -3),
        (dict(flags=1), -1),
        (dict(results=None), -1),
        (dict(p=pos, quiesce=9, capacity=1), -1),    # (the order: the root sources, the depth and the quiescence ...
        (dict(depth=0, quiesce=9, capacity=1), -1),
        (dict(quiesce=9, capacity=1), -1),           #  ... come before the capacity)
        (dict(capacity=1, flags=2), -3),             # (the capacity before the flags)
        (dict(flags=2, results=None), -1),
    ]
    for i, (kw, code) in enumerate(cases):
        rc = call(**kw)
        assert rc == code and lib.bo_last_error(), (i, rc, code, lib.bo_last_error())
    # the message names what was refused first
    assert call(depth=0, quiesce=9) == -1 and b"depth" in lib.bo_last_error()
    assert call(quiesce=9, capacity=1) == -1 and b"quiesce" in lib.bo_last_error()
    assert call(quiesce=-1, flags=1) == -1 and b"quiesce" in lib.bo_last_error()
    assert call(capacity=1, flags=2) == -3 and b"capacity" in lib.bo_last_error()
    bad = (C.c_char_p * 1)(b"8/8/8/8/8/8/8/K7 w - - 0 1")  # one king: BO_E_FEN, parsed on the host
    assert call(f=bad) == -4 and b"root 0" in lib.bo_last_error()
    assert call(n_roots=0) == 0
    with pytest.raises(ValueError):
        A.search(MC.KRK, 0, quiesce=1, device="cpu")  # (before the library is asked)
    for kw in (dict(depth=0, quiesce=1), dict(depth=2, quiesce=-1), dict(depth=2, quiesce=A.MAX_QUIESCE + 1)):
        with pytest.raises(ValueError):  # (before an engine is made)
            A.AnchorRollout(None, 2, **kw)


def test_names_and_json():
    assert A.anchor_name(3, 15) == A.anchor_name(3, 15, 0) == "anchor(depth=3,margin=15)"
    assert A.anchor_name(3, 15, 4) == "anchor(depth=3,quiesce=4,margin=15)"
    r = A.AnchorResult("f", "ok", 2, 10, "e2e4", 796, 1, 20, None, None, 5, 0, 0.5)  # (positional construction as before)
    assert r.quiesce == 0 and "quiesce" not in r.to_json()
    r.quiesce = 3
    assert r.to_json()["quiesce"] == 3


def test_command_line_best():
    QC.check_cli_best(B, QC.POISONED, 1, 1)
