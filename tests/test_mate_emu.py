"""Forced mates (betaone_amd/mate.py, csrc/bo_mate.h) under the wave emulator, and the refusals on the CPU.  The bodies are
mate_cases.py's; the emulator runs one lane at a time, so the sets here are the subsets it can afford in seconds: few-men positions,
and of the KRK / KQK sets the roots the reference spent least on.  The full sets run on the MI355X (test_mate_gpu.py)."""
import ctypes as C

import pytest

import mate_cases as MC
from betaone_amd import build, engine as E, mate as M

B = "emu"
# Every class at N = 2 in a batch the emulator walks in seconds: three named positions and, of the king-and-pawn positions two plies
# below two of them, those without a new queen or rook (a handful of moves a side), fewest positions two plies further down first,
# until there are more than 340 of those -- so the two smallest capacities have to split a level.
def _emu_set():
    named = [MC.STALE_TRAP, MC.PROMO_KEYS, MC.KPK_5]
    pure = {f for f in MC.below(MC.STALE_TRAP, 2) + MC.below(MC.KPK_5, 2) if "Q" not in f and "R" not in f}
    out, total = list(named), sum(len(MC.below(f, 2)) for f in named)
    for f in sorted(pure, key=lambda f: (len(MC.below(f, 2)), f)):
        if total > 340:
            break
        out.append(f)
        total += len(MC.below(f, 2))
    return tuple(out)


EMU_SET = _emu_set()
EMU_FEW = MC.cheapest(EMU_SET, 2, 1, (1, 3, 0))


@pytest.mark.parametrize("fen,n", [(MC.EP_MATE, 1), (MC.EP_GONE, 2), (MC.STALE_TRAP, 3), (MC.PROMO_KEYS, 1), (MC.KRK, 3), (MC.KPK_5, 3)])
def test_values_of_the_named_positions(fen, n):
    r = MC.check_values(B, (fen,), n)[0]
    want = {MC.EP_MATE: (1, ["f5g6"]), MC.EP_GONE: (0, []), MC.STALE_TRAP: (3, ["f7f8r"]), MC.KRK: (3, ["f6f7", "f6g6"])}.get(fen)
    if want:  # (what the position is there for: the reference must see it too)
        assert (r.dtm, r.keys) == want
    if fen == MC.PROMO_KEYS:
        assert r.dtm == 1 and len(r.keys) > 1 and all(len(k) == 5 for k in r.keys)
    if fen == MC.KPK_5:
        assert r.dtm == 5 and r.searched == 3  # the walk went to depth 5: two defender levels, backups through four levels


def test_statuses_of_roots_without_moves():
    res = MC.check_values(B, (MC.MATED, MC.STALEMATED, MC.PROMO_KEYS), 2)
    assert [r.status for r in res] == ["checkmated", "stalemated", "ok"]


def test_values_of_krk_and_kqk_subsets():
    for root in (MC.KRK, MC.KQK):
        MC.check_values(B, MC.cheapest(MC.below(root, 2), 3, 2, (1, 3)), 3)


def test_mate_in_two_set_has_every_class():
    cl = MC.classes(EMU_SET, 2)
    assert cl.get(1) and cl.get(3) and cl.get(0), cl
    MC.check_values(B, EMU_SET, 2)


@pytest.mark.parametrize("capacity", [256, 300])
def test_chunking_does_not_change_the_results(capacity):
    MC.check_chunking(B, EMU_SET, 2, (capacity,), (256, 300))


def test_batch_invariance_and_position_input():
    MC.check_batch_invariance(B, EMU_FEW, 2)


def test_iterative_deepening_stops_at_the_budget():
    MC.check_budget(B, EMU_FEW, 2)


def test_principal_variations():
    MC.check_pv(B, (MC.KPK_5,), 3)
    MC.check_pv(B, EMU_SET, 2, capacity=256)


def test_positions_that_are_none_get_their_status():
    import engine_harness as H

    arr = MC.to_bo_positions([MC.PROMO_KEYS] * 4 + ["k7/1Q6/1K6/8/8/8/8/8 w - - 0 1"])
    arr[1].bb[5] = 0               # no kings
    arr[2].bb[6] |= arr[2].bb[7]   # a man of both colours
    arr[3].ep_square = 99          # a field out of range
    with H.emulator_backend():     # (the last one: white to move while black is in check -- the device sees that)
        res = M.mate(arr, 1, device="cpu")
    assert [r.status for r in res] == ["ok"] + ["not a position"] * 4
    assert res[0].dtm == 1 and all(r.dtm == 0 and r.keys == [] and r.searched == 0 for r in res[1:])


def test_command_line_epd(tmp_path):
    MC.check_epd(B, tmp_path)


def test_command_line_audit(tmp_path):
    MC.check_audit(B, tmp_path)


def test_command_line_prints_the_mate_and_its_line():
    rc, text = MC.cli(B, [MC.STALE_TRAP, "--moves", "3", "--pv"])
    assert rc == 0 and text.splitlines()[0] == "Mate in 2 (3 plies): f7f8r (unique)" and text.splitlines()[1].startswith("pv f7f8r ")
    rc, text = MC.cli(B, [MC.EP_GONE, "--moves", "1", "--json"])
    import json
    assert rc == 0 and json.loads(text)["dtm"] == 0 and json.loads(text)["searched"] == 1


def test_bad_arguments_are_refused_before_any_device_call():
    """Check 6, on the product library with no device here: each case returns its code with a message, in the documented order."""
    lib = E.bind(C.CDLL(build.build()))
    lib.bo_last_error.restype = C.c_char_p
    fens = (C.c_char_p * 1)(MC.KRK.encode())
    pos = MC.to_bo_positions([MC.KRK])
    res = (M.BoMateResult * 1)()

    def call(n_roots=1, f=fens, p=None, moves=2, capacity=256, flags=0, results=C.addressof(res), pv=None):
        return lib.bo_mate(0, n_roots, f, C.addressof(p) if p is not None else None, moves, capacity, 0, flags, results, None, pv, None, None)

    cases = [
        (dict(p=pos), -1),                           # both root sources
        (dict(f=None), -1),                          # neither
        (dict(n_roots=(1 << 20) + 1), -1),
        (dict(moves=0), -1), (dict(moves=17), -1),   # N out of range
        (dict(capacity=255), -3), (dict(capacity=(1 << 26) + 1), -3),
        (dict(flags=2), -1),                         # unknown flag bits
        (dict(results=None), -1),
        (dict(flags=M.PV), -1),                      # BO_MATE_PV without pv
        (dict(p=pos, moves=0, capacity=1), -1),      # (the order: the root sources come first ...
        (dict(moves=0, capacity=1), -1),             #  ... then N, before the capacity)
        (dict(capacity=1, flags=2), -3),             # (the capacity before the flags)
    ]
    for i, (kw, code) in enumerate(cases):
        rc = call(**kw)
        assert rc == code and lib.bo_last_error(), (i, rc, code, lib.bo_last_error())
    bad = (C.c_char_p * 1)(b"8/8/8/8/8/8/8/K7 w - - 0 1")  # one king: BO_E_FEN, as for bo_perft (parsed on the host)
    assert call(f=bad) == -4 and b"root 0" in lib.bo_last_error()
    assert call(n_roots=0) == 0
