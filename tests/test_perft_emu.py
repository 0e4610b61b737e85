"""CPU tests (library host code + wave emulator) of perft on the device: published counts, divide against the oracle, the move
statistics and the ORDER checksum against a walk over the oracle, level splitting under a small capacity, the edges of the entry
point, and the command line."""
import ctypes as C
import io

import pytest

import engine_harness as H
import perft_cases as PC
from betaone_amd import engine as E
from betaone_amd import perft as P
from test_oracle_rules import PERFT


@pytest.mark.parametrize("fen,expected", PERFT)
def test_published_counts_and_divide(fen, expected):
    PC.check_counts_and_divide("emu", fen, expected, (1, 2, 3))


@pytest.mark.parametrize("depth", (1, 2, 3))
@pytest.mark.parametrize("fen", PC.STATS_FENS)
def test_stats_and_order_checksum_against_the_oracle_walk(fen, depth):
    PC.check_stats_and_order("emu", fen, depth)


def test_oracle_walk_knows_the_published_kiwipete_breakdown():
    """The walk's definitions are the published ones: Kiwipete at depth 2 and 3 (chessprogramming.org "Perft Results", position 2)."""
    assert PC.oracle_walk(PC.KIWIPETE, 2)[:2] == (2039, dict(captures=351, en_passant=1, castles=91, promotions=0, checks=3, checkmates=0,
                                                             stalemates=0))
    assert PC.oracle_walk(PC.KIWIPETE, 3)[:2] == (97862, dict(captures=17102, en_passant=45, castles=3162, promotions=0, checks=993,
                                                              checkmates=1, stalemates=0))


def test_checksum_depends_on_the_order():
    """What the ORDER check stands on: the hash of a list with two moves swapped differs, here for the root's list of every case."""
    from oracle import oracle as O

    for fen in PC.STATS_FENS:
        words = [PC.word(m) for m in O.Board(fen).legal_moves()]

        def h(ws):
            x = PC.FNV_BASIS
            for w in ws:
                x = ((x ^ w) * PC.FNV_PRIME) & PC.MASK
            return x

        assert PC.run("emu", fen, 1, order=True).checksum == h(words)
        assert h(words) != h([words[1], words[0]] + words[2:])


def test_results_do_not_depend_on_the_capacity():
    big = PC.run("emu", PC.KIWIPETE, 3, divide=True, stats=True, order=True)
    assert big.splits == 0
    for cap in (256, 300):
        small = PC.run("emu", PC.KIWIPETE, 3, divide=True, stats=True, order=True, capacity=cap)
        assert small.splits > 0
        PC.same_result(small, big)


def test_edges_of_the_entry_point():
    for fen in (PC.START, PC.KIWIPETE, PC.MATED):
        r = PC.run("emu", fen, 0, divide=True, stats=True, order=True)
        assert r.nodes == 1 and r.checksum == 0 and not any(r.stats.values()) and r.moves == []
    for fen in (PC.MATED, PC.STALEMATED):
        for d in (1, 2, 3):
            r = PC.run("emu", fen, d, divide=True, stats=True, order=True)
            assert r.nodes == 0 and r.moves == [] and not any(r.stats.values())
            assert r.checksum == PC.FNV_BASIS  # one empty move list was generated: the root's
    with H.emulator_backend():
        with pytest.raises(ValueError, match="FEN"):
            P.perft("rnbqkbnr/ppppxppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", 2, device="cpu")
        with pytest.raises(ValueError, match="root 1"):
            P.perft([None, "8/8/8/8/8/8/8/K7 w - - 0 1"], 1, device="cpu")  # no black king
        with pytest.raises(E.EngineError, match="capacity"):
            P.perft(None, 2, capacity=255, device="cpu")
        assert P.perft([], 3, device="cpu") == []
        lib = H.emu_lib()
        res = P.BoPerftResult()
        call = lambda n, fen, depth, cap, flags=0: lib.bo_perft(0, n, (C.c_char_p * 1)(fen), depth, cap, flags, C.addressof(res), None, None, None, None)
        assert call(1, None, 2, 255) == -3                      # BO_E_CONFIG
        assert call(1, None, 2, (1 << 26) + 1) == -3
        assert call(1, b"not a fen", 2, 1 << 20) == -4
        assert call(1, None, -1, 1 << 20) == -1
        assert call(1, None, 2, 1 << 20, flags=P.DIVIDE) == -1  # divide without its arrays
        assert call(0, None, 2, 1 << 20) == 0
        assert call(1, None, 2, 256) == 0 and res.nodes == 400 and res.n_moves == 20


def test_several_roots_in_one_call():
    fens = (PC.START, PC.KIWIPETE, PC.MATED, PC.POS3, None)
    for d in (1, 2):
        res = PC.run("emu", fens, d, divide=True, order=True)
        want = [PERFT[0][1][d - 1], PERFT[1][1][d - 1], 0, PERFT[2][1][d - 1], PERFT[0][1][d - 1]]
        assert [r.nodes for r in res] == want
        for r, fen in zip(res, fens):
            PC.same_result(r, PC.run("emu", fen if fen else PC.START, d, divide=True, order=True))


def cli(argv):
    out = io.StringIO()
    with H.emulator_backend():
        rc = P.main(list(argv) + ["--device", "cpu"], out=out)
    return rc, out.getvalue()


def test_command_line_divide_text():
    rc, text = cli(["--depth", "3", "--divide"])
    lines = text.splitlines()
    assert rc == 0
    assert lines[:20] == [f"{u}: {n}" for u, n in PC.run("emu", PC.START, 3, divide=True).moves]
    assert lines[0] == "g1h3: 400" and "e2e4: 600" in lines[:20]
    assert lines[20] == "" and lines[21] == "Nodes searched: 8902"
    assert "nodes/s" in lines[-1] and lines[-1].split()[1] == "s,"
    rc, text = cli([PC.KIWIPETE, "--depth", "2", "--stats", "--order"])
    assert rc == 0 and "Nodes searched: 2039" in text and "captures=351" in text and "castles=91" in text and "Order checksum: 0x" in text


def test_command_line_epd_suite(tmp_path):
    good = tmp_path / "suite.epd"
    rows = [fen + " " + " ".join(f";D{d + 1} {n}" for d, n in enumerate(exp)) for fen, exp in PERFT]
    good.write_text("# perft suite\n" + "\n".join(rows) + "\n")
    rc, text = cli(["--epd", str(good), "--max-depth", "2"])
    assert rc == 0 and text.count(": ok ") == len(PERFT) and "FAIL" not in text
    bad = tmp_path / "bad.epd"
    rows[2] = rows[2].replace(";D2 191", ";D2 192")
    bad.write_text("# perft suite\n" + "\n".join(rows) + "\n")
    rc, text = cli(["--epd", str(bad), "--max-depth", "2"])
    assert rc == 1
    failed = [l for l in text.splitlines() if "FAIL" in l]
    assert len(failed) == 1 and failed[0].startswith(f"{bad}:4: FAIL {PERFT[2][0]}") and "D2 191 (expected 192)" in failed[0]
    assert text.count(": ok ") == len(PERFT) - 1
