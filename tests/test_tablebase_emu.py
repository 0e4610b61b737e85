"""CPU tests (library host code + wave emulator) of the endgame tablebases.  An emulated move generation costs about a millisecond, so
only KK is built completely here; of KQK the classification pass runs (a full pass over its 368 452 legal entries would take ten
minutes) and its checkmates are checked against the oracle.  The file format, the probe, rescoring and the command line run against
KRK's classification (its checkmates; every other position reads as a draw), uploaded through bo_tb_upload into a fresh table."""
import ctypes as C
import io

import numpy as np
import pytest

import engine_harness as H
import tablebase_cases as TC
from betaone_amd import engine as E
from betaone_amd import tablebase as TB


def test_kk_built_completely():
    with H.emulator_backend():
        ts = TB.TableSet("cpu")
        t = ts.add("KK")
        assert t.build() == 1
        info = t.info()
        codes = t.download()
        assert t.verify() == 0
        ts.close()
    assert info["complete"] and info["n_entries"] == 8192 and set(np.unique(codes).tolist()) == {0, 1}
    assert info["strong_to_move"]["legal"] == info["weak_to_move"]["legal"] == 3612  # 64 * 63 - adjacent pairs (420)
    assert info["fnv1a"] == TB.fnv1a(codes.astype("<u2").tobytes())


def test_kqk_classification_and_its_checkmates_against_the_oracle():
    with H.emulator_backend():
        ts = TB.TableSet("cpu")
        t = ts.add("KQK")
        assert t.build(max_passes=0) == 0
        info, codes = t.info(), t.download()
        ts.close()
    assert not info["complete"]
    assert info["weak_to_move"]["losses"] == int((codes == 2).sum()) == 364 and info["strong_to_move"]["losses"] == 0
    # every code-2 entry is the oracle's checkmate; every other legal entry is not; legality of a sample by the oracle's rules
    from oracle import oracle as O

    L = O.lib()
    rs = np.random.RandomState(0)
    for idx in np.nonzero(codes == 2)[0].tolist() + rs.choice(np.nonzero(codes == 1)[0], 3000, replace=False).tolist():
        b = O.Board(TB.entry_fen("KQK", idx))
        mate = not b.legal_moves() and bool(L.bo_is_check(C.byref(b.pos)))
        assert mate == (codes[idx] == 2), (idx, b.fen())
    for idx in rs.randint(0, len(codes), 3000).tolist():  # code 0 <=> not a position
        e = TB.entry_bitboards("KQK", idx)
        legal = e is not None
        if legal:
            bb, wtm = e
            other = O.Board(TB.bitboards_fen(bb, not wtm))  # the side NOT to move, given the move: is it in check?
            k = [(s & 7, s >> 3) for s in TB.decode("KQK", idx)[1]]
            legal = max(abs(k[0][0] - k[2][0]), abs(k[0][1] - k[2][1])) > 1 and not L.bo_is_check(C.byref(other.pos))
        assert legal == (codes[idx] != 0), idx


@pytest.mark.parametrize("name", ["KQK", "KPK"])
def test_host_index_round_trips_every_index(name):
    n = TB.n_entries(name)
    assert n == 524288
    for idx in range(n):
        e = TB.entry_bitboards(name, idx)
        if e is not None:
            assert TB.position_index(*e) == (name, idx), idx


def test_host_mirror_and_identical_men():
    bb, wtm = TB.entry_bitboards("KRK", TB.index("KRK", 1, [0, 7, 18]))
    assert TB.bitboards_fen(bb, wtm) == "8/8/8/8/8/2k5/8/K6R b - - 0 1"
    mb, mw = TB.mirror(bb, wtm)
    assert TB.bitboards_fen(mb, mw) == "k6r/8/2K5/8/8/8/8/8 w - - 0 1"
    assert TB.position_index(mb, mw) == TB.position_index(bb, wtm) == ("KRK", TB.index("KRK", 1, [0, 7, 18]))
    assert TB.mirror(mb, mw) == (bb, wtm)
    # two identical men: the ascending ordering is the position's index
    bb, wtm = TB.entry_bitboards("KRRK", TB.index("KRRK", 0, [0, 9, 5, 60]))
    assert TB.position_index(bb, wtm) == ("KRRK", TB.index("KRRK", 0, [0, 5, 9, 60]))
    assert TB.position_index(*TB.entry_bitboards("KK", 77)) == (None, None)
    assert TB.canonical("KPKR") == "KRKP" and TB.canonical("KNBK") == "KBNK" and TB.canonical("KKQ") == "KQK"


def test_closure_ordering_and_refusals():
    assert TB.closure(["KPK"]) == ["KQK", "KRK", "KPK"]
    assert TB.closure(["KBNK"]) == ["KBNK"] and TB.closure(["KBK", "KNK", "KK"]) == []
    assert TB.closure(["KQKR", "KRK"]) == ["KQK", "KRK", "KQKR"]
    c = TB.closure(["KRKP"])
    assert c[-1] == "KRKP" and all(c.index(s) < c.index(m) for m in c for s in TB.children(m) if s in c)
    with pytest.raises(ValueError, match="follow-up"):
        TB.closure(["KPKP"])
    with pytest.raises(ValueError, match="2 to 4 men"):
        TB.closure(["KQRKR"])
    with pytest.raises(ValueError, match="not a material"):
        TB.closure(["QK"])


_KRK = []


def krk_set():
    """KRK as far as the budget allows here -- the classification pass -- uploaded into a fresh table (an uploaded table counts as
    complete).  Call inside emulator_backend()."""
    if not _KRK:
        t = TB.Table("KRK", [], "cpu")
        assert t.build(max_passes=0) == 0 and not t.info()["complete"]
        _KRK.append(t.download())
        t.close()
    ts = TB.TableSet("cpu")
    t = ts.add("KRK")
    t.upload(_KRK[0], 0)
    assert t.info()["complete"] and t.info()["fnv1a"] == TB.fnv1a(_KRK[0].astype("<u2").tobytes())
    return ts


def test_file_format_round_trip_and_corruption(tmp_path):
    with H.emulator_backend():
        ts = krk_set()
        ts.save(str(tmp_path))
        info = ts.tables["KRK"].info()
        ts.close()
        p = tmp_path / "KRK.botb"
        head, codes = TB.read_table(str(p))
        assert head["fnv1a"] == info["fnv1a"] and head["passes"] == info["passes"] and len(codes) == 524288
        assert head["weak_to_move"]["max_loss_ply"] == 0 and head["weak_to_move"]["losses"] == info["weak_to_move"]["losses"] > 0
        back = TB.TableSet.load(str(tmp_path), "cpu")
        assert back.tables["KRK"].info() == info
        back.close()
        raw = p.read_bytes()
        p.write_bytes(raw[:-2])
        with pytest.raises(ValueError, match="truncated"):
            TB.TableSet.load(str(tmp_path), "cpu")
        p.write_bytes(raw[:70000] + bytes([raw[70000] ^ 1]) + raw[70001:])
        with pytest.raises(ValueError, match="wrong checksum"):
            TB.TableSet.load(str(tmp_path), "cpu")
        p.write_bytes(b"BOGB" + raw[4:])
        with pytest.raises(ValueError, match="not a tablebase file"):
            TB.TableSet.load(str(tmp_path), "cpu")


def test_probe_rescore_and_command_line_with_the_uploaded_table(tmp_path):
    with H.emulator_backend():
        ts = krk_set()
    ts.payload = {"KRK": ts.tables["KRK"].download()}
    TC.check_probe("emu", ts, ("KRK",), n_sample=300)
    with H.emulator_backend():
        wdl, dtm, status = ts.probe([TB.position_from_fen(f) for f in ("8/8/8/8/8/2k5/8/K6R w - - 0 1", "4k3/4p3/8/8/8/8/8/4K3 w - - 0 1",
                                                                       "4k3/8/8/8/8/8/PP6/K6R w - - 0 1", "4k3/8/8/8/8/8/8/4K2R w K - 0 1",
                                                                       "4k3/4p3/8/8/8/8/4P3/4K3 w - - 0 1", "4k3/8/8/8/8/8/8/4KN2 b - - 0 1")])
    assert status.tolist() == [TB.COVERED, TB.NO_TABLE, TB.TOO_MANY_MEN, TB.CASTLING, TB.PAWNS_BOTH, TB.COVERED]
    assert wdl[0] == 0 and dtm[0] == 0 and wdl[5] == 0 and dtm[5] == 0
    TC.check_rescore("emu", ts, tmp_path, complete=False)
    # the command line: probe, verify is left to the GPU (a Bellman check of KRK is a full pass), rescore
    tb_dir = tmp_path / "TB"
    with H.emulator_backend():
        ts.save(str(tb_dir))
        ts.close()
        out = io.StringIO()
        assert TB.main(["probe", "--dir", str(tb_dir), "--device", "cpu", "8/8/8/8/8/2k5/8/K6R w - - 0 1", "k6R/8/1K6/8/8/8/8/8 b - - 0 1",
                        "4k3/8/8/8/8/8/PP6/K6R w - - 0 1"], out=out) == 0
        lines = out.getvalue().splitlines()
        assert lines[0].endswith(": draw") and lines[1].endswith("loss for the side to move, mate in 0 plies (0 moves)")
        assert lines[2].endswith("not covered (too many men)")
        out = io.StringIO()
        assert TB.main(["rescore", str(tmp_path / "iter_0"), "--dir", str(tb_dir), "--device", "cpu"], out=out) == 0
        assert out.getvalue().splitlines() == ["4 games, 41 positions", "3 games reach a covered position (mean ply 1.0)",
                                               "0 recorded results disagree with the table at the first covered ply",
                                               "3 games would be cut, 30 plies saved"]
        out = io.StringIO()
        assert TB.main(["build", "KPKP", "--dir", str(tb_dir), "--device", "cpu"], out=out) == 2 and "follow-up" in out.getvalue()


def test_argument_errors_of_the_entry_points():
    lib = H.emu_lib()
    h = C.c_void_p()
    err = lambda: lib.bo_last_error().decode()
    assert lib.bo_tb_create(0, b"KQK", None, 0, None) == -1
    assert lib.bo_tb_create(0, b"QK", None, 0, C.byref(h)) == -1 and lib.bo_tb_create(0, b"KQRKR", None, 0, C.byref(h)) == -1 and "5 men" in err()
    assert lib.bo_tb_create(0, b"KPKP", None, 0, C.byref(h)) == -3 and "follow-up" in err()
    assert lib.bo_tb_create(0, b"KKQ", None, 0, C.byref(h)) == -1 and "write KQK" in err()      # the strong side comes first
    assert lib.bo_tb_create(0, b"KPKR", None, 0, C.byref(h)) == -1 and "write KRKP" in err() and not h.value
    TC.check_missing_sub_table("emu")
    assert lib.bo_tb_create(0, b"KQK", None, 0, C.byref(h)) == 0 and h.value
    sub = (C.c_void_p * 1)(h.value)
    q = C.c_void_p()
    assert lib.bo_tb_create(0, b"KPK", sub, 1, C.byref(q)) == -5 and "KQK is not complete" in err()  # given, but neither built nor uploaded
    codes = np.zeros(524288, np.uint16)
    pos, st = (E.BoPosition * 1)(), np.zeros(1, np.int32)
    assert lib.bo_tb_build(None, -1, None, None) == -1 and lib.bo_tb_verify(h, None, None) == -1 and lib.bo_tb_stats(h, None) == -1
    assert lib.bo_tb_download(h, codes.ctypes.data, 8192) == -1 and lib.bo_tb_upload(h, codes.ctypes.data, 8192, 0) == -1 and "524288" in err()
    assert lib.bo_tb_probe(sub, 1, C.addressof(pos), 1, codes.ctypes.data, st.ctypes.data, None) == -5 and "not complete" in err()
    assert lib.bo_tb_probe(sub, 65, C.addressof(pos), 1, codes.ctypes.data, st.ctypes.data, None) == -1
    assert lib.bo_tb_probe(None, 0, None, 0, None, None, None) == 0
    assert lib.bo_tb_probe(None, 0, C.addressof(pos), 1, codes.ctypes.data, st.ctypes.data, None) == 0 and st[0] == TB.NOT_A_POSITION
    assert lib.bo_tb_upload(h, codes.ctypes.data, 524288, 0) == 0
    assert lib.bo_tb_create(0, b"KQKR", sub, 1, C.byref(q)) == -5 and "KRK, which was not given" in err() and not q.value  # KQK is there, KRK is not
    lib.bo_tb_destroy(h)
    lib.bo_tb_destroy(None)


def test_library_and_python_name_the_same_sub_tables():
    """The material grammar lives twice, in bo_tb_create and in tablebase.children / closure.  For every supported 3- and 4-man material
    the library's BO_E_STATE message must name a table Python lists, until every table Python lists has been given; then it accepts.
    (Where the named table is a 4-man one, 64 MB, only that first name is compared.)"""
    import itertools
    import re

    lib = H.emu_lib()
    zeros = np.zeros(524288, np.uint16)
    made = {}

    def create(name, subs):
        h = C.c_void_p()
        arr = (C.c_void_p * max(1, len(subs)))(*[made[s].value for s in subs])
        return lib.bo_tb_create(0, name.encode(), arr, len(subs), C.byref(h)), h

    def complete_table(name):  # a 3-man table with its sub-tables, counted as complete once uploaded
        if name not in made:
            subs = [c for c in TB.children(name) if not TB.needs_no_table(c)]
            for c in subs:
                complete_table(c)
            rc, h = create(name, subs)
            assert rc == 0, (name, lib.bo_last_error())
            assert lib.bo_tb_upload(h, zeros.ctypes.data, zeros.size, 0) == 0
            made[name] = h
        return name

    pieces = "QRBNP"
    names = ["K" + x + "K" for x in pieces] + ["K" + x + y + "K" for x, y in itertools.combinations_with_replacement(pieces, 2)]
    names += ["K" + x + "K" + y for x, y in itertools.combinations_with_replacement(pieces, 2) if x + y != "PP"]
    assert len(names) == 5 + 15 + 14 and all(TB.canonical(n) == n for n in names)
    for name in names:
        need = [c for c in TB.children(name) if not TB.needs_no_table(c)]
        assert set(need) <= set(TB.closure([name])[:-1])  # (closure holds them, with the sub-tables of sub-tables)
        given = []
        while True:
            rc, h = create(name, given)
            if rc == 0:
                lib.bo_tb_destroy(h)
                assert sorted(given) == sorted(need), (name, given, need)
                break
            assert rc == -5, (name, rc, lib.bo_last_error())
            missing = re.search(r"needs the sub-table (\w+), which was not given", lib.bo_last_error().decode()).group(1)
            assert missing in need and missing not in given, (name, missing, need)
            if len(TB.piece_list(missing)) > 3:
                break
            given.append(complete_table(missing))
    for h in reversed(list(made.values())):
        lib.bo_tb_destroy(h)
