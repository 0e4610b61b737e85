"""MI355X tests of the endgame tablebases: complete builds of KQK, KRK, KPK (with its closure) and KBNK against the published DTM
maxima, the device's Bellman check, byte-identical rebuilds, a sample of every table against the oracle's rules through the host's
index function, the probe with its mirror and statuses, rescoring a synthetic record file, and the missing sub-table error."""
import pytest

import tablebase_cases as TC

pytestmark = pytest.mark.gpu

THREE = ("KQK", "KRK", "KPK")


def three():
    return TC.built("hip", THREE)


@pytest.mark.parametrize("name,all_strong_wins", [("KQK", True), ("KRK", True), ("KPK", False)])
def test_complete_build(name, all_strong_wins):
    ts = three()
    assert list(ts.tables) == ["KQK", "KRK", "KPK"]
    TC.check_complete_build("hip", ts, name, all_strong_wins)


@pytest.mark.parametrize("name", THREE)
def test_sampled_entries_follow_from_the_oracles_moves(name):
    assert TC.check_against_the_oracle(three().payload, name, 5000) == 5000


def test_kbnk():
    """One 4-man table: 33 554 432 entries; captures lead to KBK / KNK / KK, so its closure is empty."""
    ts = TC.built("hip", ("KBNK",))
    assert list(ts.tables) == ["KBNK"]
    TC.check_complete_build("hip", ts, "KBNK", False)


def test_probe_returns_the_stored_code_also_for_the_mirror():
    TC.check_probe("hip", three(), THREE)
    TC.check_probe_statuses("hip", three())


def test_rescore(tmp_path):
    TC.check_rescore("hip", three(), tmp_path)


def test_missing_sub_table_is_named():
    TC.check_missing_sub_table("hip")


def test_command_line_build_and_verify(tmp_path):
    """`build` prints per table its passes, seconds and the stats line and writes NAME.botb; `verify` prints a line per table."""
    import io
    import re

    from betaone_amd import tablebase as TB

    out = io.StringIO()
    assert TB.main(["build", "KQK", "--dir", str(tmp_path)], out=out) == 0
    lines = out.getvalue().splitlines()
    info = three().tables["KQK"].info()
    assert len(lines) == 2 and re.fullmatch(rf"KQK: {info['passes']} passes, \d+\.\d{{3}} s", lines[0]), lines
    assert lines[1] == TB.stats_line(info) and "largest win 19 plies" in lines[1] and f"fnv1a 0x{info['fnv1a']:016x}" in lines[1]
    assert (tmp_path / "KQK.botb").stat().st_size == 64 + 2 * 524288
    out = io.StringIO()
    assert TB.main(["verify", "--dir", str(tmp_path)], out=out) == 0
    assert out.getvalue().splitlines() == ["KQK: 0 mismatches"]
    raw = bytearray((tmp_path / "KQK.botb").read_bytes())
    head, codes = TB.read_table(str(tmp_path / "KQK.botb"))
    wrong = codes.copy()
    i = int((codes == 3).nonzero()[0][0])
    wrong[i] = 5  # a mate in 1 stored as a mate in 3: one entry, and every parent that relied on it
    ts = TB.TableSet("cuda:0")
    t = ts.add("KQK")
    t.upload(wrong, head["passes"])
    assert t.verify() >= 1
    ts.close()
