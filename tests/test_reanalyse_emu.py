"""CPU tests (wave emulator) of reanalysis: ring entries made from bo_position (bo_records_ring) against the PGN replay's, the reanalysis
record (bo_reanalysis_result) against bo_search_result and against a NumPy float64 restatement, and betaone_amd.reanalyse end to end --
reanalysing with the net that played gives the input files back byte for byte, another net changes only pi and root values and every
new pi is the pi of the same root set up from strings, --fraction, the command line."""
import io
import json
import os

import numpy as np
import pytest
import torch

import engine_harness as H
import reanalyse_cases as RC
from fake_model import FakeNet, fake_logits_values

from betaone_amd import engine as E
from betaone_amd import records as R

SIMS, BATCH, G, MOVES = 12, 8, 4, 6
SEARCH = dict(mcts_batch_size=BATCH, cpuct=1.0, widen_coeff=1.5, dirichlet_epsilon=0.25)


def test_ring_entries_from_records_equal_the_pgn_replay_s():
    assert RC.check_ring_bytes("emu") > 2000


def test_record_against_search_result():
    widest = two = 0
    for widen in (1.5, 6.0):                                        # the reference's widening; a root with more than two children
        for flat in (True, False):                                  # all ties; a softmax of hashed logits
            n, t = RC.check_record_against_search_result("emu", widen, flat)
            widest, two = max(widest, n), two + t
    assert widest > 2 and two >= 1


def test_old_against_new_bit_for_bit():
    RC.check_old_against_new("emu")


def test_entry_points_refuse_what_they_do_not_cover():
    with H.emulator_backend():
        fast = E.Engine(2, num_simulations=8, fast=True, leaves_per_step=4, max_plies=32)
        plain = E.Engine(2, num_simulations=8, dirichlet_alpha=0.0, max_plies=32)
    a = np.zeros(256, np.int64).ctypes.data
    for eng, code in ((fast, -3), (plain, -5)):                      # BO_E_CONFIG: fast mode; BO_E_STATE: root values are off
        assert eng.lib.bo_reanalysis_result(eng.h, None, None, None, None, None, 8, a, a, a, 0) == code
        with pytest.raises(E.EngineError):
            eng.reanalysis_result(0, 0, 0, 0, 0, 8, a, a, a)
    assert H.emu_lib().bo_records_ring(None, 4, a, 0) == -1 and H.emu_lib().bo_records_ring(a, -1, a, 0) == -1


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _play(tmp, name, n_games=5, **rkw):
    """A few short self-play games of FakeNet() on the emulator, saved as DATA/<name>/iter_3/games_rank0.bog."""
    from betaone_amd.rollout import Rollout

    fins = {}
    with H.emulator_backend():
        ro = Rollout(FakeNet(), G, num_simulations=SIMS, dirichlet_alpha=0.0, device="cpu", use_graph=False, rng_mode="native",
                     policy_kind="logits", temperature=(3, 1.0, 0.1), max_game_moves=MOVES, **SEARCH, **rkw)
        ro.start_games(list(range(G)), list(range(G)), [900 + g for g in range(G)])
        nxt = [G]

        def refill(slot):
            if nxt[0] >= n_games:
                return None
            nxt[0] += 1
            return nxt[0] - 1, 900 + nxt[0] - 1, None

        for _ in range(4 * MOVES):
            ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f), refill=refill)
            if len(fins) == n_games:
                break
        ro.eng.check_status()
        ro.close()
    assert len(fins) == n_games
    d = tmp / name / "iter_3"
    R.save_games(str(d / "games_rank0.bog"), [fins[g] for g in sorted(fins)])
    return d


def _reanalyse(src, out, model=None, **kw):
    from betaone_amd import reanalyse as RA

    with H.emulator_backend():
        return RA.reanalyse_records([str(src)], model or FakeNet(), str(out), sims=SIMS, slots=G, device="cpu", **SEARCH, **kw)


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reanalyse")
    return tmp, _play(tmp, "bog1"), _play(tmp, "bog2", record_values=True)


def _bytes(d):
    return [open(p, "rb").read() for p in RC.bog_files(d)]


def test_the_net_that_played_gives_the_files_back(played):
    """(4) a self-play search is a function of its root and the net: same net, simulations, constants and slots -> the same bytes."""
    tmp, d1, d2 = played
    assert all(g["root_values"] is None for g in RC.games_of(d1)) and all(g["root_values"] is not None for g in RC.games_of(d2))
    for d, name in ((d1, "same1"), (d2, "same2")):
        rep = _reanalyse(d, tmp / name)
        assert _bytes(tmp / name / "iter_3") == _bytes(d)
        n = sum(g["n_plies"] for g in RC.games_of(d))
        assert rep["roots_searched"] == n > 12 and rep["roots_kept"] == 0 and rep["mean_tv"] == 0.0 and rep["top1_agreement"] == 1.0
        assert rep["batch_copy_bytes"] == G * (64 + 8 * 8)
    assert rep["mean_abs_dq"] == 0.0 and rep["q_sign_changed_share"] == 0.0 and rep["roots_with_values"] == n
    # --values turns a record without root values into one with them (flags 0): the values the BOG2 run of the same games recorded
    _reanalyse(d1, tmp / "vals", values=True)
    assert _bytes(tmp / "vals" / "iter_3") == _bytes(d2)


def _pi_from_strings(games, salt):
    """Every root of `games` set up from FEN + UCI strings (bo_games_reset) and searched with FakeNet(salt=salt)'s logits."""
    roots = [(g, k) for g in games for k in range(g["n_plies"])]
    eng = H.make_engine("emu", G, dict(num_simulations=SIMS, batch_size=BATCH, dirichlet_alpha=0.0), max_plies=MOVES + 4)
    eng.root_values(True)
    nn_in, pol, val = H.Buf("emu", (G, 120, 8, 8)), H.Buf("emu", (G, E.NUM_ACTIONS)), H.Buf("emu", (G,))
    out = {}
    for b0 in range(0, len(roots), G):
        part = roots[b0:b0 + G]
        n = len(part)
        eng.reset(list(range(n)), [None] * n, [" ".join(E.move_to_uci(int(m)) for m in g["moves"][:k]) or None for g, k in part])
        _, term, _ = eng.root_info()
        go = np.zeros(G, np.int32)
        go[:n] = term[:n] == 0
        eng.search_begin(go, None, nn_in.ptr)
        eng.step(0, 0, E.POLICY_NONE, nn_in.ptr)
        while True:
            running, _, mask = eng.poll()
            if running == 0:
                break
            logits, v = fake_logits_values(nn_in.numpy(), 6.0, salt)
            pol.set(logits)
            val.set(v)
            eng.step(pol.ptr, val.ptr, E.POLICY_LOGITS, nn_in.ptr)
        res, rv = eng.result(), eng.search_root_value()
        for j, (g, k) in enumerate(part):
            m = int(res["n"][j])
            out[(g["game_id"], k)] = (res["idx"][j, :m].copy(), res["val"][j, :m].copy(), rv[j].copy()) if go[j] else None
    return out


def test_another_net_changes_only_the_targets(played):
    tmp, _, d2 = played
    rep = _reanalyse(d2, tmp / "other", model=FakeNet(salt=5))
    old, new = RC.games_of(d2), RC.games_of(tmp / "other" / "iter_3")
    RC.same_but_targets(old, new)
    want = _pi_from_strings(old, 5)
    differ = 0
    for go, gn in zip(old, new):
        for k in range(gn["n_plies"]):
            w = want[(gn["game_id"], k)]
            assert w is not None
            assert np.array_equal(gn["pis"][k][0], w[0]) and np.array_equal(gn["pis"][k][1].view(np.uint32), w[1].view(np.uint32))
            assert gn["root_values"][k:k + 1].view(np.uint32)[0] == w[2].view(np.uint32)
            differ += int(not (np.array_equal(gn["pis"][k][0], go["pis"][k][0]) and np.array_equal(gn["pis"][k][1], go["pis"][k][1])))
    assert differ >= 1 and rep["mean_tv"] > 0.0 and rep["mean_abs_dq"] > 0.0 and 0.0 <= rep["top1_agreement"] <= 1.0
    assert rep["roots_searched"] == sum(g["n_plies"] for g in old)


def test_fraction_selects_by_the_holdout_hash_alone(played):
    from betaone_amd import validate as V

    tmp, _, d2 = played
    blobs = {gid: (off, size) for gid, _n, off, size in R.scan_games(_bytes(d2)[0])}
    src = _bytes(d2)[0]
    F, K = 0.5, next(k for k in range(64) if 0 < sum(V.is_held_out(3, g, 0.5, k) for g in blobs) < len(blobs))
    picked = {g for g in blobs if V.holdout_hash(3, g, K) < F * 2 ** 64}
    # the same games in another file order
    rev = tmp / "rev" / "iter_3"
    rev.mkdir(parents=True)
    (rev / "games_rank0.bog").write_bytes(b"".join(src[blobs[g][0]:blobs[g][0] + blobs[g][1]] for g in sorted(blobs, reverse=True)))
    outs = []
    for d, name in ((d2, "frac"), (rev, "frac_rev")):
        rep = _reanalyse(d, tmp / name, model=FakeNet(salt=5), fraction=F, seed=K)
        assert rep["games_reanalysed"] == len(picked) and rep["games"] == len(blobs)
        o = _bytes(tmp / name / "iter_3")[0]
        outs.append({gid: o[off:off + size] for gid, _n, off, size in R.scan_games(o)})
    assert outs[0] == outs[1]                                        # a game's fate and bytes do not depend on the file's order
    full = _bytes(tmp / "other" / "iter_3")[0] if (tmp / "other").exists() else None
    for g, (off, size) in blobs.items():
        if g in picked:
            assert outs[0][g] != src[off:off + size]
        else:
            assert outs[0][g] == src[off:off + size]                 # copied byte for byte
    if full is not None:
        fo = {gid: full[off:off + size] for gid, _n, off, size in R.scan_games(full)}
        assert all(outs[0][g] == fo[g] for g in picked)


def _tiny(monkeypatch):
    from betaone_amd import dropin

    dropin.install()
    import config

    monkeypatch.setattr(config, "RESIDUAL_BLOCKS", 1)
    monkeypatch.setattr(config, "SE_RESIDUAL_BLOCKS", 0)
    monkeypatch.setattr(config, "CONV_FILTERS", 16)
    monkeypatch.setattr(config, "MCTS_BATCH_SIZE", BATCH)
    import network

    torch.manual_seed(5)
    return network.PolicyValueNet().eval()


def test_the_command_line(played, tmp_path, monkeypatch, capsys):
    from betaone_amd import reanalyse as RA

    tmp, d1, d2 = played
    ck = tmp_path / "net.pth"
    torch.save(_tiny(monkeypatch).state_dict(), ck)
    # a file whose writer was killed inside a record, and a game without plies in front of it
    src = tmp_path / "data" / "iter_3"
    src.mkdir(parents=True)
    whole = _bytes(d2)[0]
    empty = R.unpack_games(whole)[0]
    zero = np.array([R.MAGIC, 99, 0, 0, 0, 0], np.int32).tobytes() + bytes(empty["positions"])[:R.POS_BYTES] + np.zeros(1, np.int32).tobytes()
    (src / "games_rank0.bog").write_bytes(zero + whole + whole[:100])
    out, rep_path, buf = tmp_path / "out", tmp_path / "report.json", io.StringIO()
    args = [str(src), "--model", str(ck), "-o", str(out), "--sims", str(SIMS), "--slots", "5", "--report", str(rep_path), "--device", "cpu"]
    with H.emulator_backend():
        assert RA.main(args, out=buf) == 0
        rep = json.load(open(rep_path))
        line = buf.getvalue()
        assert line.startswith("[reanalyse] games 6 (reanalysed 6)  roots searched ") and "mean |dq|" in line and line.endswith(f"roots/s at {SIMS} simulations\n")
        got = (out / "iter_3" / "games_rank0.bog").read_bytes()
        assert got[:len(zero)] == zero and len(R.scan_games(got)) == 6 and len(got) == len(zero) + len(whole)    # the tail is cut, the empty game copied
        RC.same_but_targets(R.unpack_games(zero + whole), R.unpack_games(got))
        n = sum(g["n_plies"] for g in R.unpack_games(whole))
        assert rep["roots_searched"] + rep["roots_kept"] == rep["roots"] == n and rep["batches"] >= -(-n // 5) and rep["roots_retried"] >= 0
        for key in ("mean_tv", "top1_agreement", "mean_played_prob", "mean_abs_dq", "q_sign_changed_share", "roots_per_second"):
            assert rep[key] is not None
        # refusals: an existing output file; an output directory that is, or lies inside, an input directory; a pi wider than the rows
        assert RA.main(args, out=buf) == 2 and "exists already" in capsys.readouterr().err
        for o in (src, src / "sub", src.parent / "iter_3" / "x" / "y"):
            assert RA.main(args[:3] + ["-o", str(o)] + args[5:], out=buf) == 2
            assert "inside" in capsys.readouterr().err
        assert not (src / "sub").exists()
        assert RA.main([str(tmp_path / "data"), "--model", str(ck), "-o", str(tmp_path / "o2"), "--device", "cpu"], out=buf) == 2
        with pytest.raises(ValueError):
            RA.reanalyse_records([str(src)], FakeNet(), str(tmp_path / "o3"), sims=SIMS, slots=G, device="cpu", fast=True)
    capsys.readouterr()


def test_a_pi_wider_than_the_rows_names_the_flag(played, tmp_path):
    from betaone_amd import reanalyse as RA

    tmp, d1, _ = played
    with H.emulator_backend():
        with pytest.raises(E.EngineError, match="--pi-width"):     # widen_coeff 6: roots with three children, rows of one entry
            RA.reanalyse_records([str(d1)], FakeNet(), str(tmp_path / "w"), sims=SIMS, slots=G, pi_width=1, device="cpu",
                                 **{**SEARCH, "widen_coeff": 6.0})
    assert not os.path.exists(tmp_path / "w" / "iter_3" / "games_rank0.bog")


def test_a_root_that_is_not_searched_keeps_its_pi(tmp_path):
    """A game that played on past a claimable draw has roots that are over (code 2): they keep the old pi and value and are counted;
    the other roots of the game get what analyse finds for the same positions of the PGN."""
    import types

    import analyse_cases as AC
    import pgn_util as U
    from betaone_amd import analyse as A
    from betaone_amd import reanalyse as RA

    text = "".join(U.write_game(AC._sans(None, m), [None] * len(m), "*") for m in (AC.REPETITION, AC.MATE))
    ing = RC.ingest("emu", text)
    fins = []
    for g in range(2):
        o, n = int(ing.tok_off[g]), int(ing.n_plies[g])
        w0 = int(ing.n_plies[:g].sum())
        act = ing.act.numpy()[o:o + n]
        fins.append(types.SimpleNamespace(
            game_id=40 + g, terminal=0, outcome=0.0, moves=[int(m) for m in ing.moves[w0:w0 + n]],
            positions=list(A.ring_to_positions(np.concatenate([ing.pos_host[o:o + n], ing.final[g][None]])))[:n + 1],
            pis=[(np.array([a], np.int32), np.array([1.0], np.float32)) for a in act], root_values=np.full(n, 0.25, np.float32)))
        assert np.array_equal(RA.moves_to_actions(np.array(fins[-1].moves)), act)          # the host's move -> action index
    src = tmp_path / "d" / "iter_1"
    R.save_games(str(src / "games_rank0.bog"), fins)
    with H.emulator_backend():
        rep = RA.reanalyse_records([str(src)], FakeNet(), str(tmp_path / "o"), sims=SIMS, slots=G, device="cpu", **SEARCH)
        ana = A.analyse_games(text, FakeNet(), sims=SIMS, slots=G, device="cpu", **SEARCH)
    old, new = RC.games_of(src), RC.games_of(tmp_path / "o" / "iter_1")
    RC.same_but_targets(old, new)
    kept = 0
    for go, gn, ga in zip(old, new, ana["games"]):
        for k in range(gn["n_plies"]):
            if ga["plies"]["phase"][k] == E.PH_DONE:
                assert gn["root_values"][k:k + 1].view(np.uint32)[0] == ga["plies"]["root_value"][k:k + 1].view(np.uint32)[0]
                assert abs(float(gn["pis"][k][1].sum()) - 1.0) < 1e-6
            else:
                kept += 1
                assert ga["plies"]["terminal"][k] == 2
                assert np.array_equal(gn["pis"][k][0], go["pis"][k][0]) and np.array_equal(gn["pis"][k][1], go["pis"][k][1])
                assert gn["root_values"][k] == np.float32(0.25)
    assert kept >= 2 and rep["roots_kept"] == kept and rep["roots_searched"] == 17 - kept
