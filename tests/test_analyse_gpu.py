"""GPU tests of the analysis path (csrc/bo_analyse.h, betaone_amd/analyse.py) on an MI355X: the bodies of tests/test_analyse_emu.py on
the product library, the command end to end with a small random-init PolicyValueNet on the hand-written evaluate stage, and slot reuse
under the pipeline (many small batches against one large one, bit for bit)."""
import json
import os

import numpy as np
import pytest
import torch

import analyse_cases as AC

from betaone_amd import engine as E

pytestmark = pytest.mark.gpu


def test_setup_from_the_device_equals_setup_from_strings_every_ply_gpu():
    games, text = AC.make_corpus()
    st = AC.check_setup_and_analysis("hip", games, text, G=64, sims=24, batch=8, oracle_every=20)
    assert st["compared"] == sum(len(m) for _, m in games)
    assert st["oracle"] >= 100 and st["code2"] >= 2 and st["ties"] >= 1, st


def test_capacity_and_ranges_gpu():
    assert AC.check_capacity("hip")


def _net():
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 2, 1, 64
    try:
        torch.manual_seed(3)
        net = network.PolicyValueNet().eval()
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    return net


def test_the_command_end_to_end_and_into_pretrain_gpu(tmp_path, capsys):
    import test_analyse_emu as TE
    from betaone_amd import analyse as A
    from betaone_amd import pretrain

    games, text = AC.make_corpus(seed=9, n_random=6, max_plies=40)
    src = tmp_path / "in.pgn"
    src.write_text(text)
    ck = tmp_path / "net.pth"
    torch.save(_net().state_dict(), ck)
    sims, outs = 48, []
    for run in range(2):
        o, j, r = (tmp_path / f"{n}{run}" for n in ("out.pgn", "pos.jsonl", "report.json"))
        assert A.main([str(src), "--model", str(ck), "-o", str(o), "--sims", str(sims), "--slots", "64", "--jsonl", str(j), "--report", str(r)]) == 0
        outs.append((o, j, r))
    assert "[analyse] games" in capsys.readouterr().out
    assert open(outs[0][0], "rb").read() == open(outs[1][0], "rb").read() and open(outs[0][1], "rb").read() == open(outs[1][1], "rb").read()
    lib = E.load_hip_library()
    eng = E.Engine(1, num_simulations=1, max_plies=8)

    def movegen(lines):
        dev = torch.device("cuda:0")
        ing = A.Ingested(lib, dev, "in", text.encode())
        ing.finish(lib, dev)
        pos = A.ring_to_positions(ing.pos_host[:ing.n_roots])
        mv, _ = eng.movegen([pos[i] for i in range(ing.n_roots)])
        return [[E.move_to_uci(m) for m in row] for row in mv]

    lines, rep = TE.check_command_outputs(lib, text, *outs[0], sims, movegen)
    assert rep["games_read"] == len(games) and rep["batches"] > 3 and rep["positions_per_second"] > 0
    data = tmp_path / "pgn"
    data.mkdir()
    os.replace(outs[0][0], data / "annotated.pgn")
    assert pretrain.main([str(src), "--count", "--batch", "32"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["samples"] == 0
    out = tmp_path / "s.json"
    assert pretrain.main([str(data), "--save-dir", str(tmp_path / "ck"), "--batch", "32", "--max-steps", "1", "--workers", "1", "--out", str(out),
                          "--init", str(ck)]) == 0
    s = json.load(open(out))
    assert s["steps"] == 1 and s["counts"]["samples"] >= 32


def test_slot_reuse_under_the_pipeline_gpu():
    """(g): more roots than three batches at 64 slots against one batch that holds them all -- the same roots in different slots and
    batch compositions, bit for bit."""
    from betaone_amd import analyse as A

    games, text = AC.make_corpus(seed=12, n_random=8, max_plies=60)
    n_roots = sum(len(m) for _, m in games)
    assert n_roots > 3 * 64
    net = _net().to("cuda:0")
    a = A.analyse_games(text, net, sims=48, slots=64)
    b = A.analyse_games(text, net, sims=48, slots=n_roots)
    assert a["report"]["batches"] > 3 and b["report"]["batches"] == 1
    assert a["report"]["positions_analysed"] == b["report"]["positions_analysed"] > 0
    for ga, gb in zip(a["games"], b["games"]):
        assert ga["plies"].tobytes() == gb["plies"].tobytes(), ga["index"]
