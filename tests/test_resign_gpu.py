"""GPU tests (MI355X): resignation and per-ply root values with a real evaluate stage (hash_init_ net, hand-written tower kernels,
hipGraph-captured step).  The device-made turn resigns the games the host-made turn resigns, with the same v_i bits; a
`selfplay_main --records compact --resign-threshold` run writes BOG2 records that feed the betaone_amd.resign report and the PGN
converter, whose eval comments parse back to the recorded values (PGN reader and the device ingest)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (a random-init net's root values sit close to 0: a threshold this high makes every enabled game resign within its first plies, and
# the check games run to the move limit)
RESIGN = dict(resign_threshold=0.5, resign_plies=2, resign_check_fraction=0.25)


def _net():
    import torch

    from betaone_amd import dropin

    dropin.install()
    import config
    import network
    from betaone_amd.fused_net import FusedPolicyValueNet
    from fake_model import hash_init_

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 3, 1, 64
    try:
        net = hash_init_(network.PolicyValueNet().eval()).to("cuda:0")
        return FusedPolicyValueNet(net, conv="tower_wg").to("cuda:0")
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
        torch.cuda.synchronize()


def _play(net, device_turn, cohorts=1, G=16, n_games=28, plies=60):
    from betaone_amd.rollout import CohortRollout, Rollout

    kw = dict(num_simulations=50, mcts_batch_size=48, device="cuda:0", rng_mode="native", max_game_moves=30, **RESIGN)
    ro = CohortRollout(net, G, cohorts=cohorts, **kw) if cohorts > 1 else Rollout(net, G, **kw)
    parts = ro.parts if cohorts > 1 else [ro]
    for p in parts:
        p.device_turn = device_turn
    ro.start_games(list(range(G)), list(range(G)), [900 + g for g in range(G)])
    nxt, fins = [G], {}

    def refill(slot):
        if nxt[0] >= n_games:
            return None
        nxt[0] += 1
        return nxt[0] - 1, 900 + nxt[0] - 1, None

    for _ in range(plies):
        ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f), refill=refill)
    if cohorts > 1:
        ro.drain()
    states = [p.eng.rng_get_state(g)[1][:8].tolist() for p in parts for g in range(p.G)]
    for p in parts:
        p.eng.check_status()
    ro.close()
    return fins, states


def test_device_turn_resigns_like_the_host_turn_on_the_gpu():
    from test_resign_emu import _first_firing, _key

    net = _net()
    a, sa = _play(net, False)
    b, sb = _play(net, True)
    assert _key(a) == _key(b) and sa == sb
    assert len(a) >= 20 and any(f.terminal == 3 for f in a.values())
    for f in a.values():
        fire = _first_firing(f.root_values, RESIGN["resign_threshold"], RESIGN["resign_plies"])
        if f.resign_check:
            assert f.terminal != 3
        else:
            assert fire is None
    c, _ = _play(net, True, cohorts=2)
    assert _key(c) == _key(a)


def test_selfplay_with_resignation_report_and_pgn(tmp_path):
    import torch

    from betaone_amd import dropin
    from betaone_amd import pgn as P
    from betaone_amd import pgn_write as W
    from betaone_amd import records as R
    from betaone_amd import resign as RS
    from betaone_amd import selfplay_main as M
    from test_resign_emu import check_pgn_eval_comments

    dropin.install()
    import config

    keys = ("RESIDUAL_BLOCKS", "SE_RESIDUAL_BLOCKS", "CONV_FILTERS", "NUM_SIMULATIONS", "MCTS_BATCH_SIZE", "DATA_DIR", "SAVE_DIR", "MAX_GAME_MOVES")
    saved = {k: getattr(config, k) for k in keys}
    try:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 3, 1, 64
        config.NUM_SIMULATIONS, config.MCTS_BATCH_SIZE, config.MAX_GAME_MOVES = 50, 48, 40
        config.DATA_DIR, config.SAVE_DIR = str(tmp_path / "data"), str(tmp_path / "models")
        torch.manual_seed(0)
        M.main(["--iteration", "1", "--games", "12", "--slots", "12", "--records", "compact", "--resign-threshold", "0.99",
                "--resign-plies", "2", "--resign-check-fraction", "0.25"])
    finally:
        for k, v in saved.items():
            setattr(config, k, v)
    d = os.path.join(str(tmp_path / "data"), "iter_1")
    path = R.compact_path(str(tmp_path / "data"), 1, 0)
    with open(path, "rb") as fh:
        assert fh.read(4) == b"BOG2"
    games = sorted(R.load_games(path), key=lambda g: g["game_id"])
    assert len(games) == 12 and all(g["root_values"] is not None and len(g["root_values"]) == g["n_plies"] for g in games)
    assert any(g["terminal"] == 3 for g in games)
    rep = RS.main([d, "--threshold", "0.99", "--plies", "2", "--json"])
    assert rep["games"] == 12 and rep["resigned"] == sum(g["terminal"] == 3 for g in games)
    assert rep["check_games"] == sum(1 for g in games if g["resign_check"] and g["terminal"] != 3)
    out = tmp_path / "it1.pgn"
    assert W.main([path, "-o", str(out), "--date", "2026.10.16", "--sims", "50"]) == 0
    text = out.read_text()
    assert check_pgn_eval_comments(games, text, 50) > 0
    # the device ingest takes every ply whose next move carries an eval as a sample
    ex = P.parse_text(text).export()
    want = 0
    for k in range(len(games)):
        a, b = int(ex["tok_off"][k]), int(ex["tok_off"][k + 1])
        want += int(np.count_nonzero(ex["has_eval"][a + 1:b]))
    ing = P.PgnIngest([str(out)], device="cuda:0", window_plies=4096, workers=1)
    assert ing.count() == want > 0
    print(json.dumps({k: rep[k] for k in ("games", "resigned", "plies", "check_games", "false_positives")}))
