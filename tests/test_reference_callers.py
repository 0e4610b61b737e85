"""The reference's own caller uci.py on top of the drop-in modules.

tests/golden/g6_uci_calls.json holds every call the UNMODIFIED uci.py made into the drop-in modules over a short UCI session
(recorded by tests/golden/record_uci_calls.py): the config names it reads, how it builds and loads the net, its
RepetitionTrackers and the boards it adds, and its run_mcts(board, model, history, tracker) calls.  This test makes the same
calls, in the same order, in a subprocess with sys.path = [betaone_amd/dropin, oracle/shim (stands in for python-chess, which
is not installed here), ...]; the engine behind mcts.run_mcts is the wave-emulator build (no GPU in this container)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = os.path.join(ROOT, "tests", "golden", "g6_uci_calls.json")

REPLAY = r"""
import json, os, sys
root, calls = {root!r}, json.load(open({calls!r}))["calls"]
sys.path[:0] = [os.path.join(root, "betaone_amd", "dropin"), os.path.join(root, "oracle", "shim"), root, os.path.join(root, "tests")]
import numpy as np
import torch
import chess
import config
config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 1, 32
config.NUM_SIMULATIONS = 120
import network, mcts, utils
from engine_harness import emulator_backend
_emu = emulator_backend(); _emu.__enter__()      # no GPU here: the emulator build of the same device code, for this whole process
os.makedirs("checkpoints", exist_ok=True)
torch.manual_seed(0)
torch.save(network.PolicyValueNet().state_dict(), os.path.join("checkpoints", "stable_model(half).pth"))


def board(rec):                                   # (start FEN, "uci moves" or None) -> a board with that move stack
    b = chess.Board(rec[0])
    for m in (rec[1] or "").split():
        b.push(b.parse_uci(m))
    return b


model, trackers, searched = None, [], []
for c in calls:
    op = c["op"]
    if op == "config":
        getattr(config, c["name"])
    elif op == "net":
        model = network.PolicyValueNet()
    elif op == "net.to":
        model = model.to(c["device"])
    elif op == "net.load_state_dict":
        path = os.path.join(config.SAVE_DIR, "stable_model(half).pth")
        model.load_state_dict(torch.load(path, map_location=config.DEVICE))
    elif op == "net.eval":
        model.eval()
    elif op == "tracker":
        assert c["tracker"] == len(trackers)
        trackers.append(utils.RepetitionTracker())
    elif op == "add_board":
        trackers[c["tracker"]].add_board(board(c["board"]))
    elif op == "run_mcts":
        root_board = board(c["board"])
        best, pi = mcts.run_mcts(root_board, model, [board(h) for h in c["history"]], trackers[c["tracker"]])
        assert best in root_board.legal_moves, (c["board"], best)
        assert pi.dtype == np.float32 and pi.shape == (4672,) and abs(float(pi.sum()) - 1.0) < 1e-5
        searched.append((root_board.fen(), best.uci()))
    else:
        raise AssertionError(op)
print(json.dumps(searched))
"""


def test_reference_uci_calls_replay_on_the_dropin_modules(tmp_path):
    calls = json.load(open(CALLS))["calls"]
    ops = [c["op"] for c in calls]
    # what the session made uci.py do: load the net, set two positions, search each (two run_mcts calls per search kept)
    assert ops.index("net") < ops.index("net.to") < ops.index("net.load_state_dict") < ops.index("net.eval") < ops.index("run_mcts")
    assert ops.count("run_mcts") >= 2 and any(c["op"] == "add_board" and c["board"][1] for c in calls)
    p = subprocess.run([sys.executable, "-c", REPLAY.format(root=ROOT, calls=CALLS)], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    searched = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(searched) == ops.count("run_mcts")
    starts = [c["board"] for c in calls if c["op"] == "run_mcts"]
    assert starts[0] == ["rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", "e2e4 e7e5 g1f3"]
    assert starts[-1][0] == "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
    for fen, mv in searched:
        assert len(mv) in (4, 5) and mv[0] in "abcdefgh" and mv[2] in "abcdefgh" and mv != "0000"
