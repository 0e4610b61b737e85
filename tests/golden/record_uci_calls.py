#!/usr/bin/env python3
"""
tests/golden/record_uci_calls.py -- produces tests/golden/g6_uci_calls.json from a checkout of the reference project.

Runs the UNMODIFIED reference uci.py over a short UCI session on top of the drop-in modules (betaone_amd/dropin, with
oracle/shim standing in for python-chess and the wave-emulator build behind mcts.run_mcts) and records every call uci.py
makes into them: the config names it reads, how it builds and loads the net, every RepetitionTracker it makes and every
board it adds, and every run_mcts(board, model, history, tracker) with its arguments (boards as start FEN + UCI moves).
tests/test_reference_callers.py replays that call sequence on the drop-in modules; the reference file itself stays
outside the repository.

    python tests/golden/record_uci_calls.py <directory of the reference project (kevinh-e/BetaOne)>
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "g6_uci_calls.json")

# the session the fixture records (and tests/test_reference_callers.py's expectations follow it)
SESSION = [("uci", "uciok"), ("isready", "readyok"),
           ("position startpos moves e2e4 e7e5 g1f3", "info string Position set"), ("go movetime 300", "bestmove"),
           ("position fen r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1", "info string Position set"),
           ("go movetime 200", "bestmove"), ("quit", None)]

BOOT = r"""
import atexit, json, os, sys, types
root, uci, out = {root!r}, {uci!r}, {out!r}
sys.path[:0] = [os.path.join(root, "betaone_amd", "dropin"), os.path.join(root, "oracle", "shim"), root, os.path.join(root, "tests")]
import torch
import config
config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 1, 32
config.NUM_SIMULATIONS = 120
import network, mcts, utils
from engine_harness import emulator_backend
_emu = emulator_backend(); _emu.__enter__()
os.makedirs("checkpoints", exist_ok=True)
torch.manual_seed(0)
torch.save(network.PolicyValueNet().state_dict(), os.path.join("checkpoints", "stable_model(half).pth"))

calls = []
atexit.register(lambda: json.dump(calls, open(out, "w")))
stack = lambda b: list(mcts.board_to_stack(b))          # (start FEN, "uci moves" or None)


class Config(types.ModuleType):                          # what uci.py reads of config
    def __getattr__(self, name):
        calls.append({{"op": "config", "name": name}})
        return getattr(config, name)


sys.modules["config"] = Config("config")
trackers = []


class RepetitionTracker(utils.RepetitionTracker):
    def __init__(self):
        super().__init__()
        trackers.append(self)
        calls.append({{"op": "tracker", "tracker": len(trackers) - 1}})

    def add_board(self, board):
        calls.append({{"op": "add_board", "tracker": trackers.index(self), "board": stack(board)}})
        super().add_board(board)


utils.RepetitionTracker = RepetitionTracker


class PolicyValueNet(network.PolicyValueNet):
    def __init__(self, *a, **k):
        calls.append({{"op": "net", "args": len(a) + len(k)}})
        super().__init__(*a, **k)

    def to(self, *a, **k):
        calls.append({{"op": "net.to", "device": str(a[0] if a else k.get("device"))}})
        return super().to(*a, **k)

    def load_state_dict(self, sd, *a, **k):
        calls.append({{"op": "net.load_state_dict"}})
        return super().load_state_dict(sd, *a, **k)

    def eval(self):
        calls.append({{"op": "net.eval"}})
        return super().eval()


network.PolicyValueNet = PolicyValueNet
_run = mcts.run_mcts


def run_mcts(board, model, history, tracker):
    rec = {{"op": "run_mcts", "board": stack(board), "history": [stack(b) for b in history], "tracker": trackers.index(tracker)}}
    best, pi = _run(board, model, history, tracker)
    rec["best"] = best.uci() if best else None
    calls.append(rec)
    return best, pi


mcts.run_mcts = run_mcts
import runpy
runpy.run_path(uci, run_name="__main__")
"""


def main():
    uci = os.path.join(sys.argv[1], "uci.py")
    with tempfile.TemporaryDirectory() as tmp:
        trace = os.path.join(tmp, "calls.json")
        p = subprocess.Popen([sys.executable, "-u", "-c", BOOT.format(root=ROOT, uci=uci, out=trace)], cwd=tmp,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        for cmd, expect in SESSION:
            p.stdin.write(cmd + "\n")
            p.stdin.flush()
            t0 = time.time()
            while expect is not None:
                line = p.stdout.readline()
                assert line or p.poll() is None, "uci.py ended early"
                assert time.time() - t0 < 300, f"no {expect!r} from uci.py"
                if line.startswith(expect):
                    break
        p.wait(timeout=60)
        assert p.returncode == 0, p.returncode
        calls = json.load(open(trace))
    # a search thread's run_mcts calls (and its config read after each) repeat until its time limit: the fixture keeps the
    # first two of each search -- the one uci.py always makes and one repeat with the same arguments
    kept, last, count, dropping = [], None, 0, False
    for c in calls:
        if c["op"] == "run_mcts":
            key = (json.dumps(c["board"]), json.dumps(c["history"]), c["tracker"])
            count = count + 1 if key == last else 1
            last, dropping = key, count > 2
        elif c["op"] != "config":
            last, count, dropping = None, 0, False
        if not dropping:
            kept.append(c)
    with open(OUT, "w") as f:
        json.dump({"source": "reference uci.py, session below, on the drop-in modules", "session": [c for c, _ in SESSION],
                   "calls": kept}, f, indent=1)
    print(f"{OUT}: {len(kept)} calls ({sum(c['op'] == 'run_mcts' for c in kept)} run_mcts)")


if __name__ == "__main__":
    main()
