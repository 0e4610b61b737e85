"""
betaone_amd/uci.py -- a UCI front end on the FAST search mode (csrc/bo_fastw.h): `python -m betaone_amd.uci --model best.pth`.

One fast-mode engine with one game slot; `evaluate -> bo_step` captured once as a graph and replayed with at most RUN_AHEAD replays in
flight; the search is ended through bo_search_stop (the step in flight is dropped) and looked at through bo_search_info (csrc/bo_info.h)
-- no host wait is added to a timed search.  Between moves the tree is kept: a `position` that extends the previous one plays the
new moves with bo_play, whose re-rooting keeps the played child's subtree.

This is NOT the reference's search (virtual loss, L distinct leaves per step, full-width expansion); the reference's semantics stay
available through the reference's own uci.py on the drop-in modules (betaone_amd.dropin).  Neither python-chess nor the reference is
imported here: moves are plain integers (from | to << 6 | promotion << 12), legality comes from the device's move generator.

UciEngine is usable without stdin: handle(line) takes one command, `out` receives every line the engine prints, wait() returns when
the search thread has nothing left to do.  All GPU work runs on that one thread.
"""
from __future__ import annotations

import argparse
import math
import queue
import sys
import threading
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as E

RUN_AHEAD = 4          # replays in flight, as in dropin/mcts.py
INFO_INTERVAL = 1.0    # seconds between two printed sets of info lines
LOOK_EVERY = 8         # steps between two looks at the search (bo_search_info + an event; the host only polls the event)
NAME = "BetaOne-AMD (fast search)"
STARTPOS = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# MaxNodes: the engine's num_simulations.  The arenas are sized for it (bo_engine_create: 24 granules of 128 bytes per possible expansion
# of this and of the previous search, two arenas); a link addresses 2^24 granules, which bounds it.
# Leaves: 64 is the fastest of 8 / 16 / 32 / 64 measured on the MI355X with the 8 + 2 SE x 128 net (profiles/uci.md).
OPTIONS = {"MultiPV": (1, 1, E.INFO_LINES), "Leaves": (64, 1, 64), "MaxNodes": (400000, 16, 690000), "MoveOverhead": (10, 0, 5000)}
_REBUILD = ("Leaves", "MaxNodes", "Model")
_QUEEN_DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
_KNIGHT_DIRS = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)]
_PROMO_DIRS = [(-1, 1), (0, 1), (1, 1)]


# ---- moves as plain integers -------------------------------------------------------------------------------------------------------
def parse_move(text: str) -> Optional[int]:
    """UCI text -> from | to << 6 | promotion << 12 (2 knight .. 5 queen), None when it is not a move's text."""
    if len(text) not in (4, 5) or text[0] not in "abcdefgh" or text[2] not in "abcdefgh" or text[1] not in "12345678" or text[3] not in "12345678":
        return None
    promo = 0
    if len(text) == 5:
        if text[4] not in "nbrq":
            return None
        promo = "nbrq".index(text[4]) + 2
    return (ord(text[0]) - 97 + 8 * (int(text[1]) - 1)) | (ord(text[2]) - 97 + 8 * (int(text[3]) - 1)) << 6 | promo << 12


def move_to_index(m: int) -> int:
    """The action index (from_square * 73 + plane) of a move: dropin/utils.move_to_index restated on plain integers."""
    f, t, promo = m & 63, (m >> 6) & 63, (m >> 12) & 7
    fr, ff = f >> 3, f & 7
    dr, df = (t >> 3) - fr, (t & 7) - ff
    if promo and promo != 5:
        key = (df, dr) if fr == 6 else (df, -dr)
        return f * 73 + 64 + (promo - 2) * 3 + _PROMO_DIRS.index(key)
    if (abs(dr), abs(df)) in ((1, 2), (2, 1)):
        return f * 73 + 56 + _KNIGHT_DIRS.index((dr, df))
    dist = max(abs(dr), abs(df))
    step = ((dr > 0) - (dr < 0), (df > 0) - (df < 0))
    return f * 73 + _QUEEN_DIRS.index(step) * 7 + dist - 1


# ---- the clock ---------------------------------------------------------------------------------------------------------------------
def parse_go(tokens: Sequence[str]) -> Dict:
    """`go` arguments -> {name: int | True}; unknown words are skipped, `searchmoves` swallows the moves behind it."""
    out: Dict = {}
    ints = ("movetime", "wtime", "btime", "winc", "binc", "movestogo", "nodes", "depth", "mate")
    i = 0
    while i < len(tokens):
        w = tokens[i]
        if w in ints and i + 1 < len(tokens):
            try:
                out[w] = int(float(tokens[i + 1]))
            except ValueError:
                pass
            i += 2
        elif w in ("infinite", "ponder"):
            out[w] = True
            i += 1
        elif w == "searchmoves":
            out[w] = True
            i += 1
            while i < len(tokens) and parse_move(tokens[i]) is not None:
                i += 1
        else:
            i += 1
    return out


def time_limit_ms(go: Dict, white_to_move: bool, overhead_ms: float = 0.0) -> Optional[float]:
    """The search's time in ms, a pure function of the `go` parameters and the side to move -- the reference's rule (uci.py:240-247):
    movetime x 0.95; else max(100, time / 30 + 0.9 inc) of the side to move; else 5 s; MoveOverhead is subtracted from each (at
    least 1 ms is left).  None: no clock (`infinite`, or `nodes` without a time)."""
    if go.get("infinite"):
        return None
    time_key, inc_key = ("wtime", "winc") if white_to_move else ("btime", "binc")
    if "movetime" in go:
        t = go["movetime"] * 0.95
    elif time_key in go:
        t = max(100.0, go[time_key] / 30.0 + 0.9 * go.get(inc_key, 0))
    elif "nodes" in go:
        return None
    else:
        t = 5000.0
    return max(1.0, t - overhead_ms)


def score_cp(w: float, visits: int) -> int:
    """The project's eval rule (pgn_write.eval_text) in centipawns: 100 * 2 ln((1 + v) / (1 - v)), v = w / visits, clamped to +-9999."""
    v = float(w) / visits if visits > 0 else 0.0
    if v >= 1.0:
        return 9999
    if v <= -1.0:
        return -9999
    return int(round(min(9999.0, max(-9999.0, 200.0 * math.log((1.0 + v) / (1.0 - v))))))


def format_info(rec, elapsed_s: float, multipv: int) -> List[str]:
    """The info lines of one bo_search_info record (E.INFO_DTYPE)."""
    nodes, ms = int(rec["sims_done"]), int(round(elapsed_s * 1000.0))
    nps = int(nodes / elapsed_s) if elapsed_s > 0 else 0
    hashfull = 1000 * int(rec["arena_top"]) // max(1, int(rec["arena_granules"]))
    out = []
    for i in range(min(int(rec["n_lines"]), multipv)):
        ln = rec["line"][i]
        n = int(ln["pv_len"])
        pv = " ".join(E.move_to_uci(int(m)) for m in ln["pv"][:n])
        out.append(f"info depth {n} multipv {i + 1} score cp {score_cp(float(ln['w']), int(ln['visits']))} nodes {nodes} nps {nps} "
                   f"time {ms} hashfull {hashfull} pv {pv}")
    return out


class _Look:
    """One bo_search_info record on its way to the host: device buffer -> pinned buffer + an event (CUDA); at once on a CPU backend."""

    def __init__(self, dev, G: int = 1):
        self.cuda = dev.type == "cuda"
        self.buf = torch.zeros((G, E.INFO_WORDS), dtype=torch.int32, device=dev)
        self.pinned = torch.zeros((G, E.INFO_WORDS), dtype=torch.int32, pin_memory=True) if self.cuda else self.buf
        self.event = torch.cuda.Event() if self.cuda else None
        self.busy, self.t = False, 0.0

    def enqueue(self, eng, n_lines: int, stream, t: float):
        eng.search_info(n_lines, self.buf.data_ptr(), stream.cuda_stream if self.cuda else 0)
        if self.cuda:
            self.pinned.copy_(self.buf, non_blocking=True)
            self.event.record(stream)
        self.busy, self.t = True, t

    def ready(self) -> bool:
        return self.busy and (not self.cuda or self.event.query())

    def take(self, wait: bool = False):
        if wait and self.cuda:
            self.event.synchronize()
        self.busy = False
        return self.pinned.numpy().copy().view(E.INFO_DTYPE).reshape(-1)[0]


class UciEngine:
    def __init__(self, out: Callable[[str], None] = None, model=None, device: str = "cuda:0", options: Optional[Dict] = None):
        """model: a checkpoint's path or a PolicyValueNet (None: `setoption name Model value PATH` before `isready`)."""
        self.out = out or (lambda s: print(s, flush=True))
        self.device_name = device
        self.opt: Dict = {k: v[0] for k, v in OPTIONS.items()}
        self.opt["Model"] = model
        self.opt.update(options or {})
        self.eng = None
        self.stale = True                       # an option that shapes the engine changed: rebuild at the next isready / go
        self.want = (STARTPOS, [])              # the last `position`
        self.have: Optional[Tuple[str, List[str]]] = None   # what the slot holds
        self.stop_event = threading.Event()
        self.searching = threading.Event()
        self.parked = threading.Event()         # set while a search that is over waits for `stop` (go infinite)
        self.jobs: "queue.Queue" = queue.Queue()
        self.thread = threading.Thread(target=self._work, name="betaone-uci-search", daemon=True)
        self.thread.start()
        self.alive = True
        self.last_search: Dict = {}             # of the most recent `go`: nodes, reused visits, steps, stopped_by

    # ---- the command side (any thread) -------------------------------------------------------------------------------------------
    def handle(self, line: str) -> bool:
        """One command; False after `quit`."""
        tok = line.split()
        if not tok:
            return True
        cmd, rest = tok[0], tok[1:]
        if cmd == "uci":
            self.out(f"id name {NAME}")
            self.out("id author betaone_amd")
            for k, (d, lo, hi) in OPTIONS.items():
                self.out(f"option name {k} type spin default {d} min {lo} max {hi}")
            self.out("option name Model type string default <empty>")
            self.out("uciok")
        elif cmd == "isready":
            if self.searching.is_set():
                self.out("readyok")  # (the protocol: answered at once during a search)
            else:
                self.jobs.put(("ready", None))
        elif cmd == "setoption":
            self._setoption(rest)
        elif cmd == "ucinewgame":
            self.jobs.put(("newgame", None))
        elif cmd == "position":
            p = self._parse_position(rest)
            if p is not None:
                self.jobs.put(("position", p))
        elif cmd == "go":
            self.stop_event = threading.Event()  # (one per search: a `stop` belongs to the latest `go`, whatever follows it)
            self.jobs.put(("go", (parse_go(rest), self.stop_event)))
        elif cmd == "stop":
            self.stop_event.set()
        elif cmd == "quit":
            self.close()
            return False
        return True  # (unknown input is ignored, as the protocol asks)

    def wait(self):
        """Returns when every command given so far has been carried out."""
        self.jobs.join()

    def close(self):
        if self.alive:
            self.alive = False
            self.stop_event.set()
            self.jobs.put(("quit", None))
            self.thread.join()

    def _setoption(self, tok: Sequence[str]):
        if "name" not in tok:
            return
        i = tok.index("name")
        j = tok.index("value") if "value" in tok else len(tok)
        name, value = " ".join(tok[i + 1:j]), " ".join(tok[j + 1:])
        key = next((k for k in list(OPTIONS) + ["Model"] if k.lower() == name.lower()), None)
        if key is None:
            self.out(f"info string unknown option {name}")
            return
        if key == "Model":
            val = value
        else:
            try:
                val = int(value)
            except ValueError:
                self.out(f"info string option {key} needs a number")
                return
            _, lo, hi = OPTIONS[key]
            val = min(hi, max(lo, val))
        self.jobs.put(("option", (key, val)))

    def _parse_position(self, tok: Sequence[str]):
        if not tok:
            return None
        moves = list(tok[tok.index("moves") + 1:]) if "moves" in tok else []
        head = tok[:tok.index("moves")] if "moves" in tok else tok
        if head[0] == "startpos":
            return STARTPOS, moves
        if head[0] == "fen" and len(head) >= 5:
            f = list(head[1:7])
            f += ["0", "1"][len(f) - 4:] if len(f) < 6 else []
            return " ".join(f), moves
        self.out("info string position: neither startpos nor a FEN")
        return None

    # ---- the search thread ---------------------------------------------------------------------------------------------------------
    def _work(self):
        while True:
            kind, arg = self.jobs.get()
            try:
                if kind == "quit":
                    self._teardown()
                    return
                if kind in ("ready", "go"):
                    self._ensure_engine()
                with torch.cuda.stream(self._stream) if self._stream is not None else _null():
                    self._do(kind, arg)
            except Exception as ex:  # a command must not kill the thread: say what happened and go on
                self.out(f"info string error: {type(ex).__name__}: {ex}")
                if kind == "go":
                    self.out("bestmove 0000")
                elif kind == "ready":
                    self.out("readyok")
            finally:
                self.searching.clear()
                self.jobs.task_done()

    _stream = None

    def _do(self, kind, arg):
        if kind == "option":
            key, val = arg
            if self.opt.get(key) != val:
                self.opt[key] = val
                self.stale = self.stale or key in _REBUILD
        elif kind == "ready":
            self.out("readyok")
        elif kind == "newgame":
            self.have = None  # the next position is set up from scratch: the tree is dropped
        elif kind == "position":
            self.want = arg
        elif kind == "go":
            self._go(*arg)

    def _teardown(self):
        if self.eng is not None:
            if self.dev.type == "cuda":
                torch.cuda.synchronize(self.dev)
            self.graph = None
            self.eng.close()
            self.eng = None

    def _ensure_engine(self):
        if self.eng is not None and not self.stale:
            return
        model = self.opt.get("Model")
        if model is None or model == "":
            raise E.EngineError("no net: start with --model PATH or `setoption name Model value PATH`")
        self._teardown()
        from . import nn_tune

        self.dev = dev = E.runtime_device(self.device_name)
        cuda = dev.type == "cuda"
        if isinstance(model, str):
            from .match import build_net, load_state_dict

            model = build_net(load_state_dict(model), dev)
        L, S = int(self.opt["Leaves"]), int(self.opt["MaxNodes"])
        if cuda and self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        with torch.cuda.stream(self._stream) if cuda else _null():
            self.L = L
            self.net = nn_tune.best_inference_copy(model, L, dev, next(model.parameters()).dtype)
            self.eng = E.Engine(1, fast=True, leaves_per_step=L, num_simulations=S, dirichlet_alpha=0.0, max_plies=2048,
                                device=dev.index if cuda and dev.index is not None else 0)
            self.nn_in = torch.zeros((L, E.INPUT_CHANNELS, 8, 8), dtype=torch.float32, device=dev)
            self.looks = [_Look(dev) for _ in range(3)]
            self.graph = None
            if cuda:
                self._capture()
        self.have, self.stale = None, False

    def _evaluate(self):
        with torch.no_grad():
            logits, value = self.net(self.nn_in)
        return logits.float().contiguous(), value.float().reshape(-1).contiguous()

    def _capture(self):
        """`evaluate -> bo_step` on L rows as one graph, captured once per engine (thread-local: stdin's thread is not held to capture-safe calls)."""
        dev, s = self.dev, self._stream
        for _ in range(2):
            self._evaluate()
        torch.cuda.synchronize(dev)
        inner = getattr(self.net, "net", self.net)
        words = getattr(inner, "overflow_words", None)
        self.eng.watch(*(words() if words is not None else (0, 1)))
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=s, capture_error_mode="thread_local"):
            self.keep = self._evaluate()
            self.eng.step(self.keep[0].data_ptr(), self.keep[1].data_ptr(), E.POLICY_LOGITS, self.nn_in.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)

    def _sid(self) -> int:
        return self._stream.cuda_stream if self.dev.type == "cuda" else 0

    def _step(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.keep = self._evaluate()
            self.eng.step(self.keep[0].data_ptr(), self.keep[1].data_ptr(), E.POLICY_LOGITS, self.nn_in.data_ptr(), 0)

    # ---- positions -----------------------------------------------------------------------------------------------------------------
    def _legal_now(self) -> List[int]:
        """The device's legal moves of the slot's current position."""
        pos, _ = self.eng.export_game(0, self._sid())
        return self.eng.movegen([pos[len(pos) - 1]], self._sid())[0][0]

    def _play_checked(self, texts: Sequence[str]) -> List[str]:
        """Play the moves one by one with bo_play, each checked against the device's legal moves first (bo_play substitutes another move
        for an illegal action).  -> the moves played: the legal prefix."""
        done = []
        for t in texts:
            m = parse_move(t)
            if m is None or m not in self._legal_now():
                self.out(f"info string illegal move {t}: the position stays at the last legal prefix ({len(done)} of {len(texts)} moves)")
                break
            self.eng.play(np.array([move_to_index(m)], dtype=np.int32), self._sid())
            done.append(t)
        return done

    def _sync_position(self):
        """Bring the slot to the last `position`: further moves of the same game are played (the tree is re-rooted and kept), anything
        else is a fresh bo_games_reset.  bo_games_reset makes the moves of its list without a legality check, so on that path the
        moves are first played one by one from the bare FEN, checked, and the slot is then reset with the legal prefix."""
        fen, moves = self.want
        if self.have is not None and self.have[0] == fen and moves[:len(self.have[1])] == self.have[1]:
            more = moves[len(self.have[1]):]
            self.have = (fen, self.have[1] + self._play_checked(more))
            return
        self.eng.reset([0], [fen], [None], self._sid())
        good = self._play_checked(moves) if moves else []
        if good:
            self.eng.reset([0], [fen], [" ".join(good)], self._sid())
        self.have = (fen, good)

    # ---- one search ----------------------------------------------------------------------------------------------------------------
    def _go(self, go: Dict, stop: threading.Event):
        t0 = time.perf_counter()
        eng, sid = self.eng, self._sid()
        self._sync_position()
        for w in ("depth", "mate", "searchmoves", "ponder"):
            if w in go:
                self.out(f"info string go {w} is not supported and is ignored")
        nl, term, _ = eng.root_info(sid)
        white = self._white_to_move()
        limit = time_limit_ms(go, white, float(self.opt["MoveOverhead"]))
        nodes_limit, infinite, multipv = go.get("nodes"), bool(go.get("infinite")), int(self.opt["MultiPV"])
        if term[0] != 0 or nl[0] == 0:
            why = {1: "checkmate", 2: "draw (stalemate, or claimable by repetition or the 50-move rule)"}.get(int(term[0]), "no legal move")
            self.out(f"info string the root is terminal: {why}")
            if infinite:
                self._park(stop)
            self.out("bestmove 0000")
            self.last_search = dict(nodes=0, reused=0, steps=0, stopped_by="terminal")
            return
        self.searching.set()
        look = self.looks[0]
        look.enqueue(eng, 1, self._stream, 0.0)
        reused = int(look.take(wait=True)["root_visits"])
        if reused > 0:
            self.out(f"info string tree reused: the root starts with {reused} visits")
        eng.search_begin([1], None, self.nn_in.data_ptr(), sid)
        eng.step(0, 0, E.POLICY_NONE, self.nn_in.data_ptr(), sid)
        steps, ahead, pending, rec, last_print, why = 1, [], [], None, t0, None
        lock_step = nodes_limit is not None  # `go nodes`: the host follows the device step by step, so that the end is the same every time
        cuda = self.dev.type == "cuda"
        while why is None:
            self._step()
            steps += 1
            now = time.perf_counter()
            if cuda:
                ev = torch.cuda.Event()
                ev.record(self._stream)
                ahead.append(ev)
                if len(ahead) > RUN_AHEAD:
                    ahead.pop(0).synchronize()
            free = next((k for k in self.looks if not k.busy), None)
            if free is not None and (lock_step or steps % LOOK_EVERY == 0 or now - last_print >= INFO_INTERVAL):
                free.enqueue(eng, multipv, self._stream, now - t0)
                pending.append(free)
            while pending and (lock_step or pending[0].ready()):
                t_rec = pending[0].t
                rec = pending.pop(0).take(wait=lock_step)
                hard = int(rec["status"]) & ~eng.soft_status_bits()
                if hard or int(rec["watch"]):
                    why = "fault"
                    self.out("info string the search ends on a fault: " + (eng.describe_status(hard) if hard else "the evaluate stage's fault word is set"))
                elif int(rec["phase"]) == E.PH_DONE:
                    why = "maxnodes"
                elif nodes_limit is not None and int(rec["sims_done"]) >= nodes_limit:
                    why = "nodes"
                if why is None and time.perf_counter() - last_print >= INFO_INTERVAL and int(rec["n_lines"]) > 0:
                    for s in format_info(rec, t_rec, multipv):
                        self.out(s)
                    last_print = time.perf_counter()
            if why is None and steps >= 3:  # the root's own evaluation and one step of descents are behind us: time and `stop` count now
                if stop.is_set():
                    why = "stop"
                elif limit is not None and (time.perf_counter() - t0) * 1000.0 >= limit:
                    why = "time"
        sims = int(eng.search_stop(None, sid)[0])  # (a search that finished on its own is left as it is)
        for k in self.looks:
            k.busy = False
        look.enqueue(eng, multipv, self._stream, 0.0)
        rec = look.take(wait=True)
        res = eng.result(sid)
        elapsed = time.perf_counter() - t0
        for s in format_info(rec, elapsed, multipv):
            self.out(s)
        hard = int(rec["status"]) & ~eng.soft_status_bits()
        if hard or eng.watch_seen():
            self.out("info string fault during this search: " + (eng.describe_status(hard) if hard else "the evaluate stage's fault word is set"))
        elif int(rec["status"]):
            self.out("info string the arena is full (hashfull 1000): new leaves stay unexpanded, their values are still backed up")
        best = int(rec["line"][0]["move"]) if int(rec["n_lines"]) > 0 else int(res["best_move"][0])
        if infinite and why != "stop":
            self._park(stop)  # the protocol: an infinite search answers only after `stop`
        self.last_search = dict(nodes=sims, reused=reused, steps=steps, stopped_by=why, best=E.move_to_uci(best), root_visits=int(rec["root_visits"]))
        self.out(f"bestmove {E.move_to_uci(best)}")

    def _park(self, stop: threading.Event):
        self.parked.set()
        stop.wait()
        self.parked.clear()

    def _white_to_move(self) -> bool:
        fen, moves = self.have
        return (fen.split()[1] == "w") == (len(moves) % 2 == 0)


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.uci", description="UCI engine on the fast search mode (MI355X).")
    ap.add_argument("--model", default=None, metavar="CHECKPOINT.pth", help="weights (state_dict); also `setoption name Model value PATH`")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    eng = UciEngine(model=a.model, device=a.device)
    try:
        for line in sys.stdin:
            if not eng.handle(line.strip()):
                break
    finally:
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
