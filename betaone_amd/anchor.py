"""betaone_amd/anchor.py -- the anchor opponent: a fixed, deterministic classical player on the GPU, and net-versus-anchor matches.

Every other strength number of the project is relative to another net.  The anchor does not move: a fixed-depth FULL-WIDTH negamax
with a small integer static evaluation (DESIGN.md "Anchor opponent"; bo_anchor, csrc/bo_anchor.h), searched for whole batches of
roots over perft's frontier.  Draw rules are ignored inside the tree, as in perft and mate: only a position without legal moves ends
a line.  A mate in 1 scores MATE - 1, so a depth-D search finds every mate of at most D plies and prefers the shortest.

    search("r1bqkbnr/pppp1ppp/2n5/4p2Q/2B1P3/8/PPPP1PPP/RNB1K1NR w KQkq - 4 4", 1)[0].best      # 'h5f7'
    python -m betaone_amd.anchor best "FEN" --depth 3 [--quiesce 4] [--scores] [--json]
    python -m betaone_amd.anchor best --epd FILE --depth 3
    python -m betaone_amd.anchor match NET.pth --depth 3 [--quiesce 4] [--margin 15] [--games 200 --slots 64 --sims 800 --openings book.txt
        --open-plies 8 --t-final 0.1 --max-game-moves 512 --pgn out.pgn --out result.json --seed-iteration 0]

roots: a FEN, a sequence of FENs, or a ctypes array of engine.BoPosition, as mate.mate takes them.

Quiescence (quiesce=Q, 1 .. 8; bo_anchor_q): at the horizon a position with a legal move gets qs(P, D, Q) in place of ev(P) -- up to Q
further plies over the TACTICAL moves only (captures and promotions; every evasion when in check), standing pat on ev(P) when not in
check.  The anchor then no longer evaluates in the middle of an exchange.  A mate score out of the quiescence plies is a forced mate (the
mated side was in check at each of its nodes, so all its replies were searched): a found mate is a score >= MATE - (depth + quiesce).
With quiesce 0 every call, byte and printed line is the fixed-depth anchor's.

Move choice in games (pick): with `margin` centipawns and a seeded numpy RandomState, uniformly among the moves whose score is within
the margin of the best; once the score is a found mate (score >= MATE - (depth + quiesce)) only the moves that equal it qualify, so
the anchor never gives up a mate.  No generator: the deterministic lowest-index best move.  Depth 0 is a uniformly random legal move.

A match (AnchorRollout under match.play_match) plays the net -- one evaluate stage, the reference search, no Dirichlet noise -- against
the anchor on the host-made turn: each ply the slots where the net is to move are searched and sampled as Rollout.play_ply does, the
slots where the anchor is to move become one bo_anchor batch of their current roots, and all moves go out in one play call.  The net
is side B of match.summarize: score and Elo are the net's against the anchor.  Anchor plies carry an empty pi; such games are match
games, never training records.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import engine as E
from .perft import DEFAULT_CAPACITY, MAX_MOVES, START_FEN

MATE = 30000     # BO_ANCHOR_MATE (include/betaone_engine.h)
MAX_DEPTH = 8    # BO_ANCHOR_MAX_DEPTH
MAX_QUIESCE = 8  # BO_ANCHOR_MAX_QUIESCE
NONE = -(1 << 31)
STATUS_NAMES = ("ok", "checkmated", "stalemated", "not a position")


class BoAnchorResult(C.Structure):  # bo_anchor_result
    _fields_ = [("status", C.c_int32), ("score", C.c_int32), ("best", C.c_int32), ("n_best", C.c_int32), ("n_moves", C.c_int32),
                ("reserved", C.c_int32), ("nodes", C.c_uint64)]


@dataclass
class AnchorResult:
    fen: Optional[str]                 # None for a BoPosition root
    status: str                        # STATUS_NAMES
    depth: int
    score: int                         # centipawns from the side to move's view; MATE - p: it mates in p plies
    best: Optional[str]                # the lowest-index move that reaches the score (UCI)
    best_word: int                     # ... as from | to << 6 | promo << 12, -1 none
    n_best: int
    n_moves: int
    move_words: Optional[List[int]] = None   # scores=True: the root's moves in generated order ...
    scores: Optional[List[int]] = None       # ... and the score of each
    nodes: int = 0                     # frontier entries of levels 0 .. depth + quiesce - 1, of the whole call
    splits: int = 0                    # of the whole call
    seconds: float = 0.0               # of the whole call
    quiesce: int = 0                   # quiescence plies behind the horizon

    @property
    def moves(self) -> Optional[List[str]]:
        return None if self.move_words is None else [E.move_to_uci(w) for w in self.move_words]

    def to_json(self) -> dict:
        d = {"fen": self.fen, "status": self.status, "depth": self.depth, "score": self.score, "best": self.best, "n_best": self.n_best,
             "n_moves": self.n_moves, "nodes": self.nodes, "splits": self.splits, "seconds": self.seconds}
        if self.quiesce:
            d["quiesce"] = self.quiesce
        if self.scores is not None:
            d["moves"], d["scores"] = self.moves, list(self.scores)
        return d


def _stream(dev) -> int:
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
        return torch.cuda.current_stream(dev).cuda_stream
    return 0


def search(roots: Union[str, Sequence[Optional[str]], C.Array], depth: int, *, quiesce: int = 0, scores: bool = False,
           capacity: int = DEFAULT_CAPACITY, device="cuda:0", lib=None) -> List[AnchorResult]:
    """The depth-`depth` anchor search of every root, with `quiesce` quiescence plies behind the horizon, in one device call on torch's
    current stream of `device`."""
    quiesce = int(quiesce)
    if quiesce and int(depth) < 1:
        raise ValueError("anchor.search: quiescence needs a depth of at least 1 (depth 0 is a random mover)")
    lib = lib or E.load_hip_library()
    dev = E.runtime_device(device)
    fens, arr, pos = None, None, None
    if isinstance(roots, C.Array) and getattr(roots, "_type_", None) is E.BoPosition:
        pos, n = roots, len(roots)
    else:
        if roots is None or isinstance(roots, str):
            roots = [roots]
        fens = [START_FEN if f is None else f for f in roots]
        n = len(fens)
        arr = (C.c_char_p * max(n, 1))(*[f.encode() for f in fens])
    res = (BoAnchorResult * max(n, 1))()
    words = np.full((max(n, 1), MAX_MOVES), -1, np.int32) if scores else None
    vals = np.full((max(n, 1), MAX_MOVES), NONE, np.int32) if scores else None
    splits = C.c_int64(0)
    stream = _stream(dev)
    t0 = time.perf_counter()
    tail = (int(capacity), 0, C.addressof(res), words.ctypes.data if scores else None, vals.ctypes.data if scores else None, C.byref(splits), stream)
    head = (int(dev.index or 0), n, arr, C.addressof(pos) if pos is not None else None, int(depth))
    rc = lib.bo_anchor_q(*head, quiesce, *tail) if quiesce else lib.bo_anchor(*head, *tail)
    dt = time.perf_counter() - t0
    if rc != 0:
        msg = f"bo_anchor: {lib.bo_last_error().decode()}"
        raise (ValueError if rc in (-1, -4) else E.EngineError)(msg)
    out = []
    for i in range(n):
        r = res[i]
        k = int(r.n_moves)
        out.append(AnchorResult(fens[i] if fens is not None else None, STATUS_NAMES[int(r.status)], int(depth), int(r.score),
                                E.move_to_uci(int(r.best)) if r.best >= 0 else None, int(r.best), int(r.n_best), k,
                                [int(w) for w in words[i, :k]] if scores else None, [int(v) for v in vals[i, :k]] if scores else None,
                                nodes=int(r.nodes), splits=int(splits.value), seconds=dt, quiesce=quiesce))
    return out


def evaluate(positions, *, device="cuda:0", lib=None) -> np.ndarray:
    """ev of every position (a ctypes array or a sequence of engine.BoPosition): int32 [n], centipawns from the side to move's view;
    the smallest int32 for a record that is not a position."""
    lib = lib or E.load_hip_library()
    dev = E.runtime_device(device)
    if not (isinstance(positions, C.Array) and getattr(positions, "_type_", None) is E.BoPosition):
        positions = (E.BoPosition * len(positions))(*positions)
    n = len(positions)
    if n == 0:
        return np.zeros(0, np.int32)
    out = np.full(n, NONE, np.int32)
    rc = lib.bo_anchor_eval(int(dev.index or 0), n, C.addressof(positions), out.ctypes.data, _stream(dev))
    if rc != 0:
        raise E.EngineError(f"bo_anchor_eval: {lib.bo_last_error().decode()}")
    return out[:n]


def candidates(result: AnchorResult, margin: int = 0) -> List[int]:
    """Indices (into the root's move list) of the moves pick chooses among: within `margin` of the score; a found mate
    (score >= MATE - (depth + quiesce): a mate out of the quiescence plies is forced too) only by the moves that equal it."""
    if result.scores is None:
        raise ValueError("anchor.candidates: the result has no per-move scores (search(..., scores=True))")
    m = 0 if result.score >= MATE - (result.depth + result.quiesce) else max(int(margin), 0)
    return [i for i, v in enumerate(result.scores) if v >= result.score - m]


def pick(result: AnchorResult, margin: int = 0, rng=None) -> int:
    """The anchor's move (from | to << 6 | promo << 12) at a searched root.  rng None: the lowest-index best move (margin must be 0).
    With a numpy RandomState: uniformly among candidates(result, margin).  A depth-0 result (random_result): uniformly among the moves."""
    if result.status != "ok" or result.n_moves < 1:
        raise ValueError(f"anchor.pick: the root has no move ({result.status})")
    if result.depth == 0:
        if rng is None:
            raise ValueError("anchor.pick: depth 0 is a random move and needs a generator")
        return result.move_words[int(rng.randint(result.n_moves))]
    if rng is None:
        if margin:
            raise ValueError("anchor.pick: a margin needs a generator")
        return result.best_word
    c = candidates(result, margin)
    return result.move_words[c[int(rng.randint(len(c)))]]


def random_result(move_words: Sequence[int], fen: Optional[str] = None) -> AnchorResult:
    """The depth-0 anchor's view of a root: its legal moves, nothing searched."""
    w = [int(m) for m in move_words]
    return AnchorResult(fen, "ok", 0, 0, None, -1, 0, len(w), w, [0] * len(w))


def anchor_name(depth: int, margin: int, quiesce: int = 0) -> str:
    if int(quiesce):
        return f"anchor(depth={int(depth)},quiesce={int(quiesce)},margin={int(margin)})"
    return f"anchor(depth={int(depth)},margin={int(margin)})"


# ---- the game loop ------------------------------------------------------------------------------------------------------------------
class AnchorRollout:
    """The stand-in match.play_match drives for net-versus-anchor games: a one-net Rollout on the host-made turn whose slots with the
    anchor to move are moved by bo_anchor (Rollout.external_moves).  net_of_white[g] == 1: the net plays white -- the net is side B.
    The seeds handed to start_games / refill are integers (selfplay_main.game_seed); the net's sampling stream is RandomState(seed),
    the anchor's RandomState(seed ^ 0x5bd1e995)."""

    def __init__(self, model, n_games: int, depth: int, margin: int = 0, *, quiesce: int = 0, capacity: int = DEFAULT_CAPACITY, **rollout_kw):
        from .rollout import Rollout

        if not 0 <= int(depth) <= MAX_DEPTH:
            raise ValueError(f"AnchorRollout: depth must be 0 .. {MAX_DEPTH}")
        if int(margin) < 0:
            raise ValueError("AnchorRollout: margin must be >= 0")
        if not 0 <= int(quiesce) <= MAX_QUIESCE or (int(quiesce) and int(depth) == 0):
            raise ValueError(f"AnchorRollout: quiesce must be 0 .. {MAX_QUIESCE}, and 0 at depth 0 (a random mover)")
        for k in ("resign_threshold", "record_values", "fast", "rng_mode", "dirichlet_alpha"):
            if rollout_kw.get(k):
                raise ValueError(f"AnchorRollout: {k} is not supported (the net plays the reference search on the host-made turn, without noise)")
            rollout_kw.pop(k, None)
        self.depth, self.margin, self.quiesce, self.capacity = int(depth), int(margin), int(quiesce), int(capacity)
        self.ro = Rollout(model, n_games, rng_mode="python", dirichlet_alpha=0.0, **rollout_kw)
        self.ro.external_moves = self._anchor_moves
        self.G, self.eng, self.device = self.ro.G, self.ro.eng, self.ro.device
        self._net_white = np.zeros(self.G, np.int32)
        self._rng: List = [None] * self.G
        self._step = 0               # (match.play_match's default step_of reads it: the host-made turn has no cohort plies)
        self.anchor_seconds = 0.0    # in bo_anchor calls
        self.anchor_nodes = 0
        self.anchor_plies = 0

    n_plies = property(lambda self: self.ro.n_plies)
    n_sims = property(lambda self: self.ro.n_sims)

    def _admit(self, slot: int, seed: int, net_of_white) -> "np.random.RandomState":
        if net_of_white not in (0, 1):
            raise ValueError("AnchorRollout: every game needs net_of_white (0: the anchor plays white, 1: the net does)")
        self._net_white[slot] = int(net_of_white)
        self._rng[slot] = np.random.RandomState((int(seed) ^ 0x5BD1E995) & 0xFFFFFFFF)
        return np.random.RandomState(int(seed) & 0xFFFFFFFF)

    def start_games(self, slots, game_ids, seeds, fens=None, moves=None, net_of_white=None):
        if net_of_white is None or len(net_of_white) != len(slots):
            raise ValueError("AnchorRollout.start_games: net_of_white (0 / 1) is needed for every game")
        rngs = [self._admit(s, seeds[i], net_of_white[i]) for i, s in enumerate(slots)]
        self.ro.start_games(slots, game_ids, rngs, fens, moves)

    def play_ply(self, on_finished=None, refill=None, while_searching=None) -> int:
        def wrapped(slot):
            nxt = refill(slot)
            if nxt is None:
                return None
            rng = self._admit(slot, nxt[1], nxt[4] if len(nxt) > 4 else None)
            return (nxt[0], rng, nxt[2], nxt[3] if len(nxt) > 3 else None)

        return self.ro.play_ply(on_finished, wrapped if refill is not None else None, while_searching)

    def _anchor_moves(self, live: np.ndarray):
        """Rollout.external_moves: the live slots where the anchor is to move, and its moves as action indices."""
        from .reanalyse import moves_to_actions

        ro = self.ro
        mask = np.zeros(self.G, bool)
        actions = np.full(self.G, -1, np.int32)
        for g in np.nonzero(live)[0]:
            gs = ro.games[g]
            white = gs.start_white ^ bool(gs.plies & 1)
            mask[g] = white != bool(self._net_white[g])
        slots = np.nonzero(mask)[0]
        if not len(slots):
            return mask, actions
        roots = (E.BoPosition * len(slots))()
        for i, g in enumerate(slots):  # the slot's current root: the last position of its game so far
            positions, _ = self.eng.export_game(int(g), ro._stream(), n_plies=ro.games[g].plies)
            roots[i] = positions[len(positions) - 1]
        if self.depth == 0:
            lists, _ = self.eng.movegen(list(roots), ro._stream())
            res = [random_result(m) for m in lists]
        else:
            res = search(roots, self.depth, quiesce=self.quiesce, scores=self.margin > 0, capacity=self.capacity, device=self.device)
            self.anchor_seconds += res[0].seconds
            self.anchor_nodes += res[0].nodes
        use_rng = self.depth == 0 or self.margin > 0
        words = [pick(r, self.margin, self._rng[g] if use_rng else None) for r, g in zip(res, slots)]
        actions[slots] = moves_to_actions(np.array(words, np.int64))
        self.anchor_plies += len(slots)
        return mask, actions

    def close(self):
        self.ro.close()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def _line(r: AnchorResult) -> str:
    if r.status != "ok":
        return "not a position" if r.status == "not a position" else f"the side to move is {r.status}"
    h = r.depth + r.quiesce  # the deepest ply a mate can be found at
    s = f"mate in {(MATE - r.score + 1) // 2}" if r.score >= MATE - h else f"mated in {(MATE + r.score) // 2}" if r.score <= -(MATE - h) \
        else f"{r.score:+d} cp"
    return f"best {r.best} ({s}, score {r.score}), {r.n_best} of {r.n_moves} moves reach it"


def main_best(argv, out) -> int:
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.anchor best", description="the anchor's move at a position")
    ap.add_argument("fen", nargs="?", default=None, help="FEN (default: the start position)")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--quiesce", type=int, default=0, metavar="Q", help=f"quiescence plies behind the horizon, 0 .. {MAX_QUIESCE}")
    ap.add_argument("--scores", action="store_true", help="the score of every root move")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--epd", default=None, metavar="FILE", help="one position per line (a FEN of four or six fields; operations are ignored)")
    ap.add_argument("--capacity", type=int, default=DEFAULT_CAPACITY)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    E.load_hip_library()  # (outside the timed call)
    if a.epd:
        if a.fen:
            ap.error("--epd takes its positions from the file")
        from .mate import parse_epd

        suite = parse_epd(open(a.epd).read())
        res = search([s[1] for s in suite], a.depth, quiesce=a.quiesce, capacity=a.capacity, device=a.device) if suite else []
        for (ln, fen, _, _), r in zip(suite, res):
            print(f"{a.epd}:{ln}: {fen}: {_line(r)}", file=out)
        nodes, secs = (res[0].nodes, res[0].seconds) if res else (0, 0.0)
        at = f"depth {a.depth}" + (f", quiesce {a.quiesce}" if a.quiesce else "")
        print(f"{len(suite)} positions at {at}; {nodes} nodes in {secs:.3f} s", file=out)
        return 0
    fen = None if a.fen in (None, "startpos") else a.fen
    r = search(fen, a.depth, quiesce=a.quiesce, scores=a.scores, capacity=a.capacity, device=a.device)[0]
    if a.json:
        print(json.dumps(r.to_json()), file=out)
        return 0
    print(_line(r)[0].upper() + _line(r)[1:] + ".", file=out)
    if a.scores and r.scores is not None:
        print(" ".join(f"{m} {v}" for m, v in zip(r.moves, r.scores)), file=out)
    rate = r.nodes / r.seconds if r.seconds > 0 else 0.0
    at = f"depth {r.depth}" + (f", quiesce {r.quiesce}" if r.quiesce else "")
    print(f"{at}: {r.nodes} nodes, {r.seconds:.3f} s, {rate / 1e6:.2f} M nodes/s" + (f", {r.splits} level splits" if r.splits else ""), file=out)
    return 0


def main_match(argv, out) -> int:
    from . import match as M
    from . import nn_tune

    ap = argparse.ArgumentParser(prog="python -m betaone_amd.anchor match", description="Play a checkpoint against the anchor on the GPU.")
    ap.add_argument("net", help="the checkpoint")
    ap.add_argument("--depth", type=int, default=3, help=f"the anchor's search depth in plies, 0 (a random mover) .. {MAX_DEPTH}")
    ap.add_argument("--quiesce", type=int, default=0, metavar="Q", help=f"the anchor's quiescence plies behind the horizon, 0 .. {MAX_QUIESCE}")
    ap.add_argument("--margin", type=int, default=0, help="the anchor picks uniformly among the moves within this many centipawns of its best")
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--mcts-batch", type=int, default=96)
    ap.add_argument("--openings", default=None, help="file: one FEN (or 'startpos') per line, optionally '; <uci moves>'")
    ap.add_argument("--open-plies", type=int, default=8, help="the net's moves with a fullmove number below this are sampled at temperature 1")
    ap.add_argument("--t-final", type=float, default=0.1)
    ap.add_argument("--max-game-moves", type=int, default=512)
    ap.add_argument("--seed-iteration", type=int, default=0, help="the iteration argument of selfplay_main.game_seed")
    ap.add_argument("--capacity", type=int, default=DEFAULT_CAPACITY)
    ap.add_argument("--pgn", default=None, metavar="FILE")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    sd = M.load_state_dict(a.net)
    dev = E.runtime_device(a.device)
    net = nn_tune.best_inference_copy(M.build_net(sd, dev), a.slots, dev)
    openings = M.parse_openings(open(a.openings).read()) if a.openings else [(None, "")]
    name = anchor_name(a.depth, a.margin, a.quiesce)
    print(f"[anchor] net {M.net_shape(sd)} vs {name}", file=out)
    ro = AnchorRollout(net, a.slots, a.depth, a.margin, quiesce=a.quiesce, capacity=a.capacity, num_simulations=a.sims, mcts_batch_size=a.mcts_batch,
                       temperature=(a.open_plies, 1.0, a.t_final), max_game_moves=a.max_game_moves, device=str(dev))
    sched = M.MatchScheduler(openings, a.games, a.slots, 1)
    finished: Optional[Dict] = {} if a.pgn else None
    try:
        played = M.play_match(ro, sched, step_of=lambda s: 0, seed_iteration=a.seed_iteration, log=lambda m: print(m, file=out), finished=finished)
    finally:
        ro.close()
    if a.pgn:
        with open(a.pgn, "w", encoding="utf-8", newline="\n") as fh:
            M.write_match_pgn(fh, played, finished, name, a.net, device=str(dev))
    st = M.summarize(played, with_pairs=a.openings is not None)
    st.update(anchor_plies=ro.anchor_plies, anchor_nodes=ro.anchor_nodes, anchor_seconds=ro.anchor_seconds)
    print(f"[anchor] net vs {name}: +{st['wins']} ={st['draws']} -{st['losses']}  score {st['score']:.3f}  Elo {st['elo']:+.1f} "
          f"[{st['elo_95'][0]:+.1f}, {st['elo_95'][1]:+.1f}] ({st['interval']})  LOS {st['los']:.3f}  {st['plies_per_second']:.0f} plies/s", file=out)
    if a.out:
        settings = {k: getattr(a, k) for k in ("depth", "margin", "games", "slots", "sims", "mcts_batch", "openings", "open_plies", "t_final",
                                               "max_game_moves", "seed_iteration")}
        if a.quiesce:
            settings["quiesce"] = a.quiesce
        with open(a.out, "w") as f:
            json.dump(M.json_safe({"a": name, "b": a.net, "settings": settings, "summary": st, "games": played["games"]}), f, indent=1,
                      allow_nan=False)
    return 0


def main(argv=None, out=None) -> int:
    out = out or sys.stdout
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "match":
        return main_match(argv[1:], out)
    if argv and argv[0] == "best":
        return main_best(argv[1:], out)
    print("usage: python -m betaone_amd.anchor best \"FEN\" --depth D [--quiesce Q] [--scores] [--json] | best --epd FILE | match NET.pth --depth D ...", file=out)
    return 2


if __name__ == "__main__":
    sys.exit(main())
