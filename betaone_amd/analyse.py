"""betaone_amd/analyse.py -- "here is a file of games, what does my net think of them?"

    python -m betaone_amd.analyse games.pgn [more.pgn | dir/] --model best.pth -o annotated.pgn
           [--sims S] [--slots G] [--jsonl positions.jsonl] [--report report.json] [--device cuda:0]

Every game the PGN reader accepts is replayed on the device (bo_pgn_replay, betaone_amd/pgn.py); for every position P_k before a
replayed move m_k one search of the reference's semantics runs from P_k with the game's own past as context (history planes, repetition
tracker), Dirichlet noise off -- the output is a function of the file and the net.  The roots never leave the device: a batch of
`slots` roots is set up from the replayed positions (bo_games_reset_dev), begun on the device (bo_search_begin_dev), searched by
Rollout's evaluate stage and its captured graph of evaluate -> step iterations, and read out as one bo_analysis record per root
(bo_analysis_result): root value, best move, principal variation, how the played move fared.  The host enqueues batch b + 1 behind batch
b without waiting and reads batch b's records from one of two pinned buffers meanwhile.

The annotated PGN carries "{<e>/<S> 0.00s}" after move k, e from the root value v_k of P_k (pgn_write.eval_text; v_k is the value for
the side to move at P_k, which is what pretrain's sample rule expects of move k's comment): any PGN becomes pretraining input.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import json
import os
import re
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import engine as E
from . import pgn as P
from . import pgn_write as W

DPOS_DTYPE = np.dtype([("bb", "<u8", (8,)), ("flags", "<u4"), ("halfmove", "<i4"), ("fullmove", "<i4"), ("khash", "<u4")])  # csrc/bo_chess.h
BOPOS_DTYPE = np.dtype([("bb", "<u8", (8,)), ("turn", "<i4"), ("castling", "<u4"), ("ep_square", "<i4"), ("ep_key", "<i4"),
                        ("halfmove_clock", "<i4"), ("fullmove_number", "<i4")])                                            # bo_position
assert DPOS_DTYPE.itemsize == P.POSITION_BYTES and BOPOS_DTYPE.itemsize == C.sizeof(E.BoPosition)
RESULTS = ("1-0", "0-1", "1/2-1/2", "*")
WRITER_TAGS = ("SetUp", "FEN", "PlyCount")  # written from the replayed game, not copied from the input
_TAG = re.compile(rb'\s*\[\s*([A-Za-z0-9_]+)\s*"((?:[^"\\]|\\.)*)"\s*\]')


def ring_to_positions(raw: np.ndarray):
    """Ring entries (uint8 [n, 80]) -> a ctypes array of n bo_position (what bo_game_export returns for the same positions)."""
    d = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1).view(DPOS_DTYPE)
    out = np.zeros(len(d), BOPOS_DTYPE)
    fl = d["flags"].astype(np.int64)
    out["bb"] = d["bb"]
    out["turn"] = fl & 1
    out["castling"] = (fl >> 1) & 0xF
    out["ep_square"] = ((fl >> 8) & 0x7F) - 1
    out["ep_key"] = ((fl >> 16) & 0x7F) - 1
    out["halfmove_clock"] = d["halfmove"]
    out["fullmove_number"] = d["fullmove"]
    return (E.BoPosition * max(1, len(d))).from_buffer_copy(out.tobytes() if len(d) else bytes(BOPOS_DTYPE.itemsize))


_SKIP = re.compile(rb"(?:\s+|(?:^|(?<=[\n\r]))%[^\n\r]*|;[^\n\r]*)+")  # blanks, '%' escape lines, ';' comments (csrc/bo_pgn.h skips them too)


def game_tags(text: bytes) -> List[Tuple[str, str]]:
    """The tag pairs at the head of one game's text, in input order ('%' lines and ';' comments around them are skipped)."""
    out, i = [], 0
    while True:
        k = _SKIP.match(text, i)
        if k:
            i = k.end()
        m = _TAG.match(text, i)
        if not m:
            return out
        v = re.sub(rb'\\(["\\])', rb"\1", m.group(2))
        out.append((m.group(1).decode("utf-8", "replace"), v.decode("utf-8", "replace")))
        i = m.end()


def game_result(text: bytes, tags: Sequence[Tuple[str, str]]) -> str:
    """The game's result as in the input: its termination token, else its Result tag, else '*'."""
    words = text.split()
    if words and words[-1].decode("ascii", "replace") in RESULTS:
        return words[-1].decode()
    r = dict(tags).get("Result")
    return r if r in RESULTS else "*"


def _read(path: str) -> bytes:
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        return f.read()


def _sources(paths_or_text) -> List[Tuple[str, bytes]]:
    """PGN text is given as bytes, or as a str that names no existing file or directory and has a line break; every other str is a path."""
    if isinstance(paths_or_text, bytes):
        return [("<text>", paths_or_text)]
    if isinstance(paths_or_text, str):
        if not os.path.exists(paths_or_text) and "\n" in paths_or_text:
            return [("<text>", paths_or_text.encode())]
        paths_or_text = [paths_or_text]
    return [(p, _read(p)) for p in P.pgn_paths(list(paths_or_text))]


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


class Ingested:
    """One PGN text replayed into device memory: pos (uint8 [T * 80]) and act (int32 [T]), game g's plies in entries tok_off[g] ..;
    the work list -- every (game, ply) with a replayed move, in file order -- as device arrays padded to whole batches."""

    def __init__(self, lib, dev, name: str, data: bytes):
        self.name, self.data = name, data
        pg = P.parse_chunk(lib, data, 0, True)[0]
        x = pg.export()
        G, T = pg.n_games, max(pg.n_tokens, 1)
        self.n_games, self.T = G, T
        b, e = np.zeros(max(G, 1), np.int64), np.zeros(max(G, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        if lib.bo_pgn_spans(pg.h, b.ctypes.data_as(i64p), e.ctypes.data_as(i64p)) != 0:
            raise E.EngineError(f"bo_pgn_spans: {lib.bo_last_error().decode()}")
        self.spans = [(int(b[g]), int(e[g])) for g in range(G)]
        self.tok_off, self.roots = x["tok_off"].astype(np.int64), x["roots"]
        self.pos = torch.zeros(T * P.POSITION_BYTES, dtype=torch.uint8, device=dev)
        self.act = torch.full((T,), -1, dtype=torch.int32, device=dev)
        z, smp = torch.zeros(T, dtype=torch.float32, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)
        scratch = torch.empty(max(pg.scratch_bytes, 16), dtype=torch.uint8, device=dev)
        self.n_plies, self.status = np.zeros(max(G, 1), np.int32), np.zeros(max(G, 1), np.int32)
        slot0 = self.tok_off[:-1].copy() if G else np.zeros(1, np.int64)
        if G:
            rc = lib.bo_pgn_replay(pg.h, slot0.ctypes.data_as(i64p), T, scratch.data_ptr(), scratch.numel(), self.pos.data_ptr(),
                                   self.act.data_ptr(), z.data_ptr(), smp.data_ptr(), self.n_plies.ctypes.data_as(E._I32P),
                                   self.status.ctypes.data_as(E._I32P), _stream(dev))
            if rc != 0:
                raise E.EngineError(f"bo_pgn_replay: {lib.bo_last_error().decode()}")
        self.n_plies, self.status = self.n_plies[:G], self.status[:G]
        pg.close()
        self.w_game = np.repeat(np.arange(G, dtype=np.int64), self.n_plies)
        self.w_ply = (np.arange(len(self.w_game), dtype=np.int64) - np.repeat(np.cumsum(self.n_plies) - self.n_plies, self.n_plies)).astype(np.int32)
        self.n_roots = len(self.w_game)

    def finish(self, lib, dev):
        """The moves of the ring's action indices and each game's position after its last move (bo_pgn_after), to the host."""
        N, G = self.n_roots, self.n_games
        self.moves = np.zeros(0, np.int32)
        self.final = {}
        if N == 0:
            return
        idx = torch.from_numpy(self.tok_off[self.w_game] + self.w_ply).to(dev)
        self.moves_dev = torch.zeros(N, dtype=torch.int32, device=dev)
        if lib.bo_pgn_after(self.pos.data_ptr(), self.act.data_ptr(), self.T, N, idx.data_ptr(), None, self.moves_dev.data_ptr(), _stream(dev)) != 0:
            raise E.EngineError(f"bo_pgn_after: {lib.bo_last_error().decode()}")
        played = [g for g in range(G) if self.n_plies[g] > 0]
        last = torch.from_numpy(np.array([self.tok_off[g] + self.n_plies[g] - 1 for g in played], np.int64)).to(dev)
        fin = torch.zeros(len(played) * P.POSITION_BYTES, dtype=torch.uint8, device=dev)
        if lib.bo_pgn_after(self.pos.data_ptr(), self.act.data_ptr(), self.T, len(played), last.data_ptr(), fin.data_ptr(), None, _stream(dev)) != 0:
            raise E.EngineError(f"bo_pgn_after: {lib.bo_last_error().decode()}")
        self.moves = self.moves_dev.cpu().numpy()
        fin_h = fin.cpu().numpy().reshape(-1, P.POSITION_BYTES)
        self.final = {g: fin_h[i] for i, g in enumerate(played)}
        self.pos_host = self.pos.cpu().numpy().reshape(self.T, P.POSITION_BYTES)

    def work_arrays(self, dev, G: int, order: Optional[np.ndarray] = None):
        """(first int64, ply int32, played int32, want int32, n_batches) on the device for the roots `order` (default: all, in file
        order), padded to whole batches of G with roots the set-up kernel refuses (ply -1) and nobody wants."""
        order = np.arange(self.n_roots) if order is None else np.asarray(order, dtype=np.int64)
        n = len(order)
        nb = max(1, -(-n // G))
        first, ply = np.zeros(nb * G, np.int64), np.full(nb * G, -1, np.int32)
        played, want = np.full(nb * G, -1, np.int32), np.zeros(nb * G, np.int32)
        first[:n], ply[:n], played[:n], want[:n] = self.tok_off[self.w_game[order]], self.w_ply[order], self.moves[order], 1
        return tuple(torch.from_numpy(a).to(dev) for a in (first, ply, played, want)) + (nb,)


class Analyser:
    """The search side: a Rollout's engine and evaluate stage (noise off, root values on), driven batch by batch.

    What a batch's read-out is -- which result call fills which pinned buffers -- is three small methods (_make_buffers, _records,
    _collect) and the hook _took; reanalyse.Reanalyser replaces them and keeps everything else."""

    NAME = "analyse"
    RECORD_DTYPE = E.ANALYSIS_DTYPE

    def __init__(self, model, slots: int, sims: int, max_plies: int, device, mcts_batch_size: Optional[int] = None, use_graph: bool = True,
                 iterations: Optional[int] = None, **search_cfg):
        from .rollout import Rollout

        if getattr(model, "is_pair", False):
            raise ValueError("analyse: two-net analysis is not supported")
        self.G, self.S = int(slots), int(sims)
        if self.G < 1 or self.S < 0:
            raise ValueError("analyse: slots >= 1 and sims >= 0")
        cfg = _search_config()
        cfg.update(search_cfg)
        if mcts_batch_size is not None:
            cfg["mcts_batch_size"] = int(mcts_batch_size)
        self.ro = Rollout(model, self.G, num_simulations=self.S, dirichlet_alpha=0.0, max_plies=int(max_plies), device=device,
                          use_graph=use_graph, record_values=True, **cfg)
        self.dev = self.ro.device
        self.eng = self.ro.eng
        self.slots_dev = torch.arange(self.G, dtype=torch.int32, device=self.dev)
        cuda = self.dev.type == "cuda"
        self._make_buffers(cuda)
        self.events = [torch.cuda.Event() for _ in range(2)] if cuda else None
        # evaluate -> step iterations enqueued per batch: what a search is expected to need (Rollout: 1 + ceil(S / MCTS_BATCH_SIZE))
        self.iterations = int(iterations) if iterations else self.ro.expected_evals
        self.n_batches = self.n_retried = 0

    def close(self):
        self.ro.close()

    def _make_buffers(self, cuda: bool):
        self.out_dev = torch.zeros((self.G, 32), dtype=torch.int32, device=self.dev)
        self.pinned = [torch.zeros((self.G, 32), dtype=torch.int32, pin_memory=cuda) for _ in range(2)]

    def _soft_bits(self) -> int:
        return self.eng.soft_status_bits()

    def _took(self, ids: np.ndarray, rows: np.ndarray):
        """Roots `ids` got their records from rows `rows` of the batch _collect returned last."""

    def _enqueue(self, ing: Ingested, arrays, b: int, extra: int, buf: int):
        """Batch b of `arrays`: set-up -> begin -> the search's iterations -> result + records -> copy to pinned[buf].  No host wait."""
        first, ply, want = arrays[0], arrays[1], arrays[3]
        ro, eng, G, s = self.ro, self.eng, self.G, _stream(self.dev)
        eng.reset_dev(G, self.slots_dev.data_ptr(), ing.pos.data_ptr(), ing.T, first.data_ptr() + 8 * b * G, ply.data_ptr() + 4 * b * G, s)
        eng.search_begin_dev(want.data_ptr() + 4 * b * G, ro.nn_in.data_ptr(), s)
        eng.step(0, 0, E.POLICY_NONE, ro.nn_in.data_ptr(), s)
        ro._eval_and_step_n(self.iterations + extra)
        self._records(arrays, b, buf)
        self.n_batches += 1

    def _records(self, arrays, b: int, buf: int):
        """Batch b's result call and its copy to pinned[buf], enqueued."""
        self.eng.analysis_result(arrays[2].data_ptr() + 4 * b * self.G, self.out_dev.data_ptr(), _stream(self.dev))
        self.pinned[buf].copy_(self.out_dev, non_blocking=True)
        self._recorded(buf)

    def _recorded(self, buf: int):
        if self.events is not None:
            self.events[buf].record(torch.cuda.current_stream(self.dev))

    def _read(self, buf: int) -> np.ndarray:
        return self.pinned[buf].numpy().copy().view(self.RECORD_DTYPE).reshape(self.G)

    def _collect(self, buf: int) -> np.ndarray:
        if self.events is not None:
            self.events[buf].synchronize()
        rec = self._read(buf)
        if (rec["watch"] != 0).any():  # the evaluate stage's fault word, as Rollout checks it once per ply
            chk = getattr(getattr(self.ro.model, "net", self.ro.model), "check_overflow", None)
            if chk is not None and self.dev.type == "cuda":
                torch.cuda.synchronize(self.dev)
                chk()
            raise E.EngineError(self.ro._watch_msg)
        return rec

    def run(self, ing: Ingested) -> np.ndarray:
        """One record (RECORD_DTYPE: bo_analysis) per root of `ing`, in work-list order."""
        N, G = ing.n_roots, self.G
        out = np.zeros(N, self.RECORD_DTYPE)
        if N == 0:
            return out
        arrays = ing.work_arrays(self.dev, G)
        nb = arrays[-1]
        again: List[int] = []

        def take(b, rec, order=None):
            n = min(G, N - b * G) if order is None else min(G, len(order) - b * G)
            ids = np.arange(b * G, b * G + n) if order is None else order[b * G:b * G + n]
            r = rec[:n]
            bad = r["status"] & ~self._soft_bits()
            if bad.any():
                k = int(np.nonzero(bad)[0][0])
                raise E.EngineError(f"{self.NAME}: {ing.name} game {int(ing.w_game[ids[k]])} ply {int(ing.w_ply[ids[k]])}: "
                                    f"{self.eng.describe_status(int(bad[k]))}")
            running = r["phase"] == E.PH_RUN
            out[ids[~running]] = r[~running]
            self._took(ids[~running], np.nonzero(~running)[0])
            return [int(i) for i in ids[running]]

        for b in range(nb):  # batch b + 1 is enqueued before batch b's records are read
            self._enqueue(ing, arrays, b, 0, b & 1)
            if b > 0:
                again += take(b - 1, self._collect((b - 1) & 1))
        again += take(nb - 1, self._collect((nb - 1) & 1))
        # A search that needed more iterations than 1 + ceil(S / MCTS_BATCH_SIZE) (a game that absorbed a long run of terminal
        # simulations yields without a request) was still running when its slot was set up for the next batch: its root is searched
        # again from scratch -- noise is off, a search is a function of its root -- and given iterations until it has finished.
        if again:
            order = np.array(sorted(again), np.int64)
            self.n_retried += len(order)
            arr2 = ing.work_arrays(self.dev, G, order)
            for b in range(arr2[-1]):
                self._enqueue(ing, arr2, b, 1, 0)
                rec = self._collect(0)
                for _ in range(4 * self.S + 8):
                    if not (rec["phase"] == E.PH_RUN).any():
                        break
                    self.ro._eval_and_step_n(1)
                    self._records(arr2, b, 0)
                    rec = self._collect(0)
                if take(b, rec, order):
                    raise E.EngineError(f"{self.NAME}: a search did not finish")
        return out


def _search_config() -> Dict:
    from . import dropin

    dropin.install()
    import config

    return dict(mcts_batch_size=int(config.MCTS_BATCH_SIZE), cpuct=float(config.CPUCT), widen_coeff=float(config.WIDEN_COEFF),
                dirichlet_epsilon=float(config.DIRICHLET_EPSILON))


def analyse_games(paths_or_text, model, sims: Optional[int] = None, slots: int = 256, device="cuda:0", fast: bool = False,
                  resign_threshold=None, use_graph: bool = True, mcts_batch_size: Optional[int] = None, iterations: Optional[int] = None,
                  **search_cfg) -> Dict:
    """Analyse every game of the PGN files / directories `paths_or_text` (or of one PGN text given as bytes or a str with a newline).

    Returns {"games": [...], "report": {...}, "sims": S}.  A game: index (over all inputs, in order), source, status (pgn.STATUS_NAMES),
    tags [(name, value)] and result as in the input, n_plies, moves [n_plies] (from | to << 6 | promo << 12), positions (bo_position
    [n_plies + 1]; None for a skipped game) and plies: a NumPy array [n_plies] of engine.ANALYSIS_DTYPE -- terminal, n_legal, phase
    (2: searched, 0: the root is over), total_visits, best_move, root_value, played_is_child / played_visits / played_q, pv_len, pv.
    iterations: evaluate -> step iterations enqueued per batch (default: what a search is expected to need); a search that needs more is
    searched again at the end of its file with as many as it takes."""
    if fast:
        raise ValueError("analyse: fast mode is not supported (the reference's search semantics only)")
    if resign_threshold is not None:
        raise ValueError("analyse: resignation does not apply to analysis")
    if getattr(model, "is_pair", False):
        raise ValueError("analyse: two-net analysis is not supported")
    if sims is None:
        sims = W._default_sims()
    t0 = time.perf_counter()
    lib = E.load_hip_library()
    dev = E.runtime_device(device)
    files = [Ingested(lib, dev, name, data) for name, data in _sources(paths_or_text)]
    for f in files:
        f.finish(lib, dev)
    max_plies = max([int(f.n_plies.max()) if f.n_games else 0 for f in files] + [0]) + 2
    from .nn_tune import best_inference_copy

    net = best_inference_copy(model, int(slots), dev) if hasattr(model, "for_inference") else model
    an = Analyser(net, slots, sims, max_plies, dev, mcts_batch_size=mcts_batch_size, use_graph=use_graph, iterations=iterations, **search_cfg)
    games: List[Dict] = []
    by_status = {n: 0 for n in P.STATUS_NAMES}
    t_search = 0.0
    try:
        for f in files:
            t1 = time.perf_counter()
            recs = an.run(f)
            t_search += time.perf_counter() - t1
            start = np.cumsum(f.n_plies) - f.n_plies
            for g in range(f.n_games):
                n, st = int(f.n_plies[g]), P.STATUS_NAMES[int(f.status[g])]
                by_status[st] += 1
                text = f.data[f.spans[g][0]:f.spans[g][1]]
                tags = game_tags(text)
                o = int(f.tok_off[g])
                positions = None
                if st not in ("variant", "bad_fen"):
                    raw = np.concatenate([f.pos_host[o:o + n], f.final[g][None]]) if n else None
                    positions = ring_to_positions(raw) if n else (E.BoPosition * 1)(f.roots[g])
                games.append(dict(index=len(games), source=f.name, status=st, tags=tags, result=game_result(text, tags), n_plies=n,
                                  moves=[int(m) for m in f.moves[start[g]:start[g] + n]], positions=positions,
                                  plies=recs[start[g]:start[g] + n].copy()))
    finally:
        an.close()
    allr = np.concatenate([g["plies"] for g in games]) if games else np.zeros(0, E.ANALYSIS_DTYPE)
    searched = allr["phase"] == E.PH_DONE
    n_s = int(searched.sum())
    played = np.concatenate([np.asarray(g["moves"], np.int32) for g in games]) if games else np.zeros(0, np.int32)
    wall = time.perf_counter() - t0
    report = {
        "games_read": len(games), "games_by_status": {k: v for k, v in by_status.items() if v},
        "games_skipped": sum(v for k, v in by_status.items() if k in ("variant", "bad_fen")),
        "replayed_moves": int(len(allr)), "positions_analysed": n_s, "positions_not_searched": int(len(allr) - n_s),
        "best_is_played": int((allr["best_move"][searched] == played[searched]).sum()),
        "best_is_played_share": float((allr["best_move"][searched] == played[searched]).mean()) if n_s else None,
        "mean_value": float(allr["root_value"][searched].astype(np.float64).mean()) if n_s else None,
        "sims": int(sims), "slots": int(slots), "batches": an.n_batches, "roots_searched_again": an.n_retried,
        "seconds": wall, "search_seconds": t_search, "positions_per_second": (n_s / t_search) if t_search > 0 else None,
    }
    return {"games": games, "report": report, "sims": int(sims)}


# ---- output -------------------------------------------------------------------------------------------------------------------------
def writer_games(games: Sequence[Dict]) -> Tuple[List[Dict], List[Dict]]:
    """(games, tags) for pgn_write.write_pgn: every game that was not skipped; root value v_k after move k, none where the root is over."""
    out, tags = [], []
    for g in games:
        if g["positions"] is None:
            continue
        pl = g["plies"]
        rv = [np.float32(pl["root_value"][k]) if pl["phase"][k] == E.PH_DONE else None for k in range(g["n_plies"])]
        out.append(dict(game_id=g["index"], positions=g["positions"], moves=g["moves"], terminal=0, root_values=rv, result=g["result"]))
        t = {k: v for k, v in g["tags"] if k not in WRITER_TAGS and k != "Result"}
        t.setdefault("Date", "????.??.??")
        tags.append(t)
    return out, tags


def write_annotated(fh, result: Dict, device="cuda:0", lib=None) -> int:
    games, tags = writer_games(result["games"])
    return W.write_pgn(fh, games, tags=tags, device=device, lib=lib, sims=result["sims"]) if games else 0


def jsonl_lines(result: Dict):
    """One JSON object per replayed move, in file order."""
    for g in result["games"]:
        pl = g["plies"]
        for k in range(g["n_plies"]):
            r = pl[k]
            done = int(r["phase"]) == E.PH_DONE
            yield json.dumps({
                "game": g["index"], "ply": k, "terminal": int(r["terminal"]), "searched": done,
                "value": float(r["root_value"]) if done else None,
                "best": E.move_to_uci(int(r["best_move"])) if done and r["n_legal"] > 0 else None,
                "pv": [E.move_to_uci(int(m)) for m in r["pv"][:int(r["pv_len"])]] if done else [],
                "visits": int(r["total_visits"]) if done else 0,
                "played": E.move_to_uci(g["moves"][k]), "played_visits": int(r["played_visits"]) if done else 0,
                "played_q": float(r["played_q"]) if done and r["played_is_child"] else None,
            })


def summary_text(rep: Dict) -> str:
    share = "-" if rep["best_is_played_share"] is None else f"{100.0 * rep['best_is_played_share']:.1f}%"
    mean = "-" if rep["mean_value"] is None else f"{rep['mean_value']:+.4f}"
    pps = "-" if rep["positions_per_second"] is None else f"{rep['positions_per_second']:.1f}"
    by = ", ".join(f"{k} {v}" for k, v in rep["games_by_status"].items())
    return (f"[analyse] games {rep['games_read']} ({by}; skipped {rep['games_skipped']})  positions analysed {rep['positions_analysed']}, "
            f"root over {rep['positions_not_searched']}  best == played {share}  mean value {mean}  "
            f"{rep['seconds']:.1f} s, {pps} positions/s at {rep['sims']} simulations")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.analyse",
                                 description="Search every position of PGN games with a checkpoint; write the root values as eval comments.")
    ap.add_argument("paths", nargs="+", metavar="PATH", help="a .pgn / .pgn.gz file, or a directory searched for them")
    ap.add_argument("--model", required=True, metavar="CHECKPOINT.pth")
    ap.add_argument("-o", "--out", required=True, metavar="ANNOTATED.pgn")
    ap.add_argument("--sims", type=int, default=None, help="simulations per position (default: config.NUM_SIMULATIONS)")
    ap.add_argument("--slots", type=int, default=256, help="roots searched together")
    ap.add_argument("--jsonl", default=None, metavar="FILE", help="one line per analysed position")
    ap.add_argument("--report", default=None, metavar="FILE")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--fast", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--resign-threshold", type=float, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    from .match import build_net, load_state_dict

    dev = E.runtime_device(args.device)
    model = build_net(load_state_dict(args.model), dev)
    res = analyse_games(args.paths, model, sims=args.sims, slots=args.slots, device=args.device, fast=args.fast,
                        resign_threshold=args.resign_threshold)
    with open(args.out, "w", encoding="utf-8", newline="\n") as fh:
        write_annotated(fh, res, device=args.device)
    if args.jsonl:
        with open(args.jsonl, "w", encoding="utf-8", newline="\n") as fh:
            for line in jsonl_lines(res):
                fh.write(line + "\n")
    if args.report:
        with open(args.report, "w", encoding="utf-8") as fh:
            json.dump(res["report"], fh, indent=1)
            fh.write("\n")
    print(summary_text(res["report"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
