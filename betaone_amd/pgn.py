"""betaone_amd/pgn.py -- PGN games -> compact records in HBM -> pretraining batches.

The reference pretrains on PGN games through PGNDataset (train.py:81-160) and a DataLoader (train.py:356-396): python-chess reads each
game, replays its SAN and encodes the 120 planes of every position in worker processes.  Here the text is tokenised by the library's host
code (csrc/bo_pgn.h, in reader threads), the SAN is replayed on the device (bo_k_pgn_replay: one wave per game) into a ring of position
slots, and a batch is encoded on the device from those records (bo_k_pgn_sample), with the reference's LIVE repetition tracker.

    ing = PgnIngest(["fishtest/"], device="cuda:0", window_plies=1 << 22)
    for states, pi_idx, pi_val, z in ing.loader(256):      # train.train_steps(..., sparse=True)
        ...
    ing.counts                                             # games per status, plies replayed, samples

Orders: "reference" reproduces DataLoader(PGNDataset(sorted paths), batch_size=B, num_workers=W) -- worker w reads files w, w + W, ...,
cuts its stream of samples into batches of B (its last partial batch kept), and batches come round-robin over the workers that still
have data.  "shuffle" draws batches uniformly from the resident window (seeded).
"""
from __future__ import annotations

import ctypes as C
import glob
import gzip
import os
import queue
import threading
import time
from collections import deque
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import engine as E

STATUS_NAMES = ["ok", "variant", "bad_fen", "unsupported", "null_move", "illegal", "ambiguous", "mismatch"]  # BO_PGN_* of include/betaone_engine.h
POSITION_BYTES = 80  # BO_PGN_POSITION_BYTES
MAX_READER_THREADS = 16  # host threads a pretraining run may use
_CLOSE_LOCK = threading.Lock()


def pgn_paths(args: Sequence[str]) -> List[str]:
    """Files as given; a directory contributes every **/*.pgn and **/*.pgn.gz under it (train.py:363 globs **/*.pgn).  Sorted."""
    out = []
    for a in args:
        if os.path.isdir(a):
            for pat in ("*.pgn", "*.pgn.gz"):
                out.extend(glob.glob(os.path.join(a, "**", pat), recursive=True))
        else:
            out.append(a)
    return sorted(set(out))


class ParsedGames:
    """A bo_pgn handle: games tokenised on the host."""

    def __init__(self, lib, handle):
        self.lib, self.h = lib, handle
        g, t, s = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(lib.bo_pgn_size(handle, C.byref(g), C.byref(t), C.byref(s)))
        self.n_games, self.n_tokens, self.scratch_bytes = int(g.value), int(t.value), int(s.value)
        self._exp = None

    def _check(self, rc):
        if rc != 0:
            raise E.EngineError(f"pgn: {self.lib.bo_last_error().decode()}")

    def export(self) -> dict:
        """status [games], tok_off [games + 1], roots (BoPosition [games]), tokens uint32, has_eval int32, target float32 [tokens]."""
        if self._exp is None:
            G, T = self.n_games, self.n_tokens
            st, off = np.zeros(G, np.int32), np.zeros(G + 1, np.int32)
            roots = (E.BoPosition * max(G, 1))()
            tok, ev, tg = np.zeros(max(T, 1), np.uint32), np.zeros(max(T, 1), np.int32), np.zeros(max(T, 1), np.float32)
            self._check(self.lib.bo_pgn_export(self.h, st.ctypes.data_as(E._I32P), off.ctypes.data_as(E._I32P), roots,
                                               tok.ctypes.data, ev.ctypes.data_as(E._I32P), tg.ctypes.data_as(E._F32P)))
            self._exp = {"status": st, "tok_off": off, "roots": roots, "tokens": tok[:T], "has_eval": ev[:T], "target": tg[:T]}
        return self._exp

    def close(self):
        with _CLOSE_LOCK:  # (the destroy call releases the GIL: two threads must not both find the handle set)
            h, self.h = self.h, None
        if h:
            self.lib.bo_pgn_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_chunk(lib, buf: bytes, offset: int, final: bool, max_games: int = -1, max_tokens: int = -1):
    """(ParsedGames of the complete games in buf[offset:], bytes consumed)."""
    h, used = C.c_void_p(), C.c_int64()
    addr = C.cast(C.c_char_p(buf), C.c_void_p).value + offset
    rc = lib.bo_pgn_parse(addr, len(buf) - offset, 1 if final else 0, max_games, max_tokens, C.byref(used), C.byref(h))
    if rc != 0:
        raise E.EngineError(f"pgn: {lib.bo_last_error().decode()}")
    return ParsedGames(lib, h), int(used.value)


def parse_text(text, lib=None) -> ParsedGames:
    """All games of one PGN text (str or bytes)."""
    lib = lib or E.load_hip_library()
    b = text.encode() if isinstance(text, str) else bytes(text)
    return parse_chunk(lib, b, 0, True)[0]


def read_blocks(lib, path: str, block_tokens: int, max_games: Optional[int] = None, chunk_bytes: int = 4 << 20, stats: Optional[dict] = None):
    """The games of one .pgn / .pgn.gz file as ParsedGames blocks of about block_tokens tokens, in file order.  max_games: per file, as
    PGNDataset's (train.py:88-89)."""
    left = -1 if max_games is None else int(max_games)
    opener = gzip.open if path.endswith(".gz") else open
    carry = b""
    with opener(path, "rb") as f:
        while left != 0:
            data = f.read(chunk_bytes)
            final = not data
            buf = carry + data if carry else data
            off = 0
            while left != 0:
                t0 = time.perf_counter()
                blk, used = parse_chunk(lib, buf, off, final, left, block_tokens)
                if stats is not None:
                    stats["parse_s"] = stats.get("parse_s", 0.0) + time.perf_counter() - t0
                    stats["bytes"] = stats.get("bytes", 0) + used
                off += used
                if blk.n_games == 0:
                    blk.close()
                    break
                if left > 0:
                    left -= blk.n_games
                yield blk
            carry = buf[off:]
            if final:
                break


class _Reader:
    """One stream's files parsed in a thread of its own, a few blocks ahead (the library call releases the GIL)."""

    def __init__(self, lib, files, block_tokens, max_games, stats, depth=3):
        self.q: queue.Queue = queue.Queue(maxsize=depth)
        self.err = None
        self.stop = False

        def run():
            try:
                for p in files:
                    for blk in read_blocks(lib, p, block_tokens, max_games, stats=stats):
                        handed = False
                        while not self.stop:
                            try:
                                self.q.put(blk, timeout=0.2)
                                handed = True  # the block now belongs to whoever takes it from the queue (the consumer, or close()'s drain)
                                break
                            except queue.Full:
                                pass
                        if not handed:
                            blk.close()
                        if self.stop:
                            return
            except BaseException as e:  # noqa: BLE001  (re-raised by the consumer)
                self.err = e
            finally:
                self.q.put(None)

        self.t = threading.Thread(target=run, daemon=True)
        self.t.start()

    def next(self):
        b = self.q.get()
        if b is None and self.err is not None:
            raise self.err
        return b

    def _drain(self):
        try:
            while True:
                b = self.q.get_nowait()
                if b is not None:
                    b.close()
        except queue.Empty:
            pass

    def close(self):
        """Stops the thread and waits for it: it may be inside the library's parser, and an interpreter that exits meanwhile frees
        memory under it.  The thread sees `stop` within one block's parse or one 0.2 s queue wait; draining the queue lets its final
        put go through.  (Bounded at 60 s.)"""
        self.stop = True
        for _ in range(600):
            self._drain()
            self.t.join(timeout=0.1)
            if not self.t.is_alive():
                break
        self._drain()


def _close_readers(readers):
    for r in readers:  # (stop them all first: they wind down together)
        if r is not None:
            r.stop = True
    for r in readers:
        if r is not None:
            r.close()


class _Block:
    __slots__ = ("start", "length", "g0", "k", "cur")

    def __init__(self, start, length, g0, k):
        self.start, self.length, self.g0, self.k, self.cur = start, length, g0, k, 0

    @property
    def remaining(self):
        return len(self.k) - self.cur


class PgnIngest:
    """PGN files -> a ring of window_plies position slots in HBM -> sparse training batches (pi width 1).

    paths: files and directories (pgn_paths).  order: "reference" (default) or "shuffle".  workers: the DataLoader's num_workers for the
    reference order (default config.NUM_WORKERS).  max_games: per file.  counts: games per status, plies replayed, samples."""

    def __init__(self, paths: Sequence[str], device="cuda:0", window_plies: int = 1 << 22, order: str = "reference",
                 workers: Optional[int] = None, seed: int = 0, max_games: Optional[int] = None, block_tokens: Optional[int] = None):
        from . import dropin

        dropin.install()
        import config

        if order not in ("reference", "shuffle"):
            raise ValueError(f"order {order!r}: 'reference' or 'shuffle'")
        self.lib = E.load_hip_library()
        self.device = E.runtime_device(device)
        self.paths = pgn_paths(paths)
        self.order, self.seed, self.max_games = order, int(seed), max_games
        self.workers = int(workers if workers is not None else config.NUM_WORKERS) if order == "reference" else 1
        if not 1 <= self.workers <= MAX_READER_THREADS:
            raise ValueError(f"workers: 1 .. {MAX_READER_THREADS} (one reader thread each)")
        self.cap = int(window_plies)
        if self.cap < 1024:
            raise ValueError("window_plies >= 1024")
        streams = max(1, self.workers)
        self.block_tokens = int(block_tokens) if block_tokens else min(1 << 17, max(256, self.cap // (4 * streams)))
        kw = dict(device=self.device)
        self.pos = torch.empty(self.cap * POSITION_BYTES, dtype=torch.uint8, **kw)
        self.act = torch.empty(self.cap, dtype=torch.int32, **kw)
        self.z = torch.empty(self.cap, dtype=torch.float32, **kw)
        self.smp = torch.empty(self.cap, dtype=torch.int32, **kw)
        self.scratch = torch.empty(1 << 16, dtype=torch.uint8, **kw)
        self.side = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None
        self.head = 0
        self.live: deque = deque()   # resident blocks, oldest first
        self.counts = {n: 0 for n in STATUS_NAMES}
        self.counts.update(games=0, plies=0, samples=0)
        self.stats = {"parse_s": 0.0, "bytes": 0, "replay_s": 0.0}

    # ---- ingest ----
    def _ingest(self, blk: ParsedGames, keep: bool = True) -> _Block:
        """Replay one block of games into the ring; returns its samples (game slot, ply) in stream order."""
        x = blk.export()
        T = blk.n_tokens
        if T > self.cap:
            raise RuntimeError(f"pgn: a block of {T} plies does not fit window_plies={self.cap}")
        if self.head + T > self.cap:
            self.head = 0
        lo, hi = self.head, self.head + T
        while self.live and self.live[0].start < hi and self.live[0].start + self.live[0].length > lo:
            old = self.live.popleft()
            if self.order == "reference" and old.remaining:
                raise RuntimeError(f"pgn: window_plies={self.cap} is too small for {self.workers} workers' pending samples")
        if any(b.start < hi and b.start + b.length > lo for b in self.live):
            raise RuntimeError("pgn: ring placement overlaps a resident block")  # (blocks are placed in order: unreachable)
        off = x["tok_off"]
        slot0 = (lo + off[:-1]).astype(np.int64)
        if blk.scratch_bytes > self.scratch.numel():
            self.scratch = torch.empty(2 * blk.scratch_bytes, dtype=torch.uint8, device=self.device)
        G = blk.n_games
        n_plies, status = np.zeros(max(G, 1), np.int32), np.zeros(max(G, 1), np.int32)
        t0 = time.perf_counter()
        if self.side is not None:
            self.side.wait_stream(torch.cuda.current_stream(self.device))  # (queued batches may still read the slots)
            stream = self.side.cuda_stream
        else:
            stream = 0
        rc = self.lib.bo_pgn_replay(blk.h, slot0.ctypes.data_as(C.POINTER(C.c_int64)), self.cap, self.scratch.data_ptr(), self.scratch.numel(),
                                    self.pos.data_ptr(), self.act.data_ptr(), self.z.data_ptr(), self.smp.data_ptr(),
                                    n_plies.ctypes.data_as(E._I32P), status.ctypes.data_as(E._I32P), stream)
        if rc != 0:
            raise E.EngineError(f"pgn: {self.lib.bo_last_error().decode()}")
        self.stats["replay_s"] += time.perf_counter() - t0
        n_plies, status = n_plies[:G], status[:G]
        # ply t of game g is a sample when move t + 1 was replayed and has an eval (the kernel's smp flag)
        has_eval = x["has_eval"]
        game_of = np.repeat(np.arange(G), np.diff(off))
        t = np.arange(T)
        k = t - off[game_of]
        nxt = np.zeros(T, bool)
        if T > 1:
            nxt[:-1] = has_eval[1:] != 0
        is_s = (k + 1 < n_plies[game_of]) & nxt
        g0 = (lo + off[game_of[is_s]]).astype(np.int32)
        b = _Block(lo, T, g0, k[is_s].astype(np.int32))
        for s, c in zip(*np.unique(status, return_counts=True)):
            self.counts[STATUS_NAMES[int(s)]] += int(c)
        self.counts["games"] += G
        self.counts["plies"] += int(n_plies.sum())
        self.counts["samples"] += len(b.k)
        self.head = hi
        if keep:
            self.live.append(b)
        blk.close()
        return b

    def _streams(self):
        files = [self.paths[w::self.workers] for w in range(self.workers)]
        return [_Reader(self.lib, f, self.block_tokens, self.max_games, self.stats) if f else None for f in files]

    def count(self) -> int:
        """Ingest every file without training (countpgn.py's job): the number of samples."""
        readers = [r for r in self._streams() if r is not None]
        try:
            for r in readers:
                while True:
                    blk = r.next()
                    if blk is None:
                        break
                    self._ingest(blk, keep=False)
        finally:
            _close_readers(readers)
        return self.counts["samples"]

    # ---- batches ----
    def batch(self, game_slot, ply):
        """(states [n,120,8,8], pi_idx [n,1] int32, pi_val [n,1], z [n,1]) of the samples at (game slot, ply)."""
        q = np.ascontiguousarray(np.stack([np.asarray(game_slot, np.int32), np.asarray(ply, np.int32)]))
        n = q.shape[1]
        qt = torch.from_numpy(q)
        if self.device.type == "cuda":
            qt = qt.pin_memory().to(self.device, non_blocking=True)
        kw = dict(dtype=torch.float32, device=self.device)
        states, zs, val = torch.empty((n, E.INPUT_CHANNELS, 8, 8), **kw), torch.empty((n, 1), **kw), torch.empty((n, 1), **kw)
        idx = torch.empty((n, 1), dtype=torch.int32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else 0
        rc = self.lib.bo_pgn_sample(self.pos.data_ptr(), self.act.data_ptr(), self.z.data_ptr(), n, qt[0].data_ptr(), qt[1].data_ptr(),
                                    states.data_ptr(), idx.data_ptr(), val.data_ptr(), zs.data_ptr(), stream)
        if rc != 0:
            raise E.EngineError(f"pgn: {self.lib.bo_last_error().decode()}")
        if self.device.type == "cuda":
            qt.record_stream(torch.cuda.current_stream(self.device))
        return states, idx, val, zs

    def _take(self, pend: deque, n: int):
        gs, ks = [], []
        while n and pend:
            b = pend[0]
            m = min(n, b.remaining)
            gs.append(b.g0[b.cur:b.cur + m])
            ks.append(b.k[b.cur:b.cur + m])
            b.cur += m
            n -= m
            if not b.remaining:
                pend.popleft()
        if not gs:
            return None
        return np.concatenate(gs), np.concatenate(ks)

    def sample_refs(self, batch_size: int) -> Iterable:
        """The loader's batches as (game slots, plies) arrays, without encoding them."""
        if self.order == "reference":
            yield from self._refs_reference(int(batch_size))
        else:
            yield from self._refs_shuffle(int(batch_size))

    def _refs_reference(self, B: int):
        readers = self._streams()
        pend = [deque() for _ in readers]
        active = [w for w, r in enumerate(readers) if r is not None]
        try:
            while active:
                for w in list(active):
                    have = sum(b.remaining for b in pend[w])
                    while have < B and readers[w] is not None:
                        blk = readers[w].next()
                        if blk is None:
                            readers[w] = None
                            break
                        b = self._ingest(blk)
                        pend[w].append(b)
                        have += b.remaining
                    got = self._take(pend[w], B)
                    if got is None:
                        active.remove(w)
                        continue
                    yield got
        finally:
            _close_readers(readers)

    def _refs_shuffle(self, B: int):
        rng = np.random.default_rng(self.seed)
        reader = _Reader(self.lib, self.paths, self.block_tokens, self.max_games, self.stats)
        owed, done = 0, False
        try:
            while not done:
                # ingest until the next block would evict a resident one (or the files end)
                while True:
                    blk = reader.next()
                    if blk is None:
                        done = True
                        break
                    evicts = self.live and (self.head + blk.n_tokens > self.cap or any(
                        b.start < self.head + blk.n_tokens and b.start >= self.head for b in self.live))
                    owed += len(self._ingest(blk).k)
                    if evicts:
                        break
                g0 = np.concatenate([b.g0 for b in self.live]) if self.live else np.zeros(0, np.int32)
                ks = np.concatenate([b.k for b in self.live]) if self.live else np.zeros(0, np.int32)
                if not len(ks):
                    continue
                while owed >= B or (done and owed > 0):
                    m = min(B, owed)
                    q = rng.integers(0, len(ks), size=m)
                    owed -= m
                    yield g0[q], ks[q]
        finally:
            reader.close()

    def loader(self, batch_size: int, sparse: bool = True, max_steps: Optional[int] = None):
        """An iterable of batches with GpuReplayBuffer.loader's contract: (states, pi_idx [B,1], pi_val [B,1], z [B,1]) with sparse=True,
        (states, pi [B,4672], z [B,1]) otherwise."""
        return _PgnLoader(self, int(batch_size), sparse, max_steps)

    def close(self):
        self.live.clear()


class _PgnLoader:
    def __init__(self, ing: PgnIngest, batch_size: int, sparse: bool, max_steps: Optional[int]):
        self.ing, self.batch_size, self.sparse, self.max_steps = ing, batch_size, sparse, max_steps

    def __iter__(self):
        for i, (g0, k) in enumerate(self.ing.sample_refs(self.batch_size)):
            if self.max_steps is not None and i >= self.max_steps:
                return
            states, idx, val, z = self.ing.batch(g0, k)
            if self.sparse:
                yield states, idx, val, z
            else:
                pi = torch.zeros((len(k), E.NUM_ACTIONS), dtype=torch.float32, device=states.device)
                yield states, pi.scatter_(1, idx.long(), val), z


def token_str(t: int) -> str:
    """A packed token as canonical text: O-O / O-O-O, else [piece][file][rank]square[=promotion] (no capture or check marks)."""
    t = int(t)
    kind = (t >> 20) & 3
    if kind:
        return "O-O" if kind == 1 else "O-O-O"
    to, ff, fr, pc, pr = t & 63, ((t >> 6) & 15) - 1, ((t >> 10) & 15) - 1, (t >> 14) & 7, (t >> 17) & 7
    s = " PNBRQK"[pc].strip() + ("abcdefgh"[ff] if ff >= 0 else "") + ("12345678"[fr] if fr >= 0 else "")
    s += "abcdefgh"[to & 7] + "12345678"[to >> 3]
    return s + ("=" + " PNBRQK"[pr] if pr else "")


def replay_games(parsed: ParsedGames, device="cuda:0") -> dict:
    """Every game of `parsed` replayed once into slots of its own (game g from slot tok_off[g]): per game n_plies and status, per slot the
    position bytes [T,80], act, smp and z (host arrays).  For tests and measurements."""
    lib = parsed.lib
    dev = E.runtime_device(device)
    x = parsed.export()
    T, G = max(parsed.n_tokens, 1), parsed.n_games
    pos = torch.zeros(T * POSITION_BYTES, dtype=torch.uint8, device=dev)
    act, smp = torch.full((T,), -1, dtype=torch.int32, device=dev), torch.zeros(T, dtype=torch.int32, device=dev)
    z = torch.zeros(T, dtype=torch.float32, device=dev)
    scratch = torch.empty(max(parsed.scratch_bytes, 16), dtype=torch.uint8, device=dev)
    slot0 = x["tok_off"][:-1].astype(np.int64)
    n_plies, status = np.zeros(max(G, 1), np.int32), np.zeros(max(G, 1), np.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0
    rc = lib.bo_pgn_replay(parsed.h, slot0.ctypes.data_as(C.POINTER(C.c_int64)), T, scratch.data_ptr(), scratch.numel(), pos.data_ptr(),
                           act.data_ptr(), z.data_ptr(), smp.data_ptr(), n_plies.ctypes.data_as(E._I32P), status.ctypes.data_as(E._I32P), stream)
    if rc != 0:
        raise E.EngineError(f"pgn: {lib.bo_last_error().decode()}")
    return {"n_plies": n_plies[:G], "status": status[:G], "tok_off": x["tok_off"], "pos": pos.cpu().numpy().reshape(T, POSITION_BYTES),
            "act": act.cpu().numpy(), "smp": smp.cpu().numpy(), "z": z.cpu().numpy()}
