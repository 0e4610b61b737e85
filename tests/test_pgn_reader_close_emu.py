"""CPU test of the PGN reader threads' shutdown (betaone_amd/pgn.py: _Reader): a run that stops early (pretrain --max-steps) closes its
readers while they are still parsing.  A block that a reader has put on its queue belongs to whoever takes it from there; the reader
must not close it as well -- two threads closing one block destroy its handle twice (the destroy call runs without the GIL)."""
import threading
import time

import engine_harness as H
import test_pgn_emu as T

from betaone_amd import pgn as P


def test_every_block_is_closed_by_exactly_one_owner(tmp_path, monkeypatch):
    games, text = T.make_corpus(3, 12, max_plies=40)
    files = []
    for i in range(6):
        p = tmp_path / f"f{i}.pgn"
        p.write_text(text)
        files.append(str(p))
    lib = H.emu_lib()
    closers, lock = {}, threading.Lock()
    made = []
    orig_init, orig_close = P.ParsedGames.__init__, P.ParsedGames.close

    def init(self, *a, **kw):
        orig_init(self, *a, **kw)
        made.append(self)  # (kept alive: ids stay distinct)

    def close(self):
        with lock:  # every thread that closes this block, whether or not it still finds the handle set
            closers.setdefault(id(self), set()).add(threading.get_ident())
        orig_close(self)

    monkeypatch.setattr(P.ParsedGames, "__init__", init)
    monkeypatch.setattr(P.ParsedGames, "close", close)
    for rep in range(12):
        r = P._Reader(lib, files, 64, None, {}, depth=2)
        first = r.next()
        assert first is not None
        first.close()
        time.sleep(0.01 * (rep % 3))  # the queue fills up: the thread waits in put()
        r.close()
        assert not r.t.is_alive()
    assert made and all(m.h is None for m in made if id(m) in closers)
    assert all(len(t) == 1 for t in closers.values()), [t for t in closers.values() if len(t) > 1]
