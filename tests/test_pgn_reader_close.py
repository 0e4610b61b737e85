"""CPU test (wave emulator): a pretraining loader abandoned part-way through its files stops and joins its reader threads when it is
closed, so no thread is left inside the library's parser while the process goes on (or exits)."""
import threading
import time

import engine_harness as H
import test_pgn_emu as T
from betaone_amd import pgn as P


def _new_threads(before):
    return [t for t in threading.enumerate() if t not in before and t.is_alive()]


def test_closing_an_abandoned_loader_joins_its_readers(tmp_path, monkeypatch):
    parse = P.parse_chunk

    def slow_parse(*a, **kw):  # a reader busy in the parser when the loader is closed
        out = parse(*a, **kw)
        time.sleep(0.3)
        return out

    monkeypatch.setattr(P, "parse_chunk", slow_parse)
    for f in range(6):
        _, text = T.make_corpus(200 + f, 40, max_plies=60)
        (tmp_path / f"f{f}.pgn").write_text(text)
    before = set(threading.enumerate())
    with H.emulator_backend():
        for order in ("reference", "shuffle"):
            ing = P.PgnIngest([str(tmp_path)], device="cpu", window_plies=1 << 14, order=order, workers=3, block_tokens=200, seed=1)
            it = iter(ing.loader(8))
            next(it)
            assert _new_threads(before)  # (the readers are still parsing ahead)
            it.close()                   # what happens to the loader of `pretrain --max-steps` when it goes out of scope
            assert _new_threads(before) == [], order
