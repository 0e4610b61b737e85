"""GPU tests of PGN pretraining on the MI355X: SAN resolution, the round trip bit-identical to the restatement of the reference's
PGNDataset.parse, reproducible ingests, the reference batch order, and `python -m betaone_amd.pretrain` on the 10x128 net."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pgn_reference as RF
import test_pgn_emu as T

from betaone_amd import pgn as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


@pytest.mark.parametrize("fen,cases", T.test_san_resolution.pytestmark[0].args[1])
def test_san_resolution_gpu(fen, cases):
    text = "".join(f'[FEN "{fen}"]\n\n{san} *\n\n' for san, _ in cases)
    r = P.replay_games(P.parse_text(text), device=DEV)
    for g, (san, want) in enumerate(cases):
        st, n, act = P.STATUS_NAMES[r["status"][g]], int(r["n_plies"][g]), int(r["act"][r["tok_off"][g]])
        if want in ("illegal", "ambiguous"):
            assert (st, n) == (want, 0), san
        else:
            assert (st, n, act) == ("ok", 1, T._idx(want)), san


def test_round_trip_and_reproducible_ingest_gpu(tmp_path):
    games, text = T.make_corpus(7, 600, max_plies=100)
    (tmp_path / "c0.pgn").write_text(text)
    pg = P.parse_text(text)
    r = P.replay_games(pg, device=DEV)
    assert set(r["status"].tolist()) == {0}
    for g, (fen, mv, _) in enumerate(games):
        a = r["tok_off"][g]
        assert int(r["n_plies"][g]) == len(mv) and r["act"][a:a + len(mv)].tolist() == [T._idx(u) for u in mv], g
    exp = T.expected_samples(games)
    recs = []
    for _ in range(2):
        ing = P.PgnIngest([str(tmp_path / "c0.pgn")], device=DEV, window_plies=1 << 17, workers=1, block_tokens=1 << 17)
        batches = [ing.batch(g0, k) for g0, k in ing.sample_refs(4096)]
        torch.cuda.synchronize()
        assert ing.counts["samples"] == len(exp)
        recs.append((ing.pos.cpu().numpy().copy(), ing.act.cpu().numpy().copy(), [tuple(t.cpu() for t in b) for b in batches]))
    s, i, v, z = (torch.cat([b[j] for b in recs[0][2]]) for j in range(4))
    T.check_batch(s, i, v, z, exp)
    n = pg.n_tokens  # (one block from slot 0: every slot of [0, n) was written, the rest of the ring was not)
    assert np.array_equal(recs[0][0][:n * P.POSITION_BYTES], recs[1][0][:n * P.POSITION_BYTES]) and np.array_equal(recs[0][1][:n], recs[1][1][:n])
    for b0, b1 in zip(recs[0][2], recs[1][2]):
        assert all(np.array_equal(x.numpy().view(np.uint8), y.numpy().view(np.uint8)) for x, y in zip(b0, b1))


def test_reference_batch_order_gpu(tmp_path):
    W, B = 3, 64
    files = []
    for f, n in enumerate([30, 90, 10, 60, 20, 0, 40]):
        games, text = T.make_corpus(300 + f, n, max_plies=60) if n else ([], "")
        (tmp_path / f"f{f:02d}.pgn").write_text(text)
        files.append(games)
    streams = [[s for g in files[w::W] for s in T.expected_samples(g)] for w in range(W)]
    batches = [[st[i:i + B] for i in range(0, len(st), B)] for st in streams]
    order, active, cur = [], list(range(W)), [0] * W
    while active:
        for w in list(active):
            if cur[w] >= len(batches[w]):
                active.remove(w)
                continue
            order.append(batches[w][cur[w]])
            cur[w] += 1
    ing = P.PgnIngest([str(tmp_path)], device=DEV, window_plies=1 << 15, workers=W, block_tokens=2000)
    got = list(ing.loader(B))
    assert len(got) == len(order)
    for (s, i, v, z), exp in zip(got, order):
        T.check_batch(s, i, v, z, exp)


def test_pretrain_command_10x128_gpu(tmp_path, monkeypatch):
    import torch as _t

    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    for k, v in (("RESIDUAL_BLOCKS", 8), ("SE_RESIDUAL_BLOCKS", 2), ("CONV_FILTERS", 128)):
        monkeypatch.setattr(config, k, v)
    _t.manual_seed(0)
    init = tmp_path / "init.pth"
    _t.save(network.PolicyValueNet().state_dict(), init)
    games, text = T.make_corpus(41, 60, max_plies=80)
    data = tmp_path / "pgn"
    data.mkdir()
    for i in range(80):
        (data / f"r{i:02d}.pgn").write_text(text)
    out = tmp_path / "s.json"
    cmd = [sys.executable, "-m", "betaone_amd.pretrain", str(data), "--init", str(init), "--save-dir", str(tmp_path / "ck"), "--batch", "256",
           "--max-steps", "300", "--log-every", "50", "--t-max", "2000", "--out", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    s = json.load(open(out))
    for k in ("counts", "steps", "samples", "samples_per_s", "intervals", "ingest_positions_per_s", "tokenizer_mb_per_s", "lr_final"):
        assert s[k] is not None, k
    assert s["steps"] == 300 and s["counts"]["ok"] > 0
    iv = [x["loss"] for x in s["intervals"]]
    assert all(np.isfinite(iv)) and iv[-1] < iv[0]
    assert os.path.exists(tmp_path / "ck" / "pretrained.pth")
