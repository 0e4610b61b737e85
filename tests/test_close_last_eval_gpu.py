"""GPU tests: the product path (hipGraph-captured iterations, the hand-written evaluate stage) ends a search's expected iterations with
bo_k_search_close in place of the last leaf evaluation (Rollout._eval_and_step_n).  Against BETAONE_CLOSE_LAST_EVAL=0 -- the search as it
was -- the games are the same, moves and pi bit for bit, with ceil(S / B) network forwards per searched ply instead of ceil(S / B) + 1,
and the close is a node of the captured n-iteration graph."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLIES, BATCH = 5, 96


@pytest.fixture(scope="module")
def net():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    sys.path.insert(0, os.path.join(ROOT, "oracle", "shim"))
    from betaone_amd import dropin
    from betaone_amd import engine as E

    E.load_hip_library()
    dropin.install()
    import config
    import network
    from betaone_amd.fused_net import FusedPolicyValueNet

    keys = ("RESIDUAL_BLOCKS", "SE_RESIDUAL_BLOCKS", "CONV_FILTERS")
    saved = {k: getattr(config, k) for k in keys}
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 3, 1, 64
    torch.manual_seed(0)
    fused = FusedPolicyValueNet(network.PolicyValueNet().to("cuda:0").eval(), conv="tower_wg").to("cuda:0")
    for k, v in saved.items():
        setattr(config, k, v)
    yield fused


def _run(monkeypatch, net, close, sims, G, cohorts):
    from betaone_amd.rollout import CohortRollout, Rollout

    monkeypatch.setenv("BETAONE_CLOSE_LAST_EVAL", "1" if close else "0")
    kw = dict(num_simulations=sims, mcts_batch_size=BATCH, device="cuda:0", use_graph=True, rng_mode="native")
    ro = CohortRollout(net, G, cohorts=cohorts, **kw) if cohorts > 1 else Rollout(net, G, **kw)
    parts = ro.parts if cohorts > 1 else [ro]
    assert all(p.close_last_eval == close for p in parts)  # (on by default where the iterations are captured graphs)
    ro.start_games(list(range(G)), list(range(G)), [300 + g for g in range(G)])
    per_ply = []
    for _ in range(PLIES):
        f0 = ro.n_forward
        assert ro.play_ply() == G
        per_ply.append(ro.n_forward - f0)
    if cohorts > 1:
        ro.drain()
    games = []
    for p in parts:
        p.eng.check_status()
        games += [p._finish(g, 0) for g in range(p.G)]
    out = dict(games=[(list(f.moves), [(np.asarray(i).tolist(), np.asarray(v, np.float32).view(np.uint32).tolist()) for i, v in f.pis]) for f in games],
               per_ply=per_ply, n_forward=ro.n_forward, turns=sum(p._step for p in parts), graph_keys=[sorted(map(str, p._graphs_n)) for p in parts])
    ro.close()
    return out


@pytest.mark.parametrize("sims", [200,    # batches of 96, 96 and 8
                                  192])   # the last batch exactly full
def test_closing_plays_the_same_games_with_one_forward_less_per_ply(monkeypatch, net, sims):
    n = math.ceil(sims / BATCH)
    a = _run(monkeypatch, net, False, sims, 16, 1)
    b = _run(monkeypatch, net, True, sims, 16, 1)
    assert a["games"] == b["games"]
    assert all(len(m) == PLIES and len(pis) == PLIES for m, pis in a["games"])
    print("forwards per ply, close off / on:", a["per_ply"], b["per_ply"])
    # (the first call holds the root's evaluation and enqueues the next ply's; every later call: the next root's evaluation + the leaves')
    assert a["per_ply"] == [2 + n] + [1 + n] * (PLIES - 1)
    assert b["per_ply"] == [1 + n] + [n] * (PLIES - 1)
    # the iterations ran as ONE captured graph per search, the close inside it: n iterations behind an early root evaluation
    assert a["graph_keys"] == [sorted([str(n), str(n + 1)])]
    assert b["graph_keys"] == [sorted([str((n, True)), str((n + 1, True))])]


def test_closing_in_cohorts_plays_the_same_games(monkeypatch, net):
    sims = 200
    a = _run(monkeypatch, net, False, sims, 32, 2)
    b = _run(monkeypatch, net, True, sims, 32, 2)
    assert a["games"] == b["games"] and len(a["games"]) == 32
    assert a["turns"] == b["turns"] == 2 * (PLIES + 1)  # (every call begins the cohorts' next ply; drain() ends that one too)
    assert a["n_forward"] - b["n_forward"] == a["turns"]  # one forward less per cohort-ply
    assert all(any("True" in k for k in keys) for keys in b["graph_keys"]) and not any("True" in k for keys in a["graph_keys"] for k in keys)
