"""GPU tests of the two-net evaluate stage (fused_net.PairedNet) and of head-to-head matches (betaone_amd.match) on the MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _net(blocks, se, filters, salt=0):
    """A hash-initialised PolicyValueNet; `salt` gives different weights of the same shape."""
    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = blocks, se, filters
    try:
        net = hash_init_(network.PolicyValueNet(), gain=0.5 + 0.125 * salt)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    return net.to(DEV).eval()


def _sel_patterns(B):
    rs = np.random.RandomState(B)
    odd = 37 if B == 64 else 101  # a boundary inside a heads tile (policy: 32 / 64 / 128 boards, value_fc1: 64)
    return {
        "all0": np.zeros(B), "all1": np.ones(B), "halves": np.arange(B) >= B // 2, "odd": np.arange(B) >= odd,
        "alternating": np.arange(B) & 1, "random": rs.randint(0, 2, B),
    }


def _inputs(B):
    g = torch.Generator().manual_seed(B)
    return (torch.rand((B, 120, 8, 8), generator=g) < 0.2).float().to(DEV)


@pytest.mark.parametrize("shape", [(10, 0, 128), (8, 2, 128), (2, 1, 256)])
@pytest.mark.parametrize("route", ["tower_split", "merge"])
def test_two_net_evaluate_is_bit_identical_to_each_net_alone(shape, route):
    _check_pair_bitwise(shape, route)


@pytest.mark.parametrize("shape", [(10, 0, 128), (8, 2, 128)])
def test_two_net_evaluate_32x32_tiles_at_128_filters(shape, monkeypatch):
    """BETAONE_SPLIT_TILE=32: the 128-filter split tower on bo_k_tower_s<128, 1, 2, 12> -- its PAIR instance."""
    monkeypatch.setenv("BETAONE_SPLIT_TILE", "32")
    _check_pair_bitwise(shape, "tower_split", tile=32)


def _check_pair_bitwise(shape, route, tile=None):
    from betaone_amd.fused_net import FusedPolicyValueNet, PairedNet

    a, b = _net(*shape, salt=0), _net(*shape, salt=1)
    conv = "tower_split" if route == "tower_split" else "tower_f16"  # (a tower_f16 pair has no shared launch: the merge path)
    fa, fb = FusedPolicyValueNet(a, conv=conv).to(DEV), FusedPolicyValueNet(b, conv=conv).to(DEV)
    if tile is not None:
        assert fa.split_tile == fb.split_tile == tile
    pair = PairedNet(fa, fb, batch=64, device=DEV)
    assert pair.route == ("pair:tower_split" if route == "tower_split" else "pair:merge")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (64, 256, 2 * n_cu + 37):  # (the shared launch's grid is min(B, n_cu) workgroups: the last batch takes three passes)
        x = _inputs(B)
        for probs in (False, True):
            with torch.no_grad():
                ref = [fa(x, probs=probs), fb(x, probs=probs)]
            for name, s in _sel_patterns(B).items():
                sel = torch.as_tensor(np.asarray(s, dtype=np.int32), device=DEV)
                with torch.no_grad():
                    lo, vo = pair(x, sel, probs=probs)
                torch.cuda.synchronize()
                m = sel.bool().cpu()
                want_l = torch.where(m[:, None].to(DEV), ref[1][0], ref[0][0])
                want_v = torch.where(m[:, None].to(DEV), ref[1][1].reshape(B, 1), ref[0][1].reshape(B, 1))
                assert torch.equal(lo, want_l), (shape, route, B, probs, name)
                assert torch.equal(vo.reshape(B, 1), want_v), (shape, route, B, probs, name)
    pair.check_overflow()


def test_pair_check_refuses_different_shapes():
    from betaone_amd import engine as E
    from betaone_amd.fused_net import FusedPolicyValueNet, PairedNet

    fa = FusedPolicyValueNet(_net(10, 0, 128), conv="tower_split").to(DEV)
    fb = FusedPolicyValueNet(_net(8, 2, 128), conv="tower_split").to(DEV)
    lib = E.load_hip_library()
    assert lib.bo_nn_tower_pair_check(fa._tower, fb._tower) == -3  # BO_E_CONFIG
    assert lib.bo_nn_tower_pair_check(fa._tower, fa._tower) == 0
    assert PairedNet(fa, fb, batch=64, device=DEV).route == "pair:merge"


def _selfplay_moves(model, ids, slots, cohorts, sims, temperature, max_moves):
    """Self-play of net `model` (alpha = 0) over the given game ids with game_seed seeds: {game_id: uci moves}."""
    from betaone_amd import engine as E
    from betaone_amd.rollout import CohortRollout
    from betaone_amd.selfplay_main import game_seed

    ro = CohortRollout(model, slots, cohorts=cohorts, num_simulations=sims, dirichlet_alpha=0.0, temperature=temperature,
                       max_game_moves=max_moves, rng_mode="native", device=DEV)
    todo = list(ids)
    out = {}
    by_slot = {}

    def fin(f):
        out[by_slot.pop(f.slot)] = [E.move_to_uci(m) for m in f.moves]

    def refill(s):
        if not todo:
            return None
        gid = todo.pop(0)
        by_slot[s] = gid
        return gid, game_seed(0, gid), None

    first = [todo.pop(0) for _ in range(min(slots, len(todo)))]
    for s, gid in enumerate(first):
        by_slot[s] = gid
    ro.start_games(list(range(len(first))), first, [game_seed(0, g) for g in first], [None] * len(first))
    try:
        while by_slot:
            ro.play_ply(on_finished=fin, refill=refill)
        ro.drain()
    finally:
        ro.close()
    return out


def _match(pair, n_games, slots, cohorts, sims, temperature, max_moves, openings=None, **kw):
    from betaone_amd import match as M
    from betaone_amd.rollout import CohortRollout

    ro = CohortRollout(pair, slots, cohorts=cohorts, num_simulations=sims, dirichlet_alpha=0.0, temperature=temperature,
                       max_game_moves=max_moves, rng_mode="native", device=DEV, **kw)
    sched = M.MatchScheduler(openings or [(None, "")], n_games, slots, cohorts)
    try:
        played = M.play_match(ro, sched)
    finally:
        ro.close()
    return played


def test_a_against_a_copy_of_a_plays_the_self_play_games():
    """Same weights in distinct tensors, through the one-launch path: the selector and the pair perturb nothing."""
    from betaone_amd.fused_net import FusedPolicyValueNet, PairedNet

    a = _net(3, 1, 128)
    a2 = _net(3, 1, 128)
    pair = PairedNet(a, a2, batch=16, device=DEV)
    assert pair.route == "pair:tower_split"
    temp, sims, maxm, n = (4, 1.0, 0.1), 48, 24, 40
    played = _match(pair, n, 32, 2, sims, temp, maxm)
    got = {g["game_id"]: g["moves"] for g in played["games"]}
    assert sorted(got) == list(range(n))
    want = _selfplay_moves(FusedPolicyValueNet(a, conv="tower_split").to(DEV), range(n), 32, 2, sims, temp, maxm)
    assert got == want


def test_a_against_b_twice_is_reproducible(tmp_path):
    """Two different nets (merge path: different shapes), openings with black to move, more games than slots: the same match twice
    gives the same games, results and statistics."""
    from betaone_amd import match as M
    from betaone_amd.fused_net import PairedNet

    openings = [(None, ""), ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", ""), (None, "d2d4")]
    runs = []
    for _ in range(2):
        pair = PairedNet(_net(2, 1, 128, salt=0), _net(3, 0, 128, salt=1), batch=8, device=DEV)
        assert pair.route == "pair:merge"
        played = _match(pair, 22, 16, 2, 32, (3, 1.0, 0.1), 20, openings)
        st = M.summarize(played, with_pairs=True)
        for k in ("seconds", "plies_per_second", "nodes_per_second"):
            st.pop(k)
        runs.append((played["games"], st))
    assert runs[0] == runs[1]
    assert sorted(g["game_id"] for g in runs[0][0]) == list(range(22))
    whites = {}
    for g in runs[0][0]:
        whites.setdefault(g["game_id"] // 2, set()).add(g["white"])
    assert all(w == {"A", "B"} for w in whites.values())


class _ProbNet(torch.nn.Module):
    """FakeNet as an evaluate stage: the probabilities are the float64 softmax of its logits rounded to float32 -- exactly what the
    oracle's eval_fn below returns -- so that the engine (policy_kind='probs') and the oracle search with the same numbers."""

    def __init__(self, salt, scale=5.0):
        super().__init__()
        self.salt, self.scale = salt, scale

    def eval_fn(self, planes):
        from fake_model import fake_logits_values

        logits, v = fake_logits_values(planes, self.scale, self.salt)
        x = logits.astype(np.float64)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), v

    def forward_probs(self, x):
        p, v = self.eval_fn(x.detach().cpu().numpy())
        return torch.from_numpy(p).to(x.device), torch.from_numpy(v).reshape(-1, 1).to(x.device)

    def forward(self, x):
        return self.forward_probs(x)


def _oracle_game(fen, prefix, fns, net_of_white, seed, sims, batch, temperature, max_moves):
    """self_play.py's game loop on the CPU oracle with the root's side to move choosing the net: every ply searched by oracle.run_mcts
    with the mover's eval_fn, the move chosen from pi with the game's own RNG -> (uci moves, final termination, white to move at the end)."""
    from oracle import oracle as O

    b = O.Board(fen or O.STARTING_FEN)
    trk = O.PyTracker()
    trk.add_board(b)
    for u in prefix.split():
        b.push(u)
        trk.add_board(b)
    rng = np.random.RandomState(seed)
    cfg = O.default_config(num_simulations=sims, batch_size=batch, dirichlet_alpha=0.0)
    th, ti, tf = temperature
    while b.termination() == 0 and len(b.moves) < max_moves:
        cur = b.pos
        pos = b.positions()
        mover = net_of_white if cur.turn == 1 else 1 - net_of_white
        r = O.run_mcts(b, pos[max(0, len(pos) - 8):-1], trk, fns[mover], rng, cfg)
        action = O.select_move_with_temperature(r["pi"].copy(), cur.fullmove_number, rng, th, ti, tf)
        try:
            played = O.index_to_move(action, cur)
        except ValueError:  # (self_play.py:127-137: an index that is no move here -> the search's best move)
            played = r["best"]
        if played not in [m.tup() for m in b.legal_moves()]:
            played = r["best"]
        m = O.Move()
        m.from_sq, m.to_sq, m.promo = played
        b.push(m)
        trk.add_board(b)
    return [O.move_to_uci(m) for m in b.moves[len(prefix.split()):]], b.termination(), b.pos.turn == 1


def test_a_against_b_matches_the_oracle_with_the_movers_net():
    """Two FakeNet salts on the merge path, openings with black to move (two near a mate), more games than slots: every game's move
    list equals a replay through oracle.run_mcts in which each ply is searched with the net of the side to move, and its result (from
    B's view) is the one the oracle's final position gives."""
    from betaone_amd.fused_net import PairedNet
    from betaone_amd.selfplay_main import game_seed

    openings = [(None, ""), ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", ""),
                ("7k/5Q2/6K1/8/8/8/8/8 w - - 0 1", ""), ("8/8/8/8/8/6k1/5q2/7K b - - 0 1", ""), (None, "e2e4 e7e5 g1f3")]
    na, nb = _ProbNet(salt=11), _ProbNet(salt=22)
    pair = PairedNet(na, nb, batch=8, device=DEV)
    assert pair.route == "pair:merge"
    temp, sims, batch, maxm, n = (3, 1.0, 0.1), 24, 8, 14, 24
    played = _match(pair, n, 16, 2, sims, temp, maxm, openings, mcts_batch_size=batch, policy_kind="probs", use_graph=False)
    assert sorted(g["game_id"] for g in played["games"]) == list(range(n))
    fns = [na.eval_fn, nb.eval_fn]
    decisive = 0
    for g in played["games"]:
        fen, prefix = openings[g["opening"]]
        now = 0 if g["white"] == "A" else 1
        moves, term, white_to_move = _oracle_game(fen, prefix, fns, now, game_seed(0, g["game_id"]), sims, batch, temp, maxm)
        assert g["moves"][len(prefix.split()):] == moves, g["game_id"]
        if term == 1:
            decisive += 1
            winner_net = now if not white_to_move else 1 - now
            assert g["termination"] == "checkmate" and g["result_b"] == (1.0 if winner_net == 1 else 0.0), g["game_id"]
        else:
            assert g["result_b"] == 0.5, g["game_id"]
    assert decisive > 0  # (the two mate-in-one openings: the results of checkmates are checked too)


def test_match_cli_writes_standard_json_and_promotes(tmp_path):
    """python -m betaone_amd.match end to end: checkpoints of two shapes, --out parsed by a strict JSON reader, --promote written."""
    import json

    from betaone_amd import match as M

    pa, pb = tmp_path / "a.pth", tmp_path / "b.pth"
    torch.save(_net(2, 1, 128).state_dict(), pa)
    torch.save(_net(3, 0, 128, salt=1).state_dict(), pb)
    op = tmp_path / "openings.txt"
    op.write_text("startpos\nrnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1\n")
    out, dest = tmp_path / "match.json", tmp_path / "best_model.pth"
    rc = M.main([str(pa), str(pb), "--games", "6", "--slots", "8", "--cohorts", "1", "--sims", "16", "--mcts-batch", "8",
                 "--openings", str(op), "--max-game-moves", "12", "--out", str(out), "--promote", str(dest), "--threshold", "0.0"])
    assert rc == 0

    def no_constants(name):
        raise ValueError(f"non-standard JSON constant {name}")

    res = json.loads(out.read_text(), parse_constant=no_constants)
    st = res["summary"]
    assert st["games"] == 6 and st["wins"] + st["draws"] + st["losses"] == 6
    assert st["interval"] == "pentanomial" and st["route"] == "pair:merge" and st["promoted"] is True
    assert len(res["games"]) == 6 and all(g["moves"] for g in res["games"])
    assert M.net_shape(torch.load(dest)) == (3, 0, 128)
