"""GPU tests of reanalysis (csrc/bo_reanalyse.h, betaone_amd/reanalyse.py) on an MI355X: the device bodies of
tests/test_reanalyse_emu.py on the product library, and the tool with a real evaluate stage -- the small net of tests/test_resign_gpu.py
(3 + 1 blocks, 64 filters, conv="tower_wg", 16 slots, 50 simulations in batches of 48, games of at most 30 moves).

The slot count and the tower choice are the same wherever two runs are compared bit for bit: nn_tune and the evaluate stage pick
kernels by shape, and different kernels need not give the same bits."""
import numpy as np
import pytest
import torch

import reanalyse_cases as RC

from betaone_amd import engine as E
from betaone_amd import records as R

pytestmark = pytest.mark.gpu

G, SIMS, BATCH, MOVES, N_GAMES = 16, 50, 48, 30, 24
SEARCH = dict(mcts_batch_size=BATCH, cpuct=1.0, widen_coeff=1.5, dirichlet_epsilon=0.25)
# game g starts from FENS[g % 4]: without noise, and with the one or two root children of the reference's widening, games from one root
# differ little -- four roots (one with castling rights and an en-passant capture on the board) give four families of games
FENS = [None, "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", "rnbqkbnr/pppppppp/8/8/3P4/8/PPP1PPPP/RNBQKBNR b KQkq - 0 1",
        "r3k2r/1P4p1/8/2pP4/8/8/1p4P1/R3K2R w KQkq c6 0 12"]


def test_ring_entries_from_records_equal_the_pgn_replay_s_gpu():
    assert RC.check_ring_bytes("hip") > 2000


def test_record_against_search_result_gpu():
    widest = two = 0
    for widen in (1.5, 6.0):
        for flat in (True, False):
            n, t = RC.check_record_against_search_result("hip", widen, flat)
            widest, two = max(widest, n), two + t
    assert widest > 2 and two >= 1


def test_old_against_new_bit_for_bit_gpu():
    RC.check_old_against_new("hip")


def _nets():
    """(the PolicyValueNet, its hand-written evaluate stage) twice: the net that plays and a second one."""
    from betaone_amd import dropin

    dropin.install()
    import config
    import network
    from betaone_amd.fused_net import FusedPolicyValueNet
    from fake_model import hash_init_

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 3, 1, 64
    try:
        out = []
        for gain in (0.5, 0.8):
            net = hash_init_(network.PolicyValueNet().eval(), gain=gain).to("cuda:0")
            out.append((net, FusedPolicyValueNet(net, conv="tower_wg").to("cuda:0")))
        return out
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
        torch.cuda.synchronize()


def _play(net, path, **rkw):
    from betaone_amd.rollout import Rollout

    ro = Rollout(net, G, num_simulations=SIMS, dirichlet_alpha=0.0, device="cuda:0", rng_mode="native", max_game_moves=MOVES, **SEARCH, **rkw)
    assert ro.use_graph
    ro.device_turn = True
    ro.start_games(list(range(G)), list(range(G)), [900 + g for g in range(G)], fens=[FENS[g % 4] for g in range(G)])
    nxt, fins = [G], {}

    def refill(slot):
        if nxt[0] >= N_GAMES:
            return None
        nxt[0] += 1
        return nxt[0] - 1, 900 + nxt[0] - 1, FENS[(nxt[0] - 1) % 4]

    for _ in range(3 * MOVES):
        ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f), refill=refill)
        if len(fins) == N_GAMES:
            break
    ro.eng.check_status()
    ro.close()
    assert len(fins) == N_GAMES
    R.save_games(str(path), [fins[g] for g in sorted(fins)])


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reanalyse_gpu")
    nets = _nets()
    d1, d2 = tmp / "bog1" / "iter_4", tmp / "bog2" / "iter_4"
    _play(nets[0][1], d1 / "games_rank0.bog")
    _play(nets[0][1], d2 / "games_rank0.bog", record_values=True)
    return tmp, nets, d1, d2


def _bytes(d):
    return [open(p, "rb").read() for p in RC.bog_files(d)]


def _reanalyse(src, out, net, slots=G, **kw):
    from betaone_amd import reanalyse as RA

    return RA.reanalyse_records([str(src)], net, str(out), sims=SIMS, slots=slots, **SEARCH, **kw)


def test_the_net_that_played_gives_the_files_back_gpu(played):
    """Self-play with graph capture and the device turn, noise off; the same net, slot count and evaluate stage: byte-identical files."""
    tmp, nets, d1, d2 = played
    for d, name in ((d1, "same1"), (d2, "same2")):
        rep = _reanalyse(d, tmp / name, nets[0][1])
        n = sum(g["n_plies"] for g in RC.games_of(d))
        assert rep["roots_searched"] + rep["roots_kept"] == n > 300 and rep["roots_kept"] == 0
        assert _bytes(tmp / name / "iter_4") == _bytes(d)
        assert rep["mean_tv"] == 0.0 and rep["top1_agreement"] == 1.0 and rep["batch_copy_bytes"] == G * (64 + 8 * 8)
    assert rep["mean_abs_dq"] == 0.0


def test_padding_and_many_batches_gpu(played):
    """A slot count that does not divide the root count: the last batch is padded, and there are many batches.  Two runs give the same
    files.  5 slots, unless every game ran to the move limit (30 plies each: 5 divides the count) -- then 7."""
    tmp, nets, _, d2 = played
    n = sum(g["n_plies"] for g in RC.games_of(d2))
    slots = 5 if n % 5 else 7
    assert n % slots != 0
    reps = [_reanalyse(d2, tmp / f"five{i}", nets[1][1], slots=slots) for i in range(2)]
    assert _bytes(tmp / "five0" / "iter_4") == _bytes(tmp / "five1" / "iter_4") != _bytes(d2)
    for rep in reps:
        assert rep["roots_searched"] == n and rep["roots_kept"] == 0 and 0 <= rep["roots_retried"] <= n
        # every root in one of ceil(n / slots) batches, every retried root in one of the batches behind them
        assert rep["batches"] - -(-n // slots) == (-(-rep["roots_retried"] // slots) if rep["roots_retried"] else 0)
    RC.same_but_targets(RC.games_of(d2), RC.games_of(tmp / "five0" / "iter_4"))


def test_analyse_and_reanalyse_agree_gpu(played):
    """Two tools, two ingests: the PGN of the games through analyse, the records through reanalyse, a second net, the same slot count."""
    from betaone_amd import analyse as A
    from betaone_amd import pgn_write as W
    from betaone_amd import reanalyse as RA

    tmp, nets, _, d2 = played
    path = RC.bog_files(d2)[0]
    pgn = tmp / "games.pgn"
    assert W.main([path, "-o", str(pgn), "--date", "2026.10.19", "--sims", str(SIMS)]) == 0
    res = A.analyse_games([str(pgn)], nets[1][1], sims=SIMS, slots=G, **SEARCH)
    assert len(res["games"]) == N_GAMES and len({tuple(g["moves"]) for g in res["games"]}) >= 4
    lib, dev = E.load_hip_library(), torch.device("cuda:0")
    f = RA.RecordFile(lib, dev, path, iteration=4)
    an = RA.Reanalyser(nets[1][1], G, SIMS, int(f.n_plies.max()) + 2, dev, pi_width=8, **SEARCH)
    try:
        an.begin_file(f)
        rec = an.run(f)
    finally:
        an.close()
    start = np.cumsum(f.n_plies) - f.n_plies
    compared = 0
    for g in range(f.n_games):
        n, s = int(f.n_plies[g]), int(start[g])
        assert res["games"][g]["moves"] == [int(m) for m in f.all_moves[s:s + n]]          # the PGN keeps the file's order
        a = res["games"][g]["plies"]
        r = rec[s:s + n]
        assert np.array_equal(a["phase"], r["phase"]) and np.array_equal(a["terminal"], r["terminal"])
        done = r["phase"] == E.PH_DONE
        assert np.array_equal(a["root_value"][done].view(np.uint32), r["root_value"][done].view(np.uint32))
        assert np.array_equal(a["total_visits"][done], r["total_visits"][done])
        for k in np.nonzero(done)[0]:
            m = int(r["pi_n"][k])
            first_max = int(an.pi_idx[s + k, int(np.argmax(an.pi_val[s + k, :m]))])
            assert int(RA.moves_to_actions(a["best_move"][k:k + 1])[0]) == first_max, (g, k)
            compared += 1
    assert compared > 300


def test_the_output_feeds_training_and_validation_gpu(played, tmp_path):
    from betaone_amd import validate as V

    tmp, nets, _, d2 = played
    out = tmp_path / "re"
    _reanalyse(d2, out, nets[1][1])
    games = RC.games_of(out / "iter_4")
    buf = R.GpuReplayBuffer(4096, pi_width=8)
    try:
        buf.add(games)
        n = sum(g["n_plies"] for g in games)
        assert len(buf) == n == buf.n_with_values
        states, idx, val, z, q = buf.batch_sparse_q(np.arange(64))
        torch.cuda.synchronize()
        assert states.shape == (64, E.INPUT_CHANNELS, 8, 8) and idx.shape == (64, 8) and q.shape == (64, 1)
        want = np.concatenate([g["root_values"] for g in games])[:64]
        assert np.array_equal(q.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))
        sums = val.cpu().numpy().astype(np.float64).sum(axis=1)
        assert np.allclose(sums, 1.0, atol=1e-6)
    finally:
        buf.close()
    ck = tmp_path / "net.pth"
    torch.save(nets[1][0].state_dict(), ck)
    assert V.main([str(out / "iter_4"), "--model", str(ck), "--all", "--with-q"]) == 0
