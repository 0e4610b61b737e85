"""CPU tests of betaone_amd.match: statistics, the scheduler (driven by a pure-Python stand-in rollout), net shapes read from
checkpoints, and the promotion gate."""
import math
import os

import numpy as np
import pytest
import torch

from betaone_amd import match as M


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
def test_score_and_elo_by_hand():
    st = M.match_stats([1.0] * 60 + [0.5] * 20 + [0.0] * 20)
    assert (st["wins"], st["draws"], st["losses"]) == (60, 20, 20)
    assert st["score"] == pytest.approx(0.70)
    assert st["elo"] == pytest.approx(147.19, abs=0.01)
    # trinomial: per-game variance of the scores, 1.96 standard errors
    var = (60 * 0.3 ** 2 + 20 * 0.2 ** 2 + 20 * 0.7 ** 2) / 100
    se = math.sqrt(var / 100)
    assert st["interval"] == "trinomial"
    assert st["elo_95"][0] == pytest.approx(M.elo(0.7 - 1.959963984540054 * se))
    assert st["elo_95"][1] == pytest.approx(M.elo(0.7 + 1.959963984540054 * se))
    assert st["los"] == pytest.approx(0.5 * (1 + math.erf(40 / math.sqrt(160))))
    assert M.elo(0.5) == 0.0 and M.elo(1.0) == math.inf and M.elo(0.0) == -math.inf


def test_pentanomial_interval_on_a_small_pair_table():
    pairs = [(1.0, 1.0), (1.0, 0.5), (0.5, 0.5), (0.0, 1.0), (0.5, 0.0)]  # pair scores 1, .75, .5, .5, .25
    st = M.match_stats([r for p in pairs for r in p], pairs)
    assert st["interval"] == "pentanomial"
    assert st["pentanomial"] == [0, 1, 2, 1, 1]
    m = 0.6
    var = ((1 - m) ** 2 + (0.75 - m) ** 2 + 2 * (0.5 - m) ** 2 + (0.25 - m) ** 2) / 5
    se = math.sqrt(var / 5)
    assert st["score"] == pytest.approx(m)
    assert st["elo_95"] == pytest.approx([M.elo(m - 1.959963984540054 * se), M.elo(m + 1.959963984540054 * se)])


def test_openings_file_format():
    ops = M.parse_openings("# comment\nstartpos\nstartpos ; e2e4 e7e5\n\n"
                           "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1 ; e7e5\n")
    assert ops[0] == (None, "") and ops[1] == (None, "e2e4 e7e5")
    assert ops[2][1] == "e7e5" and ops[2][0].split()[1] == "b"
    assert [M.black_first(f, m) for f, m in ops] == [False, False, False]
    assert M.black_first(None, "e2e4") and M.black_first(ops[2][0], "")


# ---- the scheduler under a stand-in rollout -----------------------------------------------------------------------------------------
class _Pos:
    def __init__(self, white_to_move):
        self.turn = 1 if white_to_move else 0


class _Fin:
    def __init__(self, slot, moves, positions, terminal):
        self.slot, self.moves, self.positions, self.terminal = slot, moves, positions, terminal


class StandInRollout:
    """The slot/ply mechanics of CohortRollout in pure Python: every active slot plays one move per cohort ply; a game that is over is
    reported and its slot refilled at the start of a ply, and the new game sits that ply out (its first search is at the next one).
    At every ply it checks the lane rule on every searched slot: sel = net_of_white ^ (black to move) == the lane's net."""

    def __init__(self, sched, n_slots, cohorts, lengths):
        self.sched, self.G, self.K, self.Gc = sched, n_slots, cohorts, n_slots // cohorts
        self.lengths = lengths  # game_id -> plies it lasts
        self.slot = [None] * n_slots  # [game_id, net_of_white, black to move, plies played, first step]
        self.step = [0] * cohorts
        self.n_plies = self.n_sims = 0
        self.checked = 0
        self.played_ids = []

    def start_games(self, slots, ids, seeds, fens, moves, nows):
        for i, s in enumerate(slots):
            bf = M.black_first(fens[i], (moves[i] if moves else "") or "")
            self.slot[s] = [ids[i], nows[i], bf, 0, self.step[s // self.Gc]]
            self.played_ids.append(ids[i])

    def play_ply(self, on_finished=None, refill=None):
        for k in range(self.K):
            fresh = set()
            for s in range(k * self.Gc, (k + 1) * self.Gc):
                st = self.slot[s]
                if st is not None and st[3] >= self.lengths[st[0]]:
                    on_finished(_Fin(s, [0] * st[3], [_Pos(not st[2])], 2))
                    self.slot[s] = None
                    nxt = refill(s)
                    if nxt is not None:
                        gid, seed, fen, moves, now = nxt
                        self.slot[s] = [gid, now, M.black_first(fen, moves), 0, self.step[k] + 1]
                        self.played_ids.append(gid)
                        fresh.add(s)
            for s in range(k * self.Gc, (k + 1) * self.Gc):
                st = self.slot[s]
                if st is None or s in fresh:
                    continue
                g = self.sched.admitted[st[0]]
                assert st[4] <= self.step[k]
                if not g.lane_break:
                    assert st[1] ^ int(st[2]) == M.MatchScheduler.lane_net(self.sched.lane(s), self.step[k])
                    self.checked += 1
                st[2] = not st[2]
                st[3] += 1
                self.n_plies += 1
            self.step[k] += 1
        return 0


@pytest.mark.parametrize("n_games,slots,cohorts", [(40, 8, 2), (37, 8, 2), (64, 16, 4), (23, 4, 1)])
def test_scheduler_pairs_colours_lanes_and_game_count(n_games, slots, cohorts):
    openings = [(None, ""), (None, "e2e4"), ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq - 0 1", ""), (None, "d2d4 d7d5 c2c4")]
    sched = M.MatchScheduler(openings, n_games, slots, cohorts)
    rs = np.random.RandomState(n_games)
    lengths = {g: int(rs.randint(1, 12)) for g in range(n_games)}
    ro = StandInRollout(sched, slots, cohorts, lengths)
    played = M.play_match(ro, sched, step_of=lambda s: ro.step[s // ro.Gc] + 1)
    ids = [g["game_id"] for g in played["games"]]
    assert sorted(ids) == list(range(n_games))            # --games honoured, also when not a multiple of the slots
    assert sorted(ro.played_ids) == list(range(n_games))  # no game id played twice
    by = {g["game_id"]: g for g in played["games"]}
    for i in range(0, n_games - 1, 2):                    # each opening once with each colour
        assert by[i]["opening"] == by[i + 1]["opening"]
        assert {by[i]["white"], by[i + 1]["white"]} == {"A", "B"}
    assert ro.checked > 0
    assert played["lane_breaks"] == sched.lane_breaks
    assert sched.lane_breaks <= max(2, n_games // 8)     # (only when no pending game of the needed colour is left)
    assert all(g["result_b"] == 0.5 for g in played["games"])


def test_scheduler_refuses_odd_lanes():
    with pytest.raises(ValueError):
        M.MatchScheduler([(None, "")], 4, 6, 2)


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def _net(blocks, se, filters):
    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = blocks, se, filters
    try:
        return hash_init_(network.PolicyValueNet())
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


@pytest.mark.parametrize("shape", [(3, 1, 64), (8, 2, 128), (2, 1, 256)])
def test_net_shape_from_checkpoint_keys(shape, tmp_path):
    net = _net(*shape)
    path = tmp_path / "net.pth"
    torch.save(net.state_dict(), path)
    sd = M.load_state_dict(str(path))
    assert M.net_shape(sd) == shape
    rebuilt = M.build_net(sd)  # with config at some other shape: read from the keys
    for k, v in net.state_dict().items():
        assert torch.equal(rebuilt.state_dict()[k], v), k


def test_promote_only_at_threshold_and_never_partial(tmp_path, monkeypatch):
    net = _net(1, 0, 64)
    dest = tmp_path / "best_model.pth"
    dest.write_bytes(b"old")
    assert not M.promote(net.state_dict(), str(dest), 0.5499, 0.55)
    assert dest.read_bytes() == b"old"
    assert M.promote(net.state_dict(), str(dest), 0.55, 0.55)
    sd = torch.load(dest)
    assert M.net_shape(sd) == (1, 0, 64)
    # a write that fails half-way leaves the old file and no temporary behind
    dest.write_bytes(b"old")

    def broken_save(obj, f):
        f.write(b"partial")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", broken_save)
    with pytest.raises(OSError):
        M.promote(net.state_dict(), str(dest), 0.9, 0.55)
    assert dest.read_bytes() == b"old"
    assert sorted(os.listdir(tmp_path)) == ["best_model.pth"]


@pytest.mark.parametrize("white_to_move_at_end", [True, False])
@pytest.mark.parametrize("net_of_white", [0, 1])
def test_game_result_of_a_checkmate(white_to_move_at_end, net_of_white):
    """terminal 1: the side to move in the final position is mated; B (net 1) scores 1 exactly when the winner's net is 1."""
    fin = _Fin(0, [0], [_Pos(True), _Pos(white_to_move_at_end)], 1)
    r, how = M.game_result(fin, net_of_white)
    winner_is_white = not white_to_move_at_end
    winner_net = net_of_white if winner_is_white else 1 - net_of_white
    assert how == "checkmate"
    assert r == (1.0 if winner_net == 1 else 0.0)
    # spelled out: B white (net_of_white = 1) and black to move mated -> B won
    if net_of_white == 1 and not white_to_move_at_end:
        assert r == 1.0
    if net_of_white == 0 and not white_to_move_at_end:
        assert r == 0.0
    assert M.game_result(_Fin(0, [0], [_Pos(True)], 2), net_of_white) == (0.5, "draw")
    assert M.game_result(_Fin(0, [0], [_Pos(True)], 0), net_of_white) == (0.5, "move_limit")


def test_results_file_is_standard_json():
    import json

    st = M.match_stats([1.0] * 5)  # a 100 % score: Elo +inf
    assert st["elo"] == math.inf
    text = json.dumps(M.json_safe({"summary": st}), allow_nan=False)
    assert json.loads(text)["summary"]["elo"] is None


def test_promote_keeps_the_destinations_mode_and_gives_a_new_file_the_umask(tmp_path):
    net = _net(1, 0, 64)
    dest = tmp_path / "best_model.pth"
    dest.write_bytes(b"old")
    os.chmod(dest, 0o644)
    assert M.promote(net.state_dict(), str(dest), 1.0, 0.55)
    assert (os.stat(dest).st_mode & 0o777) == 0o644
    new = tmp_path / "new.pth"
    old = os.umask(0o027)
    try:
        assert M.promote(net.state_dict(), str(new), 1.0, 0.55)
    finally:
        os.umask(old)
    assert (os.stat(new).st_mode & 0o777) == 0o640
