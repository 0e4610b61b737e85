"""tests/tb_search_cases.py -- checks of the endgame tablebases inside the search and at the root (csrc/bo_tree.h: step_body<true>,
root_prepare; bo_engine_tablebases), shared by the wave-emulator tests (test_tb_search_emu.py) and the MI355X tests
(test_tb_search_gpu.py): the same bodies, parameterised by backend ("emu" / "hip").

Tables.  On the GPU the real KQK / KRK / KPK (tablebase_cases.built).  On the emulator no pass can run, so KQK and KRK are SYNTHETIC:
the classification (illegal entries 0, checkmates 2), every other legal entry replaced by a seeded pseudo-random code of the parity
its side to move allows (the strong side to move: a draw or an odd k; the weak side: a draw or an even k >= 2), with draws, k up to 99,
a cluster of k around 45 and k above 512, plus a few entries set by hand so that the trees below are certain to meet them.  (The clamp
in m(k) cannot fire while the clock condition stands -- the halfmove clock is never negative, so an accepted k is at most 100 -- and
the k above 512 are there to show exactly that: such a leaf is refused and goes to the net.)  The search only reads the table and the host expectation reads the same array.

The value rule (DESIGN "Tablebases in the search"): a covered non-root leaf that the rules leave ongoing, with at most 4 men and no
castling rights, is a table leaf when its code is a draw or a mate in k with halfmove clock + k <= 100; bo_debug_tree reports 5 (draw,
q_value 0), 3 (the side to move wins: q_value -m(k)) or 4 (it loses: +m(k)), m(k) = 1 - min(k, 512) / 1024, and no children.

One root of the issue's list cannot exist as written -- "a 5-man root where one capture leads into KRK": a capture leaves 4 men.  Both
halves are kept: FIVE_MEN (one capture leads to 4 men without a table, every other move stays at 5 men, where the man count closes
the gate) and KRKN (one capture leads into KRK, every other move stays at 4 men without a table)."""
import contextlib
import functools
import io

import numpy as np

import engine_cases as EC
import engine_harness as H
import tablebase_cases as TC
from betaone_amd import engine as E
from betaone_amd import tablebase as TB
from oracle import oracle as O

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
KRK_WHITE = "8/8/8/4k3/8/8/8/K6R w - - 0 1"
KRK_BLACK = "k6r/8/8/8/4K3/8/8/8 b - - 0 1"       # its colour mirror: black is the strong side
KQK_WEAK = "8/8/8/4k3/8/8/8/K6Q b - - 0 1"         # the weak side to move
FIVE_MEN = "2b1k3/8/8/8/8/8/7n/K6R w - - 0 1"      # Rxh2 leaves 4 men (KRKB: no table); every other move stays at 5
KRKN = "4k3/8/8/8/8/8/7n/K6R w - - 0 1"            # Rxh2 leads into KRK; every other move stays at KRKN (no table)
CASTLING = "4k3/8/8/8/8/8/8/4K2R w K - 0 1"
KPK_PROMO = "8/P7/8/4k3/8/8/8/K7 w - - 0 1"        # a8=Q / a8=R are covered by KQK / KRK; KPK itself is not loaded
KRK_CLOCK = "8/8/8/4k3/8/8/8/K6R w - - 60 80"
TREE_ROOTS = [KRK_WHITE, KRK_BLACK, KQK_WEAK, FIVE_MEN, KRKN, CASTLING, KPK_PROMO, KRK_CLOCK]
SEARCH, ADJUDICATE = E.Engine.TB_SEARCH, E.Engine.TB_ADJUDICATE


def m_of(k):
    """m(k) = 1 - min(k, 512) / 1024 in binary32 (exact)."""
    return np.float32(1.0) - np.float32(min(int(k), 512)) / np.float32(1024.0)


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _set_children(payload, fen, k):
    """Every legal, non-mate, covered child of `fen` gets the code 2 + k (k of the parity the child's side to move allows; None: a draw)."""
    b = O.Board(fen)
    n = 0
    for mv in b.legal_moves():
        b.push(mv)
        bb, wtm = TC.pos_bitboards(b.pos)
        name, idx = TB.position_index(bb, wtm)
        if name in payload and payload[name][idx] not in (0, 2):
            strong_moves = idx < len(payload[name]) // 2
            assert k is None or (k & 1) == (1 if strong_moves else 0), (fen, k)
            payload[name][idx] = 1 if k is None else 2 + k
            n += 1
        b.pop()
    assert n > 0, fen


def _randomised(codes, seed):
    n = len(codes)
    rs = np.random.RandomState(seed)
    u = rs.randint(0, 100, n)
    k = np.where(u < 25, rs.randint(40, 51, n), np.where(u < 35, rs.randint(513, 700, n), rs.randint(1, 100, n)))
    strong = np.arange(n) < n // 2
    k = np.where(strong, k | 1, np.maximum(k & ~1, 2))
    new = np.where(u >= 85, 1, 2 + k)
    return np.where(codes == 1, new, codes).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def synthetic_set():
    """KQK and KRK with pseudo-random codes on the emulator (see the head of this file); .payload[name] = the host copy."""
    payload = {}
    with H.emulator_backend():
        for i, name in enumerate(("KQK", "KRK")):
            t = TB.Table(name, [], "cpu")
            assert t.build(max_passes=0) == 0
            payload[name] = _randomised(t.download(), 11 + i)
            t.close()
    # the trees of check_tree_invariants are certain to meet: k > 512 (every child of the KQK root: refused), k around 45 (every child of the
    # mirrored KRK root), and at the root with halfmove clock 60 children the clock condition refuses (61 + 40 > 100) whose own
    # children it accepts (62 + 37 <= 100)
    b = O.Board(KQK_WEAK)
    for mv in b.legal_moves():  # (below the refused children of the KQK root: draws)
        b.push(mv)
        _set_children(payload, b.fen(), None)
        b.pop()
    _set_children(payload, KQK_WEAK, 601)
    _set_children(payload, KRK_BLACK, 44)
    _set_children(payload, KRK_CLOCK, 40)
    b = O.Board(KRK_CLOCK)
    for mv in b.legal_moves():
        b.push(mv)
        _set_children(payload, b.fen(), 37)
        b.pop()
    _set_children(payload, KRK_CLOCK, 40)  # (a grandchild may be another child's position: the children keep their 40)
    with H.emulator_backend():
        ts = TB.TableSet("cpu")
        for name in ("KQK", "KRK"):
            ts.add(name).upload(payload[name], 0)
    ts.payload = payload
    return ts


def table_set(backend):
    """The set a backend's tests share (nobody changes it)."""
    return synthetic_set() if backend == "emu" else TC.built("hip", ("KQK", "KRK", "KPK"))


def tables_of(ts, names):
    return [ts.tables[n] for n in names]


# ---- 1. tree invariants, node by node ---------------------------------------------------------------------------------------------------
def _hashed_eval(salt, scale=4.0):
    from fake_model import fake_logits_values

    def fn(planes):
        logits, v = fake_logits_values(planes, scale, salt)
        x = logits.astype(np.float64)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32), v
    return fn


def expected_node(payload, root_fen, chain):
    """(code, q bits or None, k or None, refused by the clock) a visited non-root node must show: the position is rebuilt by replaying
    its move chain on an oracle board; the rule code is the oracle's, the table code the host index's."""
    b = O.Board(root_fen)
    for m in chain:
        b.push(E.move_to_uci(m))
    t = b.termination()
    if t != 0:
        return (1 if t == 1 else 2), None, None, False
    p = b.pos
    bb, wtm = TC.pos_bitboards(p)
    if p.castling or bin(bb[6] | bb[7]).count("1") > 4:
        return 0, None, None, False
    name, idx = TB.position_index(bb, wtm)
    code = 1 if name is None else (int(payload[name][idx]) if name in payload else 0xFFFF)
    if code == 1:
        return 5, bits(0.0), None, False
    if code in (0, 0xFFFF):
        return 0, None, None, False
    k = code - 2
    if p.halfmove_clock + k > 100:
        return 0, None, k, True
    return (3, bits(-m_of(k)), k, False) if k & 1 else (4, bits(m_of(k)), k, False)


def check_tree_invariants(backend, sims=128, batch=16):
    """Every visited node of eight searches run in one launch sequence, against the host's own reading of rules and tables; the
    counters of bo_engine_tb_stats against the dump.  KQK and KRK are loaded, KPK is not (the promotion root's other children read
    TB_NO_TABLE).  widen_coeff 4 gives the roots four children and more."""
    ts = table_set(backend)
    payload = {n: ts.payload[n] for n in ("KQK", "KRK")}
    G = len(TREE_ROOTS)
    eng = H.make_engine(backend, G, dict(num_simulations=sims, batch_size=batch, widen_coeff=4.0, dirichlet_alpha=0.3))
    eng.tablebases(tables_of(ts, ("KQK", "KRK")), SEARCH)
    eng.reset(list(range(G)), TREE_ROOTS)
    nl, term, _ = eng.root_info()
    assert term.tolist() == [0] * G  # (search mode alone adjudicates nothing)
    res = H.Searcher(backend, eng).search(np.ones(G, np.int32), [_hashed_eval(300 + g) for g in range(G)],
                                          [np.random.RandomState(g) for g in range(G)], 0.3)
    assert res["total"].tolist() == [sims] * G
    stats = eng.tb_stats()
    assert stats["adjudicated"].tolist() == [0] * G
    seen = {"refused": 0, "accepted_under_clock": 0, "above_512_refused": 0, "draw": 0, "win": 0, "loss": 0, "rule": 0, "ordinary": 0}
    for g, fen in enumerate(TREE_ROOTS):
        nodes = eng.debug_tree(g)
        assert nodes[0]["terminal"] == 0, fen  # the root is never a table terminal in search mode
        chains = {0: []}
        tb_nodes = tb_sims = 0
        for i, nd in enumerate(nodes[1:], 1):
            chains[i] = chains[nd["parent"]] + [nd["move"]]
            if nd["terminal"] < 0:  # created, never selected
                assert nd["n"] == 0 and nd["n_children"] == 0
                continue
            code, q, k, refused = expected_node(payload, fen, chains[i])
            assert nd["terminal"] == code, (fen, [E.move_to_uci(m) for m in chains[i]], nd, code, k)
            if code >= 3:
                assert nd["n_children"] == 0 and nd["n"] >= 1 and bits(nd["q"]) == q, (fen, chains[i], nd, k)
                tb_nodes += 1
                tb_sims += nd["n"]
                seen["draw" if code == 5 else "win" if code == 3 else "loss"] += 1
                assert k is None or k <= 100
                if fen == KRK_CLOCK and code != 5:
                    seen["accepted_under_clock"] += 1
            elif code in (1, 2):
                assert nd["n_children"] == 0
                seen["rule"] += 1
            else:
                seen["ordinary"] += 1
                seen["refused"] += int(refused and fen == KRK_CLOCK)
                seen["above_512_refused"] += int(refused and k > 512)
        assert (int(stats["tb_nodes"][g]), int(stats["tb_sims"][g])) == (tb_nodes, tb_sims), (fen, stats)
    print("tree invariants:", seen, "tb_nodes", stats["tb_nodes"].tolist(), "tb_sims", stats["tb_sims"].tolist())
    assert seen["win"] + seen["loss"] > 0 and seen["ordinary"] > 0
    if backend == "emu":  # (the synthetic k values are set for this; the real KRK's are all below 40)
        assert seen["refused"] >= 1 and seen["accepted_under_clock"] >= 1 and seen["above_512_refused"] >= 1 and seen["draw"] >= 1
    eng.check_status()
    eng.close()
    return seen


# ---- 2. off means off ---------------------------------------------------------------------------------------------------------------------
def _play_plain(backend, fens, attach, plies=3, sims=32, batch=16):
    """Games through the engine-level self-play loop; (moves, pi bits, final trees) per game.  attach: None, or (tables, flags)."""
    G = len(fens)
    eng = H.make_engine(backend, G, dict(num_simulations=sims, batch_size=batch, max_game_moves=plies))
    if attach is not None:
        eng.tablebases(*attach)
    eng.reset(list(range(G)), fens)
    got = EC.play_games(backend, eng, [_hashed_eval(40 + g) for g in range(G)], [np.random.RandomState(7 + g) for g in range(G)], 0.1, plies)
    out = [(g["moves"], [p.view(np.uint32).tolist() for p in g["pis"]], H.canonical_tree(eng.debug_tree(i))) for i, g in enumerate(got)]
    eng.close()
    return out


def check_off_means_off(backend):
    ts = table_set(backend)
    tabs = tables_of(ts, ("KQK", "KRK"))
    fens = [START, KRK_WHITE]
    never = _play_plain(backend, fens, None)
    assert all(len(g[0]) == 3 for g in never)
    assert _play_plain(backend, fens, (tabs, 0)) == never            # a set attached, flags 0: covered positions included
    assert _play_plain(backend, fens, ([], SEARCH | ADJUDICATE)) == never  # no set: off whatever the flags say
    assert _play_plain(backend, fens[:1], (tabs, SEARCH | ADJUDICATE)) == never[:1]  # both flags on, 32 men: the probing kernel, gate closed


def check_oracle_parity_with_tables_attached(backend):
    """engine_cases.check_multi_game_vs_oracle on engines that have the tables attached and both flags on."""
    ts = table_set(backend)
    tabs = tables_of(ts, ("KQK", "KRK"))
    made = []

    def make(*a, **kw):
        eng = H.make_engine(*a, **kw)
        eng.tablebases(tabs, SEARCH | ADJUDICATE)
        made.append(eng)
        return eng

    saved = EC.make_engine
    EC.make_engine = make
    try:
        EC.check_multi_game_vs_oracle(backend, n_games=3, plies=4, sims=40, batch=16)
    finally:
        EC.make_engine = saved
    assert len(made) == 1 and made[0].tb_stats()["tb_nodes"].tolist() == [0, 0, 0]


# ---- 3. / 4. games through Rollout ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_net():
    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 2, 1, 64
    try:
        return hash_init_(network.PolicyValueNet().eval()).to("cuda:0")
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def play_rollout(backend, fens, *, slots, cohorts=1, device_turn=True, sims=32, batch=16, max_game_moves=8, **rkw):
    """Every start FEN as one seeded self-play game (game id = its index) through Rollout / CohortRollout; {game id: FinishedGame}."""
    from betaone_amd.rollout import CohortRollout, Rollout
    from fake_model import FakeNet

    ctx = H.emulator_backend() if backend == "emu" else contextlib.nullcontext()
    with ctx:
        kw = dict(num_simulations=sims, mcts_batch_size=batch, rng_mode="native", max_game_moves=max_game_moves, **rkw)
        if backend == "emu":
            kw.update(device="cpu", use_graph=False)
            net = FakeNet()
        else:
            kw.update(device="cuda:0")
            net = gpu_net()
        ro = CohortRollout(net, slots, cohorts=cohorts, **kw) if cohorts > 1 else Rollout(net, slots, **kw)
        parts = ro.parts if cohorts > 1 else [ro]
        for p in parts:
            p.device_turn = device_turn
        n0 = min(slots, len(fens))
        ro.start_games(list(range(n0)), list(range(n0)), [500 + g for g in range(n0)], fens[:n0])
        nxt, fins = [n0], {}

        def refill(slot):
            if nxt[0] >= len(fens):
                return None
            g = nxt[0]
            nxt[0] += 1
            return g, 500 + g, fens[g]

        for _ in range((max_game_moves + 3) * (len(fens) // n0 + 1)):
            if len(fins) == len(fens):
                break
            ro.play_ply(on_finished=lambda f: fins.__setitem__(f.game_id, f), refill=refill)
        if cohorts > 1:
            ro.drain()
        assert len(fins) == len(fens), (len(fins), len(fens))
        for p in parts:
            p.eng.check_status()
        counters = dict(tb_nodes=ro.tb_nodes, tb_sims=ro.tb_sims, adjudicated=ro.n_adjudicated)
        ro.close()
    return fins, counters


def adjudication_fens(backend):
    if backend == "emu":  # KQK and KRK only (the synthetic set); a capture leaves KK, so coverage never ends mid-game
        return [KRK_WHITE, KRK_BLACK, KQK_WEAK, "8/8/8/4k3/8/8/8/K6Q w - - 0 1", "7k/8/8/8/8/8/R7/K7 b - - 3 9", START]
    return [KRK_WHITE, KRK_BLACK, KQK_WEAK, "8/8/8/4k3/8/8/8/K6Q w - - 0 1",
            "8/8/8/8/8/4k3/4P3/4K3 w - - 0 1",      # KPK, the pawn blocked by the black king: drawn
            "8/8/8/8/8/4k3/4P3/4K3 b - - 0 1",      # the same with black to move
            "4k3/8/4K3/4P3/8/8/8/8 b - - 0 1",      # KPK, black to move is lost (the white king on the sixth rank in front of its pawn)
            "8/8/8/3k4/8/3K4/3P4/8 w - - 0 1",      # KPK, white to move
            START]


def check_adjudication_equals_rescore(backend, tmp_path, *, cohorts, device_turn, slots=4, max_game_moves=8):
    """A run with tb_adjudicate writes byte for byte the records tablebase.rescore makes of the plain run's records; the adjudicated
    games are exactly the ones rescore cuts."""
    from betaone_amd import records as R

    ts = table_set(backend)
    fens = adjudication_fens(backend)
    kw = dict(slots=slots, cohorts=cohorts, device_turn=device_turn, max_game_moves=max_game_moves)
    plain, _ = play_rollout(backend, fens, **kw)
    adj, counters = play_rollout(backend, fens, tablebases=ts, tb_adjudicate=True, **kw)
    assert counters["tb_nodes"] == 0 and counters["tb_sims"] == 0  # (adjudication alone: the search never probes)
    ids = sorted(plain)
    src, out = tmp_path / "iter_0", tmp_path / "rescored"
    src.mkdir()
    blobs = [R.pack_game(plain[g]) for g in ids]
    (src / "games_rank0.bog").write_bytes(b"".join(blobs))
    with TC.backend_ctx(backend):
        rep = TB.rescore(str(src), ts, write=str(out))
    want = (out / "games_rank0.bog").read_bytes()
    got = [R.pack_game(adj[g]) for g in ids]
    assert b"".join(got) == want
    idx = R.scan_games(want)
    assert [i[0] for i in idx] == ids
    cut = [want[o:o + size] != blob for (gid, n, o, size), blob in zip(idx, blobs)]
    assert [bool(adj[g].adjudicated) for g in ids] == cut, (cut, rep)
    assert sum(cut) == rep["games_cut"] == counters["adjudicated"] and sum(cut) >= 3
    assert not adj[ids[-1]].adjudicated and len(adj[ids[-1]].moves) == max_game_moves  # the game from the start position runs on
    assert all(f.terminal in ((2, 3) if f.adjudicated else (0, 1, 2)) for f in adj.values())
    assert all(f.outcome == (1.0 if f.terminal in (1, 3) else 0.0) for f in adj.values())
    assert not any(f.adjudicated for f in plain.values())
    print("adjudication:", rep, [(g, len(plain[g].moves), len(adj[g].moves), adj[g].terminal) for g in ids])
    return rep


def check_both_flags(backend, slots=4):
    """tb_search and tb_adjudicate together: the run ends without status flags, every recorded position follows from the oracle's
    legal moves, every terminal code is one the host knows."""
    ts = table_set(backend)
    fens = [KRK_WHITE, KRK_BLACK, KQK_WEAK, "8/8/8/4k3/8/8/8/K6Q w - - 0 1", KRKN, "8/8/8/4k3/8/8/8/K6R w - - 90 70"]
    fins, counters = play_rollout(backend, fens, slots=slots, tablebases=ts, tb_search=True, tb_adjudicate=True, max_game_moves=10)
    assert sorted(fins) == list(range(len(fens)))
    for g, f in fins.items():
        assert f.terminal in (0, 1, 2, 3)
        b = O.Board(fens[g])
        assert len(f.positions) == len(f.moves) + 1
        for i, m in enumerate(f.moves):
            assert bytes(f.positions[i])[:64] == bytes(EC.to_bo_position(b.pos))[:64], (g, i)
            legal = {(x.from_sq, x.to_sq, x.promo) for x in b.legal_moves()}
            assert (m & 63, (m >> 6) & 63, (m >> 12) & 7) in legal, (g, i, E.move_to_uci(m))
            b.push(E.move_to_uci(m))
        assert bytes(f.positions[-1])[:64] == bytes(EC.to_bo_position(b.pos))[:64]
    print("both flags:", counters, [(g, len(f.moves), f.terminal, f.adjudicated) for g, f in sorted(fins.items())])
    assert counters["adjudicated"] >= 1
    return counters


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
class _raises:
    def __init__(self, exc, match):
        self.exc, self.match = exc, match

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        assert et is not None and issubclass(et, self.exc), f"expected {self.exc.__name__}, got {et}"
        assert self.match in str(ev), (self.match, str(ev))
        return True


def check_refusals(backend):
    import torch

    from betaone_amd.rollout import Rollout
    from fake_model import FakeNet

    ts = table_set(backend)
    tabs = tables_of(ts, ("KQK", "KRK"))
    dev = TC.DEVICE[backend]
    with TC.backend_ctx(backend):
        eng = E.Engine(2, num_simulations=16, mcts_batch_size=8)
        with _raises(ValueError, "unknown flag bits"):
            eng.tablebases(tabs, 4)
        with _raises(ValueError, "at most 64"):
            eng.tablebases([tabs[0]] * 65, SEARCH)
        eng.tablebases([tabs[0]] * 64, SEARCH)  # 64 are taken
        eng.tablebases([], 0)
        part = TB.Table("KRK", [], dev)
        assert part.build(max_passes=0) == 0
        with _raises(E.EngineError, "KRK is not complete"):
            eng.tablebases([part], SEARCH)
        part.close()
        lib = E.load_hip_library()
        assert lib.bo_engine_tablebases(eng.h, None, 1, 1) == -1 and lib.bo_engine_tablebases(None, None, 0, 0) == -1
        eng.close()
        fast = E.Engine(2, num_simulations=16, mcts_batch_size=8, fast=True, leaves_per_step=4)
        with _raises(ValueError, "reference-semantics engines only"):
            fast.tablebases(tabs, SEARCH)
        fast.close()
        kw = dict(num_simulations=16, mcts_batch_size=8, device=dev, use_graph=False)
        for flags in (dict(tb_search=True), dict(tb_adjudicate=True)):
            with _raises(ValueError, "need tablebases"):
                Rollout(FakeNet(), 2, **kw, **flags)
        with _raises(ValueError, "fast=False"):
            Rollout(FakeNet(), 2, fast=True, tablebases=ts, tb_search=True, **kw)

        class Elsewhere:
            dev, tables = torch.device("cuda", 7), {}

        with _raises(ValueError, "live on cuda:7"):
            Rollout(FakeNet(), 2, tablebases=Elsewhere(), tb_adjudicate=True, **kw)


def check_command_line_refusals(tmp_path):
    from betaone_amd import match, selfplay_main

    for argv in (["--iteration", "0", "--tb-search"], ["--iteration", "0", "--tb-adjudicate"],
                 ["--iteration", "0", "--tablebases", str(tmp_path)], ["--iteration", "0", "--tablebases", str(tmp_path / "missing"), "--tb-search"]):
        try:
            selfplay_main.main(argv)
        except SystemExit as ex:
            assert ex.code == 2, argv
        else:
            raise AssertionError(f"selfplay_main accepted {argv}")
    for argv in (["a.pth", "b.pth", "--tb-adjudicate"], ["a.pth", "b.pth", "--tablebases", str(tmp_path)]):
        try:
            match.main(argv)
        except SystemExit as ex:
            assert ex.code == 2, argv
        else:
            raise AssertionError(f"match accepted {argv}")


# ---- 6. match ------------------------------------------------------------------------------------------------------------------------------
def check_match_scores_an_adjudicated_game(backend):
    """A game the tables ended (terminal 3, adjudicated) is a loss for the side to move in W/D/L and in the PGN, whose tags name the
    termination."""
    from betaone_amd import match as M
    from test_match_cpu import StandInRollout

    class Fin(TC.Fin):
        def __init__(self, gid, slot):
            super().__init__(gid, TC.KRK_START, ["c3c2", "h1h8"], 3)  # black, to move in KRK, is lost
            self.slot, self.adjudicated = slot, True

    class Adjudicating(StandInRollout):
        def play_ply(self, on_finished=None, refill=None):
            return super().play_ply(on_finished=lambda f: on_finished(Fin(self.slot[f.slot][0], f.slot)), refill=refill)

    sched = M.MatchScheduler([(TC.KRK_START, "")], 2, 2, 1)
    ro = Adjudicating(sched, 2, 1, {0: 2, 1: 2})
    fins = {}
    played = M.play_match(ro, sched, step_of=lambda s: ro.step[s // ro.Gc] + 1, finished=fins)
    games = played["games"]
    assert [g["termination"] for g in games] == ["adjudication"] * 2
    assert {g["white"] for g in games} == {"A", "B"}
    for g in games:  # white wins both: B scores 1 with white, 0 with black
        assert g["result_b"] == (1.0 if g["white"] == "B" else 0.0)
    st = M.summarize(played, with_pairs=True)
    assert (st["wins"], st["draws"], st["losses"]) == (1, 0, 1) and st["score"] == 0.5
    assert M.game_result(type("F", (), dict(terminal=2, adjudicated=True, positions=fins[0].positions))(), 0) == (0.5, "adjudication")
    text = io.StringIO()
    with TC.backend_ctx(backend):
        M.write_match_pgn(text, played, fins, "a.pth", "b.pth", device=TC.DEVICE[backend], date="2026.01.02")
    text = text.getvalue()
    assert text.count('[Termination "adjudication"]') == 2 and text.count('[Result "1-0"]') == 2 and "resigns" not in text
    assert text.count("1-0") == 4  # (the tag and the movetext's result token)
