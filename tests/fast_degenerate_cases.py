"""tests/fast_degenerate_cases.py -- backend-independent bodies of the tests of the FAST search mode (csrc/bo_fastw.h) on the rows a
trained net produces (emu on CPU, hip on GPU).

The smooth hash evaluator of tests/test_fast_mode_emu.py never makes two children score the same, never gives a prior of 0, keeps every
count inside the kernel's reciprocal and square-root tables and every path short.  The evaluators here (fake_model: a policy family
combined with a value family) reach what it leaves out:
  ties             uniform and exact-zero priors: "first maximum in child order" decides, in each of the kernel's four comparisons
  uniform priors   no legal move holds mass: bo_k_fw_apply's 1 / n branch
  counts           n_eff > 254 (BO_FW_RCP_TAB) and parent visits >= 4096 (BO_FW_SQRT_TAB): the exact-operation side paths
  in-flight counts 15 descents of a step through one record (the 4-bit packed counters), more than 15 at L = 64
  the path cap     a descent 64 nodes deep: a draw, BO_ST_DEPTH_OVERFLOW (include/betaone_engine.h)
Every comparison is bit for bit against tests/fast_reference.py through its canonical form.  A restatement is computed once per
(position, evaluator, simulations, L, noise) and shared by every kernel variant with that L; each case asserts on the restatement's
own counters that it still reaches the path it is there for."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import test_fast_mode_emu as FM
from betaone_amd import engine as E
from engine_harness import emu_call
from fake_model import family_eval
from fast_reference import EXPANDED, canonical_from_engine
from oracle import oracle as O

START = O.STARTING_FEN
KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
KRK = "8/8/4k3/8/8/3K4/8/6R1 w - - 0 1"
WIDE = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"  # 218 legal moves: the wide-run tail, several passes per lane
FENS = dict(start=START, kiwipete=KIWIPETE, krk=KRK, wide=WIDE)
SALT, MULTI_SALT, MULTI_SEED, ALPHA = 31, 13, 5, 0.1

# Every lane grouping of bo_k_fw_select at L = 4: half a wave per game with 2 and 4 games per half-wave, one lane, eight lanes, four lanes
# per game, each plain and with its flags.  Running one case on all of them also asserts that they build the same tree.
HALF, LANE, OCT, QUAD = dict(games_per_halfwave=2, select_flags=0), dict(select_flags=8), dict(select_flags=16), dict(select_flags=32)
L4_VARIANTS = [dict(games_per_halfwave=u, select_flags=f) for u in (2, 4) for f in (0, 3)] + [dict(select_flags=f) for f in (8, 9, 16, 18, 32, 34)]
VARIANTS = {4: L4_VARIANTS,
            8: [dict(select_flags=f) for f in (0, 3, 16, 18, 32)],  # u4l8, o8l8, q4l8
            16: [dict(select_flags=f) for f in (0, 3)],              # u2l16
            64: [dict(select_flags=f) for f in (0, 3)]}              # u1l64: in-flight descents counted one by one


def vid(opts):
    return "-".join(f"{k[0]}{v}" for k, v in sorted(opts.items())) or "default"


def evaluator(policy, value=None, peak_scale=400.0, salt=SALT):
    return family_eval(policy, salt, value=value, peak_scale=peak_scale)


def noise_for(fen, moves, seed):
    b = O.Board(fen)
    for u in moves:
        b.push(u)
    nl = len(list(b.legal_moves()))
    noise = np.zeros((1, E.MAX_LEGAL))
    noise[0, :nl] = np.random.RandomState(seed).dirichlet([ALPHA] * nl)
    return noise


def _record(ref):
    zeros, denormals = ref.prior_counts()
    return SimpleNamespace(canon=ref.canonical(), visits=ref.visits(), n_evals=ref.n_evals, n_term_sims=ref.n_term_sims,
                           stats=dict(ref.stats), zeros=zeros, denormals=denormals, overflows=ref.n_depth_overflows,
                           depth_overflow=ref.depth_overflow, granules=ref.granules_needed(), n_nodes=len(ref.nodes()))


@functools.lru_cache(maxsize=None)
def reference(pos, moves, policy, value, peak_scale, salt, sims, L, noise_seed):
    """One search of the restatement: computed once, shared by every kernel variant with this L, never modified.
    noise_seed None: no Dirichlet noise."""
    fen = FENS.get(pos, pos)
    ref = FM.reference_for(fen, list(moves), evaluator(policy, value, peak_scale, salt), sims, L, use_noise=noise_seed is not None)
    ref.search(None if noise_seed is None else noise_for(fen, moves, noise_seed)[0])
    return _record(ref)


def make_fast_engine(backend, G, sims, L, opts, noise_on, arena=0):
    kw = dict(num_simulations=sims, dirichlet_alpha=ALPHA if noise_on else 0.0, fast=True, leaves_per_step=L, max_plies=256,
              fast_arena_granules=arena)
    eng = emu_call(E.Engine, G, **kw) if backend == "emu" else E.Engine(G, **kw)
    eng.fast_options(**opts)
    return eng


def run_single(backend, pos, policy, value, peak_scale, sims, L, opts, noise_seed=None, arena=0, check=True, salt=SALT):
    fen = FENS.get(pos, pos)
    eng = make_fast_engine(backend, 1, sims, L, opts, noise_seed is not None, arena)
    eng.reset([0], [fen], [None])
    noise = None if noise_seed is None else noise_for(fen, (), noise_seed)
    FM.drive_search(backend, eng, 1, L, evaluator(policy, value, peak_scale, salt), noise, check=check)
    return eng


def compare(eng, g, ref, what):
    """The engine's tree of slot g, its counters and its result against one restatement record."""
    got = canonical_from_engine(eng.debug_tree(g), E.move_to_uci)
    if got != ref.canon:
        diff = sorted(k for k in set(got) | set(ref.canon) if got.get(k) != ref.canon.get(k))
        raise AssertionError((what, len(diff), "paths differ; first:", diff[0], got.get(diff[0]), ref.canon.get(diff[0])))
    st, res = eng.status(), eng.result()
    assert int(st["evals"][g]) == ref.n_evals and int(st["term_sims"][g]) == ref.n_term_sims, what
    visits = [v for _m, v in ref.visits]
    n = int(res["n"][g])
    assert n == sum(v > 0 for v in visits) and int(res["total"][g]) == sum(visits), what
    assert E.move_to_uci(int(res["best_move"][g])) == ref.visits[int(np.argmax(visits))][0], what  # first maximum in legal-move order
    assert abs(float(res["val"][g, :n].sum()) - 1.0) < 1e-6, what


# ---- ties and uniform priors ---------------------------------------------------------------------------------------------------------
TIE_POLICIES = ["illegal_mass", "peak"]
TIE_SALT = dict(start=SALT, wide=39)  # (with most salts the peaked move of the 218-move position mates at once and the tree stays one level deep)
TIE_SINGLE = [("start", 4, 96), ("start", 8, 104), ("start", 16, 128), ("wide", 4, 96), ("wide", 8, 104), ("wide", 16, 112)]  # (position, L, sims)
TIE_SINGLE_CASES = [(pol, pos, L, sims, o) for pol in TIE_POLICIES for pos, L, sims in TIE_SINGLE for o in VARIANTS[L]]
TIE_SINGLE_IDS = [f"{pol}-{pos}-L{L}-{vid(o)}" for pol, pos, L, sims, o in TIE_SINGLE_CASES]
TIE_MULTI = [(4, 96), (8, 104), (16, 130)]  # (L, sims)
TIE_MULTI_CASES = [(pol, L, sims, o) for pol in TIE_POLICIES for L, sims in TIE_MULTI for o in VARIANTS[L]]
TIE_MULTI_IDS = [f"{pol}-L{L}-{vid(o)}" for pol, L, sims, o in TIE_MULTI_CASES]


def assert_tie_preconditions(policy, refs, what):
    levels, ties = sum(r.stats["levels"] for r in refs), sum(r.stats["tie_levels"] for r in refs)
    zeros = sum(r.zeros for r in refs)
    print(f"{what}: {ties} of {levels} levels tied, {zeros} zero and {sum(r.denormals for r in refs)} denormal priors")
    if policy == "illegal_mass":  # every legal prior is 0 before the renormalisation: uniform priors, so unvisited siblings tie
        assert 4 * ties >= levels > 0, (what, ties, levels)
    else:
        assert ties >= 5 and zeros >= 1000, (what, ties, zeros)


def tie_single_reference(policy, pos, L, sims):
    ref = reference(pos, (), policy, None, 400.0, TIE_SALT[pos], sims, L, None)
    assert_tie_preconditions(policy, [ref], (policy, pos, L))
    return ref


def check_tie_single(backend, policy, pos, L, sims, opts):
    ref = tie_single_reference(policy, pos, L, sims)
    eng = run_single(backend, pos, policy, None, 400.0, sims, L, opts, salt=TIE_SALT[pos])
    compare(eng, 0, ref, (policy, pos, L, opts))
    assert not eng.status_bits().any()
    eng.close()


def tie_multi_references(policy, L, sims):
    refs = [reference(fen, tuple(moves), policy, None, 400.0, MULTI_SALT, sims, L, MULTI_SEED + g) for g, (fen, moves) in enumerate(FM.MULTI)]
    assert_tie_preconditions(policy, refs, (policy, "every slot", L))
    return refs


def check_tie_multi(backend, policy, L, sims, opts):
    """A different position in every slot (the games interleaved per group of lanes diverge in depth, run length and end of descent)."""
    refs = tie_multi_references(policy, L, sims)
    eng, _noise, _fn = FM.run_multi(backend, L, sims, opts, seed=MULTI_SEED, eval_fn=evaluator(policy, salt=MULTI_SALT))
    for g, ref in enumerate(refs):
        compare(eng, g, ref, (policy, g, L, opts))
    assert not eng.status_bits().any()
    eng.close()


# ---- a case checkable by hand --------------------------------------------------------------------------------------------------------
BY_HAND = [(2, dict()), (8, dict())] + [(4, o) for o in L4_VARIANTS]
BY_HAND_IDS = [f"L{L}-{vid(o)}" for L, o in BY_HAND]


def check_by_hand(backend, L, opts):
    """Uniform priors 1/20, every value +-0, no noise, ten simulations from the start position.  A root child with n_eff = 0 scores
    cpuct * (1/20) * sqrt(N); one with n_eff = 1 (visited, or a descent of this step in flight through it) scores at most half of that:
    q is -1 under a virtual loss and +-0 after the backup.  So the first maximum in child order is the first unvisited child, ten
    times: children 0..9 in move order hold one visit each, children 10..19 none.  Asserted on the engine alone."""
    eng = run_single(backend, "start", "illegal_mass", "v_zero", 400.0, 10, L, opts)
    t = eng.debug_tree(0)
    root = t[0]
    kids = t[root["first_child"]:root["first_child"] + root["n_children"]]
    moves = [O.move_to_uci(m) for m in O.Board(START).legal_moves()]
    assert [E.move_to_uci(k["move"]) for k in kids] == moves and len(moves) == 20
    assert [k["n"] for k in kids] == [1] * 10 + [0] * 10, [k["n"] for k in kids]
    assert all(np.float32(k["prior"]) == np.float32(np.float32(1.0) / np.float32(20.0)) for k in kids)
    assert all(float(k["q"]) == 0.0 for k in kids) and root["n"] == 11
    assert all(k["n_children"] == 20 for k in kids[:10]) and all(k["n_children"] == 0 for k in kids[10:])
    assert len(t) == 1 + 20 + 10 * 20 and not eng.status_bits().any()
    eng.close()


# ---- counts beyond the reciprocal table ------------------------------------------------------------------------------------------------
# 300 simulations pass the table (n_eff up to 292) but only at children that win either way: with values of 0 a child's q is 0 whatever
# reciprocal multiplies it, and its u only shrinks.  A kernel that used the table's last entries there would build the same tree.  At
# 420 simulations it would not: the restatement counts the levels at which the clamped entries choose another child.
RCP_POS, RCP_POLICY, RCP_VALUE, RCP_L = "kiwipete", "peak", "v_zero", 4
RCP_SIMS = [300, 420]
RCP_CASES = [(sims, o) for sims in RCP_SIMS for o in L4_VARIANTS]
RCP_CASES_EMU = [(300, o) for o in L4_VARIANTS] + [(420, o) for o in (HALF, LANE, OCT, QUAD)]


def rcp_ids(cases):
    return [f"sims{sims}-{vid(o)}" for sims, o in cases]


def rcp_reference(sims):
    ref = reference(RCP_POS, (), RCP_POLICY, RCP_VALUE, 400.0, SALT, sims, RCP_L, None)
    print("reciprocal table:", sims, ref.stats)
    assert ref.stats["max_n_eff"] >= 256, ref.stats  # past BO_FW_RCP_TAB: rcp(n_eff) and rcp(1 + n_eff) both come from the side path
    if sims > 300:
        assert ref.stats["rcp_clamp_flips"] > 0, ref.stats
    return ref


def check_rcp_table(backend, sims, opts):
    ref = rcp_reference(sims)
    eng = run_single(backend, RCP_POS, RCP_POLICY, RCP_VALUE, 400.0, sims, RCP_L, opts)
    compare(eng, 0, ref, ("rcp", sims, opts))
    assert not eng.status_bits().any()
    eng.close()


# ---- packed in-flight counts -----------------------------------------------------------------------------------------------------------
PACKED = [("start", 300, 16), ("kiwipete", 400, 64)]
PACKED_CASES = [(pos, sims, L, o) for pos, sims, L in PACKED for o in VARIANTS[L]]
PACKED_IDS = [f"{pos}-L{L}-{vid(o)}" for pos, sims, L, o in PACKED_CASES]


def packed_reference(pos, sims, L):
    """Every leaf's value is -1: whoever moved into it sees +1, and the descents of a step pile up on one line."""
    ref = reference(pos, (), "peak", "v_m1", 400.0, SALT, sims, L, None)
    print("in-flight counts:", pos, L, ref.stats)
    if L == 16:
        assert ref.stats["max_sharing"] == 15, ref.stats  # all sixteen descents of a step through one record: 4 bits, all set
    else:
        assert ref.stats["max_sharing"] > 15, ref.stats
    return ref


def check_packed_counts(backend, pos, sims, L, opts):
    ref = packed_reference(pos, sims, L)
    eng = run_single(backend, pos, "peak", "v_m1", 400.0, sims, L, opts)
    compare(eng, 0, ref, ("packed", pos, L, opts))
    assert not eng.status_bits().any()
    eng.close()


# ---- parent visits beyond the square-root table ------------------------------------------------------------------------------------------
SQRT_SIMS, SQRT_SEED = 4300, 17
SQRT_CASES = [(4, o) for o in L4_VARIANTS] + [(64, dict(select_flags=0))]
SQRT_IDS = [f"L{L}-{vid(o)}" for L, o in SQRT_CASES]
SQRT_CASES_EMU = [(4, LANE), (4, OCT)]  # both kernel bodies; the emulator takes a minute for one such search (profiles/fast_degenerate_rows.md)
SQRT_IDS_EMU = [f"L{L}-{vid(o)}" for L, o in SQRT_CASES_EMU]


def sqrt_reference(L):
    ref = reference("krk", (), "peak", "v_pm1", 400.0, SALT, SQRT_SIMS, L, SQRT_SEED)
    print("square-root table:", L, ref.stats, ref.n_nodes, "nodes", ref.granules, "granules")
    assert ref.stats["max_parent_visits"] >= 4096 and ref.stats["max_n_eff"] >= 256, ref.stats
    return ref


def check_sqrt_table(backend, L, opts):
    """The arena is sized from the restatement's tree: exactly what the runs of its expanded nodes take, and a few granules to spare."""
    ref = sqrt_reference(L)
    eng = run_single(backend, "krk", "peak", "v_pm1", 400.0, SQRT_SIMS, L, opts, noise_seed=SQRT_SEED, arena=max(64, ref.granules + 8))
    assert not (eng.status_bits()[0] & E.ST_NODE_OVERFLOW)
    compare(eng, 0, ref, ("sqrt", L, opts))
    assert not eng.status_bits().any()
    eng.close()


# ---- the path cap --------------------------------------------------------------------------------------------------------------------------
CAP = ("kiwipete", "peak", "v_zero", 800.0, 620, 4)  # logits 800 apart and values of 0: the search runs down single lines
CAP_VARIANTS = [HALF, LANE, OCT, QUAD]
CAP_VARIANTS_EMU = [HALF, LANE]  # both kernel bodies


def cap_reference():
    pos, pol, val, scale, sims, L = CAP
    ref = reference(pos, (), pol, val, scale, SALT, sims, L, None)
    print("path cap:", ref.stats, ref.overflows, "visits cut short")
    assert ref.overflows > 0 and ref.depth_overflow and ref.stats["max_path"] == 64, (ref.stats, ref.overflows)
    return ref


def check_path_cap(backend, opts):
    pos, pol, val, scale, sims, L = CAP
    ref = cap_reference()
    eng = run_single(backend, pos, pol, val, scale, sims, L, opts, check=False)
    compare(eng, 0, ref, ("cap", opts))  # (the tree, all simulations delivered, pi sums to 1)
    assert int(eng.result()["total"][0]) == sims
    assert eng.status_bits()[0] == E.ST_DEPTH_OVERFLOW == 2
    try:
        eng.check_status()
        raise AssertionError("check_status() did not raise")
    except E.EngineError as err:
        assert "game slot 0" in str(err) and "depth overflow" in str(err), str(err)
    eng.close()


# ---- tree reuse ------------------------------------------------------------------------------------------------------------------------------
REUSE_PLIES, REUSE_SIMS, REUSE_L, REUSE_SEED = 3, 96, 4, 11
REUSE_EVALS = [("peak", "v_zero"), ("illegal_mass", None)]
REUSE_VARIANTS = [dict(), LANE, QUAD, dict(games_per_halfwave=4, select_flags=3)]
REUSE_CASES = [(pol, val, o) for pol, val in REUSE_EVALS for o in REUSE_VARIANTS]
REUSE_IDS = [f"{pol}-{val}-{vid(o)}" for pol, val, o in REUSE_CASES]


@functools.lru_cache(maxsize=None)
def reuse_reference(policy, value):
    """Three searches of one game with the played child's subtree kept; the most visited move (the first of them) is played.  Per ply:
    (noise, record after the search, move played, canonical tree after the re-rooting).  Noise is on: a kept root's priors, zeros
    among them, get it at the next search's begin."""
    ref = FM.reference_for(START, [], evaluator(policy, value), REUSE_SIMS, REUSE_L)
    rng, plies = np.random.RandomState(REUSE_SEED), []
    for _ in range(REUSE_PLIES):
        nl = len(list(ref.board.legal_moves()))
        noise = np.zeros((1, E.MAX_LEGAL))
        noise[0, :nl] = rng.dirichlet([ALPHA] * nl)
        kept_zero = sum(1 for ch in ref.root.children if ch.prior == 0)
        ref.search(noise[0])
        rec = _record(ref)
        visits = [v for _m, v in rec.visits]
        best = rec.visits[int(np.argmax(visits))][0]
        ref.play(best)
        assert ref.root.state == EXPANDED  # the played child's subtree is kept
        plies.append((noise, rec, best, ref.canonical(), kept_zero))
    if policy == "peak":
        assert sum(p[4] for p in plies[1:]) > 0, "no kept root child held a prior of 0 when the noise was added"
    return plies


def check_reuse(backend, policy, value, opts):
    plies = reuse_reference(policy, value)
    eng = make_fast_engine(backend, 1, REUSE_SIMS, REUSE_L, opts, True)
    eng.reset([0], [START], [None])
    bufs, fn = None, evaluator(policy, value)
    for ply, (noise, rec, best, after, _kz) in enumerate(plies):
        _, bufs = FM.drive_search(backend, eng, 1, REUSE_L, fn, noise, bufs)
        compare(eng, 0, rec, ("reuse", ply, opts))
        assert E.move_to_uci(int(eng.result()["best_move"][0])) == best
        eng.play(np.array([-2], dtype=np.int32))  # plays the result's best move; the engine re-roots
        assert canonical_from_engine(eng.debug_tree(0), E.move_to_uci) == after, ("after re-rooting", ply, opts)
    assert not eng.status_bits().any()
    eng.close()
