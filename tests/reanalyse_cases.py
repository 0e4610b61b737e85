"""tests/reanalyse_cases.py -- TEST HELPER: bodies shared by tests/test_reanalyse_emu.py (wave emulator) and tests/test_reanalyse_gpu.py
(MI355X) for the reanalysis path (csrc/bo_reanalyse.h, betaone_amd/reanalyse.py): ring entries made from bo_position against the PGN
replay's, the reanalysis record against bo_search_result, and its old-against-new figures against a NumPy float64 restatement."""
from __future__ import annotations

import numpy as np

import analyse_cases as AC
import engine_harness as H
from betaone_amd import engine as E

SENTINEL_I, SENTINEL_F = -77, np.float32(-3.5)


def _lib_dev(backend):
    import torch

    return (H.emu_lib() if backend == "emu" else E.load_hip_library()), torch.device("cpu" if backend == "emu" else "cuda:0")


def ingest(backend, text):
    from betaone_amd import analyse as A

    lib, dev = _lib_dev(backend)
    ing = A.Ingested(lib, dev, "corpus", text.encode())
    ing.finish(lib, dev)
    return ing


def records_ring(backend, positions, n):
    """bo_records_ring on the first n of `positions` (a ctypes array of bo_position) -> uint8 [n + 1, 80]; the last row is a guard."""
    lib, _ = _lib_dev(backend)
    src = AC.IntBuf(backend, np.frombuffer(bytes(positions), np.uint8))
    out = AC.IntBuf(backend, np.full((n + 1) * 80, 0xAB, np.uint8))
    assert lib.bo_records_ring(src.ptr, n, out.ptr, 0) == 0, lib.bo_last_error()
    return out.numpy().reshape(n + 1, 80).copy()


def check_ring_bytes(backend):
    """(1) every ply of every game of the corpus: the entries made from bo_position equal the PGN replay's, byte for byte."""
    from betaone_amd import analyse as A

    games, text = AC.make_corpus()
    assert any(f and " w KQkq c6 " in f for f, _ in games) and max(len(m) for _, m in games) > 64 and min(len(m) for _, m in games) == 0
    assert any(m == AC.REPETITION for _, m in games)
    ing = ingest(backend, text)
    assert set(ing.status.tolist()) == {0} and ing.n_plies.tolist() == [len(m) for _, m in games]
    ring = ing.pos.cpu().numpy().reshape(-1, 80)
    T = len(ring)
    assert T % 64 != 0
    pos = A.ring_to_positions(ring)
    full = records_ring(backend, pos, T)
    assert (full[T] == 0xAB).all()                                   # nothing is written behind the last entry
    irrev = 0
    for g in range(ing.n_games):
        o, k = int(ing.tok_off[g]), int(ing.n_plies[g])
        assert np.array_equal(full[o:o + k], ring[o:o + k]), g
        irrev += int(((ring[o:o + k].reshape(-1).view(A.DPOS_DTYPE)["flags"] & 0x8000) != 0).sum())
    assert irrev > 100                                               # the bit a bo_position does not carry was recovered, not absent
    for n in (0, 1, 63, 65):                                         # n == 0; n no multiple of 64; the prefix is the same entries
        part = records_ring(backend, pos, n)
        assert np.array_equal(part[:n], full[:n]) and (part[n] == 0xAB).all()
    return T


class Searched:
    """G slots set up from the device ring of a small corpus and searched: the roots of the work list `ids` (None: refused slot)."""

    def __init__(self, backend, fns_of, widen_coeff=1.5, sims=24, batch=8, G=8):
        games, text = AC.make_corpus(seed=11, n_random=2, max_plies=12, long_plies=66)
        self.backend, self.G, self.sims = backend, G, sims
        ing = self.ing = ingest(backend, text)
        rep_g = next(i for i, (_, m) in enumerate(games) if m == AC.REPETITION)
        start = np.cumsum(ing.n_plies) - ing.n_plies
        # six ordinary roots, a root where a draw can be claimed (code 2: not searched), a refused slot
        ids = [int(start[rep_g]) + 8]                                 # the position has occurred three times: claimable
        ids += [i for i in range(ing.n_roots) if ing.w_game[i] != rep_g][:G - 2]
        self.ids = ids + [None]
        self.eng = H.make_engine(backend, G, dict(num_simulations=sims, batch_size=batch, dirichlet_alpha=0.0, widen_coeff=widen_coeff),
                                 max_plies=int(ing.n_plies.max()) + 2)
        self.eng.root_values(True)
        first = AC.IntBuf(backend, np.array([ing.tok_off[ing.w_game[i]] if i is not None else 0 for i in self.ids], np.int64))
        ply = AC.IntBuf(backend, np.array([ing.w_ply[i] if i is not None else -1 for i in self.ids], np.int32))
        slots = AC.IntBuf(backend, np.arange(G, dtype=np.int32))
        self.eng.reset_dev(G, slots.ptr, ing.pos.data_ptr(), ing.T, first.ptr, ply.ptr)
        want = AC.IntBuf(backend, np.ones(G, np.int32))
        bufs = (H.Buf(backend, (G, 120, 8, 8)), H.Buf(backend, (G, E.NUM_ACTIONS)), H.Buf(backend, (G,)))
        _, self.res = AC.run_searches(backend, self.eng, *bufs, [fns_of(g) for g in range(G)], lambda: self.eng.search_begin_dev(want.ptr, bufs[0].ptr))
        self.root_value = self.eng.search_root_value()
        _, self.term, _ = self.eng.root_info()
        self.played_action = np.array([int(ing.act.cpu().numpy()[ing.tok_off[ing.w_game[i]] + ing.w_ply[i]]) if i is not None else -1 for i in self.ids], np.int32)

    def record(self, W, played=None, root=None, old_ptr=None, old_idx=None, old_val=None):
        """bo_reanalysis_result -> (records [G], pi_idx [G, W], pi_val [G, W]); the rows start out as sentinels."""
        G, be = self.G, self.backend
        out = AC.IntBuf(be, np.zeros((G, 16), np.int32))
        pi = AC.IntBuf(be, np.full((G, W), SENTINEL_I, np.int32))
        pv = AC.IntBuf(be, np.full((G, W), SENTINEL_F, np.float32).view(np.int32))
        pl = AC.IntBuf(be, np.asarray(played, np.int32)) if played is not None else None
        old = [AC.IntBuf(be, a) for a in (np.asarray(root, np.int64), np.asarray(old_ptr, np.int32), np.asarray(old_idx, np.int32),
                                          np.asarray(old_val, np.float32).view(np.int32))] if root is not None else [None] * 4
        self.eng.reanalysis_result(pl.ptr if pl else 0, *[(b.ptr if b else 0) for b in old], W, out.ptr, pi.ptr, pv.ptr)
        return out.numpy().copy().view(E.REANALYSIS_DTYPE).reshape(G), pi.numpy().copy().reshape(G, W), pv.numpy().copy().view(np.float32).reshape(G, W)


def check_record_against_search_result(backend, widen_coeff, flat):
    """(2) pi rows, pi_n, best_idx, total_visits and root_value against bo_search_result / bo_search_root_value for W = 8, 1 and
    BO_RES_CAP; the overflow bit; a root that is over and a refused slot keep phase 0 and their rows.  -> (the largest pi_n, the two-entry
    rows seen with W = 1)."""
    s = Searched(backend, (lambda g: AC.flat_eval) if flat else (lambda g: AC.softmax_eval(300 + g)), widen_coeff=widen_coeff)
    G, res = s.G, s.res
    assert int(s.term[0]) == 2 and int(s.term[G - 1]) == -1 and (s.term[1:G - 1] == 0).all()
    two = 0
    for W in (8, 1, E.RES_CAP):
        rec, pi, pv = s.record(W, played=s.played_action)
        for g in range(G):
            r = rec[g]
            assert int(r["terminal"]) == int(s.term[g]) and int(r["watch"]) == 0
            if g in (0, G - 1):
                assert int(r["phase"]) == E.PH_IDLE and int(r["pi_n"]) == 0 and int(r["best_idx"]) == -1 and int(r["total_visits"]) == 0
                assert (pi[g] == SENTINEL_I).all() and (pv[g] == SENTINEL_F).all()          # untouched
                assert int(r["status"]) == (0 if g == 0 else 128)
                continue
            n = int(res["n"][g])
            k = min(n, W)
            assert int(r["phase"]) == E.PH_DONE and int(r["sims_done"]) == s.sims and int(r["ply"]) == int(s.ing.w_ply[s.ids[g]])
            assert int(r["pi_n"]) == n and int(r["best_idx"]) == int(res["best_idx"][g]) and int(r["total_visits"]) == int(res["total"][g])
            assert r["root_value"].view(np.uint32) == s.root_value[g:g + 1].view(np.uint32)[0]
            assert np.array_equal(pi[g, :k], res["idx"][g, :k]) and np.array_equal(pv[g, :k].view(np.uint32), res["val"][g, :k].view(np.uint32))
            assert (pi[g, k:] == -1).all() and (pv[g, k:].view(np.uint32) == 0).all()
            assert int(r["status"]) == (E.ST_PI_OVERFLOW if n > W else 0)
            assert int(r["has_old"]) == 0 and int(r["agree"]) == 0 and r["tv"].view(np.uint32) == 0
            hit = np.nonzero(res["idx"][g, :n] == s.played_action[g])[0]
            want = res["val"][g, hit[0]] if len(hit) else np.float32(0)
            assert r["played_prob"].view(np.uint32) == np.float32(want).view(np.uint32)
            if W == 1 and n == 2:
                two += 1
                assert int(r["status"]) & E.ST_PI_OVERFLOW and pi[g, 0] == res["idx"][g, 0]
    assert s.eng.status_bits().tolist()[:G - 1] == [0] * (G - 1)      # the overflow bit is the record's, not the slot's
    return int(res["n"][1:G - 1].max()), two


def restate(new_idx, new_val, old_idx, old_val, played):
    """(tv, agree, played_prob) of include/betaone_engine.h (bo_reanalysis) in NumPy: float64, in the order the header gives."""
    new_idx, old_idx = [int(a) for a in new_idx], [int(a) for a in old_idx]
    acc = np.float64(0.0)
    for a, v in zip(new_idx, new_val):
        o = np.float32(0.0)
        for oa, ov in zip(old_idx, old_val):
            if oa == a:
                o = ov
                break
        acc = acc + np.abs(np.float64(v) - np.float64(o))
    for oa, ov in zip(old_idx, old_val):
        if oa not in new_idx:
            acc = acc + np.float64(ov)
    first_max = lambda idx, val: idx[int(np.argmax(np.asarray(val, np.float32)))] if len(idx) else -1   # (np.argmax: the first maximum)
    agree = int(len(old_idx) > 0 and first_max(old_idx, old_val) == first_max(new_idx, new_val))
    pp = next((np.float32(v) for a, v in zip(new_idx, new_val) if a == played), np.float32(0.0))
    return np.float32(np.float64(0.5) * acc), agree, pp


def check_old_against_new(backend):
    """(3) tv, agree and played_prob bit for bit against restate(), per slot one kind of old pi."""
    # 32 simulations in batches of 8: every visit share is a multiple of 1/4, so sums of them are exact; wide roots: rows of 1 to 3 entries
    s = Searched(backend, lambda g: AC.softmax_eval(300 + g), widen_coeff=6.0, sims=32)
    G, res = s.G, s.res
    new = {g: (res["idx"][g, :int(res["n"][g])].copy(), res["val"][g, :int(res["n"][g])].copy()) for g in range(1, G - 1)}
    assert max(len(new[g][0]) for g in new) > 2 and min(len(new[g][0]) for g in new) >= 1
    f = np.float32
    free = lambda g: [a for a in range(E.NUM_ACTIONS) if a not in new[g][0]][:3]
    top6 = new[6][0][int(np.argmax(new[6][1]))]
    old = {
        1: (new[1][0], new[1][1]),                                                   # equal to the new one: tv == 0 exactly
        2: (np.array(free(2)[:2], np.int32), np.array([0.75, 0.25], f)),             # disjoint support: tv == 1
        3: (np.array([free(3)[0], new[3][0][-1]], np.int32), np.array([0.625, 0.375], f)),  # one shared entry
        4: (np.zeros(0, np.int32), np.zeros(0, f)),                                  # empty
        5: (new[5][0], new[5][1]),                                                   # root_dev = -1 below: no old pi
        6: (np.array([free(6)[0], top6, free(6)[1]], np.int32), np.array([0.25, 0.375, 0.375], f)),   # tied maxima: the first wins
    }
    ptr, idx, val, root = [0], [], [], np.full(G, -1, np.int64)
    for g in sorted(old):
        idx += list(old[g][0]); val += list(old[g][1]); ptr.append(len(idx))
        root[g] = len(ptr) - 2
    root[5] = -1
    played = s.played_action.copy()
    played[2] = new[2][0][-1]                                                        # a move the new pi has
    played[3] = free(3)[2]                                                           # and one it does not have
    rec, _, _ = s.record(8, played=played, root=root, old_ptr=ptr, old_idx=idx or [0], old_val=val or [0.0])
    for g in range(1, G - 1):
        r = rec[g]
        has = root[g] >= 0
        assert int(r["has_old"]) == int(has)
        tv, agree, pp = restate(*new[g], *(old[g] if has else (np.zeros(0, np.int32), np.zeros(0, f))), int(played[g]))
        assert r["played_prob"].view(np.uint32) == pp.view(np.uint32)
        if not has:
            assert r["tv"].view(np.uint32) == 0 and int(r["agree"]) == 0
            continue
        assert r["tv"].view(np.uint32) == tv.view(np.uint32) and int(r["agree"]) == agree, g
    assert rec["tv"][1] == 0.0 and rec["agree"][1] == 1
    assert float(new[2][1].astype(np.float64).sum()) == 1.0 and rec["tv"][2] == 1.0 and rec["agree"][2] == 0
    assert 0.0 < rec["tv"][3] < 1.0
    assert rec["tv"][4] == 0.5 and rec["agree"][4] == 0                               # an empty old pi: half of the new one's mass
    assert rec["agree"][6] == 1                                                      # old's first maximum is its entry 1, not 2
    assert rec["played_prob"][2] == new[2][1][-1] and rec["played_prob"][3] == 0.0
    assert rec["phase"][0] == 0 and rec["has_old"][0] == 0 and rec["phase"][G - 1] == 0
    # what the host can know it refuses itself
    a = AC.IntBuf(backend, np.zeros(64 * 16, np.int32))
    lib = s.eng.lib
    assert lib.bo_reanalysis_result(s.eng.h, None, None, None, None, None, 0, a.ptr, a.ptr, a.ptr, 0) == -1
    assert lib.bo_reanalysis_result(s.eng.h, None, None, None, None, None, E.RES_CAP + 1, a.ptr, a.ptr, a.ptr, 0) == -1
    assert lib.bo_reanalysis_result(s.eng.h, None, a.ptr, None, None, None, 8, a.ptr, a.ptr, a.ptr, 0) == -1     # the old pi comes whole
    assert lib.bo_reanalysis_result(s.eng.h, None, None, None, None, None, 8, None, a.ptr, a.ptr, 0) == -1
    return rec


# ---- files ------------------------------------------------------------------------------------------------------------------------
def bog_files(d):
    import glob
    import os

    return sorted(glob.glob(os.path.join(str(d), "*.bog")))


def games_of(d):
    from betaone_amd import records as R

    return [g for p in bog_files(d) for g in R.load_games(p)]


def same_but_targets(a, b):
    """Two lists of load_games dicts: everything but pi and the root values is equal."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("game_id", "n_plies", "terminal", "outcome", "resign", "resign_check"):
            assert x[k] == y[k], k
        assert bytes(x["positions"]) == bytes(y["positions"]) and np.array_equal(x["moves"], y["moves"])
        assert (x["root_values"] is None) == (y["root_values"] is None)


def first_max_move(backend, game, ply):
    """The action index of the first maximum of game's pi at `ply` (stored order)."""
    idx, val = game["pis"][ply]
    return int(idx[int(np.argmax(val))])
