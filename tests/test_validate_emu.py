"""CPU tests (wave emulator) of held-out validation: the metrics kernels of csrc/bo_metrics.h through tests/metrics_cases.py (the
float64 reference, PyTorch's float32 path inside ONE envelope, every case against the reference, the rows that drop out,
accumulation), the split and the loader's index, and `python -m betaone_amd.train --holdout-fraction` and `python -m
betaone_amd.validate` end to end with a tiny net.  The emulator build has no _Float16: dtype pairs with fp16 are skipped, and exactly
those (bf16 logits take their place at every shape); the GPU runs them (tests/test_validate_gpu.py)."""
import json
import os

import numpy as np
import pytest
import torch

import engine_harness as H
import loss_cases as LC
import metrics_cases as MC
from fake_model import FakeNet

from betaone_amd import records as R

CASES = MC.cases()
DROPOUT = MC.dropout_cases()
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GOLDEN = os.path.join(H.ROOT, "tests", "golden", "validate_counts.json")


def test_the_columns_of_header_binding_and_helper_agree():
    from betaone_amd import engine as E

    rows, acc = MC.header_enums()
    assert rows[-1] == "COLS" and acc[-1] == "COLS"
    assert rows[:-1] == list(MC.ROW_NAMES) == list(E.METRIC_ROW) and [E.METRIC_ROW[n] for n in rows[:-1]] == list(range(MC.ROW_COLS))
    assert acc[:-1] == list(E.METRIC) and [E.METRIC[n] for n in acc[:-1]] == list(range(MC.COLS))
    assert acc[:4] == ["N_ROWS", "N_BAD", "N_POLICY_ROWS", "N_DECISIVE"] and acc[4:-1] == ["SUM_" + n for n in MC.ROW_NAMES[3:]]
    assert E.METRIC_ROW_COLS == MC.ROW_COLS and E.METRIC_COLS == MC.COLS


def test_the_list_has_what_it_promises():
    assert {(c.n, c.W) for c in CASES} == {(n, W) for n in MC.NS for W in MC.WS}
    assert {c.n_buckets for c in CASES} == set(MC.NBS) and any(c.bucket is None for c in CASES) and any(c.q is None for c in CASES)
    for nb in MC.NBS:
        assert {c.n for c in CASES if c.n_buckets == nb} & {65, 130}
    assert {c.pattern[0] for c in CASES if c.n == 1} >= {0, 1, 2, 3}
    hit, top = set(), set()
    for c in CASES:
        ok = LC.valid(c.idx)
        for b in range(c.n):
            row = c.idx[b][ok[b]]
            assert row.unique().numel() == row.numel(), (c.name, b)
        hit |= set(c.idx[ok].unique().tolist()) & set(LC.EDGE_ACTIONS)
        top |= set(c.logits.argmax(1).tolist()) & set(LC.EDGE_ACTIONS)
        if c.bucket is not None and c.n > 2:
            assert int(c.bucket[c.n // 2]) == -1 and int(c.bucket[c.n - 1]) == c.n_buckets
    assert hit == set(LC.EDGE_ACTIONS) and top == set(LC.EDGE_ACTIONS)
    big = next(c for c in CASES if (c.n, c.W) == (130, 65))
    ref = MC.reference64(big.logits, big.value, big.idx, big.val, big.z)
    r = ref.rows
    k = [b for b in range(big.n) if big.pattern[b] == 4 and r[b, MC.ROW["HAS_POLICY"]]]      # all-equal rows: rank == i*
    assert k and all(r[b, MC.ROW["RANK"]] > 5 for b in k[:3])
    both = [b for b in range(big.n) if big.pattern[b] == 3]                                    # ties on both sides of i*
    assert both and all(3 <= r[b, MC.ROW["RANK"]] for b in both)
    assert set(r[:, MC.ROW["TOP1"]]) == {0.0, 1.0} and set(r[:, MC.ROW["ARGMAX_IN_SUPPORT"]]) == {0.0, 1.0}
    empty = [b for b in range(big.n) if big.pattern[b] == 6]
    assert empty and not r[empty][:, [MC.ROW[n] for n in ("HAS_POLICY", "RANK", "CE", "NET_ENTROPY", "P_TOP")]].any() and r[empty, MC.ROW["ABS_V"]].any()
    two = next(c for c in CASES if (c.n, c.W) == (130, 2))                                     # equal pi_val maxima: the lowest action
    tied = [b for b in range(two.n) if two.pattern[b] == 2 and int((two.idx[b] >= 0).sum()) == 2 and float(two.val[b, 0]) == float(two.val[b, 1])]
    assert tied and all(int(two.idx[b, 0]) > int(two.idx[b, 1]) for b in tied)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_torch_float32_inside_one_envelope(case):
    """PyTorch's float32 computation of the float columns on the CPU within ONE envelope of the float64 reference (with the allowance
    for its sum of the exponentials, LC.TORCH_SUM_C) -- for float32 inputs and, at the shape of the nine pairs, fp16 and bf16 widened."""
    for dt in (F32, F16, BF16) if case is MC.pairs_case() else (F32,):
        t = MC.cast(case, (dt, dt))
        ref = MC.reference64(*t, n_buckets=case.n_buckets, c=LC.TORCH_SUM_C)
        got = MC.torch32_rows(*t[:6]).double().numpy()
        worst = MC.check_rows(got, ref, f"{case.name} {LC.short(dt)} torch float32", factor=1.0, exact=False)
        print(f"RATIO torch32 {case.name} {LC.short(dt)} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_check_rows_refuses_errors():
    case = MC.pairs_case()
    t = MC.cast(case, (F32, F32))
    ref = MC.reference64(*t, n_buckets=case.n_buckets)
    good = ref.rows.astype(np.float32).astype(np.float64)
    MC.check_rows(good, ref, "rounded reference", factor=1.0)
    b = int(np.nonzero(ref.rows[:, MC.ROW["HAS_POLICY"]])[0][3])
    for name, wrong in (("RANK", ref.rows[b, MC.ROW["RANK"]] + 1), ("TOP1", 1 - ref.rows[b, MC.ROW["TOP1"]]), ("P_TOP", ref.rows[b, MC.ROW["P_TOP"]] * (1 + 1e-4)),
                        ("NET_ENTROPY", ref.rows[b, MC.ROW["NET_ENTROPY"]] + 1e-3), ("CE", float("nan")), ("SE_Z", ref.rows[b, MC.ROW["SE_Z"]] + 1e-5)):
        bad = good.copy()
        bad[b, MC.ROW[name]] = wrong
        with pytest.raises(AssertionError):
            MC.check_rows(bad, ref, "a wrong element")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_under_the_emulator(case):
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, F32)):
            worst = MC.check_case(case, pair, "cpu")
            print(f"RATIO emu {case.name} {LC.short(pair[0])}/{LC.short(pair[1])} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_every_dtype_pair_at_one_shape_under_the_emulator():
    skipped = []
    with H.emulator_backend():
        for pair in LC.PAIRS:
            if F16 in pair:
                skipped.append(pair)
                continue
            MC.check_case(MC.pairs_case(), pair, "cpu")
    assert len(skipped) == 5


@pytest.mark.parametrize("case", DROPOUT, ids=lambda c: c.name)
def test_rows_that_drop_out_under_the_emulator(case):
    with H.emulator_backend():
        for pair in ((F32, F32), (BF16, BF16)):
            MC.check_dropout(case, pair, "cpu")


def test_accumulation_under_the_emulator():
    with H.emulator_backend():
        for name, pair in (("n65_W2_nb65", (F32, F32)), ("n130_W64_nb65", (BF16, F32)), ("n130_W2_nb3", (F32, BF16)), ("n64_W2_nb1", (F32, F32))):
            rep = MC.check_halves(next(c for c in CASES if c.name == name), pair, "cpu")
            assert rep["overall"]["records"] > 0
        empty = [b for b in rep["buckets"] if b["records"] == 0]
    assert not empty  # (one bucket, all rows in it)


def test_an_empty_bucket_reports_none():
    from betaone_amd.validate import MetricsAccumulator

    case = next(c for c in CASES if c.name == "n1_W2_nb3")
    with H.emulator_backend():
        acc = MetricsAccumulator(3, "cpu")
        t = MC.cast(case, (F32, F32))
        acc.add(*t[:5], q=t[5], bucket=t[6])
        rep = acc.result()
    assert sorted(b["records"] for b in rep["buckets"]) == [0, 0, 1] and rep["overall"]["records"] == 1
    for b in rep["buckets"]:
        if b["records"] == 0:
            assert all(v is None for k, v in b.items() if k not in ("records", "bad_rows", "policy_records", "decisive_records"))


def test_the_golden_counts_under_the_emulator():
    """The count columns of one seeded case are those stored under tests/golden (the GPU test compares with the same file)."""
    want = json.load(open(GOLDEN))
    case = next(c for c in CASES if c.name == want["case"])
    with H.emulator_backend():
        _, accum = MC.raw_metrics(*MC.cast(case, (F32, F32)), case.n_buckets)
    assert MC.golden_counts(accum[:case.n_buckets].numpy()) == want["counts"]


def test_bad_arguments_are_refused():
    from betaone_amd import engine as E
    from betaone_amd.validate import MetricsAccumulator

    case = MC.pairs_case()
    with H.emulator_backend():
        lib = E.load_hip_library()
        lg, v, ix, vl, z, q, bk = MC.cast(case, (F32, F32))
        rows, acc = torch.empty((case.n, MC.ROW_COLS)), torch.zeros((case.n_buckets, MC.COLS), dtype=torch.float64)
        args = lambda n=case.n, W=case.W, dt=0, nb=case.n_buckets, a=acc: (n, W, lg.data_ptr(), dt, v.data_ptr(), 0, ix.data_ptr(), vl.data_ptr(),  # noqa: E731
                                                                            z.data_ptr(), None, None, nb, rows.data_ptr(), a.data_ptr() if a is not None else None, None)
        assert lib.bo_train_metrics(*args()) == 0
        assert lib.bo_train_metrics(*args(n=0)) == -1 and lib.bo_train_metrics(*args(W=0)) == -1 and lib.bo_train_metrics(*args(nb=0)) == -1
        assert lib.bo_train_metrics(*args(a=None)) == -1 and lib.bo_train_metrics(*args(dt=7)) == -3
        m = MetricsAccumulator(case.n_buckets, "cpu")
        with pytest.raises(TypeError):
            m.add(lg.double(), v, ix, vl, z)
        with pytest.raises(ValueError):
            m.add(lg[:, :100], v, ix, vl, z)
        with pytest.raises(TypeError):
            m.add(lg, v, ix, vl, z, bucket=bk.long())


# ---- end to end ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fake_games():
    """Finished self-play games of FakeNet on the emulator (the recipe of tests/test_train_emu.py)."""
    from betaone_amd.rollout import Rollout

    with H.emulator_backend():
        ro = Rollout(FakeNet(scale=2.0, salt=7), 4, num_simulations=24, mcts_batch_size=8, device="cpu", use_graph=False, rng_mode="native",
                     policy_kind="logits", max_game_moves=12)
        ro.start_games(list(range(4)), list(range(4)), [900 + g for g in range(4)])
        nxt, fins = [4], []

        def refill(slot):
            if nxt[0] >= 8:
                return None
            nxt[0] += 1
            return nxt[0] - 1, 900 + nxt[0] - 1, None

        for _ in range(40):
            ro.play_ply(on_finished=fins.append, refill=refill)
            if len(fins) >= 8:
                break
        ro.close()
    assert len(fins) >= 6
    return fins


def _tiny_init(path, seed=0):
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 0, 16
    try:
        torch.manual_seed(seed)
        torch.save(network.PolicyValueNet().state_dict(), path)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def _dicts(fake_games, iteration=0):
    out = []
    for f in fake_games:
        g = R.unpack_games(R.pack_game(f))[0]
        g["iteration"] = iteration
        out.append(g)
    return out


def _seed_that_splits(games, fraction):
    """A seed whose split holds out at least one game and leaves at least two (the hash decides: the test looks for one)."""
    from betaone_amd import validate as V

    for seed in range(200):
        k = V.held_out_game_count(games, fraction, seed)
        if 1 <= k <= len(games) - 2:
            return seed
    raise AssertionError("no seed splits the games")


def test_splitmix64_is_the_published_generator():
    from betaone_amd import validate as V

    # the first outputs for the state 0 (Vigna's splitmix64.c: the state advances by the increment before every output)
    assert V.splitmix64(0) == 0xE220A8397B1DCDAF and V.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert V.holdout_hash(3, 17, 5) == V.holdout_hash(3, 17, 5) != V.holdout_hash(3, 18, 5)
    assert len({V.holdout_hash(i, g, s) for i in range(4) for g in range(50) for s in range(3)}) == 600
    share = sum(V.is_held_out(i, g, 0.25, 1) for i in range(10) for g in range(400)) / 4000.0
    assert 0.22 < share < 0.28


def test_holdout_games_is_deterministic_disjoint_and_stable(fake_games):
    from betaone_amd import validate as V

    games = _dicts(fake_games)
    seed = _seed_that_splits(games, 0.25)
    tr, he = V.holdout_games(games, 0.25, seed)
    tr2, he2 = V.holdout_games(games, 0.25, seed)
    total = sum(int(g["n_plies"]) for g in games)
    assert np.array_equal(tr, tr2) and np.array_equal(he, he2) and he.size > 0 and tr.size > 0
    assert not set(tr.tolist()) & set(he.tolist()) and sorted(tr.tolist() + he.tolist()) == list(range(total))
    held_ids = {int(g["game_id"]) for g in games if V.is_held_out(0, int(g["game_id"]), 0.25, seed)}
    # the reversed list, and the list with one more game: every game stays on its side
    for other in (games[::-1], games + [dict(games[0], game_id=4242)], games[1:]):
        _, h = V.holdout_games(other, 0.25, seed)
        at, ids = 0, set()
        for g in other:
            n = int(g["n_plies"])
            if set(range(at, at + n)) <= set(h.tolist()):
                ids.add(int(g["game_id"]))
            else:
                assert not set(range(at, at + n)) & set(h.tolist())
            at += n
        assert ids - {4242} == held_ids & {int(g["game_id"]) for g in other}
    # the iteration is part of the key
    assert any(V.is_held_out(0, g, 0.25, seed) != V.is_held_out(1, g, 0.25, seed) for g in range(64))
    none_tr, none_he = V.holdout_games(games, 0.0, seed)
    all_tr, all_he = V.holdout_games(games, 1.0, seed)
    assert none_he.size == 0 and none_tr.size == total and all_tr.size == 0 and all_he.size == total
    with pytest.raises(ValueError):
        V.holdout_games(games, 1.5, seed)


def test_the_loader_index_never_yields_a_held_out_record(fake_games):
    from betaone_amd import validate as V

    games = _dicts(fake_games)
    seed = _seed_that_splits(games, 0.25)
    tr, he = V.holdout_games(games, 0.25, seed)
    with H.emulator_backend():
        buf = R.GpuReplayBuffer(4096, device="cpu", pi_width=2)
        buf.add(games)
        assert len(buf) == tr.size + he.size
        held = buf.batch_sparse(he)[0].reshape(he.size, -1).numpy().view(np.uint32)
        train = buf.batch_sparse(tr)[0].reshape(tr.size, -1).numpy().view(np.uint32)
        held_set, train_set = {r.tobytes() for r in held}, {r.tobytes() for r in train}
        only_held = held_set - train_set   # (a position may occur in games of both sides: the start position does)
        assert only_held
        seen = 0
        for kw in (dict(steps=None), dict(steps=6)):
            for s, i, v, z in buf.loader(16, seed=3, sparse=True, index=tr, **kw):
                for r in s.reshape(s.shape[0], -1).numpy().view(np.uint32):
                    assert r.tobytes() in train_set and r.tobytes() not in only_held
                    seen += 1
        assert seen == tr.size + 6 * 16
        epoch = np.concatenate([s.reshape(s.shape[0], -1).numpy().view(np.uint32) for s, *_ in buf.loader(16, seed=3, sparse=True, index=tr)])
        assert sorted(r.tobytes() for r in epoch) == sorted(r.tobytes() for r in train)   # one pass: every training record once
        # index=None: the draws of the loader as it was
        a = [b[0] for b in buf.loader(16, steps=3, seed=5, sparse=True)]
        b = [b[0] for b in buf.loader(16, steps=3, seed=5, sparse=True, index=None)]
        c = [b[0] for b in buf.loader(16, steps=3, seed=5, sparse=True, index=np.arange(len(buf)))]
        assert all(torch.equal(x, y) and torch.equal(x, w) for x, y, w in zip(a, b, c))
        with pytest.raises(ValueError):
            buf.loader(16, index=np.array([len(buf)]))
        with pytest.raises(ValueError):
            buf.loader(16, index=np.zeros(0, dtype=np.int64))
        buf.close()


def test_evaluate_restores_the_mode_and_matches_the_accumulator(fake_games, tmp_path):
    from betaone_amd import match as M
    from betaone_amd import validate as V

    init = str(tmp_path / "i.pth")
    _tiny_init(init)
    games = _dicts(fake_games)
    with H.emulator_backend():
        buf = R.GpuReplayBuffer(4096, device="cpu", pi_width=2)
        buf.add(games)
        model = M.build_net(M.load_state_dict(init))
        index = np.arange(len(buf))[::2]
        for mode in (True, False):
            model.train(mode)
            rep = V.evaluate(model, buf, index, batch=16, amp=False, buckets="phase")
            assert model.training is mode
        assert rep["overall"]["records"] == index.size and sum(b["records"] for b in rep["buckets"]) == index.size
        assert rep["labels"] == ["<=10 men", "11-20 men", ">20 men"] and rep["buckets"][2]["records"] > 0
        # one batch by hand: the same numbers
        model.eval()
        s, i, v, z = buf.batch_sparse(index)
        with torch.no_grad():
            logits, value = model(s)
        ref = MC.reference64(logits, value, i, v, z, bucket=V.phase_bucket(s), n_buckets=3)
        men = s[:, 98:110].sum(dim=(1, 2, 3))
        assert bool(((men > 20) == (V.phase_bucket(s) == 2)).all()) and int(men.max()) == 32
        for k, b in enumerate(rep["buckets"]):
            assert b["records"] == int(ref.accum[k, 0])
            if b["policy_records"]:
                assert b["policy_top1"] == ref.accum[k, MC.ROW["TOP1"] + 1] / ref.accum[k, MC.ROW["HAS_POLICY"] + 1]
                assert abs(b["policy_ce"] - ref.accum[k, MC.ROW["CE"] + 1] / b["policy_records"]) < 1e-5
        cal = V.evaluate(model, buf, index, batch=7, amp=False, buckets="calibration", with_q=True)
        assert len(cal["buckets"]) == 10 and sum(b["records"] for b in cal["buckets"]) == index.size and cal["overall"]["value_mse_q"] is not None
        for k, b in enumerate(cal["buckets"]):
            if b["records"]:
                assert -1 + 0.2 * k - 1e-6 <= b["mean_value"] <= -1 + 0.2 * (k + 1) + 1e-6
        assert cal["overall"]["policy_top1"] == rep["overall"]["policy_top1"] and rep["overall"]["value_mse_q"] is None
        assert bool((V.calibration_bucket(torch.tensor([-1.0, -0.81, 0.0, 0.999, 1.0, float("nan")])) == torch.tensor([0, 0, 5, 9, 9, 5])).all())
        buf.close()


def test_train_with_a_holdout_writes_validation_and_validate_compares(fake_games, tmp_path, capsys):
    from betaone_amd import train as T
    from betaone_amd import validate as V

    data, save = str(tmp_path / "data"), str(tmp_path / "ck")
    R.save_games(R.compact_path(data, 0), fake_games[:5], append=False)
    R.save_games(R.compact_path(data, 1), fake_games[5:], append=False)
    files, _ = T.iteration_files(data, 1)
    games = T.load_window_games(files)
    assert [g["iteration"] for g in games] == [0] * 5 + [1] * (len(fake_games) - 5)
    seed = _seed_that_splits(games, 0.25)
    _, held = V.holdout_games(games, 0.25, seed)
    init = str(tmp_path / "init.pth")
    _tiny_init(init)
    common = ["--data-dir", data, "--save-dir", save, "--init", init, "--epochs", "2", "--batch", "16", "--steps-per-epoch", "3", "--no-amp",
              "--device", "cpu", "--iteration", "1"]
    with H.emulator_backend():
        cand = str(tmp_path / "cand.pth")
        assert T.main(common + ["--holdout-fraction", "0.25", "--holdout-seed", str(seed), "--out", str(tmp_path / "a.json"), "--candidate", cand]) == 0
        out = json.load(open(tmp_path / "a.json"))
        assert out["held_out_records"] == held.size and out["holdout_fraction"] == 0.25
        for e in out["epochs"]:
            val = e["validation"]
            assert val["records"] == held.size and 0.0 <= val["policy_top1"] <= 1.0 and np.isfinite(val["policy_ce"]) and val["policy_kl"] > -1e-6
            assert np.isfinite(val["value_mse_z"]) and val["bad_rows"] == 0
        assert "val policy" in capsys.readouterr().out
        # without the option: no validation, and none of the new keys
        assert T.main(common + ["--out", str(tmp_path / "b.json"), "--candidate", str(tmp_path / "c2.pth"), "--save-dir", str(tmp_path / "ck2")]) == 0
        plain = json.load(open(tmp_path / "b.json"))
        assert all("validation" not in e for e in plain["epochs"]) and "holdout_fraction" not in plain and "held_out_records" not in plain
        # a fraction that holds out nothing is an error that names the fraction and the games
        with pytest.raises(SystemExit) as err:
            T.main(common + ["--holdout-fraction", "1e-12", "--save-dir", str(tmp_path / "ck3")])
        assert "1e-12" in str(err.value) and f"{len(games)} games" in str(err.value)
        # the command: the held-out records of the same split, a net against itself
        rep = str(tmp_path / "report.json")
        dirs = [os.path.join(data, "iter_0"), os.path.join(data, "iter_1")]
        assert V.main(["--model", cand, "--compare", cand, *dirs, "--holdout-fraction", "0.25", "--seed", str(seed), "--buckets", "phase",
                       "--batch", "16", "--no-amp", "--out", rep, "--device", "cpu"]) == 0
        r = json.load(open(rep))
        assert r["records"] == held.size and r["model"]["overall"]["records"] == held.size
        assert r["model"]["overall"]["policy_top1"] == out["epochs"][-1]["validation"]["policy_top1"]
        assert abs(r["model"]["overall"]["policy_ce"] - out["epochs"][-1]["validation"]["policy_ce"]) < 1e-9
        for part in [r["difference"]["overall"]] + r["difference"]["buckets"]:
            assert all(v in (0, 0.0, None) for k, v in part.items() if k not in ("records", "bad_rows", "policy_records", "decisive_records"))
        text = capsys.readouterr().out
        assert "top1" in text and "compare - model" in text and ">20 men" in text
        assert V.main(["--model", cand, *dirs, "--all", "--device", "cpu", "--no-amp"]) == 0
        with pytest.raises(SystemExit):
            V.main(["--model", cand, *dirs, "--device", "cpu"])
