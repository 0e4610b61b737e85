"""CPU tests (wave emulator) of the training stage: the sparse replay sampler (csrc/bo_replay.h bo_k_replay_encode_sparse), the
sparse-target loss kernels (csrc/bo_train.h) against PyTorch's F.cross_entropy + F.mse_loss on the dense target and their autograd
gradients, and `python -m betaone_amd.train` end to end with a tiny net (checkpoint layout, resume, candidate, overfitting)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import engine_harness as H
from fake_model import FakeNet

from betaone_amd import records as R

A = 4672


@pytest.fixture(scope="module")
def fake_games():
    """Finished self-play games of FakeNet on the emulator (the engine's own pi: at most 2 entries per ply)."""
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


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _scatter(idx, val):
    d = torch.zeros((idx.shape[0], A), dtype=torch.float32)
    for b in range(idx.shape[0]):
        for e in range(idx.shape[1]):
            if idx[b, e] >= 0:
                d[b, int(idx[b, e])] = val[b, e]
    return d


def _compare_samplers(buf, q):
    s0, p0, z0 = buf.batch(q)
    s1, i1, v1, z1 = buf.batch_sparse(q)
    assert i1.dtype == torch.int32 and i1.shape == (len(q), buf.pi_width) and v1.shape == (len(q), buf.pi_width) and z1.shape == (len(q), 1)
    assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(_bits(z0), _bits(z1))
    assert np.array_equal(_bits(_scatter(i1, v1)), _bits(p0))
    assert bool(((i1 >= 0) | (v1 == 0)).all())  # unused slots: (-1, 0)
    return i1, v1


def test_sparse_sampler_matches_the_dense_one(fake_games):
    with H.emulator_backend():
        buf = R.GpuReplayBuffer(4096, device="cpu", pi_width=2)
        buf.add(fake_games)
        n = len(buf)
        q = np.random.default_rng(3).integers(0, n, size=48)
        i1, _ = _compare_samplers(buf, np.concatenate([q, [0, n - 1]]))
        assert int((i1 >= 0).sum(1).max()) >= 1
        # the loader yields the same batches in both forms
        for (s0, p0, z0), (s1, i, v, z1) in zip(buf.loader(16, steps=3, seed=5), buf.loader(16, steps=3, seed=5, sparse=True)):
            assert np.array_equal(_bits(s0), _bits(s1)) and np.array_equal(_bits(z0), _bits(z1))
            assert np.array_equal(_bits(_scatter(i, v)), _bits(p0))
        buf.close()


def test_sparse_sampler_width_8_with_empty_rows(fake_games):
    rng = np.random.default_rng(11)
    games = []
    for f in fake_games[:4]:
        g = R.unpack_games(R.pack_game(f))[0]
        pis = []
        for k in range(int(g["n_plies"])):
            m = int(rng.integers(0, 9)) if k % 3 else 0  # every third row has no entries
            ix = rng.choice(A, size=m, replace=False).astype(np.int32)
            pis.append((ix, rng.random(m).astype(np.float32)))
        g["pis"] = pis
        games.append(g)
    with H.emulator_backend():
        buf = R.GpuReplayBuffer(4096, device="cpu", pi_width=8)
        buf.add(games)
        i1, _ = _compare_samplers(buf, np.arange(len(buf)))
        counts = (i1 >= 0).sum(1)
        assert int(counts.min()) == 0 and int(counts.max()) == 8
        buf.close()


def _case(B, W, seed, inf_row=None):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, A), generator=g) * 3.0
    value = torch.tanh(torch.randn((B, 1), generator=g))
    z = torch.randint(-1, 2, (B, 1), generator=g).float()
    idx = torch.full((B, W), -1, dtype=torch.int32)
    val = torch.zeros((B, W))
    for b in range(B):
        m = 0 if (b == B - 1 and B > 1) else int(torch.randint(1, W + 1, (1,), generator=g))  # the last row is empty
        ix = torch.randperm(A, generator=g)[:m]
        pos = torch.randperm(W, generator=g)[:m]  # entries anywhere in the row, gaps of -1 between them
        v = torch.rand(m, generator=g) + 0.05
        v = v / v.sum() * (0.97 if b % 2 else 1.0)  # sums != 1 as well
        idx[b, pos] = ix.int()
        val[b, pos] = v.float()
    if inf_row is not None:
        logits[inf_row, 17] = float("inf")
    return logits, value, idx, val, z


def _torch_ref(logits, value, idx, val, z, w):
    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    tot, pol, vl = F.mse_loss(v, z) + F.cross_entropy(x, _scatter(idx, val)), F.cross_entropy(x, _scatter(idx, val)), F.mse_loss(v, z)
    (w[0] * tot + w[1] * pol + w[2] * vl).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


def _sparse(logits, value, idx, val, z, w):
    from betaone_amd.train import sparse_policy_value_loss

    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    tot, pol, vl = sparse_policy_value_loss(x, v, idx, val, z)
    (w[0] * tot + w[1] * pol + w[2] * vl).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


@pytest.mark.parametrize("B", [1, 7, 64])
def test_loss_and_gradients_match_torch(B):
    with H.emulator_backend():
        for seed, w in ((B, (1.0, 0.0, 0.0)), (B + 100, (0.37, 1.5, -2.25))):  # random grad_output, also through policy / value
            case = _case(B, 6, seed)
            l_ref, gx_ref, gv_ref = _torch_ref(*case, w)
            l, gx, gv = _sparse(*case, w)
            assert torch.allclose(l, l_ref, rtol=1e-6, atol=0), (l, l_ref)
            assert (gx - gx_ref).abs().max().item() <= 1e-6 and (gv - gv_ref).abs().max().item() <= 1e-6
            if B > 1:
                assert gx[B - 1].abs().max().item() == 0.0  # the empty row: no policy gradient
            l2, gx2, gv2 = _sparse(*case, w)  # bit-reproducible
            assert np.array_equal(_bits(l), _bits(l2)) and np.array_equal(_bits(gx), _bits(gx2)) and np.array_equal(_bits(gv), _bits(gv2))


def test_non_finite_logits_propagate():
    with H.emulator_backend():
        case = _case(7, 4, 5, inf_row=2)
        l_ref, gx_ref, _ = _torch_ref(*case, (1.0, 0.0, 0.0))
        l, gx, _ = _sparse(*case, (1.0, 0.0, 0.0))
        assert not torch.isfinite(l_ref[:2]).any() and not torch.isfinite(l[:2]).any()
        assert torch.isfinite(l[2]) and torch.allclose(l[2], l_ref[2], rtol=1e-6)
        assert torch.isnan(gx[2]).all() and torch.isnan(gx_ref[2]).all()
        assert torch.isfinite(gx[[0, 1, 3, 4, 5, 6]]).all()


def test_bfloat16_inputs():
    """bf16 logits / value (torch.autocast on a CPU device): float32 arithmetic inside, gradients rounded once to bf16."""
    with H.emulator_backend():
        logits, value, idx, val, z = _case(7, 4, 9)
        lb, vb = logits.bfloat16(), value.bfloat16()
        l_ref, gx_ref, gv_ref = _torch_ref(lb.float(), vb.float(), idx, val, z, (1.0, 0.0, 0.0))
        l, gx, gv = _sparse(lb, vb, idx, val, z, (1.0, 0.0, 0.0))
        assert gx.dtype == torch.bfloat16 and gv.dtype == torch.bfloat16
        assert torch.allclose(l, l_ref, rtol=1e-6)
        ulp = lambda t: torch.where(t == 0, torch.tensor(2.0 ** -133), t.abs().bfloat16().float() * 2.0 ** -7)  # noqa: E731
        assert bool(((gx.float() - gx_ref).abs() <= ulp(gx_ref)).all()) and bool(((gv.float() - gv_ref).abs() <= ulp(gv_ref)).all())


def test_bad_arguments_are_refused():
    from betaone_amd import engine as E
    from betaone_amd.train import sparse_policy_value_loss

    with H.emulator_backend():
        logits, value, idx, val, z = _case(3, 2, 1)
        with pytest.raises(TypeError):
            sparse_policy_value_loss(logits.double(), value, idx, val, z)
        with pytest.raises(ValueError):
            sparse_policy_value_loss(logits[:, :100], value, idx, val, z)
        lib = E.load_hip_library()
        assert lib.bo_train_loss_forward(3, 2, logits.data_ptr(), 7, value.data_ptr(), 0, idx.data_ptr(), val.data_ptr(), z.data_ptr(),
                                         torch.empty(12).data_ptr(), torch.empty(3).data_ptr(), None) != 0
        assert lib.bo_train_loss_forward(0, 2, logits.data_ptr(), 0, value.data_ptr(), 0, idx.data_ptr(), val.data_ptr(), z.data_ptr(),
                                         torch.empty(12).data_ptr(), torch.empty(3).data_ptr(), None) != 0


def _tiny_init(path):
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 0, 16
    try:
        torch.manual_seed(0)
        torch.save(network.PolicyValueNet().state_dict(), path)
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


def test_train_command_writes_the_reference_checkpoint_and_resumes(fake_games, tmp_path):
    from betaone_amd import match as M
    from betaone_amd import train as T

    data, save = str(tmp_path / "data"), str(tmp_path / "ck")
    R.save_games(R.compact_path(data, 0), fake_games[:5], append=False)
    R.save_games(R.compact_path(data, 1), fake_games[5:], append=False)
    init = str(tmp_path / "init.pth")
    _tiny_init(init)
    common = ["--data-dir", data, "--save-dir", save, "--init", init, "--epochs", "2", "--batch", "16", "--steps-per-epoch", "3", "--no-amp",
              "--device", "cpu"]
    with H.emulator_backend():
        assert T.main(common + ["--iteration", "0", "--out", str(tmp_path / "a.json")]) == 0
        ck = torch.load(os.path.join(save, "checkpoint_iter_0.pth"), map_location="cpu")
        assert set(ck) == {"iteration", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"} and ck["iteration"] == 0
        net = M.build_net(ck["model_state_dict"])
        assert M.net_shape(net.state_dict()) == (1, 0, 16)
        assert os.path.exists(os.path.join(save, "best_model.pth"))
        out = json.load(open(tmp_path / "a.json"))
        assert [e["steps"] for e in out["epochs"]] == [3, 3] and all(np.isfinite(e["loss"]) and e["samples_per_s"] > 0 for e in out["epochs"])
        # a second run resumes: the next iteration, the optimizer's step count, the scheduler; --candidate leaves best alone
        best = open(os.path.join(save, "best_model.pth"), "rb").read()
        cand = str(tmp_path / "cand.pth")
        assert T.main(common + ["--candidate", cand]) == 0
        ck1 = torch.load(os.path.join(save, "checkpoint_iter_1.pth"), map_location="cpu")
        assert ck1["iteration"] == 1
        assert int(ck1["optimizer_state_dict"]["state"][0]["step"]) == 12 and ck1["scheduler_state_dict"]["last_epoch"] == 12
        assert open(os.path.join(save, "best_model.pth"), "rb").read() == best
        M.build_net(M.load_state_dict(cand))
        # an iteration with pickles only is reported, not silently skipped; no records at all is an error
        os.makedirs(os.path.join(data, "iter_9"))
        open(os.path.join(data, "iter_9", "game_0.pkl"), "wb").close()
        assert T.main(common + ["--iteration", "9", "--past", "0"]) == 1


def test_training_lowers_the_loss(fake_games, capsys):
    from betaone_amd import match as M
    from betaone_amd import train as T

    torch.manual_seed(1)
    with H.emulator_backend():
        buf = R.GpuReplayBuffer(4096, device="cpu", pi_width=2)
        buf.add(fake_games)
        q = np.arange(32)
        fixed = buf.batch_sparse(q)
        import tempfile

        with tempfile.TemporaryDirectory() as d:
            _tiny_init(os.path.join(d, "i.pth"))
            model = M.build_net(M.load_state_dict(os.path.join(d, "i.pth")))
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000, eta_min=5e-7)
        scaler = torch.GradScaler("cpu", enabled=False)
        r = T.train_steps(model, opt, sched, scaler, [fixed] * 100, amp=False, log_every=50, log=print)
        assert r["steps"] == 100 and r["samples"] == 3200
        first, last = np.mean([x[0] for x in r["losses"][:5]]), np.mean([x[0] for x in r["losses"][-5:]])
        assert last < 0.7 * first, (first, last)
        assert "step 50:" in capsys.readouterr().out
        buf.close()
