"""GPU tests of the training stage on the MI355X: the sparse-target loss kernels (csrc/bo_train.h) against PyTorch on the device in
float32 and fp16 and, element by element, against the float64 reference and envelope of tests/loss_cases.py on every case and
dtype pair (with the non-finite rows, guard rows, row independence and the replay samplers at wide rows), one training step of the
bench's 10x128 net on sparse batches against the reference's dense loss, and the loop self-play -> train --candidate -> match end
to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A = 4672


def _net(blocks, se, filters, seed=0):
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = blocks, se, filters
    try:
        torch.manual_seed(seed)
        net = network.PolicyValueNet()
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    return net.to(DEV)


def _case(B, W, seed, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    logits = (torch.randn((B, A), generator=g, device=DEV) * 3.0).to(dtype)
    value = torch.tanh(torch.randn((B, 1), generator=g, device=DEV)).to(dtype)
    z = torch.randint(-1, 2, (B, 1), generator=g, device=DEV).float()
    m = torch.randint(0, W + 1, (B,), generator=g, device=DEV)
    m[0] = W
    if B > 1:
        m[-1] = 0  # an empty row
    ix = torch.argsort(torch.rand((B, A), generator=g, device=DEV), dim=1)[:, :W].int()
    keep = torch.arange(W, device=DEV)[None, :] < m[:, None]
    v = (torch.rand((B, W), generator=g, device=DEV) + 0.05) * keep
    v = v / v.sum(1, keepdim=True).clamp_min(1e-30) * torch.where(torch.arange(B, device=DEV) % 2 == 1, 0.97, 1.0)[:, None]
    idx = torch.where(keep, ix, torch.full_like(ix, -1))
    return logits, value, idx, v.float(), z


def _dense(idx, val):
    d = torch.zeros((idx.shape[0], A + 1), device=DEV)
    d.scatter_(1, torch.where(idx >= 0, idx, A).long(), val)
    return d[:, :A]


def _torch(logits, value, idx, val, z, gscale):
    """PyTorch's path: under autocast the fp16 outputs are cast to float32 for the losses, and the gradients cast back."""
    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    pol, vl = F.cross_entropy(x.float(), _dense(idx, val)), F.mse_loss(v.float(), z)
    tot = vl + pol
    (tot * gscale).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


def _sparse(logits, value, idx, val, z, gscale):
    from betaone_amd.train import sparse_policy_value_loss

    x, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
    tot, pol, vl = sparse_policy_value_loss(x, v, idx, val, z)
    (tot * gscale).backward()
    return torch.stack([tot, pol, vl]).detach(), x.grad, v.grad


@pytest.mark.parametrize("B", [1, 256, 1024])
@pytest.mark.parametrize("W", [2, 32])
def test_loss_kernels_match_torch_float32(B, W):
    case = _case(B, W, B * 100 + W)
    gscale = torch.tensor(0.75, device=DEV)
    l_ref, gx_ref, gv_ref = _torch(*case, gscale)
    l, gx, gv = _sparse(*case, gscale)
    assert torch.allclose(l, l_ref, rtol=1e-6, atol=0), (l, l_ref)
    assert (gx - gx_ref).abs().max().item() <= 1e-6 and (gv - gv_ref).abs().max().item() <= 1e-6
    l2, gx2, _ = _sparse(*case, gscale)
    assert torch.equal(l.view(torch.int32), l2.view(torch.int32)) and torch.equal(gx.view(torch.int32), gx2.view(torch.int32))
    ref = LC.reference64(*case, (0.75, 0.0, 0.0))  # every element, the small ones too, against float64
    LC.check_against_reference((l, gx, gv.reshape(-1)), ref, LC.envelope(ref), f"B={B} W={W}")


def _ulp16(t):
    a = t.float().abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-14)
    return torch.exp2(e - 10)


@pytest.mark.parametrize("B", [1, 256, 1024])
@pytest.mark.parametrize("W", [2, 32])
def test_loss_kernels_match_torch_fp16(B, W):
    logits, value, idx, val, z = _case(B, W, B * 7 + W, torch.float16)
    for gscale in (1.0, 2.0 ** 16, 2.0 ** 27 / 256 * B):  # the last overflows fp16 at the target entries (GradScaler's case)
        g = torch.tensor(gscale, device=DEV)
        l_ref, gx_ref, gv_ref = _torch(logits, value, idx, val, z, g)
        l, gx, gv = _sparse(logits, value, idx, val, z, g)
        assert gx.dtype == torch.float16 and gv.dtype == torch.float16
        assert torch.allclose(l, l_ref, rtol=1e-6, atol=0), (l, l_ref)
        for mine, ref in ((gx, gx_ref), (gv, gv_ref)):
            assert torch.equal(torch.isinf(mine), torch.isinf(ref))
            fin = torch.isfinite(ref)
            assert bool(((mine.float() - ref.float()).abs()[fin] <= _ulp16(ref)[fin]).all())
        if gscale > 2.0 ** 20:
            assert bool(torch.isinf(gx).any()) and bool(torch.isfinite(gx).any())


CASES = LC.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_and_dtype_pair_against_float64(case):
    """sparse_policy_value_loss and its backward on every dtype pair (logits, value) against reference64 with the conditions of
    tests/loss_cases.py, and a second call bit for bit.  Prints the worst error / envelope of every pair."""
    for pair in LC.PAIRS:
        t = LC.cast(case, pair, DEV)
        out = LC.run_loss(*t, case.w3)
        assert out[1].dtype == pair[0] and out[2].dtype == pair[1]
        ref = LC.reference64(*t, case.w3)
        what = f"{case.name} {LC.short(pair[0])}/{LC.short(pair[1])}"
        r = LC.check_against_reference(out, ref, LC.envelope(ref), what)
        if case.name.startswith("overflow_fp16") and pair[0] == torch.float16:
            assert bool(torch.isinf(out[1]).any()) and bool(torch.isfinite(out[1]).any())
        again = LC.run_loss(*t, case.w3)
        assert all(LC.same_bits(a, b) for a, b in zip(out, again)), what + ": a second call differs"
        print(f"RATIO gpu {what} loss {r['loss']:.3f} dlogits {r['dlogits']:.3f} dvalue {r['dvalue']:.3f}")


@pytest.mark.parametrize("case", LC.nonfinite_cases(), ids=lambda c: c.name)
def test_non_finite_logits_as_the_header_states(case):
    for pair in ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.float32)):
        LC.check_nonfinite(case, pair, DEV)


@pytest.mark.parametrize("name", ["B65_W63_dom90_last_empty_rows", "B127_W63_randn001_invalid", "B4097_W2_pos80_edges"])
def test_rows_do_not_depend_on_their_place_in_the_batch(name):
    case = next(c for c in CASES if c.name == name)
    for pair in ((torch.float32, torch.float32), (torch.float16, torch.bfloat16)):
        LC.check_row_independence(case, pair, DEV)


@pytest.mark.parametrize("name", ["B65_W2_dom60_first_full", "B65_W63_dom90_last_empty_rows", "B4097_W2_pos80_edges",
                                  "B4097_W64_randn3_invalid"])
def test_loss_kernels_write_no_row_past_the_batch(name):
    """bo_train_loss_forward / bo_train_loss_backward called directly at B = 65 and 4097 with row_stats, dlogits and dvalue 64 guard
    rows longer than the batch: the guard keeps its NaN payload, every row below B is written, and the results are the reference's."""
    case = next(c for c in CASES if c.name == name)
    for pair in ((torch.float32, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.float16)):
        LC.check_guard_rows(case, pair, DEV)


def test_the_entry_points_refuse_bad_arguments_in_their_words():
    assert LC.check_refusals(DEV) > 0


@pytest.fixture(scope="module")
def games():
    """Self-play games of a 10x128 net (CohortRollout, two cohorts), as FinishedGame objects."""
    from betaone_amd.rollout import CohortRollout

    net = _net(8, 2, 128).eval()
    ro = CohortRollout(net, 8, cohorts=2, num_simulations=16, mcts_batch_size=8, max_game_moves=24, rng_mode="native", device=DEV)
    ro.start_games(list(range(8)), list(range(8)), list(range(8)))
    nxt, fins = [8], []

    def refill(slot):
        if nxt[0] >= 16:
            return None
        nxt[0] += 1
        return nxt[0] - 1, nxt[0] - 1, None

    while len(fins) < 16:
        ro.play_ply(on_finished=fins.append, refill=refill)
    ro.close()
    return fins


def _buffer(games):
    from betaone_amd import records as R

    buf = R.GpuReplayBuffer(20000, device=DEV, pi_width=2)
    buf.add(games)
    return buf


@pytest.mark.parametrize("W", [1, 64, 65, LC.res_cap()])
def test_replay_samplers_at_wide_rows(games, W):
    """GpuReplayBuffer(pi_width=W) over the fixture's games with seeded synthetic pis of 0..W entries: batch_sparse equals the records
    entry for entry, its scatter equals batch bit for bit, and one loss forward and backward on that batch meets the reference."""
    r = LC.check_wide_replay(games, W, DEV, seed=11)
    print(f"RATIO gpu replay W={W} f32/f32 loss {r['loss']:.3f} dlogits {r['dlogits']:.3f} dvalue {r['dvalue']:.3f}")


def test_one_step_sparse_equals_dense(games):
    """The bench's 10x128 net, float32, no autocast: loss and every parameter gradient of a step on batch_sparse + the kernels equal
    those of batch + the reference's calculate_loss."""
    from betaone_amd.train import dense_policy_value_loss, sparse_policy_value_loss

    buf = _buffer(games)
    q = np.random.default_rng(0).integers(0, len(buf), size=256)
    net_s, net_d = _net(8, 2, 128, seed=3).train(), _net(8, 2, 128, seed=3).train()
    s, idx, val, z = buf.batch_sparse(q)
    ls = sparse_policy_value_loss(*net_s(s), idx, val, z)
    ls[0].backward()
    s2, pi, z2 = buf.batch(q)
    ld = dense_policy_value_loss(*net_d(s2), pi, z2)
    ld[0].backward()
    for a, b in zip(ls, ld):
        assert abs(a.item() - b.item()) <= 1e-5 * abs(b.item()), (a.item(), b.item())
    for (name, p), (_, q_) in zip(net_s.named_parameters(), net_d.named_parameters()):
        assert (p.grad - q_.grad).norm().item() <= 1e-5 * q_.grad.norm().item() + 1e-12, name
    buf.close()


def test_twenty_amp_steps_follow_the_dense_loss(games):
    """torch.autocast + GradScaler, AdamW at the reference's learning rate, 20 steps from the same weights on the same batches.  The first
    step's losses agree to the kernels' precision (measured: 2e-5 relative).  After it the runs are trajectories: under autocast even the
    dense path against itself differs by 3.7e-3 relative within 20 steps.  The scaler starts at 2^10, not at its default 2^16: at 2^16
    the first steps' overflow check sits at the edge, so that of two identical runs of the dense path one skipped a step and the other
    did not, and the curves parted by a step's worth (measured: 7e-2 relative in the total loss, 0.8 in the value loss against the
    band's 1e-1).  At 2^10 no run skips a step (asserted), and sparse against dense stayed within 7e-3 for every order of the games
    tried.  The whole curve is held to a band that a wrong gradient would leave."""
    from betaone_amd.train import train_steps

    buf = _buffer(games)
    curves = []
    for sparse in (True, False, False):
        net = _net(8, 2, 128, seed=4).train()
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=1000, eta_min=5e-7)
        scaler = torch.GradScaler("cuda", init_scale=2.0 ** 10)
        r = train_steps(net, opt, sched, scaler, buf.loader(256, steps=20, seed=9, sparse=sparse), sparse=sparse, amp=True)
        assert r["steps"] == 20
        assert scaler.get_scale() == 2.0 ** 10  # no step was skipped (and 20 steps are far from the scaler's growth interval)
        curves.append(np.array(r["losses"]))
    assert np.isfinite(curves[0]).all()
    rel = np.abs(curves[0] - curves[1]) / np.abs(curves[1])
    noise = np.abs(curves[2] - curves[1]) / np.abs(curves[1])
    print("sparse vs dense, max relative difference of the total / policy loss:", rel[:, 0].max(), rel[:, 1].max(),
          "first step:", rel[0, :2].tolist(), "dense vs dense:", noise[:, 0].max(), "first step:", noise[0, 0])
    assert rel[0, 0] <= 1e-4 and rel[0, 1] <= 1e-4
    assert rel[:, 0].max() <= 1e-1 and rel[:, 1].max() <= 1e-1
    assert np.abs(curves[0][:, 2] - curves[1][:, 2]).max() <= 1e-1  # (the value loss swings between ~1 and ~1e-4: compared absolutely)
    buf.close()


def test_selfplay_train_match_loop(games, tmp_path):
    """Records of CohortRollout games -> python -m betaone_amd.train --candidate -> python -m betaone_amd.match initial cand; the
    candidate loads through build_net and Rollout.swap_model and plays."""
    from betaone_amd import match as M
    from betaone_amd import records as R
    from betaone_amd import train as T
    from betaone_amd.rollout import Rollout

    data, save = tmp_path / "data", tmp_path / "ck"
    R.save_games(R.compact_path(str(data), 0), games, append=False)
    init, cand = tmp_path / "initial.pth", tmp_path / "cand.pth"
    torch.save(_net(8, 2, 128, seed=5).state_dict(), init)
    assert T.main(["--iteration", "0", "--data-dir", str(data), "--save-dir", str(save), "--init", str(init), "--candidate", str(cand),
                   "--epochs", "2", "--batch", "64", "--out", str(tmp_path / "train.json")]) == 0
    assert not (save / "best_model.pth").exists() and (save / "checkpoint_iter_0.pth").exists()
    assert M.main([str(init), str(cand), "--games", "4", "--slots", "4", "--cohorts", "1", "--sims", "16", "--mcts-batch", "8",
                   "--max-game-moves", "12", "--out", str(tmp_path / "match.json")]) == 0
    net = M.build_net(M.load_state_dict(str(cand)), DEV)
    ro = Rollout(_net(8, 2, 128).eval(), 4, num_simulations=16, mcts_batch_size=8, device=DEV, rng_mode="native")
    ro.start_games(list(range(4)), list(range(4)), list(range(4)))
    assert ro.play_ply() == 4
    ro.swap_model(net)
    assert ro.play_ply() == 4
    ro.eng.check_status()
    ro.close()
