"""GPU tests of the evaluate stage's persistent tower kernels at batches that make their workgroups loop (tests/evaluate_batches.py:
the grid geometry, read from the device's CU count), on distinct encoded positions from seeded random games:

  * batch invariance, bit for bit: a board's outputs do not depend on the batch around it or on its row -- twice the same batch, a
    permuted batch, a sub-batch (every board in another slot; for the fp16 tower, with another partner in its pair);
  * accuracy on later passes: sampled rows of the largest multi-pass batch against the same net in float64 on the CPU;
  * fast mode's evaluate stage (bench.py --fast: the 10x128 fp16 net at 32 768 rows, 64 passes of the h16 tower, then bo_nn_heads_f16);
  * no writes past row B: output buffers of the lab ABI calls with NaN-filled guard rows."""
import numpy as np
import pytest
import torch

import evaluate_batches as EB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (id, conv, (blocks, SE blocks, filters), environment read when the stage is built); every net has an SE block
ROUTES = [
    ("tower_split_t16_128", "tower_split", (2, 1, 128), {"BETAONE_SPLIT_TILE": "16"}),
    ("tower_split_t32_128", "tower_split", (2, 1, 128), {"BETAONE_SPLIT_TILE": "32"}),
    ("tower_split_256", "tower_split", (1, 1, 256), {}),
    ("tower_wg_64", "tower_wg", (2, 1, 64), {}),
    ("tower_wg_128", "tower_wg", (2, 1, 128), {}),
    ("tower_64", "tower", (2, 1, 64), {}),
    ("tower_128", "tower", (2, 1, 128), {}),
    ("tower_f16_t16_128", "tower_f16", (2, 1, 128), {"BETAONE_F16_TILE": "16"}),
    ("tower_f16_t32_128", "tower_f16", (2, 1, 128), {"BETAONE_F16_TILE": "32"}),
    ("tower_f16_t16_256", "tower_f16", (1, 1, 256), {"BETAONE_F16_TILE": "16"}),
    ("tower_f16_t32_256", "tower_f16", (1, 1, 256), {"BETAONE_F16_TILE": "32"}),
    ("mfma_256", "mfma", (1, 1, 256), {}),
]


@pytest.fixture(scope="module")
def n_cu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from betaone_amd import engine as E

    E.load_hip_library()
    return torch.cuda.get_device_properties(0).multi_processor_count  # what the library reads from hipDeviceProp


@pytest.fixture(scope="module")
def bases():
    return torch.from_numpy(EB.random_positions(640, seed=11)).to(DEV)


def _plain_net(size, seed=None):
    """A PolicyValueNet of this size on the GPU: hash-initialised, or torch's default initialisation after manual_seed(seed)."""
    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = size
    try:
        if seed is None:
            net = hash_init_(network.PolicyValueNet().eval())
        else:
            torch.manual_seed(seed)
            net = network.PolicyValueNet().eval()
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    return net.to(DEV)


def _stage(conv, size, env, monkeypatch):
    from betaone_amd.fused_net import FusedPolicyValueNet

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = _plain_net(size)
    fused = FusedPolicyValueNet(net, conv=conv).to(DEV)
    assert fused.layout == "nchw+" + conv
    if "BETAONE_SPLIT_TILE" in env:
        assert fused.split_tile == int(env["BETAONE_SPLIT_TILE"])
    if "BETAONE_F16_TILE" in env:
        assert fused.f16_tile == int(env["BETAONE_F16_TILE"])
    return net, fused


def _tower_out(fused, x):
    """What the tower itself writes: the tower output [B, C, 8, 8] (fp16 tower: its two fp16 head-plane buffers)."""
    if fused.conv == "tower_f16":
        return fused._tower_f16_forward(x)
    if fused.conv == "mfma":
        return (fused._tower_mfma(x),)
    return (fused._tower_forward(x),)


def _outputs(fused, x):
    with torch.no_grad():
        t = tuple(o.clone() for o in _tower_out(fused, x))
        logits, value = fused(x)
    return t + (logits, value.reshape(-1, 1))


def _assert_rows_equal(got, want, what, f16):
    names = (("policy planes", "value planes") if f16 else ("tower output",)) + ("logits", "value")
    for name, g, w in zip(names, got, want):
        if not torch.equal(g, w):
            bad = (g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(1).nonzero().flatten()
            raise AssertionError(f"{what}: {name} differs in {bad.numel()} of {w.shape[0]} rows, first {bad[:8].tolist()}")


@pytest.mark.parametrize("rid,conv,size,env", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_is_batch_invariant_bit_for_bit(n_cu, bases, rid, conv, size, env, monkeypatch):
    """For every batch of EB.batch_list (one to four passes over the grid): (a) a second evaluation of the batch, (b) the batch in a
    random order, once the order is undone, and (c) the sub-batch of rows [1, B) give the same bits in every row -- of the tower's own
    output and of the logits and value.  (The product relies on it: cohorts of a rollout evaluate a game's positions in other batches
    at other rows, and test_cohorts_on_their_own_streams_finish_the_games_of_the_single_rollout needs their games bit-identical.)"""
    _, fused = _stage(conv, size, env, monkeypatch)
    f16 = conv == "tower_f16"
    g = torch.Generator().manual_seed(size[2] + len(rid))
    ran = []
    for B in EB.batch_list(conv, size[2], n_cu):
        x = EB.make_rows(bases, B, seed=B)
        EB.assert_rows_distinct(x)
        ref = _outputs(fused, x)
        _assert_rows_equal(_outputs(fused, x), ref, f"{rid} B={B} repeated", f16)
        perm = torch.randperm(B, generator=g).to(DEV)
        inv = torch.argsort(perm)
        _assert_rows_equal([o[inv] for o in _outputs(fused, x[perm].contiguous())], ref, f"{rid} B={B} permuted", f16)
        sub = EB.sub_batch(B, conv)
        if sub is not None:
            _assert_rows_equal(_outputs(fused, x[sub].contiguous()), [o[sub] for o in ref], f"{rid} B={B} rows {sub.start}..{sub.stop - 1}", f16)
        else:  # (the fp16 tower's planes only: the heads of the smaller batch are the other kernel)
            t = _tower_out(fused, x[1:].contiguous())
            _assert_rows_equal(t, [o[1:] for o in ref[:len(t)]], f"{rid} B={B} rows 1.. (tower)", f16)
        ran.append((B, EB.passes(B, EB.boards_per_pass(conv, size[2], n_cu))))
    torch.cuda.synchronize()
    fused.check_overflow()
    print(f"[batches] {rid} n_cu={n_cu}: (B, passes) {ran}")


def _err_bound(conv, net, x_rows, l64, v64):
    """The bound of the suite's existing tests: float32 routes 4 x (torch float32 on the GPU) + 1e-5; fp16 routes max(3 x (torch
    float16), 4e-3 x max(1, |logits|))."""
    with torch.no_grad():
        if conv == "tower_f16":
            half = net.for_inference(dtype=torch.float16, channels_last=False)
            l, v = half(x_rows.half())
            e_torch = EB.row_errors(l.float(), v.float(), l64, v64).max()
            return max(3.0 * e_torch, 4e-3 * max(1.0, l64.abs().max().item())), e_torch
        l, v = net(x_rows)
        e_torch = EB.row_errors(l, v, l64, v64).max()
        return 4.0 * e_torch + 1e-5, e_torch


@pytest.mark.parametrize("rid,conv,size,env", ROUTES, ids=[r[0] for r in ROUTES])
def test_later_pass_rows_match_the_float64_net(n_cu, bases, rid, conv, size, env, monkeypatch):
    """The largest multi-pass batch (four passes; for the fp16 tower odd, its tail board alone in a looping workgroup): the first and
    last row of every pass, the tail board and the boards its workgroup held before, and a strided sample (<= 64 rows) against the
    same net in float64 on the CPU.  Every row, whatever its pass, within the bound the suite uses for first-pass rows."""
    net, fused = _stage(conv, size, env, monkeypatch)
    B = EB.largest_batch(conv, size[2], n_cu)
    x = EB.make_rows(bases, B, seed=B + 1)
    with torch.no_grad():
        logits, value = fused(x)
    rows = EB.sample_rows(B, conv, size[2], n_cu)
    idx = torch.tensor(rows, device=DEV)
    l64, v64 = EB.reference64(net, x[idx])
    err = EB.row_errors(logits[idx], value.reshape(-1, 1)[idx], l64, v64)
    bound, e_torch = _err_bound(conv, net, x[idx], l64, v64)
    per_pass = {}
    for r, e in zip(rows, err):
        p = EB.pass_of(r, conv, size[2], n_cu)
        per_pass[p] = max(per_pass.get(p, 0.0), float(e))
    assert len(per_pass) == EB.passes(B, EB.boards_per_pass(conv, size[2], n_cu)) == 4
    worst = int(np.argmax(err))
    assert err.max() <= bound, (rid, B, "row", rows[worst], "pass", EB.pass_of(rows[worst], conv, size[2], n_cu), float(err.max()), bound, e_torch, per_pass)
    fused.check_overflow()


# (conv, the smallest net of the suite that the route takes, [(batch, BETAONE_HEADS_F16 or None, the stages allowed)])
STAGE_CASES = [(conv, (2, 1, 64), [(3, None, ("heads",))]) for conv in ("mfma", "mfma_small", "tower_b1", "tower", "tower_wg")]
STAGE_CASES += [("miopen", (2, 1, 64), [(3, None, ("library",))]), ("tower_split", (2, 1, 128), [(3, None, ("heads",))]),
                ("tower_f16", (2, 1, 128), [(3, None, ("heads",)), (1024, None, ("heads",)), (1024, "0", ("heads",)),
                                            (1025, None, ("heads_f16",)), (1025, "0", ("library",))])]


@pytest.mark.parametrize("conv,size,runs", STAGE_CASES, ids=[c[0] for c in STAGE_CASES])
def test_head_stage_agrees_with_forward(bases, conv, size, runs, monkeypatch):
    """head_stage(B) names what forward runs: forward(x, tail=True) returns value_fc1's partial sums [16, B, 256] exactly when
    tail_supported(B), and raises EngineError otherwise (never the value [B, 1] in their place); forward and forward_probs stay,
    at every stage, within the bound this file uses for the route (_err_bound; for the probabilities against the float64 softmax of
    the float64 logits: |d softmax| <= max |d logits| / 2, so the logits' bound holds for them)."""
    from betaone_amd import engine as E
    from betaone_amd.fused_net import FusedPolicyValueNet

    net = _plain_net(size)
    fused = FusedPolicyValueNet(net, conv=conv).to(DEV)
    for B, heads_f16, stages in runs:
        if heads_f16 is None:
            monkeypatch.delenv("BETAONE_HEADS_F16", raising=False)
        else:
            monkeypatch.setenv("BETAONE_HEADS_F16", heads_f16)
        what = (conv, B, heads_f16)
        x = EB.make_rows(bases, B, seed=B + 3)
        stage = fused.head_stage(B)
        assert stage in stages and fused.tail_supported(B) == (stage == "heads"), (what, stage)
        with torch.no_grad():
            logits, value = fused(x)
            probs, value_p = fused.forward_probs(x)
            if fused.tail_supported(B):
                l_tail, part = fused.forward(x, tail=True)
                assert part.shape == (16, B, 256) and part.dtype == torch.float32 and torch.equal(l_tail, logits), what
                l_tail, part = fused.forward_tail(x)
                assert part.shape == (16, B, 256), what
            else:
                for call in (lambda: fused.forward(x, tail=True), lambda: fused.forward_tail(x)):
                    with pytest.raises(E.EngineError):
                        call()
        assert logits.shape == probs.shape == (B, 4672) and value.reshape(-1).shape == value_p.reshape(-1).shape == (B,), what
        idx = torch.tensor(sorted({0, 1, B // 2, B - 2, B - 1}), device=DEV)
        l64, v64 = EB.reference64(net, x[idx])
        bound, e_torch = _err_bound(conv, net, x[idx], l64, v64)
        e_logits = EB.row_errors(logits[idx].float(), value.float().reshape(-1, 1)[idx], l64, v64).max()
        e_probs = EB.row_errors(probs[idx], value_p.float().reshape(-1, 1)[idx], torch.softmax(l64, dim=1), v64).max()
        print(f"[head stage] {conv} B={B} BETAONE_HEADS_F16={heads_f16}: {stage}; errors {e_logits:.3g} / {e_probs:.3g}, bound {bound:.3g} (torch {e_torch:.3g})")
        assert e_logits <= bound and e_probs <= bound, (what, stage, float(e_logits), float(e_probs), bound)
    torch.cuda.synchronize()
    fused.check_overflow()


def test_fast_mode_evaluate_stage_at_32768_rows(n_cu, bases):
    """The evaluate stage of bench.py --fast at a quarter of the bench's batch: the 10x128 net (torch.manual_seed(0), default
    initialisation) in fp16 as bench.make_net builds it -- best_inference_copy(..., torch.float16) -> conv='tower_f16'.  The bench sizes
    it (games // cohorts) x leaves = 32 768 x 4 = 131 072 rows (bench.py:763, --leaves 4); here bo_k_tower_h16<128, 1> runs over 32 768
    rows = 16 384 pairs (64 passes of the grid at 256 CUs), then bo_nn_heads_f16.  Every probability finite, every row summing to 1;
    strided rows within the fp16 bound of the float64 net; a permuted batch gives the same bits."""
    from betaone_amd.nn_tune import best_inference_copy

    B = 32768
    net = _plain_net((8, 2, 128), seed=0)
    stage = best_inference_copy(net, B, DEV, torch.float16)
    assert stage.layout == "nchw+tower_f16" and stage.f16_tile == 16
    x = EB.make_rows(bases, B, seed=7)
    EB.assert_rows_distinct(x)
    with torch.no_grad():
        probs, value = stage.forward_probs(x)
    assert probs.shape == (B, 4672) and torch.isfinite(probs).all() and torch.isfinite(value).all()
    assert (probs.double().sum(1) - 1.0).abs().max().item() < 1e-4
    with torch.no_grad():
        logits, _ = stage(x)
    rows = list(range(0, B, B // 56)) + [2 * n_cu - 1, 2 * n_cu, B - 1]
    idx = torch.tensor(sorted(set(rows)), device=DEV)
    l64, v64 = EB.reference64(net, x[idx])
    err = EB.row_errors(logits[idx], value[idx], l64, v64)
    bound, e_torch = _err_bound("tower_f16", net, x[idx], l64, v64)
    assert err.max() <= bound, (float(err.max()), bound, e_torch)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        pp, vp = stage.forward_probs(x[perm].contiguous())
    inv = torch.argsort(perm)
    assert torch.equal(pp[inv], probs) and torch.equal(vp[inv], value)


NAN32 = 0x7FC0DEAD  # a quiet float32 NaN with a payload no kernel writes
NAN16 = 0x7E5B      # a quiet fp16 NaN with a payload


def _guarded(rows, cols, dtype, guard=64):
    t = torch.empty((rows + guard, cols), dtype=dtype, device=DEV)
    if dtype == torch.float16:
        t.view(torch.int16).fill_(NAN16)
    else:
        t.view(torch.int32).fill_(NAN32)
    return t


def _guard_intact(t, rows):
    g = t[rows:]
    bits = g.view(torch.int16) if t.dtype == torch.float16 else g.view(torch.int32)
    return bool((bits == (NAN16 if t.dtype == torch.float16 else NAN32)).all())


def test_no_writes_past_the_last_row(n_cu, bases, monkeypatch):
    """bo_nn_tower_forward (tower output and fused head planes), bo_nn_heads and bo_nn_heads_f16 with output buffers of B rows plus
    64 guard rows holding a NaN bit pattern: after the launches the guard rows hold it still, and every row below B was written.
    Batches that do not fill the last pass: B = 2 x slots + 37 for the one-board routes, an odd B with its tail board on the third pass
    for the fp16 tower.  No status word was set (check_overflow)."""
    from betaone_amd import engine as E

    # (both fill patterns are NaNs: a row below B that a launch left unwritten fails the isnan / isfinite checks below)
    assert torch.tensor([NAN32], dtype=torch.int32).view(torch.float32).isnan().all()
    assert torch.tensor([NAN16], dtype=torch.int16).view(torch.float16).isnan().all()
    lib = E.load_hip_library()
    stream = torch.cuda.current_stream().cuda_stream
    for conv, size, env in (("tower", (2, 1, 64), {}), ("tower", (2, 1, 128), {}), ("tower_wg", (2, 1, 128), {}),
                            ("tower_split", (2, 1, 128), {"BETAONE_SPLIT_TILE": "16"}), ("tower_split", (2, 1, 128), {"BETAONE_SPLIT_TILE": "32"}),
                            ("tower_split", (1, 1, 256), {}), ("tower_f16", (2, 1, 128), {"BETAONE_F16_TILE": "16"}),
                            ("tower_f16", (2, 1, 128), {"BETAONE_F16_TILE": "32"}), ("tower_f16", (1, 1, 256), {"BETAONE_F16_TILE": "16"}),
                            ("tower_f16", (1, 1, 256), {"BETAONE_F16_TILE": "32"})):
        _, fused = _stage(conv, size, env, monkeypatch)
        for k in env:
            monkeypatch.delenv(k)  # (read when the stage was built: the next one gets only its own)
        S = EB.slots(conv, size[2], n_cu)
        B = 2 * (2 * S + 1) - 1 if conv == "tower_f16" else 2 * S + 37
        what = (conv, size, env, B)
        x = EB.make_rows(bases, B, seed=B + 2)
        c = size[2]
        y = pa = pb = None
        if conv == "tower_f16":
            pa, pb = _guarded(B, 2 * 64, torch.float16), _guarded(B, 32 * 64, torch.float16)
        else:
            y = _guarded(B, c * 64, torch.float32)
            if conv in ("tower_wg", "tower_split"):
                pa, pb = _guarded(B, 2 * 64, torch.float32), _guarded(B, 32 * 64, torch.float32)
        rc = lib.bo_nn_tower_forward(fused._tower, x.data_ptr(), y.data_ptr() if y is not None else None,
                                     pa.data_ptr() if pa is not None else None, pb.data_ptr() if pb is not None else None, B, stream)
        assert rc == 0, what
        torch.cuda.synchronize()
        for t in (y, pa, pb):
            if t is not None:
                assert _guard_intact(t, B), what
                assert not t[:B].isnan().any(), what  # (every row below B written; the tower output and ReLU'd planes have no NaN)
        if y is not None:
            with torch.no_grad():
                assert torch.equal(y[:B].reshape(B, c, 8, 8), fused._tower_forward(x)), what
        fused.check_overflow()
        if pa is None:
            continue
        # the heads on these planes: bo_nn_heads (float32 planes, or fp16 planes with flag 2), and bo_nn_heads_f16 on fp16 planes
        f16 = pa.dtype == torch.float16
        for kind, call, n_scr in [("heads", lib.bo_nn_heads, 4096)] + ([("heads_f16", lib.bo_nn_heads_f16, 20)] if f16 else []):
            wp, w1 = (fused.policy_fc_h, fused.value_fc1_h) if kind == "heads_f16" else (fused.policy_fc, fused.value_fc1)
            for probs in (0, 1):  # (fresh NaN-filled buffers for each launch)
                out, value = _guarded(B, 4672, torch.float32), _guarded(B, 1, torch.float32)
                scr = _guarded(n_scr * B, 1, torch.float32)  # (value_fc1 partial sums / softmax statistics: n_scr floats per row)
                flags = probs | (2 if f16 and kind == "heads" else 0)
                rc = call(pa.data_ptr(), pb.data_ptr(), wp.weight.data_ptr(), fused.policy_fc.bias.data_ptr(), w1.weight.data_ptr(),
                          fused.value_fc1.bias.data_ptr(), fused.value_fc2.weight.data_ptr(), fused.value_fc2.bias.data_ptr(),
                          out.data_ptr(), value.data_ptr(), scr.data_ptr(), B, flags, stream)
                assert rc == 0, (what, kind)
                torch.cuda.synchronize()
                assert _guard_intact(out, B) and _guard_intact(value, B) and _guard_intact(scr, n_scr * B), (what, kind, probs)
                assert torch.isfinite(out[:B]).all() and torch.isfinite(value[:B]).all(), (what, kind, probs)
        fused.check_overflow()
