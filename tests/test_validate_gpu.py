"""GPU tests of held-out validation on the MI355X: the cases of tests/metrics_cases.py through the gfx950 kernels of
csrc/bo_metrics.h -- float32 and fp16 logits at every shape, all nine dtype pairs at one -- the rows that drop out, accumulation, the
count columns against the file under tests/golden that the emulator test compares with too, and evaluate() on a side stream and with
its metrics call captured in a graph against the eager result, bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
import metrics_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = MC.cases()
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
GOLDEN = os.path.join(MC.ROOT, "tests", "golden", "validate_counts.json")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_on_the_gpu(case):
    for pair in ((F32, F32), (F16, F16)):
        worst = MC.check_case(case, pair, DEV)
        print(f"RATIO gpu {case.name} {LC.short(pair[0])}/{LC.short(pair[1])} " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("pair", LC.PAIRS, ids=lambda p: f"{LC.short(p[0])}-{LC.short(p[1])}")
def test_every_dtype_pair_at_one_shape_on_the_gpu(pair):
    MC.check_case(MC.pairs_case(), pair, DEV)


@pytest.mark.parametrize("case", MC.dropout_cases(), ids=lambda c: c.name)
def test_rows_that_drop_out_on_the_gpu(case):
    for pair in ((F32, F32), (F16, BF16), (BF16, F16)):
        MC.check_dropout(case, pair, DEV)


def test_accumulation_on_the_gpu():
    for name, pair in (("n65_W2_nb65", (F32, F32)), ("n130_W64_nb65", (F16, F32)), ("n130_W2_nb3", (BF16, F16)), ("n64_W2_nb1", (F16, F16))):
        MC.check_halves(next(c for c in CASES if c.name == name), pair, DEV)


def test_the_golden_counts_on_the_gpu():
    want = json.load(open(GOLDEN))
    case = next(c for c in CASES if c.name == want["case"])
    _, accum = MC.raw_metrics(*MC.cast(case, (F32, F32), DEV), case.n_buckets)
    assert MC.golden_counts(accum[:case.n_buckets].cpu().numpy()) == want["counts"]


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


def test_the_metrics_call_on_a_side_stream_and_under_a_graph_matches_eager():
    from betaone_amd import validate as V

    case = next(c for c in CASES if c.name == "n130_W2_nb3")
    t = MC.cast(case, (F16, F32), DEV)
    eager = V.MetricsAccumulator(case.n_buckets, DEV)
    eager.add(*t[:5], q=t[5], bucket=t[6])
    want = eager.sums()
    torch.cuda.synchronize()
    # a side stream
    side = V.MetricsAccumulator(case.n_buckets, DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side.add(*t[:5], q=t[5], bucket=t[6])
    s.synchronize()
    assert np.array_equal(side.sums().view(np.uint64), want.view(np.uint64))
    # the call captured in a graph and replayed twice: the accumulator holds twice the eager sums, the counts exactly
    graphed = V.MetricsAccumulator(case.n_buckets, DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.add(*t[:5], q=t[5], bucket=t[6])
    graphed.reset()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(graphed.sums().view(np.uint64), want.view(np.uint64))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(graphed.sums(), 2.0 * want)


def test_evaluate_a_net_on_the_gpu_restores_the_mode_and_a_side_stream_matches():
    """evaluate() end to end on the device over the records of a few short self-play games: the phase buckets add up, amp and float32
    agree roughly, a model in train mode stays in train mode, and the pass on a side stream is the eager pass bit for bit."""
    from betaone_amd import records as R
    from betaone_amd import validate as V
    from betaone_amd.rollout import Rollout

    net = _net(1, 0, 16)
    ro = Rollout(net.eval(), 4, num_simulations=16, mcts_batch_size=8, device=DEV, rng_mode="native", max_game_moves=6)
    ro.start_games(list(range(4)), list(range(4)), list(range(4)))
    fins = []
    for _ in range(12):
        ro.play_ply(on_finished=fins.append)
        if len(fins) >= 4:
            break
    ro.close()
    assert fins
    buf = R.GpuReplayBuffer(1024, device=DEV, pi_width=2)
    buf.add(fins)
    index = np.arange(len(buf))
    net.train()
    a = V.evaluate(net, buf, index, batch=8, amp=True, buckets="phase")
    assert net.training
    b = V.evaluate(net, buf, index, batch=5, amp=False)
    assert a["overall"]["records"] == b["overall"]["records"] == len(buf) and sum(k["records"] for k in a["buckets"]) == len(buf)
    assert a["overall"]["bad_rows"] == 0 and abs(a["overall"]["policy_ce"] - b["overall"]["policy_ce"]) < 0.05
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = V.evaluate(net, buf, index, batch=5, amp=False)
    assert c["overall"] == b["overall"]
    buf.close()
