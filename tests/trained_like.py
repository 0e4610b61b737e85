"""tests/trained_like.py -- TEST HELPER for tests/test_trained_like_cpu.py and tests/test_trained_like_gpu.py: PolicyValueNets whose
WEIGHTS look like a trained net's, a float64 trace of the net, the conditions each family of nets has to meet (checked on that
trace alone), and a float64 model of the split-precision towers' arithmetic.

Every net starts as fake_model.hash_init_(network.PolicyValueNet().eval()) at one of SIZES and is changed by a family -- a function
(net, x) -> net applied BEFORE any evaluate stage is built, so for_inference() folds what the family set.  Every number comes from
fake_model._splitmix64 (uniform(n, salt)): no torch RNG, no weight files.  The hash nets themselves have BatchNorm buffers var in
[1, 1.5], |mean| <= 0.1, gamma in [0.9, 1.1]: activations <= 1.5, a flat softmax, a value of -0.08 in every row and one split_scale
exponent for the whole tower -- a kernel that read its neighbour layer's scale would pass on them.

Families and their constants (a family that misses a condition of check_conditions gets other constants, never another condition):

  bn_spread    per BatchNorm channel: running_var = 10^(-3 + 5u) (log-uniform in [1e-3, 1e2]); gamma = +-(0.05 + 1.95u), negative
               where a third draw is < 0.25; running_mean = (2u - 1) sqrt(var); beta = u - 0.5.  Then, layer by layer from the input
               on, every convolution's output rows are scaled so that the per-channel standard deviation of its output over the
               sample x equals sqrt(running_var) (what the buffers mean in a trained net).  A BatchNorm then emits about gamma *
               N(mean offset <= 1, 1) + beta.
  ladder       bn_spread, then block i: bn1.weight, bn1.bias *= 2^e_i, conv2.weight *= 2^-e_i, e_i = (+6, -4, +3)[i % 3].  The
               function is unchanged (ReLU is positively homogeneous); the folded conv1 and conv2 of a block differ by 2^(2 e_i).
  dead_half    bn_spread, then in every BatchNorm of C channels the C // 8 channels of lowest hash rank get gamma = 0, beta =
  dead_sat     -(0.1 + 0.4u) (dead behind a ReLU), the next C // 8 gamma = 0, beta = +(0.1 + 0.4u) (constant); the first block's
               conv1.weight = 0 (split_scale's m == 0 branch; the layer's output is its bias).  SE block, `half`: excitation[0].weight
               = -|w| on the channels whose pooled mean is > 0 on every row of x and 0 elsewhere: the hidden ReLU is dead, every
               gate exactly 0.5.  `sat`: excitation[2].weight times 1.05 * 30 / min(q75, -q25) of the pre-sigmoid gates over x: at
               least a quarter of them >= +30 and a quarter <= -30 (sigmoid = 1 and < 1e-13 in float32).
  sharp_heads  bn_spread, then policy_fc.weight *= 60 / median row spread of the logits; policy_fc.bias = -1e4 on the 16 actions
               BIASED (exp underflows to 0, must not become NaN); value_fc2.bias = -(median pre-tanh value over x), then
               value_fc2.weight and .bias *= 12 / min(largest, -smallest centred pre-tanh value): the value reaches far into both
               tails of the tanh and one row stays in its linear part.
  sharp_flat   sharp_heads with policy_fc.weight = 0 and policy_fc.bias = 0.25: a row of 4672 equal logits.
  edge_of_range(net, x, factor)  bn_spread with bn_input's gamma and beta times one t > 0, found by bisection so that the float64
               trace's largest tower activation is factor * 65504 (0.9: below the split towers' saturation constant, 1.1: above).
               Its first block carries one ladder step of 2^EDGE_E = 4 (function unchanged), so that the largest activation is that
               block's conv1 output -- a layer every split route hands on as (hi, lo) pairs.  (Without it the maximum sat in the tower's
               OUTPUT, which the one-launch tower hands to the float32 head convolution unrounded and so, rightly, does not flag.)

Inputs: sample_inputs(n) = the first n - 3 rows of evaluate_batches.random_positions(.., seed=11) as encoded (entries 0 .. 9, not
rescaled), the all-zero board, and two evaluate_batches.make_rows rows (scaled by factors in [0.5, 1))."""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import evaluate_batches as EB
from fake_model import _splitmix64, hash_init_

SIZES = [(2, 1, 128), (1, 1, 256), (2, 1, 64)]
LADDER_E = (6, -4, 3)
BIASED = tuple(range(7, 4672, 4672 // 16))[:16]  # the 16 actions whose policy bias is -1e4 in sharp_heads
F16_MAX = 65504.0  # bo_split4_pos's saturation constant (csrc/bo_tower_s.h)
EDGE_E = 2
TOWER_B = 7  # odd (the fp16 tower's last pair holds one board) and below every grid


def uniform(n: int, salt: int) -> torch.Tensor:
    """n float64 numbers in [0, 1) from the integer hash hash_init_ uses, one stream per salt."""
    with np.errstate(over="ignore"):
        z = _splitmix64(np.uint64(salt) * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64))
    return torch.from_numpy((z >> np.uint64(40)).astype(np.float64) / float(1 << 24))


def hash_net(size):
    """hash_init_(PolicyValueNet().eval()) of size (blocks, SE blocks, filters), float32 on the CPU."""
    from betaone_amd import dropin

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = size
    try:
        return hash_init_(network.PolicyValueNet().eval())
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved


@functools.lru_cache(maxsize=None)
def _bases(n: int):
    return torch.from_numpy(EB.random_positions(n, seed=11))


def sample_inputs(n: int = TOWER_B) -> torch.Tensor:
    """n >= 4 input rows [n, 120, 8, 8] float32 on the CPU (module docstring: Inputs)."""
    assert n >= 4
    b = _bases(64)
    return torch.cat([b[:n - 3], torch.zeros((1, 120, 8, 8)), EB.make_rows(b[32:], 2, seed=5)]).contiguous()


def _bn_pairs(net):
    """[(convolution, its BatchNorm)] from the input to the heads."""
    out = [(net.conv_input, net.bn_input)]
    for blk in net.residual_tower:
        out += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
    return out + [(net.policy_conv, net.policy_bn), (net.value_conv, net.value_bn)]


# ---------------------------------------------------------------- the float64 trace
def trace64(net, x) -> dict:
    """The net in float64 on the CPU (eval mode, unfused BatchNorm), layer by layer: `acts` = the post-ReLU tower activations
    (input layer, then conv1 and the output of every block), `bn` = every BatchNorm's output, `se_pre` / `se_gate` = the SE
    gates before / behind the sigmoid, `planes_p` / `planes_v` = the flattened ReLU'd head planes, `pre_tanh`, `logits`, `value` [B, 1]."""
    ref = copy.deepcopy(net).to("cpu").double().eval()
    x = x.detach().to("cpu").double()
    t = {"acts": [], "bn": [], "se_pre": [], "se_gate": [], "se_pooled": []}

    def bn(m, y):
        y = m(y)
        t["bn"].append(y)
        return y

    with torch.no_grad():
        h = F.relu(bn(ref.bn_input, ref.conv_input(x)))
        t["acts"].append(h)
        for blk in ref.residual_tower:
            y = F.relu(bn(blk.bn1, blk.conv1(h)))
            t["acts"].append(y)
            body = bn(blk.bn2, blk.conv2(y))
            if hasattr(blk, "seblock"):
                pooled = body.mean((2, 3))
                w1, w2 = blk.seblock.excitation[0].weight, blk.seblock.excitation[2].weight
                pre = F.relu(pooled @ w1.t()) @ w2.t()
                t["se_pooled"].append(pooled)
                t["se_pre"].append(pre)
                t["se_gate"].append(torch.sigmoid(pre))
                body = body * torch.sigmoid(pre)[:, :, None, None]
            h = F.relu(body + h)
            t["acts"].append(h)
        p = F.relu(bn(ref.policy_bn, ref.policy_conv(h))).flatten(1)
        v = F.relu(bn(ref.value_bn, ref.value_conv(h))).flatten(1)
        t["planes_p"], t["planes_v"] = p, v
        t["logits"] = ref.policy_fc(p)
        t["pre_tanh"] = ref.value_fc2(F.relu(ref.value_fc1(v)))
        t["value"] = torch.tanh(t["pre_tanh"]).reshape(-1, 1)
    t["act_max"] = [float(a.abs().max()) for a in t["acts"]]
    return t


def fold32(net):
    """The BatchNorm-folded float32 net the evaluate stages are built from (on the CPU)."""
    return copy.deepcopy(net).to("cpu").float().eval().for_inference(dtype=torch.float32, channels_last=False)


def tower_convs(folded):
    out = [folded.conv_input]
    for blk in folded.residual_tower:
        out += [blk.conv1, blk.conv2]
    return out


def split_exponents(net) -> list:
    """log2 of fused_net.split_scale of every folded tower layer, then of the joint head convolution."""
    from betaone_amd.fused_net import split_scale

    f = fold32(net)
    ws = [c.weight for c in tower_convs(f)] + [torch.cat([f.policy_conv.weight, f.value_conv.weight], 0)]
    return [int(round(np.log2(split_scale(w.detach())))) for w in ws]


# ---------------------------------------------------------------- families
def bn_spread(net, x):
    net = copy.deepcopy(net).to("cpu").double().eval()
    with torch.no_grad():
        for k, (_, bn) in enumerate(_bn_pairs(net)):
            c = bn.num_features
            var = 10.0 ** (-3.0 + 5.0 * uniform(c, 10 + k))
            g = (0.05 + 1.95 * uniform(c, 40 + k)) * torch.where(uniform(c, 70 + k) < 0.25, -1.0, 1.0)
            bn.running_var.copy_(var)
            bn.weight.copy_(g)
            bn.running_mean.copy_((2.0 * uniform(c, 100 + k) - 1.0) * var.sqrt())
            bn.bias.copy_(uniform(c, 130 + k) - 0.5)
        xd = x.double()
        for conv, bn in _bn_pairs(net):  # calibrate: std of every convolution's output channel over x = sqrt(running_var)
            got = {}
            h = conv.register_forward_hook(lambda m, i, o: got.__setitem__("o", o))
            net(xd)
            h.remove()
            sd = got["o"].transpose(0, 1).flatten(1).std(1).clamp_min(1e-12)
            conv.weight.mul_((bn.running_var.sqrt() / sd)[:, None, None, None])
    return net.float()


def ladder(net, x):
    net = bn_spread(net, x)
    with torch.no_grad():
        for i, blk in enumerate(net.residual_tower):
            e = LADDER_E[i % 3]
            blk.bn1.weight.mul_(2.0 ** e)
            blk.bn1.bias.mul_(2.0 ** e)
            blk.conv2.weight.mul_(2.0 ** -e)
    return net


def dead_plan(c: int, k: int):
    """(dead channels, constant channels) of BatchNorm number k with c channels: c // 8 each, by hash rank."""
    order = torch.argsort(uniform(c, 200 + k))
    return order[:c // 8], order[c // 8:2 * (c // 8)]


def dead(net, x, se: str):
    net = bn_spread(net, x)
    with torch.no_grad():
        for k, (_, bn) in enumerate(_bn_pairs(net)):
            c = bn.num_features
            d, p = dead_plan(c, k)
            mag = (0.1 + 0.4 * uniform(c, 230 + k)).float()
            bn.weight[d] = 0.0
            bn.bias[d] = -mag[d]
            bn.weight[p] = 0.0
            bn.bias[p] = mag[p]
        net.residual_tower[0].conv1.weight.zero_()
        for j, blk in enumerate(b for b in net.residual_tower if hasattr(b, "seblock")):
            t = trace64(net, x)  # (after the changes above, and after the SE blocks in front of this one)
            w1, w2 = blk.seblock.excitation[0].weight, blk.seblock.excitation[2].weight
            if se == "half":
                pos = (t["se_pooled"][j] > 0).all(0)
                w1.copy_(torch.where(pos[None, :], -w1.abs(), torch.zeros_like(w1)))
            else:
                pre = t["se_pre"][j].flatten()
                q75, q25 = float(torch.quantile(pre, 0.75)), float(torch.quantile(pre, 0.25))
                assert q75 > 0.0 > q25, (q25, q75)
                w2.mul_(1.05 * 30.0 / min(q75, -q25))
    return net


def sharp_heads(net, x):
    net = bn_spread(net, x)
    with torch.no_grad():
        l = trace64(net, x)["logits"]
        net.policy_fc.weight.mul_(60.0 / float((l.amax(1) - l.amin(1)).median()))
        net.policy_fc.bias[list(BIASED)] = -1.0e4
        pre = trace64(net, x)["pre_tanh"].flatten()
        net.value_fc2.bias.sub_(float(pre.median()))
        cen = pre - pre.median()
        k = 12.0 / min(float(cen.max()), -float(cen.min()))
        net.value_fc2.weight.mul_(k)
        net.value_fc2.bias.mul_(k)
    return net


def sharp_flat(net, x):
    net = sharp_heads(net, x)
    with torch.no_grad():
        net.policy_fc.weight.zero_()
        net.policy_fc.bias.fill_(0.25)
    return net


def edge_of_range(net, x, factor: float):
    """bn_spread with bn_input's gamma and beta times t: the float64 trace's largest tower activation = factor * 65504 within 1e-9
    relative (bisection over log t; the maximum grows with t)."""
    base = bn_spread(net, x)
    with torch.no_grad():  # one ladder step of 2^EDGE_E in the first block: its conv1 output is the tower's largest layer
        blk = base.residual_tower[0]
        blk.bn1.weight.mul_(2.0 ** EDGE_E)
        blk.bn1.bias.mul_(2.0 ** EDGE_E)
        blk.conv2.weight.mul_(2.0 ** -EDGE_E)

    def scaled(t):
        n = copy.deepcopy(base)
        with torch.no_grad():
            n.bn_input.weight.mul_(t)
            n.bn_input.bias.mul_(t)
        return n

    # (the scaled parameters are float32: search over the float32 t the net will really carry)
    target = factor * F16_MAX
    lo, hi = 0.0, 24.0  # log2 t
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if max(trace64(scaled(float(np.float32(2.0 ** mid))), x)["act_max"]) < target:
            lo = mid
        else:
            hi = mid
    return scaled(float(np.float32(2.0 ** (hi if factor > 1.0 else lo))))


FAMILIES = {
    "bn_spread": bn_spread,
    "ladder": ladder,
    "dead_half": lambda net, x: dead(net, x, "half"),
    "dead_sat": lambda net, x: dead(net, x, "sat"),
    "sharp_heads": sharp_heads,
    "sharp_flat": sharp_flat,
    "edge_below": lambda net, x: edge_of_range(net, x, 0.9),
    "edge_above": lambda net, x: edge_of_range(net, x, 1.1),
}
ACCURACY_FAMILIES = ["bn_spread", "ladder", "dead_half", "dead_sat", "sharp_heads", "sharp_flat"]


@functools.lru_cache(maxsize=None)
def family_net(family: str, size):
    """The family's net of this size (float32, CPU), built on sample_inputs(); 'hash' = the plain hash net.  Cached: do not change it."""
    net = hash_net(size)
    return net if family == "hash" else FAMILIES[family](net, sample_inputs()).eval()


# ---------------------------------------------------------------- conditions
def check_conditions(family: str, net, x) -> dict:
    """Assert, from the float64 trace of `net` on x alone, what the family is for; returns the figures (for the profile)."""
    t = trace64(net, x)
    l, v = t["logits"], t["value"]
    assert torch.isfinite(l).all() and torch.isfinite(v).all() and all(torch.isfinite(a).all() for a in t["acts"]), family
    fig = {"act_max": max(t["act_max"]), "act_min_layer": min(t["act_max"]), "exponents": split_exponents(net)}
    if family in ("bn_spread", "ladder", "dead_half", "dead_sat"):
        assert 4.0 <= fig["act_max"] <= 16384.0, (family, t["act_max"])
        assert fig["act_min_layer"] >= 2.0 ** -6, (family, t["act_max"])
    if family == "ladder":
        e = fig["exponents"][:-1]
        assert len(set(e)) >= 3 and max(abs(a - b) for a, b in zip(e, e[1:])) >= 6, e
    if family in ("sharp_heads", "sharp_flat"):
        free = torch.ones(l.shape[1], dtype=torch.bool)
        if family == "sharp_heads":
            free[list(BIASED)] = False
            spread = l[:, free].amax(1) - l[:, free].amin(1)
            assert int((spread >= 40.0).sum()) * 2 >= l.shape[0], spread
            assert float(torch.softmax(l, 1)[:, ~free].max()) < 1e-300
            fig["spread"] = float(spread.max())
        else:
            assert bool((l == l[:, :1]).all())
        assert float(l[:, free].abs().max()) <= 200.0, float(l[:, free].abs().max())
        pre = t["pre_tanh"].flatten()
        assert float(pre.max()) >= 9.0 and float(pre.min()) <= -9.0 and float(v.abs().min()) < 0.5, pre
        fig["pre_tanh"] = (float(pre.min()), float(pre.max()))
    if family in ("dead_half", "dead_sat"):
        pairs = _bn_pairs(net)
        assert len(pairs) == len(t["bn"])
        for k, ((_, bn), y) in enumerate(zip(pairs, t["bn"])):
            c = bn.num_features
            flat = y.transpose(0, 1).flatten(1)
            const = (flat == flat[:, :1]).all(1)
            if k == 1:  # the first block's bn1 behind the all-zero conv1: every channel is its bias
                assert bool(const.all()), k
                continue
            assert int((const & (flat[:, 0] < 0)).sum()) == int(const[dead_plan(c, k)[0]].sum()) == c // 8, k
            assert int((const & (flat[:, 0] > 0)).sum()) == int(const[dead_plan(c, k)[1]].sum()) == c // 8, k
        assert split_exponents(net)[1] == 0 and float(net.residual_tower[0].conv1.weight.detach().abs().max()) == 0.0
        assert len(t["se_gate"]) >= 1
        for g, pre in zip(t["se_gate"], t["se_pre"]):
            if family == "dead_half":
                assert bool((g == 0.5).all())
            else:
                assert float((pre >= 30.0).double().mean()) >= 0.25 and float((pre <= -30.0).double().mean()) >= 0.25
                assert float(g.float().max()) == 1.0 and float(g.min()) < 1e-13
    if family in ("edge_below", "edge_above"):
        want = (0.9 if family == "edge_below" else 1.1) * F16_MAX
        assert abs(fig["act_max"] - want) <= 1e-6 * want, (fig["act_max"], want)
        # the layer that holds the maximum hands its output to another tower layer (every split route stages and checks it there)
        fig["edge_layer"] = int(np.argmax(t["act_max"]))
    return fig


# ---------------------------------------------------------------- the split-precision model
def _halves(v, flush: bool):
    """(hi, lo) fp16 halves of float64 v as float64: hi = RN16(v), lo = RN16(v - hi); .half() keeps fp16 denormals, flush=True
    sets them to zero (diagnostic: what a matrix pipe that flushed denormal operands would see)."""
    from betaone_amd.fused_net import split_f16

    hi, lo = split_f16(v.clamp(-F16_MAX, F16_MAX))
    hi, lo = hi.double(), lo.double()
    if flush:
        tiny = 2.0 ** -14
        hi = torch.where(hi.abs() < tiny, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < tiny, torch.zeros_like(lo), lo)
    return hi, lo


def _split_conv(x, w32, flush, padding):
    """csrc/bo_tower_s.h's header: s = split_scale(w); (w_hi, w_lo) = halves of s * w, (x_hi, x_lo) of x; the sum of the three products
    the kernels form -- (w_hi + w_lo)(x_hi + x_lo) minus the dropped w_lo x_lo -- exactly (float64), divided by s."""
    from betaone_amd.fused_net import split_scale

    s = split_scale(w32)
    wh, wl = _halves(w32.double() * s, flush)
    xh, xl = _halves(x, flush)
    return (F.conv2d(xh + xl, wh + wl, padding=padding) - F.conv2d(xl, wl, padding=padding)) / s


def split_model(net, x, flush_denormals: bool = False):
    """(logits, value [B, 1]) in float64 of the split-precision towers' DOCUMENTED arithmetic on this net: the BatchNorm-folded float32
    weights, every tower and head convolution through _split_conv, everything else (bias, SE gate, skip -- kept unrounded, as the
    kernels keep it in float32 registers --, ReLU, the three Linear layers, tanh) in float64.  Written from csrc/bo_tower_s.h's header,
    not from its code: the float32 accumulation and epilogue rounding of the kernels are NOT modelled, so its error against the
    float64 net is what the operand FORMAT costs on that net (e_design)."""
    f = fold32(net)
    x = x.detach().to("cpu").double()
    with torch.no_grad():
        def conv(c, h):
            return _split_conv(h, c.weight.detach(), flush_denormals, c.padding) + c.bias.detach().double()[None, :, None, None]

        h = F.relu(conv(f.conv_input, x))
        for blk in f.residual_tower:
            y = F.relu(conv(blk.conv1, h))
            body = conv(blk.conv2, y)
            if hasattr(blk, "seblock"):
                w1, w2 = blk.seblock.excitation[0].weight.double(), blk.seblock.excitation[2].weight.double()
                body = body * torch.sigmoid(F.relu(body.mean((2, 3)) @ w1.t()) @ w2.t())[:, :, None, None]
            h = F.relu(body + h)
        wh = torch.cat([f.policy_conv.weight, f.value_conv.weight], 0).detach()
        bh = torch.cat([f.policy_conv.bias, f.value_conv.bias], 0).detach().double()
        planes = F.relu(_split_conv(h, wh, flush_denormals, 0) + bh[None, :, None, None])
        n_p = f.policy_conv.out_channels
        p, v = planes[:, :n_p].flatten(1), planes[:, n_p:].flatten(1)
        logits = p @ f.policy_fc.weight.double().t() + f.policy_fc.bias.double()
        h1 = F.relu(v @ f.value_fc1.weight.double().t() + f.value_fc1.bias.double())
        value = torch.tanh(h1 @ f.value_fc2.weight.double().t() + f.value_fc2.bias.double())
    return logits, value.reshape(-1, 1)


def free_columns(family: str) -> torch.Tensor:
    """Bool [4672]: the actions whose logits are of the net's own making (all but sharp_heads' 16 actions with a bias of -1e4, whose
    float32 ulp of 1e-3 is beyond any bound on the others and which are compared on their own)."""
    free = torch.ones(4672, dtype=torch.bool)
    if family == "sharp_heads":
        free[list(BIASED)] = False
    return free


def out_error(logits, value, l64, v64, cols=None, per_row: bool = False):
    """max |difference| over the logits (columns `cols`) and the value, in float64 on the CPU; per_row: a numpy array, one per row."""
    dl = (logits.detach().to("cpu").double() - l64).abs()
    if cols is not None:
        dl = dl[:, cols]
    dv = (value.detach().to("cpu").double().reshape(-1, 1) - v64).abs()
    rows = torch.maximum(dl.amax(1), dv.amax(1)).numpy()
    return rows if per_row else float(rows.max())


def value_rounding_rows(net, t) -> np.ndarray:
    """Per row of the trace t: what ONE float32 rounding at the magnitude of value_fc2's operands moves the value by,
    2^-24 * (sum_i |w_i h_i| + |b|) * tanh'(pre-tanh), in float64.  No float32 evaluation of the value head, in whatever order it
    sums, is closer than this to float64 in general (the standard bound is gamma_257 times the same magnitude); it is 1e-7 on every
    family but the sharp heads, where value_fc2.bias cancels a common part of ~300 of the dot product to leave the row that stays
    in the tanh's linear part: there it is 2e-5 .. 4e-5 on that row, and the logits of sharp_flat are exact, so nothing larger hides it."""
    ref = copy.deepcopy(net).to("cpu").double().eval()
    with torch.no_grad():
        h1 = F.relu(ref.value_fc1(t["planes_v"]))
        mag = (h1 * ref.value_fc2.weight.flatten()).abs().sum(1) + ref.value_fc2.bias.abs()
        return (2.0 ** -24 * mag * (1.0 - torch.tanh(t["pre_tanh"].flatten()) ** 2)).numpy()


class Reference:
    """family_net(family, size) on sample_inputs(n): x, EB.reference64's (l64, v64), the trace's pre_tanh [n], the split model's error
    against (l64, v64) per row over the free columns (e_design_rows) and at most (e_design), and value_rounding_rows (e_value_rows)."""

    def __init__(self, family, size, n):
        net = family_net(family, size)
        self.x = sample_inputs(n)
        self.l64, self.v64 = EB.reference64(net, self.x)
        t = trace64(net, self.x)
        self.pre_tanh = t["pre_tanh"].flatten()
        self.e_value_rows = value_rounding_rows(net, t)
        ls, vs = split_model(net, self.x)
        self.cols = free_columns(family)
        self.e_design_rows = out_error(ls, vs, self.l64, self.v64, self.cols, per_row=True)
        self.e_design = float(self.e_design_rows.max())


@functools.lru_cache(maxsize=None)
def reference(family: str, size, n: int = TOWER_B) -> Reference:
    """Cached: do not change its tensors."""
    return Reference(family, size, n)
