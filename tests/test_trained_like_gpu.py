"""GPU tests of the evaluate stage on nets whose WEIGHTS look trained (tests/trained_like.py: BatchNorm statistics spread over five
decades, per-layer split_scale exponents 6 and more apart, dead and constant channels, SE gates at 0 / 0.5 / 1, sharp policy logits,
values deep in both tanh tails, activations at the edge of the fp16 range) -- every other test of the stage runs hash or default
initialised nets, on which all layers carry one scale and the heads sit in their linear part.

  a. every route against the float64 net (logits, value, probabilities) on every family;
  b. the head kernels on their own (bo_nn_heads flags 0, 1, 1|2, bo_nn_heads_f16, bo_nn_heads_pair) at sharp logits, 33 and 65 rows;
  c. the saturation flag of the split-precision routes 10 % below and above 65504;
  d. two nets of different exponents in one launch (PairedNet, route pair:tower_split), bit for bit against each net alone.

Bounds (none is taken from a kernel's output).  Logits and value: the form of test_evaluate_batches_gpu._err_bound with e_torch =
torch's own GPU evaluation of the same net in the same test -- float32 routes 4 * max(e_torch, e_design) + 1e-5 * max(1, max |l64|),
e_design (the float64 model of the split-precision operand format, trained_like.split_model) counted for the split-precision routes
only and the 1e-5 floor relative because these logits are no longer of order 1; fp16 tower max(3 * e_torch16, 4e-3 * max(1, max |l64|)).
One more reference-side term stands in the float32 max(): e_value = trained_like.value_rounding_rows, one float32 rounding at the
magnitude of value_fc2's operands.  It is 1e-7 everywhere but on the sharp heads' row that stays in the tanh's linear part, where
value_fc2.bias cancels ~300 of the dot product: every float32 route (torch's included) is 1e-5 .. 2e-5 off float64 there, which only
shows on sharp_flat, whose logits are exact (tower_64 and tower_b1 split at 64 filters: 2.1e-5 against 4 x e_torch + 1e-5 = 1.9e-5).
sharp_heads' 16 actions with a bias of -1e4 are held to the same form on their own (their float32 ulp is 1e-3).  Probabilities: 2e-6
absolute, 1e-5 relative where the float64 value is >= 1e-6, rows summing to 1 within 1e-5 (the numbers of
test_fused_heads_kernel_matches_torch and test_in_kernel_softmax_close_to_torch) against the float64 softmax of the logits the route
itself returned -- as in those two tests: the softmax is what these numbers bound; a logit error d moves a probability by up to 2 d p, so
against the softmax of the float64 logits the probabilities get the logits' own bound (2e-6 + 2 x bound).  Values in the tanh tails
(|pre-tanh| >= 9 in float64): within 5e-6 of float64 (test_fused_heads_kernel_matches_torch's value tolerance)."""
import copy
import ctypes as C

import pytest
import torch

import test_evaluate_batches_gpu as TB
import trained_like as TL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (id, conv, size, environment, f32_pipe): the twelve routes of test_evaluate_batches_gpu, the per-layer small-batch route, and the
# one-launch tower on both matrix pipes
ROUTES = [r + (None,) for r in TB.ROUTES]
ROUTES += [("mfma_small_%d" % s[2], "mfma_small", s, {}, None) for s in TL.SIZES]
ROUTES += [("tower_b1_%s_%d" % ("f32" if f else "split", s[2]), "tower_b1", s, {}, f) for f in (True, False) for s in TL.SIZES]
ROUTE_IDS = [r[0] for r in ROUTES]


def _is_split(conv, f32_pipe):
    return conv == "tower_split" or (conv == "tower_b1" and f32_pipe is False)


def _stage(net_cpu, conv, env, f32_pipe, monkeypatch):
    from betaone_amd.fused_net import FusedPolicyValueNet

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net = copy.deepcopy(net_cpu).to(DEV).eval()
    fused = FusedPolicyValueNet(net, conv=conv, f32_pipe=f32_pipe).to(DEV)
    assert fused.layout == "nchw+" + conv
    if "BETAONE_SPLIT_TILE" in env:
        assert fused.split_tile == int(env["BETAONE_SPLIT_TILE"])
    if "BETAONE_F16_TILE" in env:
        assert fused.f16_tile == int(env["BETAONE_F16_TILE"])
    if conv == "tower_b1":
        assert fused.b1_precision.startswith("f32" if f32_pipe else "f16 pairs")
    return net, fused


def _torch_outputs(conv, net, x):
    """torch's own evaluation of the net on the GPU: float32, or (fp16 tower) the folded net in half precision."""
    with torch.no_grad():
        if conv == "tower_f16":
            l, v = net.for_inference(dtype=torch.float16, channels_last=False)(x.half())
            return l.float(), v.float()
        return net(x)


def _bound(conv, e_torch, e_design, scale, e_value=0.0):
    if conv == "tower_f16":
        return max(3.0 * e_torch, 4e-3 * max(1.0, scale))
    return 4.0 * max(e_torch, e_design, e_value) + 1e-5 * max(1.0, scale)


def _check_logits_value(what, conv, split, family, net, logits, value, x, ref, rows):
    """Logits / value of `rows` of the reference against float64 within the bound of the module docstring -> (err, e_torch, bound)."""
    l64, v64, cols = ref.l64[rows], ref.v64[rows], ref.cols
    lt, vt = _torch_outputs(conv, net, x)
    e_design = float(ref.e_design_rows[rows].max()) if split else 0.0
    e_torch = TL.out_error(lt, vt, l64, v64, cols)
    err = TL.out_error(logits, value, l64, v64, cols)
    e_value = float(ref.e_value_rows[rows].max())
    bound = _bound(conv, e_torch, e_design, float(l64[:, cols].abs().max()), e_value)
    ref_e = max(e_torch, e_design, e_value)
    print(f"[trained-like-gpu] {what} err {err:.3g} e_torch {e_torch:.3g} e_design {e_design:.3g} e_value {e_value:.3g} ratio {err / ref_e if ref_e else float('nan'):.2f} "
          f"bound {bound:.3g} max|l64| {float(l64[:, cols].abs().max()):.4g}")
    assert torch.isfinite(logits).all() and torch.isfinite(value).all(), what
    assert err <= bound, (what, err, bound, e_torch, e_design, e_value)
    assert float(value.abs().max()) <= 1.0, what
    if not bool(cols.all()):  # the actions with a bias of -1e4, on their own
        rest = ~cols
        zero_v = torch.zeros_like(v64)
        e_t = TL.out_error(lt, zero_v, l64, zero_v, rest)
        e_k = TL.out_error(logits, zero_v, l64, zero_v, rest)
        b = _bound(conv, e_t, 0.0, float(l64[:, rest].abs().max()))
        print(f"[trained-like-gpu] {what} biased actions err {e_k:.3g} e_torch {e_t:.3g} bound {b:.3g}")
        assert e_k <= b, (what, "biased actions", e_k, b, e_t)
    tails = (ref.pre_tanh[rows].abs() >= 9.0).nonzero().flatten()
    if tails.numel():
        e_tail = float((value.detach().cpu().double().reshape(-1, 1)[tails] - v64[tails]).abs().max())
        assert e_tail <= 5e-6, (what, "value in the tanh tails", e_tail)
    return err, e_torch, bound


def _check_probs(what, family, probs, logits, l64, cols, bound):
    """forward_probs' rows against the float64 softmax (module docstring)."""
    p = probs.detach().cpu().double()
    own = torch.softmax(logits.detach().cpu().double(), 1)
    assert torch.isfinite(probs).all() and bool((probs >= 0).all()), what
    d = (p - own).abs()
    big = own >= 1e-6
    rel = float((d[big] / own[big]).max())
    print(f"[trained-like-gpu] {what} probs abs {float(d.max()):.3g} rel {rel:.3g} sum {float((p.sum(1) - 1.0).abs().max()):.3g}")
    assert float(d.max()) <= 2e-6 and rel <= 1e-5, (what, float(d.max()), rel)
    assert float((p.sum(1) - 1.0).abs().max()) <= 1e-5, what
    assert float((p - torch.softmax(l64, 1)).abs().max()) <= 2e-6 + 2.0 * bound, what
    if family == "sharp_heads":
        assert bool((probs[:, ~cols.to(probs.device)] == 0).all()), (what, "the exponentials of the -1e4 actions underflow to exactly 0")
    if family == "sharp_flat":  # 4672 equal logits: float32(1 / 4672) within one ulp in every entry
        want = torch.tensor([1.0 / 4672.0], dtype=torch.float32).view(torch.int32).item()
        assert int((probs.detach().cpu().view(torch.int32) - want).abs().max()) <= 1, what


def _batches(fused, conv):
    """[(n of the reference sample, rows of it)]: the towers at B = 7; the one-launch tower at 1, 2 and its resident grid."""
    if conv != "tower_b1":
        return [(TL.TOWER_B, list(range(TL.TOWER_B)))]
    m = fused._b1_max
    return [(TL.TOWER_B, [5]), (TL.TOWER_B, [3, 4]), (max(m, 4), list(range(m)))]


@pytest.mark.parametrize("family", TL.ACCURACY_FAMILIES)
@pytest.mark.parametrize("rid,conv,size,env,f32_pipe", ROUTES, ids=ROUTE_IDS)
def test_every_route_matches_the_float64_net_on_trained_like_weights(rid, conv, size, env, f32_pipe, family, monkeypatch):
    """a.  Logits, value and forward_probs of every route on bn_spread, ladder, dead (SE gates all 0.5 / at 0 and 1), sharp_heads and
    its flat-policy copy, within the bounds of the module docstring; nothing flagged by check_overflow."""
    net, fused = _stage(TL.family_net(family, size), conv, env, f32_pipe, monkeypatch)
    split = _is_split(conv, f32_pipe)
    for n, rows in _batches(fused, conv):
        ref = TL.reference(family, size, n)
        x = ref.x[rows].to(DEV).contiguous()
        what = f"{rid} {family} B={len(rows)}"
        with torch.no_grad():
            logits, value = fused(x)
            probs, value_p = fused.forward_probs(x)
        torch.cuda.synchronize()
        fused.check_overflow()
        _, _, bound = _check_logits_value(what, conv, split, family, net, logits, value, x, ref, rows)
        assert torch.equal(value_p.reshape(-1), value.reshape(-1)), what
        _check_probs(what, family, probs, logits, ref.l64[rows], ref.cols, bound)


# ---------------------------------------------------------------- b. the head kernels on their own
@pytest.fixture(scope="module")
def sharp_heads_case():
    """Head planes (float64 trace, 65 rows) and head weights of the sharp_heads net at 128 filters, and of its flat-policy copy."""
    size = (2, 1, 128)
    net, flat = TL.family_net("sharp_heads", size), TL.family_net("sharp_flat", size)
    x = TL.sample_inputs(65)
    t = TL.trace64(net, x)
    cols = TL.free_columns("sharp_heads")
    spread = t["logits"][:, cols].amax(1) - t["logits"][:, cols].amin(1)
    pre = t["pre_tanh"].flatten()
    assert int((spread >= 40.0).sum()) * 2 >= 65 and float(pre.max()) >= 9.0 and float(pre.min()) <= -9.0  # sharp on these rows too
    w = lambda n: [m.detach().float().to(DEV).contiguous() for m in (n.policy_fc.weight, n.policy_fc.bias, n.value_fc1.weight, n.value_fc1.bias,
                                                                    n.value_fc2.weight, n.value_fc2.bias)]
    return t["planes_p"].float(), t["planes_v"].float(), w(net), w(flat), cols


def _heads64(p, v, w):
    """The heads in float64 on the CPU from the operands as the kernel gets them -> (logits, pre-tanh, value [B, 1])."""
    wp, bp, w1, b1, w2, b2 = [t.detach().cpu().double() for t in w]
    logits = p.cpu().double() @ wp.t() + bp
    pre = torch.relu(v.cpu().double() @ w1.t() + b1) @ w2.t() + b2
    return logits, pre.flatten(), torch.tanh(pre).reshape(-1, 1)


def _call_heads(lib, fn, p, v, w, B, flags, n_scr=4096):
    out = torch.full((B, 4672), float("nan"), device=DEV)
    val = torch.full((B, 1), float("nan"), device=DEV)
    scr = torch.empty(n_scr * B, device=DEV)
    rc = fn(p.data_ptr(), v.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), w[4].data_ptr(), w[5].data_ptr(),
            out.data_ptr(), val.data_ptr(), scr.data_ptr(), B, flags, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.bo_last_error()
    torch.cuda.synchronize()
    return out, val


@pytest.mark.parametrize("B", [33, 65])
@pytest.mark.parametrize("kind", ["heads", "heads_f16_planes", "heads_f16"])
def test_head_kernels_at_sharp_logits_match_float64(sharp_heads_case, kind, B):
    """b.  bo_nn_heads (flags 0 and 1; 1 | 2 with fp16 planes) and bo_nn_heads_f16 (fp16 planes and weights; the evaluate stage reaches it
    only above 1024 rows, so this is its sharp-logit test) through the ABI on the sharp_heads net's planes and weights: logit spreads
    of 40 and more, 16 actions at -1e4, values beyond |pre-tanh| = 9; one and two rows past the 32- and 64-row tiles of
    bo_k_heads_policy_h / bo_k_heads_value_h.  Reference: float64 from the operands as the kernel gets them (the rounded planes /
    weights); bounds of (a) with e_torch = torch's GPU evaluation of the same heads in the kernel's precision."""
    from betaone_amd import engine as E

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = E.load_hip_library()
    p64, v64p, w, _, cols = sharp_heads_case
    f16_kernel = kind == "heads_f16"
    p, v = p64[:B].to(DEV), v64p[:B].to(DEV)
    if kind != "heads":
        p, v = p.half(), v.half()
    wk = list(w)
    if f16_kernel:
        wk[0], wk[2] = w[0].half(), w[2].half()
    p, v = p.contiguous(), v.contiguous()
    l64, pre64, val64 = _heads64(p, v, wk)
    with torch.no_grad():  # torch's own heads on the GPU, in the precision of the kernel's matrix products
        if f16_kernel:
            lt = (torch.nn.functional.linear(p, wk[0]).float() + wk[1])
            vt = torch.tanh(torch.relu(torch.nn.functional.linear(v, wk[2]).float() + wk[3]) @ wk[4].t() + wk[5])
        else:
            lt = torch.nn.functional.linear(p.float(), wk[0], wk[1])
            vt = torch.tanh(torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(v.float(), wk[2], wk[3])), wk[4], wk[5]))
    fn, n_scr = (lib.bo_nn_heads_f16, 20) if f16_kernel else (lib.bo_nn_heads, 4096)
    plane_flag = 2 if kind == "heads_f16_planes" else 0
    logits, value = _call_heads(lib, fn, p, v, wk, B, 0 | plane_flag, n_scr)
    probs, value_p = _call_heads(lib, fn, p, v, wk, B, 1 | plane_flag, n_scr)
    what = f"{kind} B={B}"
    scale = float(l64[:, cols].abs().max())
    e_torch = TL.out_error(lt, vt, l64, val64, cols)
    err = TL.out_error(logits, value, l64, val64, cols)
    bound = max(3.0 * e_torch, 4e-3 * max(1.0, scale)) if f16_kernel else 4.0 * e_torch + 1e-5 * max(1.0, scale)
    print(f"[trained-like-gpu] {what} err {err:.3g} e_torch {e_torch:.3g} bound {bound:.3g} max|l64| {scale:.4g}")
    assert torch.isfinite(logits).all() and torch.isfinite(value).all() and err <= bound, (what, err, bound, e_torch)
    zero = torch.zeros_like(val64)
    e_b, e_tb = TL.out_error(logits, zero, l64, zero, ~cols), TL.out_error(lt, zero, l64, zero, ~cols)
    bound_b = max(3.0 * e_tb, 4e-3 * 1e4) if f16_kernel else 4.0 * e_tb + 1e-5 * float(l64[:, ~cols].abs().max())
    assert e_b <= bound_b, (what, "biased actions", e_b, bound_b)
    tails = (pre64.abs() >= 9.0).nonzero().flatten()
    assert tails.numel() >= 2 and float((value.cpu().double()[tails] - val64[tails]).abs().max()) <= 5e-6 and float(value.abs().max()) <= 1.0, what
    assert torch.equal(value_p, value), what
    _check_probs(what, "sharp_heads", probs, logits, l64, cols, bound)


def test_two_net_heads_at_sharp_logits_equal_each_nets_own_rows(sharp_heads_case):
    """b.  bo_nn_heads_pair on the sharp_heads net and its flat-policy copy, rows alternating and in blocks, both orders: every row
    bit for bit what bo_nn_heads returns for that row's net alone (logits, probabilities, value)."""
    from betaone_amd import engine as E

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    lib = E.load_hip_library()
    p64, v64p, w_sharp, w_flat, _ = sharp_heads_case
    stream = torch.cuda.current_stream().cuda_stream
    for B in (33, 65):
        p, v = p64[:B].to(DEV).contiguous(), v64p[:B].to(DEV).contiguous()
        for ws in ((w_sharp, w_flat), (w_flat, w_sharp)):
            alone = [[_call_heads(lib, lib.bo_nn_heads, p, v, w, B, flags) for flags in (0, 1)] for w in ws]
            hw = [E.BoHeadWeights(*[t.data_ptr() for t in w]) for w in ws]
            for sel in (torch.arange(B) % 2, (torch.arange(B) // 3) % 2):
                sel_d = sel.to(torch.int32).to(DEV)
                for flags in (0, 1):
                    out = torch.full((B, 4672), float("nan"), device=DEV)
                    val = torch.full((B, 1), float("nan"), device=DEV)
                    scr = torch.empty(4096 * B, device=DEV)
                    rc = lib.bo_nn_heads_pair(p.data_ptr(), v.data_ptr(), C.byref(hw[0]), C.byref(hw[1]), sel_d.data_ptr(), out.data_ptr(),
                                              val.data_ptr(), scr.data_ptr(), B, flags, stream)
                    assert rc == 0, lib.bo_last_error()
                    torch.cuda.synchronize()
                    for k in (0, 1):
                        rows = (sel == k).nonzero().flatten().to(DEV)
                        assert torch.equal(out[rows], alone[k][flags][0][rows]) and torch.equal(val[rows], alone[k][flags][1][rows]), (B, k, flags)


# ---------------------------------------------------------------- c. the saturation flag at its edge
EDGE_SPLIT = [r for r in ROUTES if _is_split(r[1], r[4]) and not (r[1] == "tower_b1" and r[2][2] == 256)]
EDGE_F32 = [r for r in ROUTES if r[0] in ("tower_wg_128", "tower_128", "tower_64", "mfma_256", "mfma_small_128", "tower_b1_f32_128")]


def _edge_rows(fused, conv):
    """All seven rows (the one-launch tower's grid holds 8 boards at 128 filters, 16 at 64)."""
    assert conv != "tower_b1" or fused._b1_max >= TL.TOWER_B
    return list(range(TL.TOWER_B))


@pytest.mark.parametrize("rid,conv,size,env,f32_pipe", EDGE_SPLIT, ids=[r[0] for r in EDGE_SPLIT])
def test_split_routes_flag_an_activation_ten_percent_above_the_fp16_range_and_none_below(rid, conv, size, env, f32_pipe, monkeypatch):
    """c.  edge_below (the float64 net's largest tower activation = 0.9 x 65504): evaluated within the bound of (a), nothing flagged.
    edge_above (1.1 x 65504, in a layer that is handed on as (hi, lo) pairs): check_overflow raises 'fp16 range'; the report clears
    the flag.  Every activation the kernels compute is within 1e-5 relative of float64, so +-10 % cannot tip either way: a
    saturation constant off by a factor of two (32752, 131008) fails one of the two halves."""
    from betaone_amd import engine as E

    ref = TL.reference("edge_below", size)
    net, fused = _stage(TL.family_net("edge_below", size), conv, env, f32_pipe, monkeypatch)
    rows = _edge_rows(fused, conv)
    x = ref.x[rows].to(DEV).contiguous()
    with torch.no_grad():
        logits, value = fused(x)
    torch.cuda.synchronize()
    fused.check_overflow()
    _check_logits_value(f"{rid} edge_below", conv, True, "edge_below", net, logits, value, x, ref, rows)
    net, fused = _stage(TL.family_net("edge_above", size), conv, env, f32_pipe, monkeypatch)
    with torch.no_grad():
        fused(x)
    torch.cuda.synchronize()
    with pytest.raises(E.EngineError, match="fp16 range"):
        fused.check_overflow()
    fused.check_overflow()  # the flag was cleared by the report


@pytest.mark.parametrize("rid,conv,size,env,f32_pipe", EDGE_F32, ids=[r[0] for r in EDGE_F32])
def test_fp32_pipe_routes_evaluate_beyond_the_fp16_range(rid, conv, size, env, f32_pipe, monkeypatch):
    """c.  edge_above on the routes that carry float32 activations: within the bound of (a), nothing flagged."""
    ref = TL.reference("edge_above", size)
    net, fused = _stage(TL.family_net("edge_above", size), conv, env, f32_pipe, monkeypatch)
    rows = _edge_rows(fused, conv)
    x = ref.x[rows].to(DEV).contiguous()
    with torch.no_grad():
        logits, value = fused(x)
    torch.cuda.synchronize()
    fused.check_overflow()
    _check_logits_value(f"{rid} edge_above", conv, False, "edge_above", net, logits, value, x, ref, rows)


# ---------------------------------------------------------------- d. two nets in one launch
@pytest.mark.parametrize("size", [(2, 1, 128), (1, 1, 256)], ids=["128", "256"])
def test_paired_launch_of_nets_with_different_exponents_equals_each_net_alone(size, monkeypatch):
    """d.  PairedNet on route pair:tower_split with a ladder net and a plain hash net (their split_scale exponents differ in every
    layer but at most one, by 3 and more in four; the pair was only ever tested with two nets of equal exponents): B = 9, sel alternating and in blocks, both orders of the
    nets -- every row, bit for bit, what that row's net returns alone (the class's contract): logits, probabilities, value."""
    from betaone_amd.fused_net import PairedNet

    ea, eb = TL.split_exponents(TL.family_net("ladder", size)), TL.split_exponents(TL.family_net("hash", size))
    assert sum(a != b for a, b in zip(ea, eb)) >= len(ea) - 1 and sum(abs(a - b) >= 3 for a, b in zip(ea, eb)) >= 4, (ea, eb)
    stages = [_stage(TL.family_net(f, size), "tower_split", {}, None, monkeypatch)[1] for f in ("ladder", "hash")]
    x = TL.sample_inputs(9).to(DEV)
    with torch.no_grad():
        alone = [(s(x), s.forward_probs(x)) for s in stages]
    for order in ((0, 1), (1, 0)):
        pair = PairedNet(stages[order[0]], stages[order[1]], batch=9, device=DEV)
        assert pair.route == "pair:tower_split"
        for sel in ([0, 1, 0, 1, 0, 1, 0, 1, 0], [0, 0, 0, 1, 1, 1, 0, 1, 0]):
            sel_d = torch.tensor(sel, dtype=torch.int32, device=DEV)
            with torch.no_grad():
                got = (pair(x, sel_d), pair.forward_probs(x, sel_d))
            torch.cuda.synchronize()
            pair.check_overflow()
            for b, k in enumerate(sel):
                want = alone[order[k]]
                for probs in (0, 1):
                    assert torch.equal(got[probs][0][b], want[probs][0][b]) and torch.equal(got[probs][1][b].reshape(-1), want[probs][1][b].reshape(-1)), \
                        (size, order, sel, "row", b, "net", order[k], "probs" if probs else "logits")
