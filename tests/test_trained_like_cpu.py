"""CPU tests of tests/trained_like.py (the trained-like families of nets tests/test_trained_like_gpu.py runs the evaluate stage on)
and of the host side of the split-precision routes: every family meets its conditions from the float64 trace alone; the float64
model of the split-precision arithmetic costs less than float32 rounding on the benign hash net; the (hi, lo) weight packings
unpack by their documented index formulas to the two-step rounding of s * w; fused_net.split_scale at its edges."""
import math

import numpy as np
import pytest
import torch

import evaluate_batches as EB
import trained_like as TL


@pytest.mark.parametrize("size", TL.SIZES, ids=lambda s: "%d+%dx%d" % s)
@pytest.mark.parametrize("family", list(TL.FAMILIES))
def test_every_family_meets_its_conditions_from_the_float64_trace(family, size):
    """check_conditions on the inputs the GPU tests use; the trace it reads is the net EB.reference64 evaluates (same logits and
    value to float64 rounding); e_design of the family is printed for profiles/evaluate_trained_like.md."""
    net, x = TL.family_net(family, size), TL.sample_inputs()
    fig = TL.check_conditions(family, net, x)
    t = TL.trace64(net, x)
    l64, v64 = EB.reference64(net, x)
    scale = max(1.0, float(l64.abs().max()))
    assert float((t["logits"] - l64).abs().max()) <= 1e-12 * scale and float((t["value"] - v64).abs().max()) <= 1e-12
    if family.startswith("edge"):
        assert fig["edge_layer"] < len(t["acts"]) - 1  # (the maximum is in a layer that another tower layer reads)
    print(f"[trained-like] {family} {size}: e_design {TL.reference(family, size).e_design:.3g} act_max {fig['act_max']:.6g} "
          f"smallest layer {fig['act_min_layer']:.3g} exponents {fig['exponents']}")


def test_sample_inputs_are_as_encoded_with_a_zero_board_and_scaled_rows():
    x = TL.sample_inputs()
    assert x.shape == (TL.TOWER_B, 120, 8, 8) and x.dtype == torch.float32 and TL.TOWER_B % 2 == 1
    assert bool((x[:4] == x[:4].round()).all()) and float(x[:4].max()) > 1.0  # as encoded: counts, not rescaled
    assert float(x[4].abs().max()) == 0.0
    assert not bool((x[5:] == x[5:].round()).all())
    EB.assert_rows_distinct(x)
    assert torch.equal(TL.sample_inputs(16)[-3:], x[-3:]) and torch.equal(TL.sample_inputs(16)[:4], x[:4])


def test_the_plain_hash_net_is_as_benign_as_the_families_are_not():
    """What the trained-like families are for: on the hash net no activation exceeds 2, the logits of a row are within 2 of each
    other, the values of all rows are within 0.05 of each other and below 0.2, and every tower layer carries the same split_scale exponent (+-1)."""
    net, x = TL.family_net("hash", (2, 1, 128)), TL.sample_inputs()
    t = TL.trace64(net, x)
    assert max(t["act_max"]) < 2.0 and float((t["logits"].amax(1) - t["logits"].amin(1)).max()) < 2.0
    assert float(t["value"].max() - t["value"].min()) < 0.05 and float(t["value"].abs().max()) < 0.2  # the tanh's linear part
    e = TL.split_exponents(net)[:-1]
    assert max(e) - min(e) <= 1, e


@pytest.mark.parametrize("size", TL.SIZES, ids=lambda s: "%d+%dx%d" % s)
def test_split_model_costs_less_than_float32_rounding_on_the_hash_net(size):
    """The documented operand format (22-bit (hi, lo) pairs, the lo x lo term dropped) on benign weights: below the same net's float32
    CPU error against float64 (DESIGN section 2 quotes 2.6e-7 for the kernel, which adds its float32 accumulation)."""
    net = TL.family_net("hash", size)
    r = TL.reference("hash", size)
    x, l64, v64, e_design = r.x, r.l64, r.v64, r.e_design
    with torch.no_grad():
        l32, v32 = net(x)
    e32 = TL.out_error(l32, v32, l64, v64)
    lf, vf = TL.split_model(net, x, flush_denormals=True)
    print(f"[trained-like] hash {size}: e_design {e_design:.3g} float32 CPU {e32:.3g} (denormal operands flushed: {TL.out_error(lf, vf, l64, v64):.3g})")
    assert 0.0 < e_design < e32 < 1e-6, (e_design, e32)


def test_ladder_block_weights_differ_by_two_to_the_2e_and_keep_the_function():
    size = (2, 1, 128)
    x = TL.sample_inputs()
    a, b = TL.family_net("bn_spread", size), TL.family_net("ladder", size)
    la, va = EB.reference64(a, x)
    lb, vb = EB.reference64(b, x)
    assert float((la - lb).abs().max()) <= 1e-9 * float(la.abs().max()) and float((va - vb).abs().max()) <= 1e-9
    ea, eb = TL.split_exponents(a), TL.split_exponents(b)
    for i in range(3):  # conv1 of block i: 2^e larger (exponent e smaller), conv2: 2^e smaller
        e = TL.LADDER_E[i % 3]
        assert eb[1 + 2 * i] == ea[1 + 2 * i] - e and eb[2 + 2 * i] == ea[2 + 2 * i] + e, (ea, eb)


# ---------------------------------------------------------------- packing round trips
def _two_step(v64: np.ndarray):
    """hi = RN16(v), lo = RN16(v - hi) in numpy (direct float64 -> fp16 conversions, denormals kept)."""
    hi = v64.astype(np.float16)
    lo = (v64 - hi.astype(np.float64)).astype(np.float16)
    return hi, lo


@pytest.fixture(scope="module")
def ladder_weight():
    """A folded [128, 128, 3, 3] convolution of the ladder net with three small-magnitude output channels and one all-zero one."""
    f = TL.fold32(TL.family_net("ladder", (2, 1, 128)))
    w = f.residual_tower[1].conv2.weight.detach().clone()
    w[3] *= 2.0 ** -14
    w[5] *= 2.0 ** -22
    w[6] *= 2.0 ** -30
    w[7] = 0.0
    return w


def _check_unpacked(got_hi, got_lo, w, s, oc, ic, tap):
    """got_* [...]: the packed halves; oc / ic / tap: index arrays of the same shape by the packing's documented formula."""
    v = w.double().numpy()[oc, ic, tap // 3, tap % 3] * s
    hi, lo = _two_step(v)
    assert np.array_equal(got_hi.view(np.uint16), hi.view(np.uint16)) and np.array_equal(got_lo.view(np.uint16), lo.view(np.uint16))
    both = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(got_hi.astype(np.float64) + got_lo.astype(np.float64), both)
    assert np.all(np.abs(both - v) <= np.abs(v) * 2.0 ** -21 + 2.0 ** -25)
    a = np.abs(lo.astype(np.float64))
    assert ((a > 0) & (a < 2.0 ** -14)).any() and (a[v != 0] == 0).any(), "the weights were to give denormal and zero lo halves"


def test_split16_packing_unpacks_to_the_two_step_rounding(ladder_weight):
    """pack_conv_weight_split16: element (tap, g, ot, hl, lane, i) = split(s * W[16*ot + (lane & 15)][32*g + 8*(lane >> 4) + i][tap])."""
    from betaone_amd.fused_net import pack_conv_weight_split16, split_scale

    w = ladder_weight
    co, ci = w.shape[:2]
    s = split_scale(w)
    p = pack_conv_weight_split16(w, s)
    assert p.dtype == torch.float16 and p.numel() == 2 * w.numel()
    flat = p.reshape(9, ci // 32, co // 16, 2, 64, 8).numpy()
    tap, g, ot, lane, i = np.meshgrid(np.arange(9), np.arange(ci // 32), np.arange(co // 16), np.arange(64), np.arange(8), indexing="ij")
    _check_unpacked(flat[:, :, :, 0], flat[:, :, :, 1], w, s, 16 * ot + (lane & 15), 32 * g + 8 * (lane >> 4) + i, tap)


def test_split32_packing_unpacks_to_the_two_step_rounding(ladder_weight):
    """pack_conv_weight_split (tests/test_abi.py samples 200 elements of a random tensor to 2^-21): every element, exactly.
    Element (step, mt, hl, lane, i) = split(s * W[32*mt + (lane & 31)][16*(step % (c_in/16)) + 8*(lane >> 5) + i][step / (c_in/16)])."""
    from betaone_amd.fused_net import pack_conv_weight_split, split_scale

    w = ladder_weight
    co, ci = w.shape[:2]
    s = split_scale(w)
    flat = pack_conv_weight_split(w, s).reshape(9 * (ci // 16), co // 32, 2, 64, 8).numpy()
    step, mt, lane, i = np.meshgrid(np.arange(9 * (ci // 16)), np.arange(co // 32), np.arange(64), np.arange(8), indexing="ij")
    _check_unpacked(flat[:, :, 0], flat[:, :, 1], w, s, 32 * mt + (lane & 31), 16 * (step % (ci // 16)) + 8 * (lane >> 5) + i, step // (ci // 16))


def test_small_split_packing_unpacks_to_the_two_step_rounding(ladder_weight):
    """pack_conv_weight_small_split: element (ot, tap, g, lane, hl, j) = split(s * W[16*ot + (lane & 15)][16*g + 4*(lane >> 4) + j][tap])."""
    from betaone_amd.fused_net import pack_conv_weight_small_split, split_scale

    w = ladder_weight
    co, ci = w.shape[:2]
    s = split_scale(w)
    p = pack_conv_weight_small_split(w, s)
    assert p.dtype == torch.float16 and p.numel() == 2 * w.numel()
    flat = p.reshape(co // 16, 9, ci // 16, 64, 2, 4).numpy()
    ot, tap, g, lane, j = np.meshgrid(np.arange(co // 16), np.arange(9), np.arange(ci // 16), np.arange(64), np.arange(4), indexing="ij")
    _check_unpacked(flat[:, :, :, :, 0], flat[:, :, :, :, 1], w, s, 16 * ot + (lane & 15), 16 * g + 4 * (lane >> 4) + j, tap)


def test_head_packing_of_the_split_tower_unpacks_and_keeps_its_bytes(ladder_weight):
    """fused_net.pack_head_weight_split (factored out of _build_tower_split): element (mt, st, hl, lane, i) = split(s * Wh[32*mt +
    (lane & 31)][16*st + 8*(lane >> 5) + i]) -- what bo_k_tower_s's head loop reads at ((mt * C/16 + st) * 2 + hl) * 64 + lane; and
    byte for byte what the expression it replaced packed (restated here)."""
    from betaone_amd.fused_net import pack_head_weight_split, split_f16, split_scale

    c = 128
    wh = torch.zeros((64, c))  # 34 head channels padded to two 32-channel tiles
    wh[:34] = ladder_weight[:34, :, 1, 1]
    wh[34:40] = 0.0
    s = split_scale(wh)
    p = pack_head_weight_split(wh, s)
    hi, lo = split_f16(wh.double() * s)
    old = torch.stack([hi, lo], 0).reshape(2, 2, 32, c // 16, 2, 8).permute(1, 3, 0, 4, 2, 5).contiguous()
    assert p.dtype == torch.float16 and p.shape == old.shape and torch.equal(p.view(torch.int16), old.view(torch.int16))
    flat = p.reshape(2, c // 16, 2, 64, 8).numpy()
    mt, st, lane, i = np.meshgrid(np.arange(2), np.arange(c // 16), np.arange(64), np.arange(8), indexing="ij")
    w4 = wh.reshape(64, c, 1, 1).repeat(1, 1, 3, 3)
    _check_unpacked(flat[:, :, 0], flat[:, :, 1], w4, s, 32 * mt + (lane & 31), 16 * st + 8 * (lane >> 5) + i, np.zeros_like(mt))


# ---------------------------------------------------------------- split_scale at its edges
def _f32(v):
    return float(np.float32(v))


def _ulp_steps(v, n):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if n > 0 else -np.inf)))


SCALE_CASES = [1.0, _ulp_steps(1.0, -1), _ulp_steps(1.0, 1), 2.0 ** -9, _ulp_steps(2.0 ** -9, -1), _ulp_steps(2.0 ** -9, 1), 2.0 ** 40,
               _ulp_steps(2.0 ** 40, -1), _f32(0.3), _f32(3.0e38), _f32(3.4028234e38), 2.0 ** -112, _ulp_steps(2.0 ** -112, -1), 2.0 ** -126,
               _f32(1.0e-40), 2.0 ** -149]


@pytest.mark.parametrize("m", SCALE_CASES, ids=lambda m: "%.9g" % m)
def test_split_scale_is_a_power_of_two_whose_inverse_float32_carries(m):
    """s = split_scale(w) for max |w| = m: a power of two; 1 / s is a NORMAL float32 number (the kernels multiply by it: a float32
    denormal may be flushed, 2^-150 and below is 0); 2^14 <= s * m < 2^15 wherever such an s exists (m >= 2^-112), and s = 2^126 with
    s * m < 2^14 below (a float32 denormal m gave s up to 2^163 before the exponent was clamped: 1 / s = 0 in float32, every
    output of the layer its bias)."""
    from betaone_amd.fused_net import split_scale

    assert _f32(m) == m
    w = torch.zeros((4, 4, 3, 3))
    w[1, 2, 0, 1] = -m
    w[2, 1, 1, 1] = m / 3.0
    s = split_scale(w)
    mant, _ = math.frexp(s)
    assert mant == 0.5 and s > 0.0  # a power of two
    inv = np.float32(1.0 / s)
    assert float(inv) * s == 1.0 and float(inv) >= 2.0 ** -126, (m, s)
    if m >= 2.0 ** -112:
        assert 2.0 ** 14 <= s * m < 2.0 ** 15, (m, s)
    else:
        assert s == 2.0 ** 126 and s * m < 2.0 ** 14, (m, s)


def test_split_scale_of_zero_and_non_finite_weights_is_one():
    from betaone_amd.fused_net import split_scale

    assert split_scale(torch.zeros((4, 4, 3, 3))) == 1.0
    for bad in (float("inf"), float("-inf"), float("nan")):
        w = torch.ones((2, 2, 3, 3))
        w[0, 0, 0, 0] = bad
        assert split_scale(w) == 1.0
