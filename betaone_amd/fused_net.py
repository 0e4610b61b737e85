"""
betaone_amd/fused_net.py -- the evaluate stage with hand-written fused epilogues.

Same function as PolicyValueNet.forward (/root/reference/network.py:167-198) in eval mode: BatchNorm is folded into
the convolutions and every conv is followed by (or fused with) a gfx950 epilogue instead of the 3-8 separate
elementwise launches PyTorch issues (bias, ReLU, residual add, SE pooling / FCs / sigmoid / scale).  Two variants:

  conv="miopen": the 3x3 convolutions stay in MIOpen (fp32 Winograd asm kernel under PyTorch-ROCm), each followed
                 by ONE kernel from csrc/bo_nn_fused.h;
  conv="mfma":   the 3x3 convolutions run in csrc/bo_conv.h (direct implicit GEMM on the fp32 matrix cores, bias /
                 ReLU / residual fused into its epilogue); SE blocks add csrc/bo_nn_fused.h's SE kernel.

  conv="mfma_small": the small-batch form of "mfma" (bo_k_conv3x3_small: a board's layer is spread over (c_out/16) x 4
                 workgroups) for uci.py's single-position searches (BASELINE.json configs[3]).
  conv="tower_b1": the whole tower of ONE board (up to 256 / ((filters/16)*4) boards) as ONE launch of the same (c_out/16) x 4 workgroups
                 per board, the layers handed over inside the launch (csrc/bo_tower_b1.h) instead of one launch per layer: uci.py's
                 single-position searches (BASELINE.json configs[3]); larger batches fall back to "mfma_small" launches.
  conv="tower":  input conv + all residual blocks are ONE persistent kernel that keeps each board's activations in
                 LDS (csrc/bo_tower.h); 64 or 128 filters.
  conv="tower_wg": the same with Winograd F(2x2,3x3) convolutions (csrc/bo_tower_wg.h), 2.25x fewer MFMA cycles.
  conv="tower_split": float32 in and out on the fp16 matrix pipe (csrc/bo_tower_s.h): weights and activations as (hi, lo)
                 fp16 pairs, three MFMAs per product, float32 accumulation; 128 or 256 filters, one board per workgroup.
  conv="tower_f16": fp16 weights/activations, fp32 accumulation (csrc/bo_tower_h.h), 128 or 256 filters, two boards
                 per workgroup; the evaluate stage of BASELINE.json configs[4].  Takes the engine's float32 planes.

NCHW float32 only; other dtypes/layouts use PolicyValueNet.for_inference().
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

import copy
import ctypes as C
import dataclasses
import math
import os

import numpy as np

from . import engine as E


MFMA_CONV_SHAPES = {(120, 64), (64, 64), (120, 128), (128, 128), (120, 256), (256, 256)}


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[c_out, c_in, 3, 3] -> [tap 9][c_in/8][c_out][k 2][e 4], element = W[oc][8*t4 + 2*e + k][tap]: the A fragments
    of four consecutive 32x32x2 MFMA K-steps as one 16-byte load per lane (csrc/bo_conv.h)."""
    co, ci = w.shape[0], w.shape[1]
    return w.reshape(co, ci // 8, 4, 2, 9).permute(4, 1, 0, 3, 2).contiguous()


_WG_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def winograd_k_order(c_out: int, c_in: int) -> list:
    """Input channel of (K-step, row k) of a BO_TOWER_WINOGRAD layer, flattened [step][k] (include/betaone_engine.h).
    128 filters: K-step 4c + sl covers channels 16*(4*(c & 1) + sl) + 4*(c >> 1) + k -- the four channels that wave
    4*(c & 1) + sl of the kernel produced itself in the previous layer; otherwise the natural order 4*step + k."""
    if c_out == 128 and c_in == 128:
        return [16 * (4 * (c & 1) + sl) + 4 * (c >> 1) + k for c in range(8) for sl in range(4) for k in range(4)]
    return list(range(c_in))


def pack_conv_weight_winograd(w: torch.Tensor) -> torch.Tensor:
    """[c_out, c_in, 3, 3] -> U = G g G^T laid out [c_in/4][c_out/16][4][64][4] (include/betaone_engine.h,
    BO_TOWER_WINOGRAD): element (step, ob, pq, lane, e) = U[4*pq + e][16*ob + (lane & 15)][channel(step, lane >> 4)],
    channel() = winograd_k_order."""
    co, ci = w.shape[0], w.shape[1]
    u = torch.einsum("ai,ocij,bj->aboc", _WG_G, w.double(), _WG_G).reshape(16, co, ci)  # [pos][oc][ic]
    u = u[:, :, winograd_k_order(co, ci)]
    u = u.reshape(4, 4, co // 16, 16, ci // 4, 4)  # [pq][e][ob][o16][step][k]
    return u.permute(4, 2, 0, 5, 3, 1).contiguous().float()  # [step][ob][pq][k][o16][e]


def pack_conv_weight_f16(w: torch.Tensor) -> torch.Tensor:
    """[c_out, c_in, 3, 3] -> fp16 [9*c_in/16][c_out/32][64][8] (include/betaone_engine.h, BO_TOWER_DIRECT_F16):
    element (step, mt, lane, i) = W[32*mt + (lane & 31)][16*(step % (c_in/16)) + 8*(lane >> 5) + i][tap = step / (c_in/16)]."""
    co, ci = w.shape[0], w.shape[1]
    u = w.reshape(co // 32, 32, ci // 16, 2, 8, 9)  # [mt][o][cg][kg][i][tap]
    return u.permute(5, 2, 0, 3, 1, 4).contiguous().half()  # [tap][cg][mt][kg][o][i]


def pack_conv_weight_f16_t16(w: torch.Tensor) -> torch.Tensor:
    """[c_out, c_in, 3, 3] -> fp16 [9][c_in/32][c_out/16][64][8] (BO_TOWER_DIRECT_F16_T16: the A fragments of v_mfma_f32_16x16x32_f16):
    element (tap, g, ot, lane, i) = W[16*ot + (lane & 15)][32*g + 8*(lane >> 4) + i][tap]."""
    co, ci = w.shape[0], w.shape[1]
    u = w.reshape(co // 16, 16, ci // 32, 4, 8, 9)  # [ot][o][g][kb][i][tap]
    return u.permute(5, 2, 0, 3, 1, 4).contiguous().half()  # [tap][g][ot][kb][o][i]


# which MFMA tile conv='tower_f16' multiplies with, by filter count ("16": csrc/bo_tower_h16.h); BETAONE_F16_TILE overrides.  Same-box A/Bs
# (profiles/r05_all_configs.md): 128 filters (fast mode) 4.78 s against 5.00 s per ply of 16 384 games with 16x16x32 tiles; 256 filters
# (configs[4]) 13.0 against 12.2-12.5 ms -- the 256-filter instance of the new tiling spills registers.
F16_TILE_DEFAULT = {128: "16", 256: "32"}


def split_scale(w: torch.Tensor) -> float:
    """The power of two s that puts the largest |s*w| in [2^14, 2^15) (BO_TOWER_SPLIT_F16: fp16 pairs of s*w).  s <= 2^126: the
    kernels multiply by 1 / s in float32, which has to be a normal number there (a layer whose largest |w| is below 2^-112 -- a
    float32 denormal, say -- got s up to 2^163 and an inverse of 0; it now keeps s = 2^126 and fewer bits in its lo halves)."""
    m = float(w.abs().max())
    if m == 0.0 or not np.isfinite(m):
        return 1.0
    return float(2.0 ** min(126, 15 - math.frexp(m)[1]))  # frexp: m = f * 2^e with 0.5 <= f < 1, so floor(log2 m) = e - 1, exactly


def split_f16(w: torch.Tensor):
    """(hi, lo) fp16 with hi = RN16(w), lo = RN16(w - hi), computed in float64."""
    w = w.double()
    hi = w.half()
    lo = (w - hi.double()).half()
    return hi, lo


def pack_conv_weight_split(w: torch.Tensor, scale: float) -> torch.Tensor:
    """[c_out, c_in, 3, 3] float32 -> fp16 [9*c_in/16][c_out/32][2 = hi, lo][64][8] of scale*w (include/betaone_engine.h,
    BO_TOWER_SPLIT_F16; the element order of pack_conv_weight_f16 with every fragment doubled)."""
    co, ci = w.shape[0], w.shape[1]
    hi, lo = split_f16(w.double() * scale)
    u = torch.stack([hi, lo], 0).reshape(2, co // 32, 32, ci // 16, 2, 8, 9)  # [hl][mt][o][cg][kg][i][tap]
    return u.permute(6, 3, 1, 0, 4, 2, 5).contiguous()  # [tap][cg][mt][hl][kg][o][i]


def pack_head_weight_split(wh: torch.Tensor, scale: float) -> torch.Tensor:
    """[32*mt_n, c] float32 (the joint 1x1 head convolution, rows padded with zeros to whole 32-channel tiles) -> fp16
    [mt_n][c/16][2 = hi, lo][64][8] of scale*wh (bo_k_tower_s / bo_k_tower_s16, the head loop): element (mt, st, hl, lane, i) =
    split(scale * Wh[32*mt + (lane & 31)][16*st + 8*(lane >> 5) + i])."""
    mt, c = wh.shape[0] // 32, wh.shape[1]
    hi, lo = split_f16(wh.double() * scale)
    return torch.stack([hi, lo], 0).reshape(2, mt, 32, c // 16, 2, 8).permute(1, 3, 0, 4, 2, 5).contiguous()  # [mt][st][hl][kg][o][i]


SPLIT_TILE_DEFAULT = "16"  # which MFMA tile conv='tower_split' multiplies with at 128 filters ("16": csrc/bo_tower_s16.h); BETAONE_SPLIT_TILE overrides


def pack_conv_weight_split16(w: torch.Tensor, scale: float) -> torch.Tensor:
    """[c_out, c_in, 3, 3] float32 -> fp16 [9][c_in/32][c_out/16][2 = hi, lo][64][8] of scale*w (BO_TOWER_SPLIT_F16_T16: the A fragments of
    v_mfma_f32_16x16x32_f16): element (tap, g, ot, hl, lane, i) = split(scale * W[16*ot + (lane & 15)][32*g + 8*(lane >> 4) + i][tap])."""
    co, ci = w.shape[0], w.shape[1]
    hi, lo = split_f16(w.double() * scale)
    u = torch.stack([hi, lo], 0).reshape(2, co // 16, 16, ci // 32, 4, 8, 9)  # [hl][ot][o][g][kb][i][tap]
    return u.permute(6, 3, 1, 0, 4, 2, 5).contiguous()  # [tap][g][ot][hl][kb][o][i]


def pack_conv_weight_small(w: torch.Tensor) -> torch.Tensor:
    """[c_out, c_in, 3, 3] -> [c_out/16][tap 9][c_in/16][64][4] (bo_nn_conv3x3_small): element (ot, tap, g, lane, e) =
    W[16*ot + (lane & 15)][16*g + 4*e + (lane >> 4)][tap]."""
    co, ci = w.shape[0], w.shape[1]
    u = w.reshape(co // 16, 16, ci // 16, 4, 4, 9)  # [ot][o][g][e][k][tap]
    return u.permute(0, 5, 2, 4, 1, 3).contiguous()  # [ot][tap][g][k][o][e]


def pack_conv_weight_small_split(w: torch.Tensor, scale: float) -> torch.Tensor:
    """[c_out, c_in, 3, 3] float32 -> fp16 [c_out/16][tap 9][c_in/16][64][2 = hi, lo][4] of scale*w (bo_nn_b1_create, weights_split_dev):
    element (ot, tap, g, lane, hl, j) = split(scale * W[16*ot + (lane & 15)][16*g + 4*(lane >> 4) + j][tap]) -- per lane the B fragment
    of one v_mfma_f32_16x16x16_f16 K-step as (hi x4 | lo x4) = 16 bytes, at the index the float32 fragments of pack_conv_weight_small have."""
    co, ci = w.shape[0], w.shape[1]
    hi, lo = split_f16(w.double() * scale)
    u = torch.stack([hi, lo], 0).reshape(2, co // 16, 16, ci // 16, 4, 4, 9)  # [hl][ot][n][g][kq][j][tap]
    return u.permute(1, 6, 3, 4, 2, 0, 5).contiguous()  # [ot][tap][g][kq][n][hl][j]


def pack_head_weight_winograd(wh: torch.Tensor) -> torch.Tensor:
    """[16*mb, c] float32 (the joint 1x1 head convolution, rows padded with zeros to whole 16-channel tiles) -> [mb][c/16][4][16][4]
    (bo_k_tower_wg, the head loop): element (mb, g, k, o, e) = Wh[16*mb + o][16*g + 4*e + k]."""
    mb, c = wh.shape[0] // 16, wh.shape[1]
    return wh.reshape(mb, 16, c // 16, 4, 4).permute(0, 2, 4, 1, 3).contiguous()


def pack_head_weight_f16(wh: torch.Tensor) -> torch.Tensor:
    """[32*mt, c] float32 (rows padded with zeros to whole 32-channel tiles) -> fp16 [mt][c/16][2][32][8] (bo_k_tower_h / bo_k_tower_h16,
    the head loop): element (mt, st, kg, o, i) = Wh[32*mt + o][16*st + 8*kg + i]."""
    mt, c = wh.shape[0] // 32, wh.shape[1]
    return wh.reshape(mt, 32, c // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().half()


def _pad_input_weight(w_in: torch.Tensor) -> torch.Tensor:
    """The input convolution's [c, 120, 3, 3] weight with zero planes up to 128 (a whole number of K-steps in every layout)."""
    w0 = torch.zeros((w_in.shape[0], 128, 3, 3), device=w_in.device)
    w0[:, :120] = w_in
    return w0


def _split_tile(c, asked):
    # 128 filters: the products as 16x16x32 tiles (csrc/bo_tower_s16.h) or 32x32x16 (bo_tower_s.h); BETAONE_SPLIT_TILE=16 / 32 for A/B runs
    return 16 if (c == 128 and str(os.environ.get("BETAONE_SPLIT_TILE", SPLIT_TILE_DEFAULT) if asked is None else asked) == "16") else 32


def _f16_tile(c, asked):
    return 16 if str(os.environ.get("BETAONE_F16_TILE", F16_TILE_DEFAULT.get(c, "32")) if asked is None else asked) == "16" else 32


@dataclasses.dataclass(frozen=True)
class _TowerLayout:
    """What one kind x tile of bo_nn_tower_create reads differently from the others (include/betaone_engine.h, BO_TOWER_*)."""
    algo: int
    pack: object  # conv weight [c_out, c_in, 3, 3] float32 (scaled: and its scale) -> the packed tensor, float32 or fp16
    ksteps: object  # c_in -> K-steps of a layer (column 1 of the layer table)
    unit: int = 4  # a weight offset counts 16 bytes: 4 floats, or 8 halves (then wts is fp16)
    wts_multiple: int = 1  # wts gets zeros up to a multiple of this many elements
    scaled: bool = False  # (hi, lo) routes: pack(w, split_scale(w)), (1 / scale, 0, 0, 0) behind every bias (1 / scale behind the head's),
    #                       and the parameters behind an SE block padded to a multiple of 4 floats
    head_rows: int = 0  # the joint head convolution's rows, padded to whole tiles of this many, packed by head_pack; 0: no head descriptor
    head_pack: object = None
    head_in_params: bool = False  # the head weights go into params (at a multiple of 4 floats) instead of wts


@dataclasses.dataclass(frozen=True)
class _TowerKind:
    name: str  # in the messages
    filters: tuple
    se_text: str
    se_limit: object  # filters -> the largest SE hidden width
    layouts: dict  # tile (None: the kind has one) -> _TowerLayout
    tile: object = None  # (filters, tile asked for or None: the environment) -> tile
    tile_first: bool = False  # the tile is chosen in front of the shape check


_K16 = lambda c_in: 9 * c_in // 16
_HEAD_F16 = dict(head_rows=32, head_pack=pack_head_weight_f16)
_HEAD_SPLIT = dict(head_rows=32, head_pack=pack_head_weight_split)
TOWER_KINDS = {
    "tower": _TowerKind("tower", (64, 128), "16", lambda c: 16, {None: _TowerLayout(0, pack_conv_weight, lambda c_in: c_in // 8)}),
    # (the two 1x1 head convolutions run behind the tower on the LDS-resident output)
    "tower_wg": _TowerKind("tower", (64, 128), "16", lambda c: 16, {None: _TowerLayout(
        1, pack_conv_weight_winograd, lambda c_in: c_in // 4, head_rows=16, head_pack=pack_head_weight_winograd, head_in_params=True)}),
    "tower_f16": _TowerKind("tower_f16", (128, 256), "16", lambda c: 16, {
        32: _TowerLayout(2, pack_conv_weight_f16, _K16, unit=8, wts_multiple=2, **_HEAD_F16),
        16: _TowerLayout(5, pack_conv_weight_f16_t16, _K16, unit=8, wts_multiple=2, **_HEAD_F16)}, tile=_f16_tile, tile_first=True),
    "tower_split": _TowerKind("tower_split", (128, 256), "min(16, filters/16)", lambda c: min(16, c // 16), {
        32: _TowerLayout(3, pack_conv_weight_split, _K16, unit=8, wts_multiple=8, scaled=True, **_HEAD_SPLIT),
        16: _TowerLayout(4, pack_conv_weight_split16, _K16, unit=8, wts_multiple=8, scaled=True, **_HEAD_SPLIT)}, tile=_split_tile),
}


@dataclasses.dataclass
class TowerTables:
    """The host arrays of bo_nn_tower_create."""
    table: np.ndarray  # int32 [L, 8]
    wts: np.ndarray
    params: np.ndarray  # float32
    head: object  # int32 [4] (head channels, policy channels, weights offset, bias offset) or None
    algo: int
    n_weights: int  # wts in floats
    c: int
    tile: object  # 16 / 32, None for the kinds that have one layout


def flatten_tower(kind, w_in, b_in, blocks, w_head, b_head, n_policy_ch, tile=None) -> TowerTables:
    """Flatten the trunk (BatchNorm-folded float32 weights: blocks = [(w1, b1, w2, b2, (se_w1, se_w2) or None)], w_head / b_head the
    joint 1x1 head convolution) into the host arrays of bo_nn_tower_create for conv=kind.  tile (16 / 32; tower_f16 and tower_split):
    None reads BETAONE_F16_TILE / BETAONE_SPLIT_TILE.  Pure: no library call, nothing on the GPU."""
    k = TOWER_KINDS[kind]
    c = w_in.shape[0]
    if k.tile_first:
        tile = k.tile(c, tile)
    if c not in k.filters or w_in.shape[1] != 120:
        raise E.EngineError(f"conv='{k.name}' supports 120 input planes and {k.filters[0]} or {k.filters[1]} filters")
    if not k.tile_first:
        tile = k.tile(c, tile) if k.tile else None
    lay = k.layouts[tile]
    wts, params, layers = [], [], []

    def add_w(t):  # -> offset in units of 16 bytes
        off = sum(a.size for a in wts) // lay.unit
        wts.append(t.reshape(-1).numpy())
        return off

    def add_p(t):  # -> offset in floats
        off = sum(a.size for a in params)
        params.append(t.detach().float().cpu().contiguous().reshape(-1).numpy())
        return off

    def pad_p():
        n = sum(a.size for a in params)
        if n % 4:
            add_p(torch.zeros(4 - n % 4))

    def f32(t):
        return t.detach().float().cpu()

    convs = [(_pad_input_weight(f32(w_in)), b_in, 0, None)]
    for w1, b1, w2, b2, se in blocks:
        convs += [(f32(w1), b1, 1, None), (f32(w2), b2, 2 if se is None else 3, se)]
    for w, bias, mode, se in convs:
        if se is not None and se[0].shape[0] > k.se_limit(c):
            raise E.EngineError(f"conv='{k.name}' supports SE hidden widths up to {k.se_text}")
        if lay.scaled:
            s = split_scale(w)
            row = [add_w(lay.pack(w, s)), lay.ksteps(w.shape[1]), add_p(torch.cat([f32(bias).reshape(-1), torch.tensor([1.0 / s, 0.0, 0.0, 0.0])]))]
        else:
            row = [add_w(lay.pack(w)), lay.ksteps(w.shape[1]), add_p(bias)]
        if se is not None:
            row += [mode, add_p(se[0]), add_p(se[1]), se[0].shape[0], 0]
            if lay.scaled:
                pad_p()
        else:
            row += [mode, 0, 0, 0, 0]
        layers.append(row)
    layers[-1][7] = 1
    head = None
    if lay.head_pack is not None:
        ch = w_head.shape[0]
        wh = torch.zeros((-(-ch // lay.head_rows) * lay.head_rows, c))
        wh[:ch] = f32(w_head).reshape(ch, c)
        hs = split_scale(wh) if lay.scaled else None
        whp = lay.head_pack(wh, hs) if lay.scaled else lay.head_pack(wh)
        if lay.head_in_params:
            pad_p()
        w_off = add_p(whp) if lay.head_in_params else add_w(whp)
        head = np.array([ch, n_policy_ch, w_off, add_p(torch.cat([f32(b_head).reshape(-1), torch.tensor([1.0 / hs] if lay.scaled else [])]))],
                        dtype=np.int32)
    wts = np.ascontiguousarray(np.concatenate(wts), dtype=np.float16 if lay.unit == 8 else np.float32)
    if wts.size % lay.wts_multiple:
        wts = np.concatenate([wts, np.zeros(lay.wts_multiple - wts.size % lay.wts_multiple, wts.dtype)])
    params = np.ascontiguousarray(np.concatenate(params), dtype=np.float32)
    return TowerTables(np.ascontiguousarray(np.array(layers, dtype=np.int32)), wts, params, head, lay.algo, wts.nbytes // 4, c, tile)


def _check(lib, rc):
    if rc:
        raise E.EngineError(lib.bo_last_error().decode())


def _planes(x, dev, message):
    """x as the contiguous float32 [B, 120, 8, 8] tensor on `dev` that the tower launches read, or EngineError(message)."""
    if x.device != dev or x.dtype != torch.float32 or x.shape[1:] != (120, 8, 8):
        raise E.EngineError(message)
    return x.contiguous()


def _dev_index(dev) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _launch_heads(lib, dev, B, launch, n_scratch=4096, tail=False):
    """The buffers of one head launch (bo_nn_heads, bo_nn_heads_f16, bo_nn_heads_pair) and the launch itself:
    launch(out ptr, value ptr or None, scratch ptr) -> rc.  -> (out [B, 4672], value [B, 1]), with tail (out, the scratch as
    value_fc1's partial sums [16, B, 256])."""
    # the scratch (value_fc1 partial sums / softmax statistics) is allocated per call -- under graph capture it then comes from the
    # graph's own pool (a module-wide scratch that grew with a later, larger batch left earlier captured graphs writing into freed
    # memory, and was shared by concurrent streams); the caching allocator makes the eager cost a free-list lookup
    scr = torch.empty(n_scratch * B, dtype=torch.float32, device=dev)
    out = torch.empty((B, 4672), dtype=torch.float32, device=dev)
    value = None if tail else torch.empty((B, 1), dtype=torch.float32, device=dev)
    _check(lib, launch(out.data_ptr(), None if tail else value.data_ptr(), scr.data_ptr()))
    return (out, scr.view(16, B, 256)) if tail else (out, value)


def conv3x3_small(lib, x, wpacked, bias, c_in, c_out, mode=0, residual=None):
    """y = epilogue(conv3x3(x)) through bo_nn_conv3x3_small; x NCHW float32 [B, c_in_x <= c_in, 8, 8], contiguous."""
    B = x.shape[0]
    y = torch.empty((B, c_out, 8, 8), dtype=torch.float32, device=x.device)
    _check(lib, lib.bo_nn_conv3x3_small(x.data_ptr(), wpacked.data_ptr(), bias.data_ptr(), residual.data_ptr() if residual is not None else None,
                                        y.data_ptr(), B, c_in, x.shape[1], c_out, mode, torch.cuda.current_stream(x.device).cuda_stream))
    return y


def conv3x3_mfma(lib, x, wpacked, bias, c_out, mode=0, residual=None, out=None):
    """y = epilogue(conv3x3(x)) through the C ABI (bo_nn_conv3x3); x NCHW float32 [B, c_in, 8, 8], contiguous."""
    B, c_in = x.shape[0], x.shape[1]
    if not x.is_contiguous() or x.dtype != torch.float32 or x.shape[2:] != (8, 8):
        raise E.EngineError("conv3x3_mfma: x must be a contiguous float32 [B, C, 8, 8] tensor")
    y = out if out is not None else torch.empty((B, c_out, 8, 8), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _check(lib, lib.bo_nn_conv3x3(x.data_ptr(), wpacked.data_ptr(), bias.data_ptr(), residual.data_ptr() if residual is not None else None,
                                  y.data_ptr(), B, c_in, c_out, mode, stream))
    return y


class FusedPolicyValueNet(nn.Module):
    def __init__(self, net, conv="miopen", f32_pipe=None):
        """net: a PolicyValueNet (any device); weights are copied, BN folded.  f32_pipe (conv='tower_b1' only; None = the
        BETAONE_F32_TOWER setting): True keeps the tiles on the fp32 matrix pipe (exact float32 products), False multiplies them on
        the fp16 pipe with (hi, lo) operand pairs -- the precision of conv='tower_split'."""
        super().__init__()
        self.lib = E.load_hip_library()
        self.conv = conv
        self._f32_pipe = f32_pipe
        # policy FC + softmax + value head as one kernel behind the Winograd tower (needs contiguous float32 Linear weights of the
        # reference's head shapes: 2 policy planes, 32 value planes, 256 hidden units)
        self.fused_heads = conv in ("tower_wg", "tower", "mfma", "mfma_small", "tower_b1", "tower_f16", "tower_split")
        f = net.for_inference(dtype=torch.float32, channels_last=False)
        dev = next(f.parameters()).device
        if dev.type != "cuda":
            raise E.EngineError("FusedPolicyValueNet needs the net on an MI355X (cuda device)")

        def cw(conv):
            return nn.Parameter(conv.weight.detach().contiguous(), requires_grad=False), \
                nn.Parameter(conv.bias.detach().contiguous(), requires_grad=False)

        self.w_in, self.b_in = cw(f.conv_input)
        self.blocks = []
        for i, blk in enumerate(f.residual_tower):
            w1, b1 = cw(blk.conv1)
            w2, b2 = cw(blk.conv2)
            se = None
            if hasattr(blk, "seblock"):
                se = (nn.Parameter(blk.seblock.excitation[0].weight.detach().contiguous(), requires_grad=False),
                      nn.Parameter(blk.seblock.excitation[2].weight.detach().contiguous(), requires_grad=False))
            for k, p in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
                self.register_parameter(f"blk{i}_{k}", p)
            if se:
                self.register_parameter(f"blk{i}_se1", se[0])
                self.register_parameter(f"blk{i}_se2", se[1])
            self.blocks.append((w1, b1, w2, b2, se))
        # the two 1x1 head convolutions share their input: one conv with 2 + 32 output channels
        self.w_head = nn.Parameter(torch.cat([f.policy_conv.weight, f.value_conv.weight], 0).detach().contiguous(), requires_grad=False)
        self.b_head = nn.Parameter(torch.cat([f.policy_conv.bias, f.value_conv.bias], 0).detach().contiguous(), requires_grad=False)
        self.n_policy_ch = f.policy_conv.out_channels
        self.policy_fc, self.value_fc1, self.value_fc2 = f.policy_fc, f.value_fc1, f.value_fc2
        # what the hand-written head kernels are written for: 2 policy + 32 value planes into the reference's three Linear layers
        self._reference_heads = (self.n_policy_ch == 2 and self.w_head.shape[0] == 34 and self.policy_fc.weight.shape == (4672, 128)
                                 and self.value_fc1.weight.shape == (256, 2048) and self.value_fc2.weight.shape == (1, 256))
        self.layout = "nchw+fused"
        if conv in ("mfma", "mfma_small", "tower_b1"):  # one launch per layer: the packed weights stay torch tensors
            c = self.w_in.shape[0]
            if conv == "mfma":
                shapes = {(self.w_in.shape[1], c)} | {(b[0].shape[1], b[0].shape[0]) for b in self.blocks}
                if not shapes <= MFMA_CONV_SHAPES:
                    raise E.EngineError(f"conv='mfma' supports (c_in, c_out) in {sorted(MFMA_CONV_SHAPES)}, got {sorted(shapes)}")
                pack, w0 = pack_conv_weight, self.w_in
            else:
                if c not in (64, 128, 256) or self.w_in.shape[1] != 120:
                    raise E.EngineError(f"conv='{conv}' supports 120 input planes and 64, 128 or 256 filters")
                pack, w0 = pack_conv_weight_small, _pad_input_weight(self.w_in)
            self.c = c
            self.p_in = nn.Parameter(pack(w0), requires_grad=False)
            self.packed = []
            for i, (w1, _, w2, _, _) in enumerate(self.blocks):
                p1 = nn.Parameter(pack(w1), requires_grad=False)
                p2 = nn.Parameter(pack(w2), requires_grad=False)
                self.register_parameter(f"blk{i}_p1", p1)
                self.register_parameter(f"blk{i}_p2", p2)
                self.packed.append((p1, p2))
            self.zero_bias = nn.Parameter(torch.zeros(c, device=dev), requires_grad=False)
            if conv == "tower_b1":
                self._build_b1(dev)
        elif conv in TOWER_KINDS:
            self._build_tower(dev, conv)
        elif conv != "miopen":
            raise ValueError("conv must be 'miopen', 'mfma', 'mfma_small', 'tower_b1', 'tower', 'tower_wg', 'tower_split' or 'tower_f16'")
        if conv != "miopen":
            self.layout = "nchw+" + conv

    def _build_b1(self, dev):
        """bo_nn_b1_create over the SAME device tensors the per-layer route uses (pack_conv_weight_small layout): the handle keeps
        their addresses, the module keeps them alive.  Unless the fp32 matrix pipe is asked for, every layer also gets (hi, lo) fp16
        weights (pack_conv_weight_small_split, scaled per layer by a power of two like conv='tower_split')."""
        from .nn_tune import f32_pipe_default

        c = self.c
        split = not (f32_pipe_default() if self._f32_pipe is None else self._f32_pipe)
        self.b1_precision = "f16 pairs (3 MFMAs per product, f32 accumulate)" if split else "f32 MFMA"
        descs, self._b1_split = [], []

        def desc(w, wp, bias, c_in, c_in_x, mode, se=None):
            ws, inv = None, 0.0
            if split:
                wf = w.detach().float().cpu()
                sc = split_scale(wf)
                ws = nn.Parameter(pack_conv_weight_small_split(wf, sc).to(dev), requires_grad=False)
                self._b1_split.append(ws)
                inv = 1.0 / sc
            d = E.BoB1LayerDesc(wp.data_ptr(), bias.data_ptr(), se[0].data_ptr() if se else None, se[1].data_ptr() if se else None,
                                c_in, c_in_x, mode, se[0].shape[0] if se else 0, ws.data_ptr() if ws is not None else None, inv, 0)
            descs.append(d)

        desc(_pad_input_weight(self.w_in.detach().float().cpu()), self.p_in, self.b_in, 128, 120, 0)
        for (w1, b1, w2, b2, se), (p1, p2) in zip(self.blocks, self.packed):
            if se is not None and se[0].shape[0] > 16:
                raise E.EngineError("conv='tower_b1' supports SE hidden widths up to 16")
            desc(w1, p1, b1, c, c, 0)
            desc(w2, p2, b2, c, c, 2 if se is not None else 1, se)
        arr = (E.BoB1LayerDesc * len(descs))(*descs)
        self._b1_max = 256 // ((c // 16) * 4)
        handle = C.c_void_p()
        _check(self.lib, self.lib.bo_nn_b1_create(arr, len(descs), c, self._b1_max, _dev_index(dev), C.byref(handle)))
        self._b1, self._b1_dev = handle, dev

    def _tower_b1(self, x):
        """Tower output [B, C, 8, 8] from ONE launch (bo_nn_b1_forward); batches beyond the resident grid take the per-layer launches."""
        B = x.shape[0]
        if B > self._b1_max:
            return self._tower_small(x)
        x = _planes(x, self._b1_dev, "tower_b1: x must be float32 [B, 120, 8, 8] on the net's device")
        y = torch.empty((B, self.c, 8, 8), dtype=torch.float32, device=x.device)
        _check(self.lib, self.lib.bo_nn_b1_forward(self._b1, x.data_ptr(), y.data_ptr(), B, torch.cuda.current_stream(x.device).cuda_stream))
        return y

    def check_b1(self):
        """Raise if a hand-off wait inside the last tower_b1 launch gave up (its bounded spin ran out: the evaluation is invalid).
        Synchronises torch's current stream."""
        t = self.__dict__.get("_b1")
        if not t:
            return
        code = C.c_int32(0)
        _check(self.lib, self.lib.bo_nn_b1_status(t, C.byref(code), torch.cuda.current_stream(self._b1_dev).cuda_stream))
        if code.value < 0:
            raise E.EngineError("tower_b1: an activation left the fp16 range (|v| > 65504) and was saturated -- the evaluation is wrong on the fp16 "
                                "matrix pipe; run this net with BETAONE_F32_TOWER=fp32 (FusedPolicyValueNet(..., f32_pipe=True))")
        if code.value:
            raise E.EngineError(f"tower_b1: a hand-off inside the launch timed out (phase {code.value - 1}); the evaluation is invalid")

    def _build_tower(self, dev, kind):
        """The persistent tower of conv=kind (bo_nn_tower_create over flatten_tower's arrays); the fp16 tower also gets half copies
        of the three head Linear layers."""
        t = flatten_tower(kind, self.w_in, self.b_in, self.blocks, self.w_head, self.b_head, self.n_policy_ch)
        handle = C.c_void_p()
        _check(self.lib, self.lib.bo_nn_tower_create(t.table.ctypes.data, len(t.table), t.wts.ctypes.data, t.n_weights, t.params.ctypes.data,
                                                t.params.size, t.c, t.algo, t.head.ctypes.data if t.head is not None else None,
                                                _dev_index(dev), C.byref(handle)))
        self.c, self._tower, self._tower_dev = t.c, handle, dev
        self._head_ch, self._head_split = self.w_head.shape[0], self.n_policy_ch
        if kind == "tower_split":
            self.split_tile = t.tile
        elif kind == "tower_f16":
            self.f16_tile = t.tile
            self.policy_fc_h = copy.deepcopy(self.policy_fc).half()
            self.value_fc1_h = copy.deepcopy(self.value_fc1).half()
            self.value_fc2_h = copy.deepcopy(self.value_fc2).half()
            self.wants_float32_input = True

    def _tower_f16_forward(self, x):
        if x.dtype != torch.float32:
            x = x.float()
        x = _planes(x, self._tower_dev, "tower_f16: x must be [B, 120, 8, 8] on the tower's device")
        B = x.shape[0]
        pa = torch.empty((B, self._head_split * 64), dtype=torch.float16, device=x.device)
        pb = torch.empty((B, (self._head_ch - self._head_split) * 64), dtype=torch.float16, device=x.device)
        _check(self.lib, self.lib.bo_nn_tower_forward(self._tower, x.data_ptr(), None, pa.data_ptr(), pb.data_ptr(), B,
                                                 torch.cuda.current_stream(x.device).cuda_stream))
        return pa, pb

    def __del__(self):
        try:
            t = self.__dict__.get("_tower")
            if t:
                self.__dict__["_tower"] = None
                self.lib.bo_nn_tower_destroy(t)
            t = self.__dict__.get("_b1")
            if t:
                self.__dict__["_b1"] = None
                self.lib.bo_nn_b1_destroy(t)
        except Exception:  # interpreter shutdown
            pass

    def check_overflow(self):
        """conv='tower_split' carries activations as fp16 pairs: raise if any forward since the last check had to saturate one (its
        outputs were wrong) -- bo_nn_tower_status: the word is read and cleared by one atomic exchange on torch's CURRENT stream,
        which must be the stream the forwards were launched on (it is ordered behind them there).  Synchronises that stream.  The
        self-play loop does not call this per ply: it watches the word through the engine's result block (overflow_word_ptr)."""
        if self.conv == "tower_b1":  # (its own two status words: a hand-off that gave up, a saturated activation)
            return self.check_b1()
        t = self.__dict__.get("_tower")
        if not t or self.conv != "tower_split":
            return
        flag = C.c_int32(0)
        _check(self.lib, self.lib.bo_nn_tower_status(t, C.byref(flag), torch.cuda.current_stream(self._tower_dev).cuda_stream))
        if flag.value:
            raise E.EngineError(self.OVERFLOW_MESSAGE)

    OVERFLOW_MESSAGE = ("tower_split: an activation left the fp16 range (|v| > 65504) and was saturated -- the evaluations of this net are "
                        "wrong on the fp16 matrix pipe; run it with BETAONE_F32_TOWER=fp32 (best_inference_copy(..., f32_pipe=True))")

    def overflow_words(self):
        """(device address, number of words) of the evaluate stage's own fault words, (0, 1) if it has none: the split-precision tower's
        saturation word, or the one-launch tower's [hand-off timeout code | saturation flag] (conv='tower_b1': what uci.py's searches
        and small self-play batches run on).  Rollout and dropin.mcts hand them to bo_engine_watch_words, so every fetched result
        block brings them along and an invalid evaluation stops the run where it happened."""
        if self.conv == "tower_b1" and self.__dict__.get("_b1"):
            p = C.c_void_p()
            _check(self.lib, self.lib.bo_nn_b1_word(self._b1, C.byref(p)))
            return (p.value or 0), 2
        return self.overflow_word_ptr(), 1

    def overflow_word_ptr(self) -> int:
        """Device address of the split-precision tower's status word (0 for every other evaluate stage)."""
        t = self.__dict__.get("_tower")
        if not t or self.conv != "tower_split":
            return 0
        p = C.c_void_p()
        _check(self.lib, self.lib.bo_nn_tower_word(t, C.byref(p)))
        return p.value or 0

    def _tower_forward(self, x, heads=False):
        """Tower output [B, C, 8, 8]; with heads=True (conv='tower_wg') the ReLU'd policy / value planes, flattened."""
        x = _planes(x, self._tower_dev, "tower: x must be float32 [B, 120, 8, 8] on the tower's device")
        B = x.shape[0]
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if heads:
            pa = torch.empty((B, self._head_split * 64), dtype=torch.float32, device=x.device)
            pb = torch.empty((B, (self._head_ch - self._head_split) * 64), dtype=torch.float32, device=x.device)
            timed = self.__dict__.get("tower_events")  # measurement hook (bench.py): a list -> one (start, end) event pair per launch
            if timed is not None:
                timed.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                timed[-1][0].record()
            tbuf = self.__dict__.get("tower_timing_buf")  # (Rollout(time_tower=True): the kernel notes its own duration, also inside graphs)
            if tbuf is not None and self.conv == "tower_split":
                rc = self.lib.bo_nn_tower_forward_timed(self._tower, x.data_ptr(), None, pa.data_ptr(), pb.data_ptr(), B, tbuf.data_ptr(), stream)
            else:
                rc = self.lib.bo_nn_tower_forward(self._tower, x.data_ptr(), None, pa.data_ptr(), pb.data_ptr(), B, stream)
            if timed is not None:
                timed[-1][1].record()
            out = (pa, pb)
        else:
            y = torch.empty((B, self.c, 8, 8), dtype=torch.float32, device=x.device)
            wg = self.conv in ("tower_wg", "tower_split")
            dummy = torch.empty((2, B, self._head_ch * 64), dtype=torch.float32, device=x.device) if wg else None
            rc = self.lib.bo_nn_tower_forward(self._tower, x.data_ptr(), y.data_ptr(), dummy[0].data_ptr() if wg else None,
                                              dummy[1].data_ptr() if wg else None, B, stream)
            out = y
        _check(self.lib, rc)
        return out

    def _heads(self, p, v, probs, tail=False):
        """tail=True: stop behind the first launch -> (logits, value_fc1's partial sums [16, B, 256]); Engine.step_heads finishes the
        row (softmax, value) in the step kernel that consumes it (bo_nn_heads flags 4)."""
        B, dev = p.shape[0], p.device
        flags = (4 if tail else 1 if probs else 0) | (2 if p.dtype == torch.float16 else 0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        return _launch_heads(self.lib, dev, B, lambda out, value, scr: self.lib.bo_nn_heads(
            p.data_ptr(), v.data_ptr(), self.policy_fc.weight.data_ptr(), self.policy_fc.bias.data_ptr(), self.value_fc1.weight.data_ptr(),
            self.value_fc1.bias.data_ptr(), self.value_fc2.weight.data_ptr(), self.value_fc2.bias.data_ptr(), out, value, scr, B, flags, stream),
            tail=tail)

    def _heads_f16(self, p, v, probs):
        """fp16 planes and fp16 head weights on the fp16 pipe (bo_nn_heads_f16); its scratch: (max, sum of exp) per board and output range."""
        B, dev = p.shape[0], p.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        return _launch_heads(self.lib, dev, B, lambda out, value, scr: self.lib.bo_nn_heads_f16(
            p.data_ptr(), v.data_ptr(), self.policy_fc_h.weight.data_ptr(), self.policy_fc.bias.data_ptr(), self.value_fc1_h.weight.data_ptr(),
            self.value_fc1.bias.data_ptr(), self.value_fc2.weight.data_ptr(), self.value_fc2.bias.data_ptr(), out, value, scr, B,
            1 if probs else 0, stream), n_scratch=20)

    def _library_heads(self, p, v, probs, half=False, forked=False):
        """The heads as library calls: policy_fc (-> softmax) and tanh(value_fc2(relu(value_fc1))).  half: the fp16 tower's half
        copies of the three layers.  forked: the value head (2 small kernels) runs beside the policy GEMM -- a fork / join of
        streams, also inside a captured graph."""
        fc, fc1, fc2 = (self.policy_fc_h, self.value_fc1_h, self.value_fc2_h) if half else (self.policy_fc, self.value_fc1, self.value_fc2)
        if not forked:
            logits = fc(p)
            return (torch.softmax(logits.float(), dim=1) if probs else logits), torch.tanh(fc2(F.relu(fc1(v))))
        cur = torch.cuda.current_stream(p.device)
        side = self.__dict__.get("_side")
        if side is None or side.device != p.device:
            side = self.__dict__["_side"] = torch.cuda.Stream(p.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            h = torch._addmm_activation(fc1.bias, v, fc1.weight.t())  # relu(fc1)
            value = torch.empty((h.shape[0], 1), dtype=torch.float32, device=h.device)
            _check(self.lib, self.lib.bo_nn_value_tail(h.data_ptr(), fc2.weight.data_ptr(), fc2.bias.data_ptr(), value.data_ptr(), h.shape[0],
                                                       h.shape[1], torch.cuda.current_stream(h.device).cuda_stream))
        logits = fc(p)
        if probs:  # before the join: the softmax runs beside the value head instead of behind the streams' rendezvous
            logits = torch.softmax(logits.float(), dim=1)
        cur.wait_stream(side)
        return logits, value

    def head_stage(self, batch: int) -> str:
        """What runs behind the trunk's head planes at this batch:
          "heads":     bo_nn_heads -- float32 head weights, accumulation, softmax and value on the fp32 matrix pipe (behind the fp16 tower
                       up to 1024 boards -- configs[4]: 512 -- with the fp16 planes widened on load: closer to the float32 net than the
                       half-precision GEMMs; tile-parallel, so a few hundred rows still fill the chip);
          "heads_f16": the fp16 tower beyond that (fast mode: 4 096 .. 131 072 rows): fp16 weights on the fp16 pipe, the policy FC and its
                       softmax fused per 32-board wave, the value head in one kernel (bo_heads.h) -- no library launch;
                       BETAONE_HEADS_F16=0 takes "library" instead (A/B runs);
          "library" / "library_forked" (behind tower_wg / tower_split): a net without the reference's head shapes, and conv='miopen'."""
        if self.fused_heads and self._reference_heads:
            if self.conv != "tower_f16" or batch <= 1024:
                return "heads"
            if os.environ.get("BETAONE_HEADS_F16", "1") != "0":
                return "heads_f16"
        return "library_forked" if self.conv in ("tower_wg", "tower_split") else "library"

    def tail_supported(self, batch: int) -> bool:
        """forward_tail exists for this net at this batch: the evaluate stage ends in bo_nn_heads."""
        return self.head_stage(batch) == "heads"

    def tail_params(self):
        """(value_fc1.bias, value_fc2.weight, value_fc2.bias) device pointers for Engine.step_heads (a captured graph holds copies of
        them as it holds every other weight address of this module: Rollout.swap_model drops its graphs and reads these again)."""
        return self.value_fc1.bias.data_ptr(), self.value_fc2.weight.data_ptr(), self.value_fc2.bias.data_ptr()

    @torch.no_grad()
    def forward_tail(self, x):
        """(logits [B, 4672], partial sums of value_fc1 [16, B, 256]): the evaluate stage without its last launch."""
        return self.forward(x, tail=True)

    def _epi(self, x, bias, res=None):
        B, C = x.shape[0], x.shape[1]
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(self.lib, self.lib.bo_nn_bias_act(x.data_ptr(), bias.data_ptr(), res.data_ptr() if res is not None else None, B, C, stream))
        return x

    def _se(self, x, bias, se, res):
        B, C = x.shape[0], x.shape[1]
        stream = torch.cuda.current_stream(x.device).cuda_stream
        small = self.conv in ("mfma_small", "tower_b1") and C % 16 == 0 and se[0].shape[0] <= 16  # few boards: C/16 workgroups per board, result into `res`
        _check(self.lib, (self.lib.bo_nn_se_residual_small if small else self.lib.bo_nn_se_residual)(
            x.data_ptr(), bias.data_ptr(), se[0].data_ptr(), se[1].data_ptr(), res.data_ptr(), B, C, se[0].shape[0], stream))
        return res if small else x

    def _tower_mfma(self, x):
        L, C = self.lib, self.c
        x = conv3x3_mfma(L, x.contiguous(), self.p_in, self.b_in, C, 1)
        for (w1, b1, w2, b2, se), (p1, p2) in zip(self.blocks, self.packed):
            y = conv3x3_mfma(L, x, p1, b1, C, 1)
            if se is not None:
                x = self._se(conv3x3_mfma(L, y, p2, self.zero_bias, C, 0), b2, se, x)
            else:
                x = conv3x3_mfma(L, y, p2, b2, C, 2, residual=x)
        return x

    def _tower_small(self, x):
        L, C = self.lib, self.c
        x = conv3x3_small(L, x.contiguous(), self.p_in, self.b_in, 128, C, 1)
        for (w1, b1, w2, b2, se), (p1, p2) in zip(self.blocks, self.packed):
            y = conv3x3_small(L, x, p1, b1, C, C, 1)
            if se is not None:
                x = self._se(conv3x3_small(L, y, p2, self.zero_bias, C, C, 0), b2, se, x)
            else:
                x = conv3x3_small(L, y, p2, b2, C, C, 2, residual=x)
        return x

    def _tower_miopen(self, x):
        x = self._epi(F.conv2d(x, self.w_in, None, padding=1), self.b_in)
        for w1, b1, w2, b2, se in self.blocks:
            y = self._epi(F.conv2d(x, w1, None, padding=1), b1)
            y = F.conv2d(y, w2, None, padding=1)
            x = self._se(y, b2, se, x) if se is not None else self._epi(y, b2, x)
        return x

    def _trunk(self, x):
        """The ReLU'd (policy planes [B, 64 * policy channels], value planes) behind the joint head convolution: from the tower kernel
        itself (tower_f16 in fp16, tower_wg, tower_split), otherwise a 1x1 convolution and its epilogue behind the tower output."""
        conv = self.conv
        if conv == "tower_f16":
            return self._tower_f16_forward(x)
        if conv in ("tower_wg", "tower_split"):
            return self._tower_forward(x, heads=True)
        x = (self._tower_mfma(x) if conv == "mfma" else self._tower_small(x) if conv == "mfma_small" else self._tower_b1(x) if conv == "tower_b1"
             else self._tower_forward(x) if conv == "tower" else self._tower_miopen(x))
        h = self._epi(F.conv2d(x, self.w_head, None), self.b_head)
        return h[:, :self.n_policy_ch].flatten(1), h[:, self.n_policy_ch:].flatten(1)

    @torch.no_grad()
    def forward_probs(self, x):
        """(softmax(logits, dim=1) in float32, value): the policy softmax of mcts.py:185,287 issued where it costs least."""
        return self.forward(x, probs=True)

    @torch.no_grad()
    def forward(self, x, probs: bool = False, tail: bool = False):
        stage = self.head_stage(x.shape[0])
        if tail and stage != "heads":  # (every other stage returns the value [B, 1], not value_fc1's partial sums)
            raise E.EngineError(f"forward_tail: not available for conv={self.conv!r} at batch {x.shape[0]}")
        p, v = self._trunk(x)
        if stage == "heads":  # (batch 1 -- uci.py's analysis -- : the slices of the head convolution's output are contiguous already)
            return self._heads(p.contiguous(), v.contiguous(), probs, tail)
        if stage == "heads_f16":
            return self._heads_f16(p, v, probs)
        return self._library_heads(p, v, probs, half=self.conv == "tower_f16", forked=stage == "library_forked")


class PairedNet(nn.Module):
    """Two evaluate stages as one (head-to-head matches, betaone_amd/match.py): forward(x, sel) evaluates row b with net sel[b]
    (int32 [B] on the device, 0 = the first net) and returns what that net alone returns for the row -- bit for bit.

      route "pair:tower_split": both nets on the split-precision tower with the reference's head shapes and identical layer tables: ONE
                 launch of the tower (bo_nn_tower_forward_pair: each workgroup streams the weights of its own board's net) and one
                 two-net bo_nn_heads (bo_nn_heads_pair) instead of two launches of each (what a match ply costs against a
                 self-play ply, and where the difference goes: profiles/match_two_net.md, scripts/match_cost.py);
      route "pair:merge": every other pair (different shapes, the other hand-written routes, library nets, test stand-ins): BOTH nets run
                 over the whole batch and the rows are merged (bo_nn_merge_rows) -- twice the evaluate stage's time.

    model0 / model1: PolicyValueNets (an inference copy is made: nn_tune.pair_route decides), or evaluate stages already built (any
    module with forward(x) -> (logits, value); FusedPolicyValueNet(conv='tower_split') pairs share the launch).  route='merge' forces
    the merge path.  There is no forward_tail: Rollout keeps the stage's own rows kernel for a pair (the step tail stays single-net)."""

    is_pair = True

    def __init__(self, model0, model1, batch: int, device="cuda:0", route: str = None, f32_pipe=None):
        super().__init__()
        from . import nn_tune

        self.lib = E.load_hip_library()
        device = torch.device(device)

        def stage(m):
            if not hasattr(m, "for_inference"):
                return m
            r = nn_tune.pair_route(m.conv_input.out_channels, batch, torch.float32, f32_pipe)
            if r == "tower_split" and route != "merge":
                return FusedPolicyValueNet(m.to(device), conv="tower_split").to(device)
            return nn_tune.best_inference_copy(m, batch, device, f32_pipe=f32_pipe)

        self.nets = [stage(model0), stage(model1)]
        for i, n in enumerate(self.nets):  # (registered for .to() / state; forward goes through self.nets)
            if isinstance(n, nn.Module):
                self.add_module(f"net{i}", n)
        self.route = "pair:merge"
        if route != "merge" and self._can_share_launch():
            self.route = "pair:tower_split"
            self._hw = [self._head_weights(n) for n in self.nets]

    def _can_share_launch(self) -> bool:
        a, b = self.nets
        if not all(isinstance(n, FusedPolicyValueNet) and n.conv == "tower_split" and n.__dict__.get("_tower") for n in (a, b)):
            return False
        heads_ok = all(n.fused_heads and n._reference_heads for n in (a, b))
        if not heads_ok or a.split_tile != b.split_tile or a._tower_dev != b._tower_dev:
            return False
        return self.lib.bo_nn_tower_pair_check(a._tower, b._tower) == 0

    @staticmethod
    def _head_weights(n):
        return E.BoHeadWeights(n.policy_fc.weight.data_ptr(), n.policy_fc.bias.data_ptr(), n.value_fc1.weight.data_ptr(),
                               n.value_fc1.bias.data_ptr(), n.value_fc2.weight.data_ptr(), n.value_fc2.bias.data_ptr())

    OVERFLOW_MESSAGE = FusedPolicyValueNet.OVERFLOW_MESSAGE

    def overflow_words(self):
        """The first net's fault words: on the shared launch a saturation is reported into both nets' words, so watching one is watching
        both.  On the merge path the two nets' words are separate and the engine watches one consecutive run of words: only the first
        net's is checked with every ply's result block; the second net's is checked by check_overflow, which the match driver calls
        when the match ends (a saturating second net then fails the match at its end, not on the ply it happened)."""
        words = getattr(self.nets[0], "overflow_words", None)
        return words() if words is not None else (0, 1)

    def check_overflow(self):
        for n in self.nets:
            chk = getattr(n, "check_overflow", None)
            if chk is not None:
                chk()

    def forward_probs(self, x, sel):
        return self.forward(x, sel, probs=True)

    @torch.no_grad()
    def forward(self, x, sel, probs: bool = False):
        B = x.shape[0]
        if sel.dtype != torch.int32 or sel.numel() < B or sel.device != x.device:
            raise E.EngineError("PairedNet: sel must be an int32 tensor of >= batch entries on the input's device")
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if self.route == "pair:tower_split":
            a, b = self.nets
            x = _planes(x, a._tower_dev, "PairedNet: x must be float32 [B, 120, 8, 8] on the nets' device")
            pa = torch.empty((B, 2 * 64), dtype=torch.float32, device=x.device)
            pv = torch.empty((B, 32 * 64), dtype=torch.float32, device=x.device)
            _check(self.lib, self.lib.bo_nn_tower_forward_pair(a._tower, b._tower, sel.data_ptr(), x.data_ptr(), pa.data_ptr(), pv.data_ptr(), B, stream))
            return _launch_heads(self.lib, x.device, B, lambda out, value, scr: self.lib.bo_nn_heads_pair(
                pa.data_ptr(), pv.data_ptr(), C.byref(self._hw[0]), C.byref(self._hw[1]), sel.data_ptr(), out, value, scr, B, 1 if probs else 0, stream))
        # merge: both nets over the whole batch (twice the evaluate time), then each row from its own net
        outs = []
        for n in self.nets:
            fp = getattr(n, "forward_probs", None) if probs else None
            l, v = fp(x) if fp is not None else n(x)
            l = l.float()
            if probs and fp is None:
                l = torch.softmax(l, dim=1)
            outs.append((l.to(x.device).contiguous(), v.float().reshape(B, 1).to(x.device).contiguous()))
        (l0, v0), (l1, v1) = outs
        if l0.shape != l1.shape:
            raise E.EngineError(f"PairedNet: the two nets' policy widths differ ({tuple(l0.shape)} vs {tuple(l1.shape)})")
        out = torch.empty_like(l0)
        value = torch.empty_like(v0)
        _check(self.lib, self.lib.bo_nn_merge_rows(sel.data_ptr(), l0.data_ptr(), v0.data_ptr(), l1.data_ptr(), v1.data_ptr(), out.data_ptr(),
                                                   value.data_ptr(), B, l0.shape[1], stream))
        return out, value
