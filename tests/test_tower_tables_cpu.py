"""CPU tests of fused_net.flatten_tower: the host arrays bo_nn_tower_create receives (layer table, weights, parameters, head
descriptor, algorithm code, weight count) for every kind x tile are, byte for byte, the arrays the three builders this function
replaced handed over -- tests/golden/tower_tables.json holds their sha256 sums, captured from those builders (how:
profiles/fused_net_refactor.md) -- and the shapes a kind does not take are refused with the builders' messages."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import trained_like as TL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tower_tables.json")

# (kind, tile asked for) by filter count: every kind x tile a size admits (256 filters: the split tower has 32x32x16 tiles only,
# whichever is asked for)
KINDS = {
    128: [("tower", None), ("tower_wg", None), ("tower_f16", 16), ("tower_f16", 32), ("tower_split", 16), ("tower_split", 32)],
    256: [("tower_f16", 16), ("tower_f16", 32), ("tower_split", 16), ("tower_split", 32)],
    64: [("tower", None), ("tower_wg", None)],
}


def _cid(kind, family, size, tile):
    return "%s-%d+%dx%d-%s" % (family, *size, kind) + ("" if tile is None else "-t%d" % tile)


# (id, kind, family, (blocks, SE blocks, filters), tile): the hash net at TL.SIZES (its last block is an SE block); the ladder net
# (per-layer scales differ) on both split tiles; a net whose last block is a plain one
CASES = [(_cid(k, "hash", s, t), k, "hash", s, t) for s in TL.SIZES for k, t in KINDS[s[2]]]
CASES += [(_cid("tower_split", "ladder", (2, 1, 128), t), "tower_split", "ladder", (2, 1, 128), t) for t in (16, 32)]
CASES += [(_cid(k, "hash", (2, 0, 128), t), k, "hash", (2, 0, 128), t) for k, t in KINDS[128] if t != 32]


def net_of(family, size):
    return TL.family_net(family, size)


def folded(net):
    """(w_in, b_in, blocks, w_head, b_head, n_policy_ch, (policy_fc, value_fc1, value_fc2)) of the BatchNorm-folded float32 net on
    the CPU, as FusedPolicyValueNet.__init__ collects them."""
    f = TL.fold32(net)
    cw = lambda conv: (conv.weight.detach().contiguous(), conv.bias.detach().contiguous())
    blocks = []
    for blk in f.residual_tower:
        se = None
        if hasattr(blk, "seblock"):
            se = (blk.seblock.excitation[0].weight.detach().contiguous(), blk.seblock.excitation[2].weight.detach().contiguous())
        blocks.append(cw(blk.conv1) + cw(blk.conv2) + (se,))
    w_head = torch.cat([f.policy_conv.weight, f.value_conv.weight], 0).detach().contiguous()
    b_head = torch.cat([f.policy_conv.bias, f.value_conv.bias], 0).detach().contiguous()
    return cw(f.conv_input) + (blocks, w_head, b_head, f.policy_conv.out_channels, (f.policy_fc, f.value_fc1, f.value_fc2))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _sha(a):
    assert a.flags["C_CONTIGUOUS"]
    return hashlib.sha256(a.tobytes()).hexdigest()


def _summary(t):
    return {"layers": int(t.table.shape[0]), "table": _sha(t.table), "wts": _sha(t.wts), "n_weights": int(t.n_weights),
            "params": _sha(t.params), "n_params": int(t.params.size), "c": int(t.c), "algo": int(t.algo),
            "head": None if t.head is None else [int(v) for v in t.head], "tile": t.tile}


def test_the_case_list_is_the_fixture():
    with open(GOLDEN) as fh:
        assert sorted(json.load(fh)) == sorted(c[0] for c in CASES) and len(CASES) == 12 + 2 + 4


@pytest.mark.parametrize("cid,kind,family,size,tile", CASES, ids=[c[0] for c in CASES])
def test_tables_are_the_bytes_the_three_builders_made(golden, cid, kind, family, size, tile, monkeypatch):
    from betaone_amd.fused_net import flatten_tower

    monkeypatch.delenv("BETAONE_SPLIT_TILE", raising=False)
    monkeypatch.delenv("BETAONE_F16_TILE", raising=False)
    args = folded(net_of(family, size))[:6]
    t = flatten_tower(kind, *args, tile=tile)
    assert t.table.dtype == np.int32 and t.table.shape == (1 + 2 * (size[0] + size[1]), 8) and t.params.dtype == np.float32
    assert t.wts.dtype == (np.float32 if kind in ("tower", "tower_wg") else np.float16) and t.wts.nbytes == 4 * t.n_weights
    assert (t.head is None) == (kind == "tower") and (t.head is None or (t.head.dtype == np.int32 and t.head.shape == (4,)))
    assert _summary(t) == golden[cid]
    if tile is not None:  # tile=None reads the environment, where the builders read it
        monkeypatch.setenv("BETAONE_SPLIT_TILE" if kind == "tower_split" else "BETAONE_F16_TILE", str(tile))
        assert _summary(flatten_tower(kind, *args)) == golden[cid]


def test_the_default_tiles_are_the_documented_ones(golden, monkeypatch):
    from betaone_amd import fused_net as FN

    monkeypatch.delenv("BETAONE_SPLIT_TILE", raising=False)
    monkeypatch.delenv("BETAONE_F16_TILE", raising=False)
    for size in ((2, 1, 128), (1, 1, 256)):
        args = folded(net_of("hash", size))[:6]
        want = {"tower_split": int(FN.SPLIT_TILE_DEFAULT) if size[2] == 128 else 32, "tower_f16": int(FN.F16_TILE_DEFAULT[size[2]])}
        for kind, tile in want.items():
            assert _summary(FN.flatten_tower(kind, *args)) == golden[_cid(kind, "hash", size, tile)]


def test_refused_shapes_keep_their_messages():
    from betaone_amd import engine as E
    from betaone_amd.fused_net import flatten_tower

    def refused(kind, args, text):
        with pytest.raises(E.EngineError) as e:
            flatten_tower(kind, *args)
        assert str(e.value) == text, (kind, str(e.value))

    a64, a128, a256 = (folded(net_of("hash", s))[:6] for s in ((2, 1, 64), (2, 1, 128), (1, 1, 256)))
    refused("tower_split", a64, "conv='tower_split' supports 120 input planes and 128 or 256 filters")
    refused("tower_f16", a64, "conv='tower_f16' supports 120 input planes and 128 or 256 filters")
    refused("tower", a256, "conv='tower' supports 120 input planes and 64 or 128 filters")
    refused("tower_wg", a256, "conv='tower' supports 120 input planes and 64 or 128 filters")
    refused("tower", (a128[0][:, :119],) + a128[1:], "conv='tower' supports 120 input planes and 64 or 128 filters")

    def with_se_hidden(args, r):  # the last (SE) block's excitation widened / narrowed to r hidden units
        w_in, b_in, blocks, w_head, b_head, n = args
        c = w_in.shape[0]
        return w_in, b_in, blocks[:-1] + [blocks[-1][:4] + ((torch.zeros(r, c), torch.zeros(c, r)),)], w_head, b_head, n

    for kind in ("tower", "tower_wg"):
        refused(kind, with_se_hidden(a128, 17), "conv='tower' supports SE hidden widths up to 16")
        flatten_tower(kind, *with_se_hidden(a128, 16))
    refused("tower_f16", with_se_hidden(a256, 17), "conv='tower_f16' supports SE hidden widths up to 16")
    flatten_tower("tower_f16", *with_se_hidden(a256, 16))
    refused("tower_split", with_se_hidden(a256, 17), "conv='tower_split' supports SE hidden widths up to min(16, filters/16)")
    refused("tower_split", with_se_hidden(a128, 9), "conv='tower_split' supports SE hidden widths up to min(16, filters/16)")
    flatten_tower("tower_split", *with_se_hidden(a128, 8))
    flatten_tower("tower_split", *with_se_hidden(a256, 16))
