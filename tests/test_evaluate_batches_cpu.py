"""CPU test of tests/evaluate_batches.py, the helper of tests/test_evaluate_batches_gpu.py: the batch lists really make the persistent
tower kernels loop, the sampled rows cover every pass, the inputs are distinct encoded positions, and the float64 reference is the net."""
import numpy as np
import pytest

import evaluate_batches as EB


@pytest.mark.parametrize("n_cu", [256, 304, 80])
def test_batch_lists_reach_later_passes_of_every_grid(n_cu):
    for conv, filters in (("tower_split", 128), ("tower_wg", 64), ("tower", 128), ("tower", 64), ("mfma", 256), ("tower_f16", 128)):
        per = EB.boards_per_pass(conv, filters, n_cu)
        assert per == (2 * n_cu if (conv, filters) in (("tower", 64), ("tower_f16", 128)) else n_cu)
        bl = EB.batch_list(conv, filters, n_cu)
        assert [EB.passes(b, per) for b in (min(bl), max(bl))] == [1, 4]
        assert {per - (2 if conv == "tower_f16" else 1), per, per + (2 if conv == "tower_f16" else 1)} <= set(bl)
        big = EB.largest_batch(conv, filters, n_cu)
        assert EB.passes(big, per) == 4
        if conv == "tower_f16":
            odd = [b for b in bl if b % 2]
            # the lone tail board of an odd batch sits in a workgroup that already held a pair on an earlier pass
            assert len(odd) == 2 and all((b + 1) // 2 > n_cu for b in odd) and big % 2 == 1
            assert (big + 1) // 2 == 3 * n_cu + 37
        else:
            assert bl == [per - 1, per, per + 1, 2 * per + 1, 3 * per + 37]


def test_sampled_rows_cover_the_first_and_last_row_of_every_pass():
    n_cu = 256
    for conv, filters in (("tower_split", 128), ("tower", 64), ("tower_f16", 256)):
        B = EB.largest_batch(conv, filters, n_cu)
        per = EB.boards_per_pass(conv, filters, n_cu)
        rows = EB.sample_rows(B, conv, filters, n_cu)
        assert len(rows) <= 64 and rows == sorted(set(rows)) and rows[-1] == B - 1 and rows[0] == 0
        for k in range(EB.passes(B, per)):
            assert k * per in rows and min((k + 1) * per, B) - 1 in rows
        assert {EB.pass_of(r, conv, filters, n_cu) for r in rows} == set(range(EB.passes(B, per)))
    B = EB.largest_batch("tower_f16", 128, n_cu)  # 3 * 256 + 37 pairs: the tail board 1608 alone in pair 804, workgroup 804 % 256 = 36
    rows = EB.sample_rows(B, "tower_f16", 128, n_cu)
    assert B == 1609 and {72, 73, 584, 585, 1096, 1097, 1608} <= set(rows)


def test_sub_batches_stay_on_one_side_of_the_fp16_heads_switch():
    assert EB.sub_batch(1026, "tower_f16") == slice(1, 1026)
    assert EB.sub_batch(1025, "tower_f16") is None
    assert EB.sub_batch(1025, "tower_split") == slice(1, 1025)


def test_inputs_are_distinct_encoded_positions_with_history():
    import torch

    pos = EB.random_positions(600, seed=3)
    assert pos.shape == (600, 120, 8, 8) and pos.dtype == np.float32
    assert len({p.tobytes() for p in pos}) == 600
    # later plies carry earlier positions in the history planes (12 piece planes + 2 repetition planes per position)
    assert (pos[:, 14:28].reshape(600, -1).sum(1) > 0).mean() > 0.9
    again = EB.random_positions(600, seed=3)
    assert np.array_equal(pos, again)  # seeded
    x = EB.make_rows(torch.from_numpy(pos), 1500, seed=5)
    assert x.shape == (1500, 120, 8, 8)
    EB.assert_rows_distinct(x)
    dup = x.clone()
    dup[7] = dup[1200]
    with pytest.raises(AssertionError):
        EB.assert_rows_distinct(dup)


def test_float64_reference_is_the_same_net():
    import torch
    from betaone_amd import dropin
    from fake_model import hash_init_

    dropin.install()
    import config
    import network

    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = 1, 1, 64
    try:
        net = hash_init_(network.PolicyValueNet().eval())
        x = EB.make_rows(torch.from_numpy(EB.random_positions(16)), 16)
        l64, v64 = EB.reference64(net, x)
        assert l64.dtype == torch.float64 and v64.shape == (16, 1)
        with torch.no_grad():
            l, v = net(x)
        err = EB.row_errors(l, v, l64, v64)
        assert err.shape == (16,) and 0 < err.max() < 1e-4
        assert next(net.parameters()).dtype == torch.float32  # the net itself is left as it was
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
