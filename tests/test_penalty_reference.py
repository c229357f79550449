"""The repetition / presence penalty's definitions (dmcp/ops/reference.py):
penalize on hand-made values, the identity at theta 1 / alpha 0, the three
selection references under an all-zero history, history_mark / history_reset,
and select -> mark -> select on one fixed row."""
import math
import struct

import pytest
import torch

from dmcp import ops
from dmcp.ops import reference as ref


def _bits(vocab, ids):
    row = torch.zeros((vocab + 31) // 32, dtype=torch.int64)
    for v in ids:
        row[v // 32] |= 1 << (v % 32)
    return torch.where(row >= 2 ** 31, row - 2 ** 32, row).to(torch.int32)


def _bf(x):
    """The bf16 value nearest (ties to even) to the fp32 number ``x``, by integer arithmetic."""
    u, = struct.unpack("<I", struct.pack("<f", x))
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return struct.unpack("<f", struct.pack("<I", u))[0]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def test_penalize_hand_made_values():
    theta, alpha = 1.3, 0.5
    t, inv = _f32(theta), _f32(1.0 / _f32(theta))
    vals = [2.0, -2.0, 0.0, -0.0, float("inf"), float("-inf"), 1.0078125, 3.140625, -0.3359375]
    x = torch.tensor([vals, vals], dtype=torch.bfloat16)
    assert x.float().tolist()[0] == vals  # every value is a bf16 number
    hist = torch.stack([_bits(len(vals), range(len(vals))), _bits(len(vals), [])])
    y = ref.penalize(x, hist, theta, alpha)
    assert y.dtype == torch.float32
    want = [_bf(_f32(_f32(v * inv if v > 0 else v * t) - alpha)) for v in vals]
    assert y[0].tolist() == want
    assert y[0, 0] == _bf(_f32(_f32(2.0 * inv) - 0.5)) and y[0, 1] == _bf(_f32(-2.0 * t) - 0.5)
    assert y[0, 2] == -0.5 and y[0, 3] == -0.5 and y[0, 4] == math.inf and y[0, 5] == -math.inf
    # 1.0078125 / 1.3 - 0.5 is no bf16 number: the result is rounded once more
    exact = _f32(_f32(1.0078125 * inv) - 0.5)
    assert _bf(exact) != exact and y[0, 6] == _bf(exact)
    assert torch.equal(y[1].view(torch.int32), x[1].float().view(torch.int32))  # clear bits keep x, -0 included
    assert torch.equal(ref.penalize(x, None, theta, alpha), x.float())


def test_theta_one_alpha_zero_is_the_identity_on_bits():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(4, 300, generator=g) * 8).to(torch.bfloat16)
    x[0, :4] = torch.tensor([0.0, -0.0, float("inf"), float("-inf")], dtype=torch.bfloat16)
    full = torch.full((4, 10), -1, dtype=torch.int32)
    y = ref.penalize(x, full, 1.0, 0.0)
    assert torch.equal(y.to(torch.bfloat16).view(torch.int16), x.view(torch.int16))
    assert torch.equal(y.view(torch.int32), x.float().view(torch.int32))
    assert ref.Penalty(full, torch.zeros(4, dtype=torch.int32), 1.0, 0.0).off
    assert not ref.Penalty(full, torch.zeros(4, dtype=torch.int32), 1.0, 0.1).off


def _case(B=6, V=250, ld=256, n_masks=3, seed=3):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, ld, generator=g) * 4).to(torch.bfloat16)
    masks = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_masks, (V + 31) // 32), generator=g, dtype=torch.int64)
    masks = masks.to(torch.int32)
    midx = torch.randint(0, n_masks, (B,), generator=g, dtype=torch.int32)
    slots = torch.arange(B, dtype=torch.int32)
    slots[-1] = -1
    pos = torch.arange(B, dtype=torch.int32) + 11
    return logits, masks, midx, slots, pos


def test_an_all_zero_history_changes_nothing():
    logits, masks, midx, slots, pos = _case()
    B, V = logits.shape[0], 250
    pen = ops.Penalty(torch.zeros(8, (V + 31) // 32, dtype=torch.int32), slots, 1.3, 0.5)
    assert torch.equal(ops.masked_argmax(logits, masks, V, None, midx, penalty=pen),
                       ops.masked_argmax(logits, masks, V, None, midx))
    assert torch.equal(ops.masked_sample(logits, masks, V, None, midx, slots, pos, 0.7, 5, penalty=pen),
                       ops.masked_sample(logits, masks, V, None, midx, slots, pos, 0.7, 5))
    assert torch.equal(ref.sample_scores(logits, masks, V, midx, slots, pos, 0.7, 5, penalty=pen),
                       ref.sample_scores(logits, masks, V, midx, slots, pos, 0.7, 5))
    for kw in ({"top_k": 20, "top_p": 0.95}, {"min_p": 0.1}):
        s0, s1 = (torch.zeros(B, 2, dtype=torch.int32) for _ in range(2))
        a = ops.truncated_sample(logits, masks, V, None, midx, slots, pos, 0.7, 5, stats=s0, **kw)
        b = ops.truncated_sample(logits, masks, V, None, midx, slots, pos, 0.7, 5, stats=s1, penalty=pen, **kw)
        assert torch.equal(a, b) and torch.equal(s0, s1)
    x = torch.randn(B, 64).to(torch.bfloat16)
    w = torch.randn(256, 64).to(torch.bfloat16)
    m256 = torch.full((3, 8), -1, dtype=torch.int32)
    pen = ops.Penalty(torch.zeros(8, 8, dtype=torch.int32), slots, 1.3, 0.5)
    assert torch.equal(ops.lm_head_argmax(x, w, m256, midx, penalty=pen), ops.lm_head_argmax(x, w, m256, midx))
    assert torch.equal(ops.lm_head_sample(x, w, m256, midx, None, None, slots, pos, 0.7, 5, penalty=pen),
                       ops.lm_head_sample(x, w, m256, midx, None, None, slots, pos, 0.7, 5))


def test_history_mark_and_reset():
    V, W = 100, 4
    hist = torch.zeros(5, W, dtype=torch.int32)
    last = torch.tensor([40, 41, 99, 7], dtype=torch.int32)
    #            direct  gather  pad  range  range  exempt  same word, same slot (jump-forward)  top bit
    tokens = torch.tensor([3, 0, 9, -1, 100, 34, 64, 65, 31], dtype=torch.int32)
    src = torch.tensor([-1, 2, -1, -1, -1, -1, -1, -1, -1], dtype=torch.int32)
    slots = torch.tensor([0, 1, -1, 2, 2, 3, 4, 4, 4], dtype=torch.int32)
    out = ops.history_mark(hist, tokens, slots, src, last, _bits(V, [34]), V)
    assert out is hist
    want = torch.zeros(5, W, dtype=torch.int32)
    want[0] = _bits(V, [3])
    want[1] = _bits(V, [99])      # last_ids[2], not tokens[1]
    want[4] = _bits(V, [64, 65, 31])
    assert torch.equal(hist, want) and hist[4, 0] == -2 ** 31
    ops.history_mark(hist, tokens, slots, src, last, None, V)  # idempotent; the exempt id now recorded
    want[3] = _bits(V, [34])
    assert torch.equal(hist, want)
    # a slot outside the table is ignored; without `vocab` every bit of the row is an id
    ops.history_mark(hist, torch.tensor([5, 127], dtype=torch.int32), torch.tensor([9, 2], dtype=torch.int32))
    want[2] = _bits(128, [127])
    assert torch.equal(hist, want)
    ops.history_reset(hist, [1, 4, 17])
    want[1] = 0
    want[4] = 0
    assert torch.equal(hist, want)


def test_select_mark_select_moves_to_the_runner_up():
    V = 64
    logits = torch.zeros(1, V, dtype=torch.bfloat16)
    logits[0, 17], logits[0, 40] = 5.0, 4.5  # A = 17, B = 40
    masks = torch.full((2, 2), -1, dtype=torch.int32)
    midx = torch.tensor([1], dtype=torch.int32)
    slots = torch.tensor([2], dtype=torch.int32)
    for flags, second in ((None, 40), (torch.tensor([0, 1], dtype=torch.int32), 40),
                          (torch.tensor([1, 0], dtype=torch.int32), 17)):
        hist = torch.zeros(4, 2, dtype=torch.int32)
        pen = ops.Penalty(hist, slots, 1.3, 0.5, flags)
        first = ops.masked_argmax(logits, masks, V, None, midx, penalty=pen)
        ops.history_mark(hist, first, slots)
        again = ops.masked_argmax(logits, masks, V, None, midx, penalty=pen)
        assert (int(first), int(again)) == (17, second)


def test_penalty_arguments_are_checked():
    hist = torch.zeros(4, 8, dtype=torch.int32)
    slots = torch.zeros(3, dtype=torch.int32)
    logits = torch.zeros(3, 256, dtype=torch.bfloat16)
    for theta in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="theta"):
            ops.masked_argmax(logits, penalty=ops.Penalty(hist, slots, theta))
    for alpha in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            ops.masked_argmax(logits, penalty=ops.Penalty(hist, slots, 1.1, alpha))
    with pytest.raises(ValueError, match="history"):
        ops.masked_argmax(logits, penalty=ops.Penalty(hist[:, :7], slots, 1.1))
    with pytest.raises(ValueError, match="slots"):
        ops.masked_argmax(logits, penalty=ops.Penalty(hist, torch.tensor([0, 1, 4], dtype=torch.int32), 1.1))
    with pytest.raises(ValueError, match="rows"):
        ops.masked_argmax(logits, penalty=ops.Penalty(hist, slots, 1.1, 0.0, torch.ones(2, dtype=torch.int32)))
