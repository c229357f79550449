"""The ``window`` argument of the three reference attention ops
(dmcp/ops/reference.py) against a brute-force fp64 mask over an explicitly
concatenated key list: a query at logical position i attends key j iff j <= i
and j > i - W, wherever the key is stored (prefix slot, fork parent, own slot)."""
import math

import pytest
import torch

from dmcp.ops import reference
from dmcp.ops.reference import SharedPrefix

S, Hkv, G, MAXS, D = 5, 2, 2, 96, 16
Hq = Hkv * G
PREFIX, PARENT = 4, 3
P, FEND = 11, 20


@pytest.fixture(scope="module")
def caches():
    g = torch.Generator().manual_seed(7)
    return (torch.randn(S, Hkv, MAXS, D, generator=g, dtype=torch.float64),
            torch.randn(S, Hkv, MAXS, D, generator=g, dtype=torch.float64))


def _logical(kc, vc, slot, L, use_prefix, fork):
    """The keys of one row, concatenated explicitly in logical order."""
    idx = []
    for j in range(L):
        src = slot
        if fork is not None and int(fork[slot, 0]) != slot and j < min(int(fork[slot, 1]), L):
            src = int(fork[slot, 0])
        if use_prefix and j < P:
            src = PREFIX
        idx.append((src, j))
    sl = torch.tensor([a for a, _ in idx])
    ps = torch.tensor([b for _, b in idx])
    return kc[sl, :, ps].transpose(0, 1), vc[sl, :, ps].transpose(0, 1)  # [Hkv, L, D]


def _brute(q, k, v, pos, W, scale):
    """fp64 attention of one query [Hq, D] at logical position ``pos`` under the mask, key by key."""
    out = torch.zeros(Hq, D, dtype=torch.float64)
    for h in range(Hq):
        js = [j for j in range(k.shape[1]) if j <= pos and (W == 0 or j > pos - W)]
        s = torch.tensor([float(q[h] @ k[h // G, j]) * scale for j in js], dtype=torch.float64)
        p = torch.softmax(s, 0)
        out[h] = sum(p[i] * v[h // G, j] for i, j in enumerate(js))
    return out


@pytest.mark.parametrize("W", [1, 2, 7, 12, 33])
def test_decode_window_is_the_brute_force_mask(caches, W):
    kc, vc = caches
    g = torch.Generator().manual_seed(W)
    slot = torch.tensor([0, 1, 2, 1, -1], dtype=torch.int32)
    lens = torch.tensor([40, 25, 13, 30, 5], dtype=torch.int32)  # rows on the prefix hold more than P keys
    rows = torch.tensor([1, 0, 1, 1, 1], dtype=torch.int32)  # row 1 is off the shared prefix
    fork = torch.stack([torch.arange(S), torch.zeros(S, dtype=torch.long)], 1).to(torch.int32)
    fork[0] = torch.tensor([PARENT, FEND], dtype=torch.int32)
    q = torch.randn(5, Hq, D, generator=g, dtype=torch.float64)
    pre = SharedPrefix(kc[PREFIX], vc[PREFIX], torch.tensor([P], dtype=torch.int32), rows)
    scale = 1 / math.sqrt(D)
    got = reference.decode_attention(q, kc, vc, slot, lens, scale, prefix=pre, fork=fork, window=W)
    for b in range(4):
        L = int(lens[b])
        k, v = _logical(kc, vc, int(slot[b]), L, bool(rows[b]), fork)
        torch.testing.assert_close(got[b], _brute(q[b], k, v, L - 1, W, scale), atol=1e-12, rtol=1e-10)
        if W == 1:  # its own key only: the output is that key's V row
            torch.testing.assert_close(got[b], v[:, L - 1].repeat_interleave(G, 0), atol=1e-12, rtol=0)
    assert not got[4].any()  # the padding row


@pytest.mark.parametrize("W", [1, 3, 8, 30])
def test_prefill_window_is_the_brute_force_mask(caches, W):
    kc, vc = caches
    g = torch.Generator().manual_seed(W)
    scale = 1 / math.sqrt(D)
    # one prefill from 0, one extend behind the shared prefix
    offsets, slots, starts, plens = [0, 9, 21], [1, 2], [0, 17], [0, P]
    q = torch.randn(21, Hq, D, generator=g, dtype=torch.float64)
    got = reference.prefill_attention_varlen(q, kc, vc, offsets, slots, starts, PREFIX, plens, scale, window=W)
    for i in range(2):
        a, b = offsets[i], offsets[i + 1]
        one = reference.prefill_attention(q[a:b], kc, vc, slots[i], starts[i], PREFIX if plens[i] else None,
                                          plens[i], scale, window=W)
        assert torch.equal(one, got[a:b])
        k, v = _logical(kc, vc, slots[i], starts[i] + (b - a), bool(plens[i]), None)
        for t in range(b - a):
            exp = _brute(q[a + t], k, v, starts[i] + t, W, scale)
            torch.testing.assert_close(got[a + t], exp, atol=1e-12, rtol=1e-10)
            if W == 1:
                torch.testing.assert_close(got[a + t], v[:, starts[i] + t].repeat_interleave(G, 0), atol=1e-12,
                                           rtol=0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16])
def test_window_zero_or_past_the_length_is_the_unwindowed_op_bit_for_bit(caches, dtype):
    kc, vc = (c.to(dtype) for c in caches)
    g = torch.Generator().manual_seed(1)
    scale = 1 / math.sqrt(D)
    slot = torch.tensor([0, 1], dtype=torch.int32)
    lens = torch.tensor([40, 25], dtype=torch.int32)
    q = torch.randn(2, Hq, D, generator=g, dtype=torch.float64).to(dtype)
    pre = SharedPrefix(kc[PREFIX], vc[PREFIX], torch.tensor([P], dtype=torch.int32))
    base = reference.decode_attention(q, kc, vc, slot, lens, scale, prefix=pre)
    for W in (0, None, 40, 41, MAXS):
        assert torch.equal(reference.decode_attention(q, kc, vc, slot, lens, scale, prefix=pre, window=W), base)
    assert not torch.equal(reference.decode_attention(q, kc, vc, slot, lens, scale, prefix=pre, window=39), base)
    qp = torch.randn(12, Hq, D, generator=g, dtype=torch.float64).to(dtype)
    base = reference.prefill_attention(qp, kc, vc, 2, 17, PREFIX, P, scale)
    for W in (0, None, 29, 30, MAXS):
        assert torch.equal(reference.prefill_attention(qp, kc, vc, 2, 17, PREFIX, P, scale, window=W), base)
    assert not torch.equal(reference.prefill_attention(qp, kc, vc, 2, 17, PREFIX, P, scale, window=28), base)
    vb = reference.prefill_attention_varlen(qp, kc, vc, [0, 12], [2], [17], PREFIX, [P], scale)
    for W in (0, None, 29, MAXS):
        assert torch.equal(reference.prefill_attention_varlen(qp, kc, vc, [0, 12], [2], [17], PREFIX, [P], scale,
                                                              window=W), vb)


def test_bad_windows_are_value_errors(caches):
    kc, vc = caches
    q = torch.zeros(1, Hq, D, dtype=torch.float64)
    one = torch.ones(1, dtype=torch.int32)
    for bad in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="window"):
            reference.decode_attention(q, kc, vc, one, one, 1.0, window=bad)
        with pytest.raises(ValueError, match="window"):
            reference.prefill_attention(q, kc, vc, 1, 0, window=bad)
        with pytest.raises(ValueError, match="window"):
            reference.prefill_attention_varlen(q, kc, vc, [0, 1], [1], [0], window=bad)
