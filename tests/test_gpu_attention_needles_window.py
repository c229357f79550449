"""The sliding window cuts the logical sequence at the right key: the windowed
decode kernels (decode_attn_mfma_kernel / decode_attn_combine_kernel WIN, the
shared-prefix partials of prefill_attn_win_kernel) and the windowed prefill
kernels (single sequence, key-split, varlen) on the needle inputs of
tests/needles_window.py, against ``dmcp.ops.reference`` in fp64 on the decoded
caches, within REL * sum_k p_k |V_k| + ABS per element (tests/needles.py).

One head per kv head is aimed at the first visible key; the position below it
-- in the own slot, the prefix slot or the fork parent's -- holds a decoy that
hands a marker value to that head.  tests/test_attention_needles_window.py
shows on the CPU that a window one key too wide or too narrow, a bound rounded
to a tile, a window that ignores the prefix and a prefix or parent left visible
each break this bound.

MAXS = 512, D = 64 / 128, GQA groups 1 / 4, caches bf16 / fp8 / fp8s, W = 33 /
64 / 100.  Each test prints its largest error / bound."""
import pytest
import torch

from tests import needles_window as nw
from tests.needles import assert_within_bound

pytestmark = pytest.mark.gpu

GEOMS = [(64, 1), (64, 4), (128, 1), (128, 4)]  # (D, GQA group); two kv heads each
# (chunk, splits): one split per row; three; and sixteen parts of >= 32 keys for
# spans of at most 2 W + 5 keys -- most parts hold no key
PLANS = [(256, 1), (32, 3), (32, 16)]

_EXPECTED = {}


def _case(kind, D, G, kv, W):
    """The case on the GPU with its fp64 expectation (computed once, on the CPU)."""
    key = (kind, D, G, kv, W)
    if key not in _EXPECTED:
        c = (nw.decode_case if kind == "decode" else nw.prefill_case)(D, G, kv, W)
        exp, bound = c.decode_expected() if kind == "decode" else c.prefill_expected()
        _EXPECTED[key] = (c.to("cuda"), exp.cuda(), bound.cuda())
    return _EXPECTED[key]


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _check(got, exp, bound, what):
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    return assert_within_bound(got, exp, bound, what)


@pytest.mark.parametrize("W", nw.WINDOWS)
@pytest.mark.parametrize("kv", nw.KVS)
@pytest.mark.parametrize("D,G", GEOMS)
def test_decode_window(hip, D, G, kv, W):
    """Rows of W - 1, W, W + 1, W + 31 and 2 W + 5 keys off the prefix
    (prefix.rows 0), rows behind the shared prefix with the window's first key
    below, at and above P, and fork branches with it below, at and above the
    fork end -- one batch, every split plan."""
    c, exp, bound = _case("decode", D, G, kv, W)
    slot, lens, pre, fork = c.decode_inputs()
    worst = 0.0
    for chunk, splits in PLANS:
        got = hip.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, chunk=chunk, prefix=pre, splits=splits,
                                   fork=fork, kv_scale=c.kv_scale, window=W)
        worst = max(worst, _check(got, exp, bound, f"decode D={D} G={G} {kv} W={W} chunk {chunk} splits {splits}"))
    print(f"\nwindow needle error/bound [decode D={D} G={G} {kv} W={W}] = {worst:.4f}")


@pytest.mark.parametrize("W", nw.WINDOWS)
@pytest.mark.parametrize("kv", nw.KVS)
@pytest.mark.parametrize("D,G", GEOMS)
def test_prefill_window(hip, D, G, kv, W):
    """T = 70 and T = 150 from start 0 and an extend at start 90 behind a
    prefix: each alone with nsplit 1 and 3 (both wave variants at nsplit 1),
    then the three as one varlen pack."""
    c, exp, bound = _case("prefill", D, G, kv, W)
    offsets, slots, starts, pslot, plens = c.prefill_tables()
    worst = 0.0
    for i, s in enumerate(c.seqs):
        a, b = offsets[i], offsets[i + 1]
        for variant, nsplit in ((0, 1), (0, 3), (1, 1)):
            got = hip.prefill_attention(c.q[a:b].contiguous(), c.kc, c.vc, slots[i], starts[i],
                                        pslot if plens[i] else None, plens[i], c.scale, variant=variant,
                                        nsplit=nsplit, kv_scale=c.kv_scale, window=W)
            worst = max(worst, _check(got, exp[a:b], bound[a:b],
                                      f"prefill seq {i} D={D} G={G} {kv} W={W} variant {variant} nsplit {nsplit}"))
    got = hip.prefill_attention_varlen(c.q, c.kc, c.vc, offsets, slots, starts, pslot, plens, c.scale,
                                       kv_scale=c.kv_scale, window=W)
    worst = max(worst, _check(got, exp, bound, f"varlen D={D} G={G} {kv} W={W}"))
    print(f"\nwindow needle error/bound [prefill D={D} G={G} {kv} W={W}] = {worst:.4f}")


def test_window_zero_and_large_are_the_unwindowed_kernels(hip):
    """window = 0 runs the earlier entry points; a window past every length
    runs the windowed ones over every key: the same values either way."""
    c, _, _ = _case("decode", 64, 4, "fp8", 64)
    slot, lens, pre, fork = c.decode_inputs()
    base = hip.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, chunk=32, prefix=pre, splits=3, fork=fork)
    zero = hip.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, chunk=32, prefix=pre, splits=3, fork=fork,
                                window=0)
    wide = hip.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, chunk=32, prefix=pre, splits=3, fork=fork,
                                window=nw.MAXS)
    assert torch.equal(base, zero)
    torch.testing.assert_close(wide.float(), base.float(), atol=2e-2, rtol=2 ** -7)
