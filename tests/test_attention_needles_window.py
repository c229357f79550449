"""CPU: the sliding-window needle harness (tests/needles_window.py) tells a
right window from a wrong one, and the reference ops stay inside its bound.

Each wrong reader -- a window of W + 1 keys, of W - 1 keys, a lower bound
rounded down to a 32-key tile, a window counted from the own-slot keys only,
the whole prefix left visible, the fork parent's keys left visible -- must
break the REL / ABS bound of tests/needles.py on at least one row of the
listed decode batch; the true reader and the fp32 reference ops must stay
inside it on every row."""
import pytest
import torch

from dmcp.ops import reference
from tests import needles_window as nw
from tests.needles import MARKER, error_ratio


@pytest.fixture(scope="module")
def dec():
    """The decode batch per (kv, W) at D = 64, G = 4, with its fp64 expectation (computed once)."""
    out = {}
    for kv in nw.KVS:
        for W in nw.WINDOWS:
            c = nw.decode_case(64, 4, kv, W)
            out[kv, W] = (c, *c.decode_expected())
    return out


def _reader_ratio(c, exp, bound, kind):
    got = torch.stack([c.attend(r, nw.reader_keys(c, r, kind)) for r in range(len(c.row_seq))])
    return error_ratio(got, exp, bound).amax(dim=(1, 2))  # per row


@pytest.mark.parametrize("W", nw.WINDOWS)
@pytest.mark.parametrize("kv", nw.KVS)
def test_true_reader_and_reference_are_inside_the_bound(dec, kv, W):
    c, exp, bound = dec[kv, W]
    assert float(_reader_ratio(c, exp, bound, "true").max()) < 1e-6
    slot, lens, pre, fork = c.decode_inputs()
    got = reference.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, prefix=pre, fork=fork,
                                     kv_scale=c.kv_scale, window=W)
    worst = float(error_ratio(got, exp, bound).max())
    print(f"decode reference {kv} W={W}: error / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0
    # head 0 of a row whose window is cut returns the first visible key's V row, not the marker
    for r in range(len(c.row_seq)):
        if c.lo(r) >= 1:
            assert float((got[r, 0].double() - c.vhat[c.row_seq[r]][0, c.lo(r)]).abs().max()) < 0.1
            assert float((got[r, 0].double() - MARKER).abs().min()) > 1.0


@pytest.mark.parametrize("kind", nw.WRONG_READERS)
@pytest.mark.parametrize("W", nw.WINDOWS)
def test_wrong_readers_break_the_bound(dec, W, kind):
    for kv in nw.KVS:
        c, exp, bound = dec[kv, W]
        ratio = _reader_ratio(c, exp, bound, kind)
        broken = [nw.DECODE_ROWS[r] for r in range(len(ratio)) if ratio[r] > 1.0]
        print(f"{kind} {kv} W={W}: breaks {broken}")
        assert broken, f"reader {kind!r} passes every row of the {kv} W={W} batch"


def test_wrong_readers_break_where_expected(dec):
    """The rows each wrong reader must fail on (bf16, W = 64): the decoy sits
    exactly one key below the window, wherever that key is stored."""
    c, exp, bound = dec["bf16", 64]
    rows = {k: i for i, k in enumerate(nw.DECODE_ROWS)}
    need = {"W+1": ("W+1", "2W+5", "lo<P", "lo==P", "lo>P", "lo<fork", "lo==fork", "lo>fork"),
            "W-1": nw.DECODE_ROWS[1:],            # every row of at least W keys loses its first key
            "tile": ("W+1", "2W+5", "lo<P"),       # lo = 1, 69 and 57: off a tile edge
            "own-only": ("lo<P",),                 # the window reaches into the prefix; the reader stops at P
            "prefix": ("lo==P", "lo<P"),           # the decoy at lo - 1 is a prefix key and comes back
            "parent": ("lo==fork",)}               # ... or a parent key
    for kind, names in need.items():
        ratio = _reader_ratio(c, exp, bound, kind)
        for n in names:
            assert ratio[rows[n]] > 1.0, (kind, n, float(ratio[rows[n]]))
    # and a full-attention reader fails every row longer than the window
    full = torch.stack([c.attend(r, range(c.row_vis[r])) for r in range(len(c.row_seq))])
    ratio = error_ratio(full, exp, bound).amax(dim=(1, 2))
    assert all(ratio[r] > 1.0 for r in range(len(ratio)) if c.lo(r) >= 1)


@pytest.mark.parametrize("W", nw.WINDOWS)
@pytest.mark.parametrize("kv", ["bf16", "fp8s"])
def test_prefill_reference_is_inside_the_bound(kv, W):
    c = nw.prefill_case(64, 4, kv, W)
    exp, bound = c.prefill_expected()
    offsets, slots, starts, pslot, plens = c.prefill_tables()
    got = reference.prefill_attention_varlen(c.q, c.kc, c.vc, offsets, slots, starts, pslot, plens, c.scale,
                                             kv_scale=c.kv_scale, window=W)
    worst = float(error_ratio(got, exp, bound).max())
    print(f"prefill reference {kv} W={W}: error / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0
    # the unwindowed op fails it: every probed query past the window sees its decoy
    full = reference.prefill_attention_varlen(c.q, c.kc, c.vc, offsets, slots, starts, pslot, plens, c.scale,
                                              kv_scale=c.kv_scale)
    ratio = error_ratio(full, exp, bound).amax(dim=(1, 2))
    cut = [r for r in range(len(c.row_seq)) if c.probe[r] and c.lo(r) >= 1]
    assert cut and all(ratio[r] > 1.0 for r in cut)
    # so does a window one key wider or narrower
    for w in (W + 1, W - 1):
        off = reference.prefill_attention_varlen(c.q, c.kc, c.vc, offsets, slots, starts, pslot, plens, c.scale,
                                                 kv_scale=c.kv_scale, window=w)
        ratio = error_ratio(off, exp, bound).amax(dim=(1, 2))
        assert all(ratio[r] > 1.0 for r in cut), w
