"""The needle-key harness (tests/needles.py) discriminates before it is
trusted: its comparison passes the fp64 reference and rejects every
single-key mutant of it -- a key dropped, one key too many read from each slot
a row must not read, a key counted twice, two V rows swapped -- at short and
long rows, for bf16 and fp8 K / V.  (The suite's randn attention tests pass
most of these mutants from 257 keys on; see docs/KERNELS.md.)  No GPU."""
import pytest
import torch

from tests import needles
from tests.needles import Seq

D, HQ, HKV = 64, 8, 2
OWN, PARENT, PREFIX = 0, 1, 2
LAYOUT = {33: (5, 20), 257: (45, 45 + 77), 1000: (300, 900)}  # L -> (P, fend)


def _points(L):
    """The key positions the mutants hit: both ends, a 32-key tile edge and
    its predecessor, both sides of the prefix end and of the fork end."""
    P, fend = LAYOUT[L]
    tile = (L - 1) // 32 * 32 if L < 64 else (L // 2) // 32 * 32
    return dict(first=0, last=L - 1, tile=tile, tile_pred=tile - 1, p_pred=P - 1, p=P, fend_pred=fend - 1, fend=fend)


@pytest.fixture(scope="module", params=[(L, kv) for L in (33, 257, 1000) for kv in ("bf16", "fp8")],
                ids=lambda p: f"L{p[0]}-{p[1]}")
def case(request):
    """Row 0: a single-needle head per point; row 1: each point paired with
    the key half a row away (another tile, split or source)."""
    L, kv = request.param
    P, fend = LAYOUT[L]
    pts = list(_points(L).values())
    assert len(pts) == HQ
    ta = torch.tensor([pts, pts])
    tb = torch.tensor([[-1] * HQ, [(p + L // 2) % L for p in pts]])
    seq = Seq(L, OWN, P, PREFIX, fend, PARENT)
    c = needles.build(D, HQ, HKV, kv, [seq], [0, 0], [L, L], ta, tb, seed=L)
    exp, bound = c.decode_expected()
    return c, exp, bound, _points(L)


def _mutant(c, drop=None, extra=None, twice=None, swap=None):
    """Both rows' fp64 attention over a mutated read list."""
    out = []
    for r in range(2):
        k = c.reads(r)
        v = list(k)
        if drop is not None:
            del k[drop], v[drop]
        if extra is not None:
            k.append(extra), v.append(extra)
        if twice is not None:
            k.append(k[twice]), v.append(v[twice])
        if swap is not None:
            v[swap], v[swap + 1] = v[swap + 1], v[swap]
        out.append(c.attend(r, k, v))
    return torch.stack(out)


def _heads_on(c, key):
    """[2, Hq] bool: the heads with ``key`` among their targets."""
    return (c.ta == key) | (c.tb == key)


def test_reference_passes_and_is_the_needle_row(case):
    c, exp, bound, _ = case
    assert needles.assert_within_bound(exp, exp, bound, "reference") == 0.0
    assert needles.assert_within_bound(exp.to(torch.bfloat16), exp, bound, "bf16 reference") <= 0.5
    c.check_single_needles(exp)
    # the explicit read list is the reference's own reading of the layout
    same = _mutant(c)
    assert float((same - exp).abs().max()) < 1e-12
    # preconditions as recorded: one needle owns the head, a pair shares it
    single, pair = c.tb < 0, c.tb >= 0
    assert float(c.wa[single].min()) >= needles.SINGLE_MIN
    assert float(torch.minimum(c.wa, c.wb)[pair].min()) >= needles.PAIR_EACH_MIN
    assert float((c.wa + c.wb)[pair].min()) >= needles.PAIR_SUM_MIN


@pytest.mark.parametrize("point", ["first", "last", "tile", "tile_pred", "p_pred", "p", "fend_pred", "fend"])
def test_dropped_key_is_rejected(case, point):
    c, exp, bound, pts = case
    key = pts[point]
    r = needles.error_ratio(_mutant(c, drop=key), exp, bound).amax(-1)
    on = _heads_on(c, key)
    assert bool((r[on] > 1).all()), f"dropping key {key} passed: {r[on].tolist()}"
    with pytest.raises(AssertionError):
        needles.assert_within_bound(_mutant(c, drop=key), exp, bound)


@pytest.mark.parametrize("which", ["past_end", "own_copy_of_prefix", "parent_past_fork", "prefix_slot_past_prefix"])
def test_one_extra_key_is_rejected(case, which):
    """Each forbidden position holds a decoy shadowing a key some head is
    aimed at: reading it hands that head the marker."""
    c, exp, bound, pts = case
    L, (P, fend) = c.seqs[0].L, LAYOUT[c.seqs[0].L]
    slot, pos, shadowed = {"past_end": (OWN, L, 0), "own_copy_of_prefix": (OWN, P - 1, P - 1),
                           "parent_past_fork": (PARENT, fend, fend),
                           "prefix_slot_past_prefix": (PREFIX, P, P)}[which]
    got = _mutant(c, extra=(slot, pos))
    r = needles.error_ratio(got, exp, bound).amax(-1)
    on = _heads_on(c, shadowed)[0]  # the single-needle row
    assert bool((r[0][on] > 1).all())
    assert float((got[0][on] - needles.MARKER).abs().max()) < 1e-3  # the marker, whole


def test_key_counted_twice_is_rejected_by_the_pairs(case):
    c, exp, bound, pts = case
    key = pts["tile"]
    r = needles.error_ratio(_mutant(c, twice=key), exp, bound).amax(-1)
    on = _heads_on(c, key)
    assert bool((r[1][on[1]] > 1).all()), "a key counted twice passed the two-needle heads"
    assert bool((r[0][on[0]] <= 1).all())  # a lone needle cannot see it: that is what the pairs are for


@pytest.mark.parametrize("point", ["tile_pred", "p_pred", "fend_pred"])
def test_swapped_v_rows_are_rejected(case, point):
    c, exp, bound, pts = case
    key = pts[point]
    r = needles.error_ratio(_mutant(c, swap=key), exp, bound).amax(-1)
    assert bool((r[_heads_on(c, key) | _heads_on(c, key + 1)] > 1).all())


def test_decoys_fill_every_forbidden_position(case):
    c, _, _, _ = case
    s = c.seqs[0]
    k, v = needles.decode(c.kc), needles.decode(c.vc)
    real = torch.zeros(3, c.maxs, dtype=torch.bool)
    real[PREFIX, :s.P] = real[PARENT, s.P:s.fork_end] = real[OWN, s.fork_end:s.L] = True
    assert bool((v.transpose(1, 2)[~real] == needles.MARKER).all())
    want = needles.decode(needles.reference.kv_encode(
        needles.DECOY_GAIN * c.khat[0][:, torch.arange(c.maxs) % s.L], c.kc.dtype))
    for slot in range(3):
        hole = ~real[slot]
        assert torch.equal(k[slot][:, hole], want[:, hole])
    # and the real keys, each in exactly one slot
    assert int(real.sum()) == s.L and int(real.any(0).sum()) == s.L
    for slot, a, b in ((PREFIX, 0, s.P), (PARENT, s.P, s.fork_end), (OWN, s.fork_end, s.L)):
        assert torch.equal(k[slot][:, a:b], c.khat[0][:, a:b]) and torch.equal(v[slot][:, a:b], c.vhat[0][:, a:b])
    assert all(c.reads(0)[j] == (s.source(j), j) for j in (0, s.P - 1, s.P, s.fork_end - 1, s.fork_end, s.L - 1))


def test_builder_refuses_inputs_without_a_needle():
    """A query too weak to single out its key fails the precondition, before
    any kernel could be blamed."""
    ta, _ = needles.sweep_targets(257, HQ)
    with pytest.raises(AssertionError, match="single needle"):
        needles.build(D, HQ, HKV, "bf16", [Seq(257, 0)], [0] * len(ta), [257] * len(ta), ta, c1=1.0)
    ta, tb = needles.sweep_targets(257, HQ, pairs=True)
    with pytest.raises(AssertionError, match="pair"):
        needles.build(D, HQ, HKV, "bf16", [Seq(257, 0)], [0] * len(ta), [257] * len(ta), ta, tb, c2=2.0)


def test_sweep_targets_cover_every_key():
    for L, Hq in ((33, 32), (257, 24), (1000, 16), (1024, 8), (45, 12)):
        ta, tb = needles.sweep_targets(L, Hq, pairs=True)
        assert ta.shape[0] == -(-L // Hq) and set(ta.flatten().tolist()) == set(range(L))
        assert bool(((tb - ta) % L == L // 2).all())


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("T,start,P", [(1, 0, 0), (37, 0, 0), (40, 45, 45), (5, 256, 256)])
def test_prefill_targets_and_causal_leak(kv, T, start, P):
    """The prefill cycle reaches every kind that exists; the fp64 reference
    passes; a mask that lets each query see one key too many is rejected (the
    future-key heads return that key's V row, or the decoy past the end the
    marker)."""
    Hq, Hkv = 8, 2
    ta = needles.prefill_targets(T, start, P, Hq, seed=T)
    vis = torch.arange(start + 1, start + T + 1)
    seq = Seq(start + T, OWN, P, PREFIX if P else None)
    c = needles.build(D, Hq, Hkv, kv, [seq], [0] * T, vis, ta, seed=T + start, n_slots=3)
    exp, bound = c.prefill_expected()
    c.check_single_needles(exp)
    assert needles.assert_within_bound(exp, exp, bound) == 0.0
    pos = vis[:, None] - 1
    if T >= 22:
        assert bool((ta == pos).any()) and bool((ta == pos + 1).any()) and bool((ta == 0).any())
        assert bool((ta == pos // 32 * 32).any()) and bool((ta == start).any())
        if P:
            assert bool((ta == P - 1).any()) and bool((ta == P).any())
    assert bool((ta <= pos + 1).all()) and bool((ta[-1] <= pos[-1]).all())
    # the leak: every row reads the next cache position of its slot too
    leak = torch.stack([c.attend(r, c.reads(r) + [(OWN, int(vis[r]))]) for r in range(T)])
    r = needles.error_ratio(leak, exp, bound).amax(-1)
    if bool(c.future.any()):
        assert bool((r[c.future] > 1).all())
    assert bool((r[-1][c.ta[-1] == 0] > 1).all())  # past the end: the decoy shadowing key 0
