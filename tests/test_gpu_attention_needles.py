"""Every key read once, from the right slot: the decode attention kernels
(decode_attn_mfma_kernel + decode_attn_combine_kernel + the shared-prefix
partials) and the prefill kernels (single sequence, varlen) on needle-key
inputs (tests/needles.py), against ``dmcp.ops.reference`` in fp64 on the
decoded caches, within REL * sum_k p_k |V_k| + ABS per element.

Each head is aimed at one key (its output is that key's V row) or at two
(both sides of every merge carry weight); every position a row must not read
-- past its length, the own slot under the prefix and the fork, the parent
slot outside the fork range, the prefix slot past the prefix -- holds a decoy
that hands a marker value to the head it shadows.  tests/test_attention_needles.py
shows on the CPU that this comparison rejects every single-key mutant.

Largest error / bound measured on an MI355X (bf16 / fp8 KV): decode sweeps
0.81 / 0.76, through the fork table 0.67 / 0.73, alternating prefix.rows
0.63 / 0.71, prefill 0.82 / 0.77, varlen prefill 0.81 / 0.85 (docs/KERNELS.md,
"What the attention tests can and cannot see").  Each test prints its own."""
import os

import pytest
import torch

from tests import needles
from tests.needles import Seq

pytestmark = pytest.mark.gpu

MAXS = 1024
OWN, PARENT, PREFIX = 0, 1, 2
GEOMS = [(64, 32, 8), (128, 24, 8), (64, 16, 2), (64, 8, 8), (128, 12, 2), (64, 8, 4)]  # G = 4, 3, 8, 1, 6, 2
KVS = ["bf16", "fp8"]
PLANS = [(64, 1), (64, 3), (64, 6), (256, None)]  # (chunk, splits); None = the default MAXS / chunk
PREFIX_SPLITS = ("1", "5", "16")
# (L, P); L == P: rows with no keys of their own
SWEEP = [(33, 0), (257, 0), (257, 45), (1000, 0), (1000, 45), (1000, 300), (1024, 0), (1024, 300), (45, 45),
         (300, 300)]


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _report(family, worst):
    print(f"\nneedle error/bound [{family}] = {worst:.4f}")


def _decode_launches(hip, c, exp, bound, what):
    """The case through every (chunk, splits) plan -- and, with a prefix, every
    DMCP_PREFIX_SPLITS -- each within the bound; returns the worst ratio."""
    slot, lens, pre, fork = c.decode_inputs()
    worst = 0.0
    for chunk, splits in PLANS:
        for sp in (PREFIX_SPLITS if pre is not None else (None,)):
            if sp is not None:
                os.environ["DMCP_PREFIX_SPLITS"] = sp
            try:
                got = hip.decode_attention(c.q, c.kc, c.vc, slot, lens, c.scale, chunk=chunk, prefix=pre,
                                           splits=splits, fork=fork)
            finally:
                if sp is not None:
                    os.environ.pop("DMCP_PREFIX_SPLITS")
            worst = max(worst, needles.assert_within_bound(
                got, exp, bound, f"{what} chunk {chunk} splits {splits} prefix splits {sp}"))
    return worst


def _sweep(hip, D, Hq, Hkv, kv, seq, seed):
    """Both sweeps of one sequence: every key a single needle, then every key
    paired with the one half a row away."""
    worst = 0.0
    for pairs in (False, True):
        ta, tb = needles.sweep_targets(seq.L, Hq, pairs)
        B = ta.shape[0]
        c = needles.build(D, Hq, Hkv, kv, [seq], [0] * B, [seq.L] * B, ta, tb, n_slots=3, maxs=MAXS,
                          seed=seed + pairs).to("cuda")
        exp, bound = c.decode_expected()
        c.check_single_needles(exp)
        worst = max(worst, _decode_launches(hip, c, exp, bound, f"{seq} pairs={pairs}"))
    return worst


@pytest.mark.parametrize("kv", KVS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=[f"D{d}-Hq{q}-Hkv{k}" for d, q, k in GEOMS])
def test_decode_sweep(hip, gi, kv):
    """B = ceil(L / Hq) rows of one sequence, head h of row b aimed at key
    (b Hq + h) mod L: one launch shows every key position read with its own V,
    for every split plan and prefix split count."""
    D, Hq, Hkv = GEOMS[gi]
    worst = 0.0
    for i, (L, P) in enumerate(SWEEP):
        seq = Seq(L, OWN, P, PREFIX if P else None)
        worst = max(worst, _sweep(hip, D, Hq, Hkv, kv, seq, seed=100 * gi + i))
    _report(f"decode {kv}", worst)


@pytest.mark.parametrize("kv", KVS)
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=[f"D{d}-Hq{q}-Hkv{k}" for d, q, k in GEOMS])
def test_decode_sweep_fork_table(hip, gi, kv):
    """The same sweeps through the fork table: keys [P, fend) in the parent
    slot, the fork point inside a 32-key tile, on a tile edge, deep in the row
    and past its length; parent and own slot carry decoys in each other's
    ranges.  Expected: the fp64 reference through the same table."""
    D, Hq, Hkv = GEOMS[gi]
    worst = 0.0
    cases = [(L, P, fo) for L, P in ((257, 0), (1000, 300), (1000, 0), (257, 45)) for fo in (77, 96, 600, 2000)]
    for i, (L, P, fo) in enumerate(cases):
        fend = P + fo if fo < 2000 else L + 7
        seq = Seq(L, OWN, P, PREFIX if P else None, fend, PARENT)
        worst = max(worst, _sweep(hip, D, Hq, Hkv, kv, seq, seed=1000 + 100 * gi + i))
    _report(f"decode fork {kv}", worst)


@pytest.mark.parametrize("kv", KVS)
@pytest.mark.parametrize("D,Hq,Hkv", [(64, 32, 8), (128, 12, 2)])
def test_decode_rows_off_the_prefix(hip, D, Hq, Hkv, kv):
    """prefix.rows: flagged and unflagged rows alternate in one launch.  The
    flagged rows' slot holds decoys under P (their keys [0, P) are the prefix
    slot's); the unflagged rows' slot holds its own real keys there, and the
    prefix slot's rows are another sequence's to them."""
    L, P = 700, 300
    seqs = [Seq(L, OWN, P, PREFIX), Seq(L, PARENT)]  # the second sequence owns slot 1 whole
    worst = 0.0
    for pairs in (False, True):
        ta, tb = needles.sweep_targets(L, Hq, pairs)
        B = ta.shape[0]
        row_seq = torch.arange(2 * B) % 2
        ta2 = ta.repeat_interleave(2, 0)
        tb2 = None if tb is None else tb.repeat_interleave(2, 0)
        c = needles.build(D, Hq, Hkv, kv, seqs, row_seq, [L] * (2 * B), ta2, tb2, n_slots=3, maxs=MAXS,
                          seed=7 + pairs).to("cuda")
        slot, lens, pre, fork = c.decode_inputs()
        assert fork is None and pre.rows.tolist() == [1, 0] * B
        exp, bound = c.decode_expected()
        c.check_single_needles(exp)
        worst = max(worst, _decode_launches(hip, c, exp, bound, f"prefix.rows pairs={pairs}"))
    _report(f"decode prefix.rows {kv}", worst)


PREFILL_GEOMS = [(64, 32, 8), (64, 24, 8), (128, 16, 2)]
PREFILL_CASES = [(1, 0, 0), (37, 0, 0), (129, 45, 45), (200, 700, 513), (5, 256, 256)]


@pytest.mark.parametrize("kv", KVS)
@pytest.mark.parametrize("T,start,P", PREFILL_CASES)
@pytest.mark.parametrize("D,Hq,Hkv", PREFILL_GEOMS)
def test_prefill_needles(hip, D, Hq, Hkv, T, start, P, kv):
    """Token t / head h cycles its needle through the diagonal key and the
    one before, key 0, both sides of the prefix end and of ``start``, the last
    32-key tile edge at or below its position and that edge's predecessor, a
    random visible key -- and the key after its own, which it must not see
    (expected: the reference's answer without it).  Decoys past start + T and
    in the own slot under the prefix."""
    ta = needles.prefill_targets(T, start, P, Hq, seed=T + start)
    vis = torch.arange(start + 1, start + T + 1)
    seq = Seq(start + T, OWN, P, PREFIX if P else None)
    c = needles.build(D, Hq, Hkv, kv, [seq], [0] * T, vis, ta, n_slots=3, maxs=MAXS, seed=T + start + D).to("cuda")
    exp, bound = c.prefill_expected()
    c.check_single_needles(exp)
    worst = 0.0
    for variant in hip.PREFILL_VARIANTS[D]:
        for nsplit in (1, 3):
            got = hip.prefill_attention(c.q, c.kc, c.vc, OWN, start, PREFIX if P else None, P, c.scale,
                                        variant=variant, nsplit=nsplit)
            worst = max(worst, needles.assert_within_bound(got, exp, bound, f"variant {variant} nsplit {nsplit}"))
    _report(f"prefill {kv}", worst)


@pytest.mark.parametrize("kv", KVS)
@pytest.mark.parametrize("D,Hq,Hkv", PREFILL_GEOMS)
def test_prefill_varlen_needles(hip, D, Hq, Hkv, kv):
    """One packed launch over the sequence mix of
    test_prefill_varlen_matches_per_sequence_reference with the same target
    cycle; decoys past each sequence's end, under the prefix in the own slots
    and past the prefix in the prefix slot."""
    P, pslot = 300, 7
    mix = [(1, P, P), (157, P, P), (33, 0, 0), (260, P, P), (5, 0, 0), (96, 512, 0)]  # (T, start, prefix len)
    seqs = [Seq(st + T, i, pl, pslot if pl else None) for i, (T, st, pl) in enumerate(mix)]
    row_seq = torch.cat([torch.full((T,), i) for i, (T, _, _) in enumerate(mix)])
    vis = torch.cat([torch.arange(st + 1, st + T + 1) for T, st, _ in mix])
    ta = torch.cat([needles.prefill_targets(T, st, pl, Hq, seed=i) for i, (T, st, pl) in enumerate(mix)])
    c = needles.build(D, Hq, Hkv, kv, seqs, row_seq, vis, ta, n_slots=8, maxs=MAXS, seed=D + Hq).to("cuda")
    offsets, slots, starts, ps, plens = c.prefill_tables()
    assert ps == pslot and plens == [pl for _, _, pl in mix]
    exp, bound = c.prefill_expected()
    c.check_single_needles(exp)
    got = hip.prefill_attention_varlen(c.q, c.kc, c.vc, offsets, slots, starts, pslot, plens, c.scale)
    _report(f"prefill varlen {kv}", needles.assert_within_bound(got, exp, bound, "varlen"))
