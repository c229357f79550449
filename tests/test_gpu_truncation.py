"""truncated_sample on gfx950 (csrc/truncate.hip) against the definitions of
dmcp/ops/reference.py: every test compares the kernel's ``stats`` (the bits of
tau and the kept count) with the reference exactly, as well as the ids.

Sharpness: an id-only check would pass most rows of a kernel that cut nothing,
so each case that cuts picks every row's position on the CPU (scanning a few
with the reference) such that the *untruncated* Gumbel winner lies outside the
kept set where one of the scanned positions allows it; the test asserts that
this holds in at least a quarter of the rows.  (The cases whose kept set is
all of A -- k >= |A|, one allowed id, all-equal logits -- cannot have it.)

Ambiguity: the kernel sums the top-p weights in fp32.  The reference flags a
row whose running sum next to tau_p is within 1e-4 Z of p Z (the fp32 error of
a <= 131,072-term non-negative sum is ~1e-5: a 128-term chain per thread, a
tree, 1-2 ulp of expf; the margin is 10x that).  For such a row the kernel may
report the adjacent value level, and its id must be the reference's id at
that level; at most 5 % of a case's rows may be ambiguous (asserted on the CPU
inputs: with <= 17 rows that is none).  Top-k and min-p get no such allowance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, SEED = 0.7, 20240229
SHAPES = [(B, V, ld) for V, ld in ((64, 64), (1003, 1003), (1000, 1024), (128256, 128256)) for B in (1, 3, 17)]
KNOBS = {"top_k": (20, 1.0, 0.0), "top_p": (0, 0.8, 0.0), "min_p": (0, 1.0, 0.1), "all": (20, 0.95, 0.02)}


def _knobs(name, V):
    """The case's settings; over 64 ids (about 40 allowed) top-k 20 would cut almost no mass: 4 there."""
    k, p, m = KNOBS[name]
    return (4 if k and V <= 64 else k, p, m)


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32)


def _mask_table(V, g):
    """Two dense random mask rows and the all-ones row (no bits past V)."""
    W = (V + 31) // 32
    t = torch.randint(-2**31, 2**31 - 1, (3, W), generator=g, dtype=torch.int64)
    t[2] = -1
    if V % 32:
        t[:, -1] &= (1 << (V % 32)) - 1
    return t.to(torch.int32)


def _positions(logits, masks, midx, slots, V, tau, temperature, seed, tries):
    """Per row the first of ``tries`` positions at which the untruncated
    winner has a value below tau (else the first); returns (positions, share
    of rows whose untruncated winner is outside the kept set)."""
    from dmcp.ops import reference
    B = logits.shape[0]
    pos = torch.zeros(B, dtype=torch.int32)
    hit = 0
    cand = torch.arange(100, 100 + tries, dtype=torch.int32)
    for b in range(B):
        rows = logits[b:b + 1].expand(tries, logits.shape[1])
        mrow = None if masks is None else masks[min(max(int(midx[b]), 0), masks.shape[0] - 1) if midx is not None else b][None].expand(tries, -1)
        s = reference.sample_scores(rows, mrow, V, None, slots[b:b + 1].expand(tries).contiguous(), cand,
                                    temperature, seed)
        out = logits[b, :V].float()[s.argmax(1)] < tau[b]
        if int(slots[b]) >= 0 and bool(out.any()):
            pos[b] = cand[int(torch.nonzero(out)[0])]
            hit += 1
        else:
            pos[b] = cand[0]
    return pos, hit / B


def _run_and_check(hip, logits, masks, midx, slots, pos, V, knobs, temperature=T, seed=SEED):
    """The kernel on ``logits`` (CPU bf16 [B, ld]) against the reference: ids,
    tau bits and kept counts equal on every row; an ambiguous row may sit on
    the adjacent value level with the reference's id at that level."""
    from dmcp.ops import reference
    B = logits.shape[0]
    tau, kept, amb = reference.truncation_threshold(logits, masks, V, midx, slots, temperature, *knobs)
    assert float(amb.float().mean()) <= 0.05, "inputs: too many ambiguous rows"
    want, _ = reference.truncated_sample_at(tau, logits, masks, V, midx, slots, pos, temperature, seed)
    dev = [None if t is None else t.cuda() for t in (logits, masks, midx, slots, pos)]
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    stats = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    ids = hip.truncated_sample(dev[0], dev[1], V, out, dev[2], dev[3], dev[4], temperature, seed, *knobs, stats)
    assert ids is out
    ids, st = ids.cpu(), stats.cpu()
    for b in range(B):
        got_tau = torch.tensor([st[b, 0] << 16], dtype=torch.int32).view(torch.float32)
        if bool(amb[b]) and int(st[b, 0]) != int(reference.tau_bits(tau[b:b + 1])):
            ok = reference._allowed(logits[b:b + 1], masks, V, None if midx is None else midx[b:b + 1],
                                    slots[b:b + 1])[0]
            levels = torch.unique(logits[b, :V].float()[ok]).tolist()
            i = levels.index(float(tau[b]))
            assert float(got_tau) in levels[max(i - 1, 0):i + 2], f"row {b}: tau {float(got_tau)} vs {float(tau[b])}"
            sl = slice(b, b + 1)
            w, k = reference.truncated_sample_at(got_tau, logits[sl], None if masks is None else
                                                 (masks if midx is not None else masks[sl]), V,
                                                 None if midx is None else midx[sl], slots[sl], pos[sl],
                                                 temperature, seed)
            assert (int(ids[b]), int(st[b, 1])) == (int(w), int(k)), f"row {b} (ambiguous)"
            continue
        assert int(st[b, 0]) == int(reference.tau_bits(tau[b:b + 1])), \
            f"row {b}: tau bits {int(st[b, 0]):#x}, reference {float(tau[b])}"
        assert int(st[b, 1]) == int(kept[b]), f"row {b}: kept {int(st[b, 1])} vs {int(kept[b])}"
        assert int(ids[b]) == int(want[b]), f"row {b}: id {int(ids[b])} vs {int(want[b])}"
    return ids, st


def _case(B, V, ld, seed, scale=2.5, levels=None):
    g = torch.Generator().manual_seed(seed)
    if levels is None:
        logits = (torch.randn(B, ld, generator=g) * scale).to(torch.bfloat16)
    else:
        logits = torch.tensor(levels)[torch.randint(0, len(levels), (B, ld), generator=g)].to(torch.bfloat16)
    table = _mask_table(V, g)
    midx = torch.randint(0, 3, (B,), generator=g, dtype=torch.int32)
    slots = torch.randint(0, 768, (B,), generator=g, dtype=torch.int32)
    return logits, table, midx, slots


def _sharp_case(B, V, ld, seed, knobs, temperature=T, **kw):
    """Inputs chosen on the CPU by scanning data seeds and positions with the
    reference: no more than 5 % of the rows ambiguous, and the untruncated
    winner outside the kept set in at least a quarter of them (both asserted).
    Returns (logits, table, midx, slots, positions)."""
    from dmcp.ops import reference
    tries = 32 if V <= 10000 else 16 if B <= 3 else 4
    seen = []
    for off in range(8):
        logits, table, midx, slots = _case(B, V, ld, seed + 7919 * off, **kw)
        tau, _, amb = reference.truncation_threshold(logits, table, V, midx, slots, temperature, *knobs)
        pos, share = _positions(logits, table, midx, slots, V, tau, temperature, SEED, tries)
        seen.append((float(amb.float().mean()), share))
        if seen[-1][0] <= 0.05 and share >= 0.25:
            return logits, table, midx, slots, pos
    raise AssertionError(f"inputs: no seed with <= 5 % ambiguous rows and >= 25 % cut winners: {seen}")


@pytest.mark.parametrize("name", list(KNOBS))
@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_each_filter_and_all_three(hip, B, V, ld, name):
    """ld 1,003: rows not 16-B aligned (element-wise loads); V 1,000 in ld
    1,024: whole chunks and no tail; 128,256: 15 whole trips of the chunk loop
    and a partial one; 17 rows: more than one block."""
    knobs = _knobs(name, V)
    logits, table, midx, slots, pos = _sharp_case(B, V, ld, B * 1000003 + V, knobs)
    ids, st = _run_and_check(hip, logits, table, midx, slots, pos, V, knobs)
    # two calls give identical ids and stats
    ids2, st2 = _run_and_check(hip, logits, table, midx, slots, pos, V, knobs)
    assert torch.equal(ids, ids2) and torch.equal(st, st2)


EDGE_SHAPES = [(3, 1003, 1003), (17, 1000, 1024), (3, 128256, 128256)]


@pytest.mark.parametrize("B,V,ld", EDGE_SHAPES)
def test_top_k_edges(hip, B, V, ld):
    """k >= |A| cuts nothing (tau -inf, the masked_sample id); k = 1 keeps the maximum's level."""
    from dmcp.ops import reference
    logits, table, midx, slots = _case(B, V, ld, 11 * B + V)
    pos = _i32(range(7, 7 + B))
    for k in (V, V + 1000):
        ids, st = _run_and_check(hip, logits, table, midx, slots, pos, V, (k, 1.0, 0.0))
        assert st[:, 0].tolist() == [0xFF80] * B
        assert torch.equal(ids, reference.masked_sample(logits, table, V, None, midx, slots, pos, T, SEED))
    logits, table, midx, slots, pos = _sharp_case(B, V, ld, 11 * B + V, (1, 1.0, 0.0))
    ids, st = _run_and_check(hip, logits, table, midx, slots, pos, V, (1, 1.0, 0.0))
    x = logits[:, :V].float().masked_fill(~reference._allowed(logits, table, V, midx, slots), float("-inf"))
    assert torch.equal(x[torch.arange(B), ids.long()], x.max(1).values)


@pytest.mark.parametrize("B,V,ld", EDGE_SHAPES)
def test_masks_with_one_id_and_none_and_a_padding_row(hip, B, V, ld):
    logits, _, _, slots = _case(B, V, ld, 13 * B + V)
    W = (V + 31) // 32
    table = torch.zeros((3, W), dtype=torch.int64)
    one = V - 3
    table[0, one >> 5] = 1 << (one & 31)
    table[2] = _mask_table(V, torch.Generator().manual_seed(1))[0].to(torch.int64)
    table = torch.where(table >= 2**31, table - 2**32, table).to(torch.int32)
    midx = _i32([0, 1, 2] + [2] * (B - 3))
    slots[2] = -1  # a padding row among live rows
    pos = _i32(range(5, 5 + B))
    ids, st = _run_and_check(hip, logits, table, midx, slots, pos, V, KNOBS["all"])
    assert ids[:3].tolist() == [one, 0, 0]
    assert st[:3].tolist() == [[int(logits[0, one].view(torch.int16)) & 0xFFFF, 1], [0xFF80, 0], [0xFF80, 0]]


@pytest.mark.parametrize("B,V,ld", EDGE_SHAPES)
def test_heavy_ties(hip, B, V, ld):
    """Logits quantised to four values: whole levels are kept or cut; all-equal logits: nothing is cut."""
    from dmcp.ops import reference
    for knobs in ((20, 1.0, 0.0), (0, 0.5, 0.0), (V // 2, 0.9, 0.3)):
        logits, table, midx, slots, pos = _sharp_case(B, V, ld, 17 * B + V, knobs, levels=[-2.0, 0.5, 1.25, 2.75])
        _, st = _run_and_check(hip, logits, table, midx, slots, pos, V, knobs)
        assert bool((st[:, 1] >= 20).all())
    flat = torch.full((B, ld), 0.75).to(torch.bfloat16)
    pos = _i32(range(B))
    ids, st = _run_and_check(hip, flat, table, midx, slots, pos, V, (5, 0.3, 0.9))
    assert torch.equal(ids, reference.masked_sample(flat, table, V, None, midx, slots, pos, T, SEED))
    assert st[:, 0].tolist() == [0x3F40] * B


@pytest.mark.parametrize("B,V,ld", EDGE_SHAPES)
def test_large_logits_at_a_low_temperature(hip, B, V, ld):
    """x_max ~ 300 at T = 0.1: weights are exp((x - x_max) / T) <= 1, nothing
    overflows.  (bf16 steps are 2 there, 20 nats at this temperature: the
    untruncated winner is practically always on the top level, so this case
    has no sharpness precondition; tau and the kept count are still exact.)"""
    logits, table, midx, slots = _case(B, V, ld, 19 * B + V, scale=1.5)
    logits = (logits.float() + 296).to(torch.bfloat16)
    pos = _i32(range(40, 40 + B))
    for knobs in ((0, 0.9, 0.0), (0, 1.0, 0.01), (V // 3, 0.9, 0.0)):
        _, st = _run_and_check(hip, logits, table, midx, slots, pos, V, knobs, temperature=0.1)
        assert bool((st[:, 1] >= 1).all()) and bool((st[:, 0] != 0xFF80).all())


@pytest.mark.parametrize("B,V,ld", EDGE_SHAPES)
def test_mask_idx_indirection_equals_expanded_rows(hip, B, V, ld):
    logits, table, midx, slots, pos = _sharp_case(B, V, ld, 23 * B + V, KNOBS["all"])
    midx[0] = 99  # clamped into the table: the last mask row (all ids)
    a, sa = _run_and_check(hip, logits, table, midx, slots, pos, V, KNOBS["all"])
    rows = table[midx.long().clamp(0, 2)].contiguous()
    b, sb = _run_and_check(hip, logits, rows, None, slots, pos, V, KNOBS["all"])
    c, sc = _run_and_check(hip, logits, None, None, slots, pos, V, KNOBS["all"])  # no mask: every id below V
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert bool((c < V).all())


def test_argument_checks(hip):
    logits, table, midx, slots = (t.cuda() for t in _case(3, 64, 64, 1))
    pos = _i32([1, 2, 3]).cuda()
    for kw in ({"top_k": -1}, {"top_p": 0.0}, {"top_p": 1.01}, {"min_p": 1.0}, {"min_p": -0.5}):
        with pytest.raises(hip.HipOpsError, match=next(iter(kw))):
            hip.truncated_sample(logits, table, 64, None, midx, slots, pos, T, SEED, **kw)
    with pytest.raises(hip.HipOpsError, match="stats"):
        hip.truncated_sample(logits, table, 64, None, midx, slots, pos, T, SEED, 5, 1.0, 0.0,
                             torch.zeros(4, dtype=torch.int32, device="cuda"))
    with pytest.raises(hip.HipOpsError, match="slots"):
        hip.truncated_sample(logits, table, 64, None, midx, None, pos, T, SEED, 5)
    greedy = hip.truncated_sample(logits, table, 64, None, midx, slots, pos, 0.0, SEED, 5, 0.5, 0.1)
    assert torch.equal(greedy, hip.masked_argmax(logits, table, 64, None, midx))


def test_a_captured_replay_equals_the_eager_call(hip):
    B, V = 17, 128256
    logits, table, midx, slots, pos = _sharp_case(B, V, V, 5, KNOBS["all"])
    eager, est = _run_and_check(hip, logits, table, midx, slots, pos, V, KNOBS["all"])
    dev = [t.cuda() for t in (logits, table, midx, slots, pos)]
    out = torch.zeros(B, dtype=torch.int32, device="cuda")
    stats = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            hip.truncated_sample(dev[0], dev[1], V, out, dev[2], dev[3], dev[4], T, SEED, *KNOBS["all"], stats)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.fill_(-1)
        stats.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), eager) and torch.equal(stats.cpu(), est)


def test_model_steps_select_from_their_own_logits():
    """The tiny model (512 ids, so the large-tile head applies) at a <= 16-row
    step, a 40-row step (weight-streaming GEMM) and a step at
    TGEMM_HEAD_MIN_ROWS rows (large-tile GEMM): the ids equal
    reference.truncated_sample of the logits the step returned; the captured
    step has the untruncated graph's kernel-node count; with the truncation
    off the same model returns no logits at the fused-head row counts."""
    from dmcp.enrich.local import LocalEngine
    from dmcp.models.llm import DecodeGraphs, LocalLM, preset
    from dmcp.ops import reference
    m = LocalLM(preset("tiny", vocab_size=512, max_batch=192, max_rows=192, max_seq=256), device="cuda:0", seed=2)
    assert m.fused_head and m.tg_head and m.use_wgemm and m.trunc_logits is None
    V = m.cfg.vocab_size
    masks = LocalEngine(m, use_graphs=False).masks
    assert m.trunc_logits is None  # no filter configured: no logits buffer
    for s in range(m.TGEMM_HEAD_MIN_ROWS):
        m.forward_tokens(torch.tensor([256, 65 + s % 20, 66], dtype=torch.int32), s, 0)
    cut = (5, 0.9, 0.01)
    plain, trunc = DecodeGraphs(m, masks, sample=(T, SEED)), DecodeGraphs(m, masks, sample=(T, SEED), truncate=cut)
    assert m.trunc_logits is not None and tuple(m.trunc_logits.shape) == (192, V)
    differ = 0
    for B in (3, 40, m.TGEMM_HEAD_MIN_ROWS):
        g = torch.Generator().manual_seed(B)
        tok = torch.randint(32, 120, (B,), generator=g, dtype=torch.int32).tolist()
        sl, ps = list(range(B)), [3] * B
        mi = [i % int(masks.shape[0]) for i in range(B)]
        # the graphs first: a bucket's capture warms up on its zeroed inputs (slot 0, position 0)
        plain.run(tok, sl, ps, mi)
        glg, gids = (t[:B].clone() for t in trunc.run(tok, sl, ps, mi))
        b = trunc.bucket_for(B)
        assert trunc.graphs[b].kernels == plain.graphs[b].kernels > 0
        dev = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in (tok, sl, ps, mi)]
        last = torch.zeros(192, dtype=torch.int32, device="cuda")
        src = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        lg, ids = m.decode_select_gather(dev[0], src, last, dev[1], dev[2], masks, dev[3], sample=(T, SEED),
                                         truncate=cut)
        assert lg is not None and tuple(lg.shape) == (B, V)
        assert torch.equal(last[:B], ids)
        ids = ids.clone()  # a view of ``last``, which the calls below write again
        cpu = [t.cpu() for t in (lg, masks, dev[3], dev[1], dev[2])]
        _, _, amb = reference.truncation_threshold(cpu[0], cpu[1], V, cpu[2], cpu[3], T, *cut)
        want = reference.truncated_sample(cpu[0], cpu[1], V, None, cpu[2], cpu[3], cpu[4], T, SEED, *cut)
        ok = (ids.cpu() == want) | amb
        assert bool(ok.all()) and float(amb.float().mean()) <= 0.05
        lg0, ids0 = m.decode_select_gather(dev[0], src, last, dev[1], dev[2], masks, dev[3], sample=(T, SEED))
        assert (lg0 is None) == (B > 16)  # truncation off: the fused head, no logits
        lg1, ids1 = m.decode_select_gather(dev[0], src, last, dev[1], dev[2], masks, dev[3], sample=(T, SEED),
                                           truncate=(0, 1.0, 0.0))
        assert (lg1 is None) == (B > 16) and torch.equal(ids1, ids0)
        differ += int((ids0 != ids).sum())
        # the captured step: the same rule on the logits it returned (its GEMM runs the bucket's row
        # count, so its plan -- and a logit's last bit -- may differ from the eager call's)
        gwant = reference.truncated_sample(glg.cpu(), cpu[1], V, None, cpu[2], cpu[3], cpu[4], T, SEED, *cut)
        _, _, gamb = reference.truncation_threshold(glg.cpu(), cpu[1], V, cpu[2], cpu[3], T, *cut)
        assert bool(((gids.cpu() == gwant) | gamb).all()) and float(gamb.float().mean()) <= 0.05
        if torch.equal(glg, lg):
            assert torch.equal(gids, ids)
    assert differ > 0  # the truncation changed a draw
