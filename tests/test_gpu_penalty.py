"""The repetition / presence penalty on the gfx950 kernels: history_mark /
history_reset against the reference table, and the PENAL variants of the four
selection kernels against dmcp/ops/reference.py.

* masked_argmax / masked_sample / truncated_sample take the logits as inputs:
  their ids (and the truncation's tau bits and kept counts, under the
  ambiguity rule of tests/test_gpu_truncation.py) are exactly the reference's.
* The fused heads compute their own logits: the rule of
  tests/test_gpu_sampling.py on the penalised scores, its bf16-ulp term
  multiplied by 1 + max(theta, 1 / theta) -- the head's logit may differ from
  the reference's by one bf16 ulp, which the penalty scales and then rounds
  once more -- and more than 97 % of the rows exact.

Histories are about half dense with theta 1.3, alpha 0.5.  Every case asserts
that the reference selection under the penalty differs from the reference
selection without it on at least 20 % of the live rows, so none is vacuous;
the data seeds (SEEDS) were fixed after scanning on the CPU for inputs whose
reference alone meets that, whose fp32 and fp64 references agree on more than
97 % of the rows, and (truncation) with at most 5 % ambiguous rows."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

T, SEED = 0.7, 20240229
THETA, ALPHA, N_SLOTS = 1.3, 0.5, 32
KNOBS = {"k20_p95": (20, 0.95, 0.0), "min_p": (0, 1.0, 0.1)}
# data seed per case id (see the module docstring)
SEEDS = {
    ('masked', 1, 250, 0.0): 1250,
    ('masked', 1, 250, 0.7): 1252,
    ('truncated', 1, 250, 'k20_p95'): 2251,
    ('truncated', 1, 250, 'min_p'): 2251,
    ('masked', 5, 250, 0.0): 5250,
    ('masked', 5, 250, 0.7): 5250,
    ('truncated', 5, 250, 'k20_p95'): 10251,
    ('truncated', 5, 250, 'min_p'): 10251,
    ('masked', 64, 250, 0.0): 64251,
    ('masked', 64, 250, 0.7): 64253,
    ('truncated', 64, 250, 'k20_p95'): 128254,
    ('truncated', 64, 250, 'min_p'): 128252,
    ('masked', 1, 16413, 0.0): 1414,
    ('masked', 1, 16413, 0.7): 1416,
    ('truncated', 1, 16413, 'k20_p95'): 2413,
    ('truncated', 1, 16413, 'min_p'): 2413,
    ('masked', 5, 16413, 0.0): 5414,
    ('masked', 5, 16413, 0.7): 5416,
    ('truncated', 5, 16413, 'k20_p95'): 10413,
    ('truncated', 5, 16413, 'min_p'): 10413,
    ('masked', 64, 16413, 0.0): 64413,
    ('masked', 64, 16413, 0.7): 64416,
    ('truncated', 64, 16413, 'k20_p95'): 128414,
    ('truncated', 64, 16413, 'min_p'): 128414,
    ('wgemm', 78, 320, 0.0): 398,
    ('wgemm', 78, 320, 0.7): 406,
    ('wgemm', 320, 320, 0.0): 640,
    ('wgemm', 320, 320, 0.7): 774,
    ('wgemm', 700, 320, 0.0): 1020,
    ('wgemm', 700, 320, 0.7): 3866,
    ('wgemm', 78, 32000, 0.0): 32078,
    ('wgemm', 78, 32000, 0.7): 32091,
    ('tgemm', 257, 512, 0.0): 769,
    ('tgemm', 257, 512, 0.7): 769,
    ('tgemm', 300, 512, 0.0): 812,
    ('tgemm', 300, 512, 0.7): 825,
}


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _masks(V, g):
    """Three dense random mask rows, one with 40 allowed ids, one empty (tests/test_gpu_sampling.py)."""
    W = (V + 31) // 32
    dense = torch.randint(-2**31, 2**31 - 1, (3, W), generator=g, dtype=torch.int64)
    sp = torch.zeros(1, W, dtype=torch.int64)
    for v in torch.randint(0, V, (40,), generator=g).tolist():
        sp[0, v >> 5] |= 1 << (v & 31)
    sp = torch.where(sp >= 2**31, sp - 2**32, sp)
    if V % 32:  # no bits past the vocabulary
        dense[:, -1] &= (1 << (V % 32)) - 1
    return torch.cat([dense, sp, torch.zeros(1, W, dtype=torch.int64)]).to(torch.int32)


def _keys(M, g, pad=()):
    slots = torch.randint(0, N_SLOTS, (M,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, 8192, (M,), generator=g, dtype=torch.int32)
    for r in pad:
        slots[r] = -1
    return slots, pos


def _history(V, g):
    """A half-dense table: every id of every slot seen with probability 1/2."""
    return torch.randint(-2**31, 2**31 - 1, (N_SLOTS, (V + 31) // 32), generator=g, dtype=torch.int64).to(torch.int32)


def _penalty(hist, slots, flags=None, dev=None):
    from dmcp import ops
    mv = (lambda t: t) if dev is None else (lambda t: None if t is None else t.to(dev))
    return ops.Penalty(mv(hist), mv(slots), THETA, ALPHA, mv(flags))


def _live(masks, midx, slots, V, B):
    from dmcp.ops import reference
    return reference._allowed(torch.zeros(B, V), masks, V, midx, slots).any(1)


def _differs(with_pen, without, live):
    """Share of the live rows on which two reference selections differ."""
    n = int(live.sum())
    return float(((with_pen != without) & live).sum()) / n if n else 1.0


# ---- the logits-input kernels ------------------------------------------------
def _masked_case(B, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, ld, generator=g) * 2).to(torch.bfloat16)
    table = _masks(V, g)
    # the empty mask row (4) only where another row stays live
    midx = torch.randint(0, 5 if B > 1 else 4, (B,), generator=g, dtype=torch.int32)
    slots, pos = _keys(B, g, pad=(3,) if B > 3 else ())
    flags = torch.ones(5, dtype=torch.int32)
    if B > 1:
        flags[int(midx[0])] = 0  # a choice mask: its rows are not penalised
    return logits, table, midx, slots, pos, _history(V, g), flags


def masked_reference(B, V, ld, temperature, seed):
    """(inputs, want ids, share of live rows the penalty changes, fp32/fp64 agreement) on the CPU."""
    from dmcp.ops import reference
    logits, table, midx, slots, pos, hist, flags = case = _masked_case(B, V, ld, seed)
    pen = _penalty(hist, slots, flags)
    live = _live(table, midx, slots, V, B)
    if temperature == 0:
        want = reference.masked_argmax(logits, table, V, None, midx, pen)
        plain = reference.masked_argmax(logits, table, V, None, midx)
        agree = 1.0
    else:
        s64 = reference.sample_scores(logits, table, V, midx, slots, pos, temperature, SEED, torch.float64, pen)
        want = reference.masked_sample(logits, table, V, None, midx, slots, pos, temperature, SEED, pen)
        plain = reference.masked_sample(logits, table, V, None, midx, slots, pos, temperature, SEED)
        agree = float(((s64.argmax(1) == want) | ~live).float().mean())
    return case, want, _differs(want, plain, live), agree


def truncated_reference(B, V, ld, knobs, seed):
    from dmcp.ops import reference
    logits, table, midx, slots, pos, hist, flags = case = _masked_case(B, V, ld, seed)
    pen = _penalty(hist, slots, flags)
    live = _live(table, midx, slots, V, B)
    tau, kept, amb = reference.truncation_threshold(logits, table, V, midx, slots, T, *knobs, pen)
    want, _ = reference.truncated_sample_at(tau, logits, table, V, midx, slots, pos, T, SEED, pen)
    tau0, _, _ = reference.truncation_threshold(logits, table, V, midx, slots, T, *knobs)
    plain, _ = reference.truncated_sample_at(tau0, logits, table, V, midx, slots, pos, T, SEED)
    return case, (tau, kept, amb, want), _differs(want, plain, live), float(amb.float().mean())


SHAPES = [(B, V, ld) for V, ld in ((250, 250), (16384 + 29, 16384 + 32)) for B in (1, 5, 64)]


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_masked_selection_equals_the_reference(hip, B, V, ld, temperature, with_idx):
    """ld = 250: the element-wise path; V = 16,413: a second trip of the chunk
    loop, the clamped duplicate chunk and a 5-id tail (tests/test_gpu_sampling.py)."""
    (logits, table, midx, slots, pos, hist, flags), want, diff, agree = masked_reference(
        B, V, ld, temperature, SEEDS["masked", B, V, temperature])
    print(f"B={B} V={V} T={temperature}: penalty changes {diff:.3f} of the live rows, fp32/fp64 {agree:.3f}")
    assert diff >= 0.2 and agree > 0.97
    if with_idx:
        masks, mi, fl = table, midx, flags
    else:
        masks, mi, fl = table[midx.long()].contiguous(), None, flags[midx.long()].contiguous()
    pen = _penalty(hist, slots, fl, "cuda")
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    args = (logits.cuda(), masks.cuda(), V, out, None if mi is None else mi.cuda())
    if temperature == 0:
        ids = hip.masked_argmax(*args, penalty=pen)
    else:
        ids = hip.masked_sample(*args, slots.cuda(), pos.cuda(), temperature, SEED, penalty=pen)
    assert ids is out and torch.equal(ids.cpu(), want)


@pytest.mark.parametrize("name", list(KNOBS))
@pytest.mark.parametrize("B,V,ld", SHAPES)
def test_truncated_selection_equals_the_reference(hip, B, V, ld, name):
    from dmcp.ops import reference
    (logits, table, midx, slots, pos, hist, flags), (tau, kept, amb, want), diff, amb_share = truncated_reference(
        B, V, ld, KNOBS[name], SEEDS["truncated", B, V, name])
    print(f"B={B} V={V} {name}: penalty changes {diff:.3f} of the live rows, ambiguous {amb_share:.3f}")
    assert diff >= 0.2 and amb_share <= 0.05
    pen_cpu = _penalty(hist, slots, flags)
    stats = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    ids = hip.truncated_sample(logits.cuda(), table.cuda(), V, None, midx.cuda(), slots.cuda(), pos.cuda(), T, SEED,
                               *KNOBS[name], stats, penalty=_penalty(hist, slots, flags, "cuda")).cpu()
    st = stats.cpu()
    values = reference.penalized(logits, V, table, midx, pen_cpu, "test")
    for b in range(B):
        sl = slice(b, b + 1)
        if bool(amb[b]) and int(st[b, 0]) != int(reference.tau_bits(tau[sl])):
            # the adjacent value level, with the reference's id at that level (tests/test_gpu_truncation.py)
            got_tau = torch.tensor([st[b, 0] << 16], dtype=torch.int32).view(torch.float32)
            ok = reference._allowed(logits[sl], table, V, midx[sl], slots[sl])[0]
            levels = torch.unique(values[b][ok] + 0.0).tolist()
            i = levels.index(float(tau[b]))
            assert float(got_tau) in levels[max(i - 1, 0):i + 2], f"row {b}: tau {float(got_tau)} vs {float(tau[b])}"
            w, k = reference.truncated_sample_at(got_tau, logits[sl], table, V, midx[sl], slots[sl], pos[sl], T, SEED,
                                                 _penalty(hist, slots[sl], flags))
            assert (int(ids[b]), int(st[b, 1])) == (int(w), int(k)), f"row {b} (ambiguous)"
            continue
        assert int(st[b, 0]) == int(reference.tau_bits(tau[sl])), f"row {b}: tau bits {int(st[b, 0]):#x}"
        assert int(st[b, 1]) == int(kept[b]), f"row {b}: kept {int(st[b, 1])} vs {int(kept[b])}"
        assert int(ids[b]) == int(want[b]), f"row {b}: id {int(ids[b])} vs {int(want[b])}"


# ---- the fused heads -----------------------------------------------------------
def _head_case(M, V, K, seed, pad):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * (0.02 if K >= 2048 else 0.08)).to(torch.bfloat16)
    masks = _masks(V, g)
    midx = torch.randint(0, 5, (M,), generator=g, dtype=torch.int32)
    slots, pos = _keys(M, g, pad)
    flags = torch.ones(5, dtype=torch.int32)
    flags[2] = 0
    return x, w, masks, midx, slots, pos, _history(V, g), flags


def _ulp(x, mant):
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -100))) - mant)


def head_scores(logits, case, temperature, dtype, penalty=True):
    """Scores [M, V] of the head's selection in ``dtype``: the (penalised)
    bf16 logits at temperature 0, :func:`sample_scores` above it."""
    from dmcp.ops import reference
    _, _, masks, midx, slots, pos, hist, flags = case
    V = masks.shape[1] * 32
    pen = _penalty(hist, slots, flags) if penalty else None
    lg = logits.to(torch.bfloat16)
    if temperature > 0:
        return reference.sample_scores(lg, masks, V, midx, slots, pos, temperature, SEED, dtype, pen)
    s = reference.penalized(lg, V, masks, midx, pen, "test").to(dtype)
    s[~reference._allowed(lg, masks, V, midx, torch.zeros_like(slots))] = float("-inf")
    return s


def head_reference(logits, case, temperature):
    """(fp64 scores, live rows, share the penalty changes, fp32/fp64 agreement) of fp32 ``logits`` [M, V]."""
    s64 = head_scores(logits, case, temperature, torch.float64)
    s32 = head_scores(logits, case, temperature, torch.float32)
    plain = head_scores(logits, case, temperature, torch.float64, penalty=False)
    live = torch.isfinite(s64).any(1)
    agree = float(((s32.argmax(1) == s64.argmax(1)) | ~live).float().mean())
    return s64, live, _differs(s64.argmax(1), plain.argmax(1), live & torch.isfinite(plain).any(1)), agree


def _check_head(ids, logits, case, temperature):
    ids = ids.cpu().long()
    M = ids.numel()
    s64, live, diff, agree = head_reference(logits, case, temperature)
    print(f"M={M} T={temperature}: penalty changes {diff:.3f} of the live rows, fp32/fp64 {agree:.4f}")
    assert diff >= 0.2 and agree > 0.97
    sampled_pad = (case[4] < 0) if temperature > 0 else torch.zeros(M, dtype=torch.bool)
    assert bool((ids[~live | sampled_pad] == 0).all()), "rows that allow nothing / padding rows select 0"
    inv_t = float(torch.tensor(1.0 / temperature, dtype=torch.float32)) if temperature > 0 else 1.0
    best = s64.max(1).values
    big_logit = logits.to(torch.bfloat16).double().abs().max(1).values
    big_score = s64.masked_fill(~torch.isfinite(s64), 0.0).abs().max(1).values
    bound = _ulp(big_logit, 7) * inv_t * (1 + max(THETA, 1 / THETA))
    if temperature > 0:
        bound = bound + 64 * _ulp(big_score, 23)
    got = s64[torch.arange(M), ids]
    for m in torch.nonzero(live).flatten().tolist():
        assert math.isfinite(got[m]), f"row {m}: id {int(ids[m])} is not allowed"
        assert got[m] >= best[m] - bound[m], f"row {m}: score {got[m]} vs {best[m]} (bound {bound[m]})"
    exact = ((ids == s64.argmax(1)) | ~live).float().mean().item()
    print(f"M={M}: exact {exact:.4f}")
    assert exact > 0.97


@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("M,V,K", [(78, 320, 256), (320, 320, 256), (700, 320, 256), (78, 32000, 2048)])
def test_lm_head_selection_matches_the_fp64_reference(hip, M, V, K, temperature):
    case = _head_case(M, V, K, SEEDS["wgemm", M, V, temperature], pad=(5, M - 1))
    x, w, masks, midx, slots, pos, hist, flags = case
    logits = (x.cuda().float() @ w.cuda().float().t()).cpu()
    pen = _penalty(hist, slots, flags, "cuda")
    if temperature == 0:
        ids = hip.lm_head_argmax(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), penalty=pen)
    else:
        ids = hip.lm_head_sample(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), slots=slots.cuda(),
                                 positions=pos.cuda(), temperature=temperature, seed=SEED, penalty=pen)
    _check_head(ids, logits, case, temperature)


@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("M", [257, 300])
def test_tgemm_lm_head_selection_matches_the_fp64_reference(hip, M, temperature):
    V, K = 512, 256
    case = _head_case(M, V, K, SEEDS["tgemm", M, V, temperature], pad=(0, 256))
    x, w, masks, midx, slots, pos, hist, flags = case
    logits = (x.cuda().float() @ w.cuda().float().t()).cpu()
    pen = _penalty(hist, slots, flags, "cuda")
    if temperature == 0:
        ids = hip.tgemm_lm_head_argmax(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), penalty=pen)
    else:
        ids = hip.tgemm_lm_head_sample(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), slots=slots.cuda(),
                                       positions=pos.cuda(), temperature=temperature, seed=SEED, penalty=pen)
    _check_head(ids, logits, case, temperature)


def test_an_all_zero_history_selects_the_unpenalised_ids_on_all_four_kernels(hip):
    M, V, K = 300, 512, 256
    x, w, masks, midx, slots, pos, hist, flags = (t.cuda() for t in _head_case(M, V, K, 99, pad=(17,)))
    logits = hip.wgemm(x, w)
    from dmcp import ops
    pen = ops.Penalty(torch.zeros_like(hist), slots, THETA, ALPHA, flags)
    for t in (0.0, T):
        kw = {"slots": slots, "positions": pos, "temperature": t, "seed": SEED}
        assert torch.equal(hip.lm_head_sample(x, w, masks, midx, penalty=pen, **kw),
                           hip.lm_head_sample(x, w, masks, midx, **kw))
        assert torch.equal(hip.tgemm_lm_head_sample(x, w, masks, midx, penalty=pen, **kw),
                           hip.tgemm_lm_head_sample(x, w, masks, midx, **kw))
        assert torch.equal(hip.masked_sample(logits, masks, V, None, midx, penalty=pen, **kw),
                           hip.masked_sample(logits, masks, V, None, midx, **kw))
    kw["temperature"] = T
    s0, s1 = (torch.zeros(M, 2, dtype=torch.int32, device="cuda") for _ in range(2))
    a = hip.truncated_sample(logits, masks, V, None, midx, top_k=20, top_p=0.95, stats=s0, **kw)
    b = hip.truncated_sample(logits, masks, V, None, midx, top_k=20, top_p=0.95, stats=s1, penalty=pen, **kw)
    assert torch.equal(a, b) and torch.equal(s0, s1)
    # a full history with every flag clear, and slots outside the table: not penalised either
    full = torch.full_like(hist, -1)
    for p in (ops.Penalty(full, slots, THETA, ALPHA, torch.zeros_like(flags)),
              ops.Penalty(full, torch.full_like(slots, -1), THETA, ALPHA)):
        assert torch.equal(hip.lm_head_argmax(x, w, masks, midx, penalty=p), hip.lm_head_argmax(x, w, masks, midx))
        assert torch.equal(hip.masked_argmax(logits, masks, V, None, midx, penalty=p),
                           hip.masked_argmax(logits, masks, V, None, midx))


# ---- the history ---------------------------------------------------------------
def test_history_mark_and_reset_equal_the_reference_table(hip):
    """64 rows over 5 slots of an 8-slot table: many duplicate (slot, word)
    pairs, padding rows, src gathers from a last_ids buffer, tokens outside
    the vocabulary and exempt ids; then a reset of two of the slots."""
    from dmcp.ops import reference
    V, W, rows = 1003, 32, 64
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, 96, (rows,), generator=g, dtype=torch.int32)  # three words: collisions
    tokens[::7] = torch.randint(0, V, (len(tokens[::7]),), generator=g, dtype=torch.int32)
    tokens[5], tokens[6], tokens[8] = -1, V, 2 ** 30
    slots = torch.tensor([1, 2, 4, 5, 7], dtype=torch.int32)[torch.randint(0, 5, (rows,), generator=g)]
    slots[::9] = -1
    slots[11] = 8  # outside the table
    last = torch.randint(0, 96, (40,), generator=g, dtype=torch.int32)
    src = torch.where(torch.rand(rows, generator=g) < 0.4, torch.randint(0, 40, (rows,), generator=g), -1)
    src = src.to(torch.int32)
    exempt = torch.zeros(W, dtype=torch.int32)
    exempt[0] = 0b1010
    exempt[1] = -2 ** 31  # id 63
    want = torch.zeros(8, W, dtype=torch.int32)
    want[3, 5] = 77  # an untouched slot keeps what it holds
    hist = want.clone().cuda()
    reference.history_mark(want, tokens, slots, src, last, exempt, V)
    assert int((want != 0).sum()) > 12
    out = hip.history_mark(hist, tokens.cuda(), slots.cuda(), src.cuda(), last.cuda(), exempt.cuda(), V)
    assert out is hist and torch.equal(hist.cpu(), want)
    hip.history_mark(hist, tokens.cuda(), slots.cuda(), vocab=V)  # no gather, nothing exempt
    reference.history_mark(want, tokens, slots, vocab=V)
    assert torch.equal(hist.cpu(), want)
    hip.history_reset(hist, [2, 7, -1, 8])
    reference.history_reset(want, [2, 7, -1, 8])
    assert torch.equal(hist.cpu(), want) and bool((want[[1, 4, 5]] != 0).any(1).all())
    hip.history_reset(hist, list(range(8)) * 9)  # more slots than one launch carries
    assert int(hist.abs().sum()) == 0


# ---- the captured step ---------------------------------------------------------
def test_captured_pipelined_steps_record_first_and_add_one_kernel_node():
    """Three consecutive pipelined DecodeGraphs steps on the tiny preset with
    the penalty on (greedy, the default): from the second step every token is
    gathered from last_ids, and one slot carries two rows of a step.  At 40
    rows (the fused head) and at 3 rows (logits + selection) the ids equal the
    eager decode_select_gather calls', the history table equals the reference
    table of the tokens fed, and the graph has the penalty-off graph's kernel
    nodes + 1; at 3 rows the ids also equal the CPU reference fed the step's
    logits.  The penalty-off graph is the one built with no penalty argument.
    If history_mark ran after the head it would record this step's
    selections instead of the gathered ones: the table would differ."""
    from dmcp import ops
    from dmcp.enrich.local import LocalEngine
    from dmcp.models.llm import DecodeGraphs, LocalLM, preset
    from dmcp.ops import reference
    m = LocalLM(preset("tiny", max_batch=64, max_rows=64, max_seq=512), device="cuda:0", seed=2)
    assert m.fused_head
    eng = LocalEngine(m, use_graphs=False, repetition_penalty=THETA, presence_penalty=ALPHA)
    masks, pen = eng.masks, eng._penalty
    theta, alpha, flags, exempt = pen
    V, n_masks = m.cfg.vocab_size, int(masks.shape[0])
    for s in range(40):
        m.forward_tokens(torch.tensor([256, 65 + s % 20, 66], dtype=torch.int32), s, 0)
    plain, off, on = DecodeGraphs(m, masks), DecodeGraphs(m, masks, penalty=(1.0, 0.0, flags, exempt)), \
        DecodeGraphs(m, masks, penalty=pen)
    assert off.penalty is None and on.penalty is pen
    for B in (40, 3):
        g = torch.Generator().manual_seed(B)
        tok = torch.randint(32, 120, (B,), generator=g, dtype=torch.int32).tolist()
        sl = list(range(B))
        sl[1] = sl[0]  # rows 0 and 1: one slot, consecutive positions (a jump-forward pair)
        mi = [i % 2 if i % 5 else 2 % n_masks for i in range(B)]  # free text, and a choice mask (not penalised)
        steps = []
        for t in range(3):
            ps = [3 + 2 * t, 4 + 2 * t] + [3 + t] * (B - 2)
            steps.append((tok if t == 0 else [0] * B, sl, ps, mi, [-1] * B if t == 0 else list(range(B))))
        # the captured, pipelined run: nothing is read between the steps
        m.history.zero_()
        on.last_ids.zero_()
        got, lgs = [], []
        for tk, s_, ps, mi_, src in steps:
            lg, ids = on.run(tk, s_, ps, mi_, src)
            got.append(ids.clone())
            lgs.append(None if lg is None else lg.clone())
        hist_graph = m.history.clone()
        b = on.bucket_for(B)
        for tk, s_, ps, mi_, src in steps[:1]:
            plain.run(tk, s_, ps, mi_, src)
            off.run(tk, s_, ps, mi_, src)
        assert on.graphs[b].kernels == plain.graphs[b].kernels + 1 > 1
        assert off.graphs[b].kernels == plain.graphs[b].kernels
        # the eager path, and the reference table of the tokens fed
        m.history.zero_()
        last = torch.zeros(64, dtype=torch.int32, device="cuda")
        want_hist = torch.zeros_like(hist_graph).cpu()
        for t, (tk, s_, ps, mi_, src) in enumerate(steps):
            dev = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in (tk, src, s_, ps, mi_)]
            fed = tk if t == 0 else got[t - 1].cpu().tolist()
            reference.history_mark(want_hist, torch.tensor(fed, dtype=torch.int32),
                                   torch.tensor(s_, dtype=torch.int32), None, None, exempt.cpu(), V)
            lg, eager = m.decode_select_gather(dev[0], dev[1], last, dev[2], dev[3], masks, dev[4], penalty=pen)
            assert (lg is None) == (B > 16) == (lgs[t] is None)
            assert torch.equal(eager, got[t]), f"B={B} step {t}"
            if lg is not None:
                p = ops.Penalty(want_hist.clone(), torch.tensor(s_, dtype=torch.int32), theta, alpha, flags.cpu())
                want = reference.masked_argmax(lgs[t].cpu(), masks.cpu(), V, None,
                                               torch.tensor(mi_, dtype=torch.int32), p)
                assert torch.equal(got[t].cpu(), want), f"B={B} step {t} vs the CPU reference"
        assert torch.equal(m.history.cpu(), want_hist) and torch.equal(hist_graph.cpu(), want_hist)
        assert int((want_hist != 0).sum()) >= B - 1
