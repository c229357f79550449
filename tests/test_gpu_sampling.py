"""Temperature sampling on the gfx950 selection kernels (masked_sample,
lm_head_sample, tgemm_lm_head_sample) against the fp64 reference on the same
bf16 inputs, by the rule tests/test_gpu_wgemm.py uses for the greedy head,
applied to scores (score = bf16 logit / T + Gumbel noise):

* every id is allowed by its row's mask (0 for a row that allows nothing or
  has slot -1);
* its fp64 score is within the rounding bound of the row's maximum: one bf16
  ulp of the row's largest |logit| times 1 / T (the GEMM's accumulation order)
  plus 64 fp32 ulps of the row's largest |score| (one multiply-add and two
  logs of a few ulps each, the outer log turning the inner one's relative
  error into an absolute one);
* more than 97 % of the rows equal the reference argmax exactly (the
  project's figure for near-ties).

The seeds below were fixed after checking on the CPU that the fp32 reference
agrees with the fp64 reference on more than 97 % of the rows of every input
used here (it agrees on all of them: the smallest fp64 gap between a row's top
two scores is 3e-4, far above fp32 rounding); ``_check`` asserts it again."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

T, SEED = 0.7, 20240229


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _masks(V, g):
    """Three dense random mask rows, one with 40 allowed ids, one empty."""
    W = (V + 31) // 32
    dense = torch.randint(-2**31, 2**31 - 1, (3, W), generator=g, dtype=torch.int64)
    sp = torch.zeros(1, W, dtype=torch.int64)
    for v in torch.randint(0, V, (40,), generator=g).tolist():
        sp[0, v >> 5] |= 1 << (v & 31)
    sp = torch.where(sp >= 2**31, sp - 2**32, sp)
    if V % 32:  # no bits past the vocabulary
        keep = (1 << (V % 32)) - 1
        dense[:, -1] &= keep
    return torch.cat([dense, sp, torch.zeros(1, W, dtype=torch.int64)]).to(torch.int32)


def _keys(M, g, pad=()):
    slots = torch.randint(0, 768, (M,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, 8192, (M,), generator=g, dtype=torch.int32)
    for r in pad:
        slots[r] = -1
    return slots, pos


def _ulp(x, mant):
    """Unit in the last place of |x| (fp64 tensor) in a format of ``mant`` explicit mantissa bits."""
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -100))) - mant)


def _check(ids, logits, masks, midx, slots, pos, V, temperature=T, seed=SEED):
    """``ids`` (any device) against the fp64 reference of ``logits`` [M, >= V]
    (CPU: bf16, or fp32 to be rounded to bf16); returns the exact-match share."""
    from dmcp.ops import reference
    ids = ids.cpu().long()
    M = ids.numel()
    lg = logits[:, :V].to(torch.bfloat16)
    s64 = reference.sample_scores(lg, masks, V, midx, slots, pos, temperature, seed, torch.float64)
    s32 = reference.sample_scores(lg, masks, V, midx, slots, pos, temperature, seed, torch.float32)
    live = torch.isfinite(s64).any(1)
    ref = s64.argmax(1)
    agree32 = ((s32.argmax(1) == ref) | ~live).float().mean().item()
    assert agree32 > 0.97, f"fp32 vs fp64 reference agree on {agree32:.4f} of the rows"
    assert bool((ids[~live] == 0).all()), "rows that allow nothing / padding rows select 0"
    inv_t = float(torch.tensor(1.0 / temperature, dtype=torch.float32))
    best = s64.max(1).values
    big_logit = lg.double().abs().max(1).values
    big_score = s64.masked_fill(~torch.isfinite(s64), 0.0).abs().max(1).values
    bound = _ulp(big_logit, 7) * inv_t + 64 * _ulp(big_score, 23)
    got = s64[torch.arange(M), ids]
    for m in torch.nonzero(live).flatten().tolist():
        assert math.isfinite(got[m]), f"row {m}: id {int(ids[m])} is not allowed"
        assert got[m] >= best[m] - bound[m], f"row {m}: score {got[m]} vs {best[m]} (bound {bound[m]})"
    exact = ((ids == ref) | ~live).float().mean().item()
    print(f"M={M} V={V}: exact {exact:.4f}, fp32 reference {agree32:.4f}")
    assert exact > 0.97
    return exact


@pytest.mark.parametrize("with_idx", [True, False])
@pytest.mark.parametrize("V,ld", [(250, 250), (16384 + 29, 16384 + 32)])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_masked_sample_matches_fp64_reference(hip, B, V, ld, with_idx):
    """ld = 250: rows not 16-B aligned, the element-wise path.  V = 16,413:
    2,051 whole chunks -- a second trip of the chunk loop for 3 threads, the
    clamped duplicate chunk for the others -- and a 5-id tail."""
    g = torch.Generator().manual_seed(B * 100003 + V)
    logits = (torch.randn(B, ld, generator=g) * 2).to(torch.bfloat16)
    table = _masks(V, g)
    midx = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32)
    slots, pos = _keys(B, g, pad=(3,) if B > 3 else ())
    if with_idx:
        masks, mi = table, midx
    else:
        masks, mi = table[midx.long()].contiguous(), None
    out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ids = hip.masked_sample(logits.cuda(), masks.cuda(), V, out, None if mi is None else mi.cuda(), slots.cuda(),
                            pos.cuda(), T, SEED)
    assert ids is out
    _check(ids, logits, masks, mi, slots, pos, V)
    # no mask at all: every id of the vocabulary may be drawn, none past it
    free = hip.masked_sample(logits.cuda(), None, V, None, None, slots.cuda(), pos.cuda(), T, SEED)
    _check(free, logits, None, None, slots, pos, V)


def _head_case(M, V, K, seed, pad):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    w = (torch.randn(V, K, generator=g) * (0.02 if K >= 2048 else 0.08)).to(torch.bfloat16)
    masks = _masks(V, g)
    midx = torch.randint(0, 5, (M,), generator=g, dtype=torch.int32)
    slots, pos = _keys(M, g, pad)
    logits = (x.cuda().float() @ w.cuda().float().t()).cpu()  # fp32: rounded to bf16 by _check
    return x, w, masks, midx, slots, pos, logits


# V = 320: 64-id tiles; V = 32,000: 128-id tiles.  M = 78: not a multiple of
# 16; 320: two M parts; 700: two launches of <= 512 rows.
@pytest.mark.parametrize("M,V,K", [(78, 320, 256), (320, 320, 256), (700, 320, 256), (78, 32000, 2048)])
def test_lm_head_sample_matches_fp64_reference(hip, M, V, K):
    x, w, masks, midx, slots, pos, logits = _head_case(M, V, K, V + M, pad=(5, M - 1))
    ids = hip.lm_head_sample(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), slots=slots.cuda(),
                             positions=pos.cuda(), temperature=T, seed=SEED)
    _check(ids, logits, masks, midx, slots, pos, V)


@pytest.mark.parametrize("M", [257, 300])
def test_tgemm_lm_head_sample_matches_fp64_reference(hip, M):
    V, K = 512, 256
    x, w, masks, midx, slots, pos, logits = _head_case(M, V, K, 7 * M, pad=(0, 256))
    ids = hip.tgemm_lm_head_sample(x.cuda(), w.cuda(), masks.cuda(), midx.cuda(), slots=slots.cuda(),
                                   positions=pos.cuda(), temperature=T, seed=SEED)
    _check(ids, logits, masks, midx, slots, pos, V)


def test_the_three_paths_agree_and_temperature_zero_is_the_greedy_op(hip):
    M, V, K = 300, 512, 256
    x, w, masks, midx, slots, pos, _ = _head_case(M, V, K, 99, pad=(17,))
    x, w, masks, midx, slots, pos = (t.cuda() for t in (x, w, masks, midx, slots, pos))
    logits = hip.wgemm(x, w)  # bf16 [M, V]
    kw = {"slots": slots, "positions": pos, "temperature": T, "seed": SEED}
    a = hip.lm_head_sample(x, w, masks, midx, **kw)
    b = hip.tgemm_lm_head_sample(x, w, masks, midx, **kw)
    c = hip.masked_sample(logits, masks, V, None, midx, **kw)
    for p, q in ((a, b), (a, c), (b, c)):
        assert (p == q).float().mean().item() > 0.97
    assert int(a[17]) == int(b[17]) == int(c[17]) == 0  # the padding row
    # another seed draws other ids; the same seed the same ids
    assert (hip.lm_head_sample(x, w, masks, midx, slots=slots, positions=pos, temperature=T, seed=SEED + 1)
            != a).float().mean().item() > 0.25
    assert torch.equal(hip.lm_head_sample(x, w, masks, midx, **kw), a)
    kw["temperature"] = 0.0
    assert torch.equal(hip.lm_head_sample(x, w, masks, midx, **kw), hip.lm_head_argmax(x, w, masks, midx))
    assert torch.equal(hip.tgemm_lm_head_sample(x, w, masks, midx, **kw),
                       hip.tgemm_lm_head_argmax(x, w, masks, midx))
    assert torch.equal(hip.masked_sample(logits, masks, V, None, midx, **kw),
                       hip.masked_argmax(logits, masks, V, None, midx))


def test_captured_decode_step_samples_with_the_greedy_graph_shape():
    """DecodeGraphs with sampling on (tiny model): the same kernel-node count
    as the greedy graph of the bucket (fused head at 40 rows, logits +
    selection at 3), deterministic replays, and the ids of the uncaptured
    decode_select_gather call."""
    from dmcp.enrich.local import LocalEngine
    from dmcp.models.llm import DecodeGraphs, LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=64, max_rows=64, max_seq=512), device="cuda:0", seed=2)
    assert m.fused_head
    masks = LocalEngine(m, use_graphs=False).masks
    for s in range(40):
        m.forward_tokens(torch.tensor([256, 65 + s % 20, 66], dtype=torch.int32), s, 0)
    greedy, sampled = DecodeGraphs(m, masks), DecodeGraphs(m, masks, sample=(T, SEED))
    for B in (40, 3):
        g = torch.Generator().manual_seed(B)
        tok = torch.randint(32, 120, (B,), generator=g, dtype=torch.int32).tolist()
        sl, ps = list(range(B)), [3] * B
        mi = [i % int(masks.shape[0]) for i in range(B)]
        _, gids = greedy.run(tok, sl, ps, mi)
        gids = gids.clone()
        _, ids1 = sampled.run(tok, sl, ps, mi)
        ids1 = ids1.clone()
        _, ids2 = sampled.run(tok, sl, ps, mi)
        b = sampled.bucket_for(B)
        assert sampled.graphs[b].kernels == greedy.graphs[b].kernels > 0
        assert torch.equal(ids1, ids2)
        dev = [torch.tensor(v, dtype=torch.int32, device="cuda") for v in (tok, sl, ps, mi)]
        last = torch.zeros(64, dtype=torch.int32, device="cuda")
        src = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        lg, eager = m.decode_select_gather(dev[0], src, last, dev[1], dev[2], masks, dev[3], sample=(T, SEED))
        assert (lg is None) == (B > 16)
        assert torch.equal(eager, ids1)
        if B == 40:
            assert not torch.equal(ids1, gids)  # it does sample
