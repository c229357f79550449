"""Top-k / top-p / min-p truncation on the CPU: ``truncation_threshold`` of
dmcp/ops/reference.py against a brute-force sort-and-cumsum, its edge cases,
the statistics of ``truncated_sample`` against the renormalised truncated
softmax, and the three knobs through the model, the engine, the configuration
and the worker frames.  csrc/truncate.hip follows the same definitions
(tests/test_gpu_truncation.py)."""
import json
import math
import random

import numpy as np
import pytest
import torch

from dmcp.ops import reference

NEG = float("-inf")


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32)


def _mask_rows(allowed):
    """bool [B, V] -> int32 bit-set rows [B, ceil(V / 32)]."""
    B, V = allowed.shape
    words = torch.zeros((B, (V + 31) // 32), dtype=torch.int64)
    for v in range(V):
        words[:, v // 32] |= allowed[:, v].to(torch.int64) << (v % 32)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def _brute(x, allowed, temperature, top_k, top_p, min_p):
    """(tau, kept) of one row, element by element in Python floats (fp64):
    sort, walk, cumulative sum -- nothing shared with the reference."""
    vals = sorted((float(v) for v, a in zip(x, allowed) if a), reverse=True)
    if not vals:
        return NEG, 0
    n, x_max = len(vals), vals[0]
    inv_t = float(np.float32(1.0 / temperature))
    tk = vals[top_k - 1] if 0 < top_k < n else NEG
    tp = NEG
    if top_p < 1.0:
        surv = [v for v in vals if v >= tk]
        w = [math.exp((v - x_max) * inv_t) for v in surv]
        z, run = sum(w), 0.0
        tp = surv[-1]
        for i, v in enumerate(surv):
            run += w[i]
            if (i + 1 == len(surv) or surv[i + 1] != v) and run >= top_p * z:  # the end of a value level
                tp = v
                break
    tm = NEG
    if min_p > 0.0:
        ln = np.float32(math.log(min_p))
        tm = min(v for v in vals if (np.float32(v) - np.float32(x_max)) * np.float32(inv_t) >= ln)
    tau = max(tk, tp, tm)
    return tau, sum(1 for v in vals if v >= tau)


@pytest.mark.parametrize("V", [8, 33, 97, 300])
def test_threshold_equals_a_brute_force_sort_and_cumsum(V):
    rng = random.Random(V)
    g = torch.Generator().manual_seed(V)
    B = 24
    logits = (torch.randn(B, V, generator=g) * 2.5).to(torch.bfloat16)
    logits[B // 2:] = (logits[B // 2:].float() * 2).round().div(2).to(torch.bfloat16)  # ties
    allowed = torch.rand(B, V, generator=g) < 0.7
    allowed[:, 0] = True
    masks = _mask_rows(allowed)
    slots = _i32(range(B))
    checked = 0
    for top_k, top_p, min_p, T in [(0, 1.0, 0.0, 1.0), (3, 1.0, 0.0, 0.7), (0, 0.9, 0.0, 0.7), (0, 1.0, 0.1, 0.7),
                                   (5, 0.8, 0.05, 0.6), (V + 5, 0.5, 0.0, 1.3), (1, 0.3, 0.5, 0.2),
                                   (rng.randint(1, V), rng.uniform(0.05, 0.99), rng.uniform(0.001, 0.5), 0.9)]:
        tau, kept, amb = reference.truncation_threshold(logits, masks, V, None, slots, T, top_k, top_p, min_p)
        for b in range(B):
            if bool(amb[b]):
                continue  # a running sum within 1e-4 Z of p Z: the two fp64 sums may differ in order
            want = _brute(logits[b].float().tolist(), allowed[b].tolist(), T, top_k, top_p, min_p)
            assert (float(tau[b]), int(kept[b])) == want, (V, b, top_k, top_p, min_p)
            checked += 1
    assert checked >= 0.9 * 8 * B


def _case(B=6, V=40, seed=0, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(B, V, generator=g) * scale).to(torch.bfloat16)
    return logits, _i32(range(3, 3 + B)), _i32(range(50, 50 + B))


def test_top_k_past_the_allowed_count_cuts_nothing():
    logits, slots, pos = _case()
    allowed = torch.zeros(6, 40, dtype=torch.bool)
    allowed[:, 5:15] = True
    masks = _mask_rows(allowed)
    for k in (10, 11, 4000):
        tau, kept, amb = reference.truncation_threshold(logits, masks, 40, None, slots, 0.7, k)
        assert torch.equal(tau, torch.full((6,), NEG)) and kept.tolist() == [10] * 6 and not bool(amb.any())
    tau, kept, _ = reference.truncation_threshold(logits, masks, 40, None, slots, 0.7, 9)
    assert bool((tau > NEG).all()) and bool((kept >= 9).all())


@pytest.mark.parametrize("seed", [0, 7, 123456789])
def test_top_k_one_is_the_masked_argmax(seed):
    logits, slots, pos = _case(B=32, V=70, seed=3)
    allowed = torch.rand(32, 70, generator=torch.Generator().manual_seed(1)) < 0.5
    allowed[:, 69] = True
    masks = _mask_rows(allowed)
    ids = reference.truncated_sample(logits, masks, 70, None, None, slots, pos, 0.9, seed, 1)
    x = logits.float().masked_fill(~allowed, NEG)
    unique_max = (x == x.max(dim=1, keepdim=True).values).sum(dim=1) == 1
    assert int(unique_max.sum()) >= 24
    greedy = reference.masked_argmax(logits, masks, 70)
    assert torch.equal(ids[unique_max], greedy[unique_max])
    assert bool((x[torch.arange(32), ids.long()] == x.max(dim=1).values).all())  # tied maxima: one of them


def test_one_allowed_id_and_none():
    logits, slots, pos = _case()
    allowed = torch.zeros(6, 40, dtype=torch.bool)
    allowed[:3, 17] = True
    masks = _mask_rows(allowed)
    stats = torch.full((6, 2), -1, dtype=torch.int32)
    ids = reference.truncated_sample(logits, masks, 40, None, None, slots, pos, 0.7, 1, 5, 0.5, 0.2, stats)
    assert ids.tolist() == [17, 17, 17, 0, 0, 0]
    assert stats[3:].tolist() == [[0xFF80, 0]] * 3
    assert stats[:3, 1].tolist() == [1, 1, 1]
    assert torch.equal(stats[:3, 0], reference.tau_bits(logits[:3, 17].float()))


def test_a_padding_row_selects_zero():
    logits, slots, pos = _case()
    slots[2] = -1
    stats = torch.zeros((6, 2), dtype=torch.int32)
    ids = reference.truncated_sample(logits, None, 40, None, None, slots, pos, 0.7, 1, 4, 0.9, 0.0, stats)
    assert int(ids[2]) == 0 and stats[2].tolist() == [0xFF80, 0]
    live = [0, 1, 3, 4, 5]
    alone = reference.truncated_sample(logits[live], None, 40, None, None, slots[live], pos[live], 0.7, 1, 4, 0.9)
    assert torch.equal(ids[live], alone)


def test_ties_are_kept_together():
    g = torch.Generator().manual_seed(5)
    levels = torch.tensor([-1.5, 0.25, 1.0, 3.0])
    logits = levels[torch.randint(0, 4, (8, 64), generator=g)].to(torch.bfloat16)
    slots, pos = _i32(range(8)), _i32(range(8))
    for top_k, top_p in ((1, 1.0), (20, 1.0), (0, 0.6), (30, 0.9)):
        tau, kept, _ = reference.truncation_threshold(logits, None, 64, None, slots, 1.0, top_k, top_p)
        for b in range(8):
            assert int(kept[b]) == int((logits[b].float() >= tau[b]).sum())
            assert float(tau[b]) in levels.tolist()
            if top_k and top_p == 1.0:
                assert int(kept[b]) >= top_k  # the whole level of the k-th value
    flat = torch.full((3, 64), 0.75).to(torch.bfloat16)
    tau, kept, _ = reference.truncation_threshold(flat, None, 64, None, slots[:3], 0.7, 5, 0.3, 0.9)
    assert tau.tolist() == [0.75] * 3 and kept.tolist() == [64] * 3
    ids = reference.truncated_sample(flat, None, 64, None, None, slots[:3], pos[:3], 0.7, 9, 5, 0.3, 0.9)
    assert torch.equal(ids, reference.masked_sample(flat, None, 64, None, None, slots[:3], pos[:3], 0.7, 9))


def test_large_logits_at_a_low_temperature_do_not_overflow():
    logits, slots, pos = _case(scale=1.0)
    logits = (logits.float() + 300).to(torch.bfloat16)
    tau, kept, _ = reference.truncation_threshold(logits, None, 40, None, slots, 0.1, 0, 0.9, 0.01)
    assert bool(torch.isfinite(tau).all()) and bool((kept >= 1).all())
    for b in range(6):
        want = _brute(logits[b].float().tolist(), [True] * 40, 0.1, 0, 0.9, 0.01)
        assert (float(tau[b]), int(kept[b])) == want


def test_mask_idx_picks_the_rows_mask():
    logits, slots, pos = _case()
    allowed = torch.zeros(2, 40, dtype=torch.bool)
    allowed[0, :20] = True
    allowed[1, 20:] = True
    table = _mask_rows(allowed)
    midx = _i32([0, 1, 1, 0, 9, -3])  # clamped into the table
    rows = _mask_rows(allowed[[0, 1, 1, 0, 1, 0]])
    a = reference.truncation_threshold(logits, table, 40, midx, slots, 0.7, 3, 0.8, 0.1)
    b = reference.truncation_threshold(logits, rows, 40, None, slots, 0.7, 3, 0.8, 0.1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ids = reference.truncated_sample(logits, table, 40, None, midx, slots, pos, 0.7, 2, 3, 0.8, 0.1)
    assert torch.equal(ids, reference.truncated_sample(logits, rows, 40, None, None, slots, pos, 0.7, 2, 3, 0.8, 0.1))
    assert all(allowed[[0, 1, 1, 0, 1, 0][b], int(ids[b])] for b in range(6))


def test_all_filters_off_is_masked_sample():
    logits, slots, pos = _case(B=64, V=96, seed=9)
    allowed = torch.rand(64, 96, generator=torch.Generator().manual_seed(2)) < 0.6
    masks = _mask_rows(allowed)
    stats = torch.zeros((64, 2), dtype=torch.int32)
    ids = reference.truncated_sample(logits, masks, 96, None, None, slots, pos, 0.8, 77, 0, 1.0, 0.0, stats)
    assert torch.equal(ids, reference.masked_sample(logits, masks, 96, None, None, slots, pos, 0.8, 77))
    assert stats[:, 0].tolist() == [0xFF80] * 64 and torch.equal(stats[:, 1].long(), allowed.sum(dim=1))
    greedy = reference.truncated_sample(logits, masks, 96, None, None, slots, pos, 0.0, 77, 3, 0.5, 0.2)
    assert torch.equal(greedy, reference.masked_argmax(logits, masks, 96))  # temperature 0: the knobs are ignored


def test_the_kept_set_shrinks_monotonically_in_each_knob():
    logits, slots, pos = _case(B=16, V=120, seed=4)

    def kept_sets(**kw):
        tau, kept, _ = reference.truncation_threshold(logits, None, 120, None, slots, 0.7, **kw)
        sets = logits.float() >= tau[:, None]
        assert torch.equal(sets.sum(dim=1), kept)
        return sets
    for name, values in (("top_k", [119, 60, 20, 5, 2, 1]), ("top_p", [1.0, 0.99, 0.9, 0.5, 0.1, 0.001]),
                         ("min_p", [0.0, 0.001, 0.05, 0.3, 0.9, 0.999])):
        sets = [kept_sets(**{name: v}) for v in values]
        for wide, narrow in zip(sets, sets[1:]):
            assert bool((narrow & ~wide).sum() == 0), name
        assert int(sets[-1].sum()) < int(sets[0].sum()), name
        assert bool(sets[-1].any(dim=1).all()), name  # the maximum always survives


STAT_ROWS = 65536


@pytest.mark.parametrize("seed", [1, 0xDEADBEEF])
@pytest.mark.parametrize("knobs", [(12, 1.0, 0.0), (0, 0.8, 0.0), (0, 1.0, 0.08), (20, 0.9, 0.02)])
def test_sample_frequencies_follow_the_truncated_softmax(knobs, seed):
    """Pearson chi-square of 65,536 draws of one bf16 logit vector over 64 ids
    against softmax(logits / T) renormalised over the kept set, bins of
    expected count < 5 merged: below the 1e-4 upper quantile (as
    test_sampling_reference.py); no draw falls outside the kept set."""
    from scipy.stats import chi2
    T = 0.7
    logit = torch.randn(64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    i = torch.arange(STAT_ROWS)
    slots, pos = (i % 768).to(torch.int32), (100 + i // 768).to(torch.int32)
    rows = logit[None].expand(STAT_ROWS, 64).contiguous()
    tau, kept, _ = reference.truncation_threshold(rows[:1], None, 64, None, slots[:1], T, *knobs)
    assert 1 < int(kept) < 64
    # every row has row 0's threshold (same values): skip the per-row search ...
    ids, _ = reference.truncated_sample_at(tau.expand(STAT_ROWS), rows, None, 64, None, slots, pos, T, seed)
    # ... after checking that it is what truncated_sample does
    assert torch.equal(ids[:512], reference.truncated_sample(rows[:512], None, 64, None, None, slots[:512],
                                                             pos[:512], T, seed, *knobs))
    keep = logit.float() >= tau
    count = torch.bincount(ids.long(), minlength=64).double()
    assert float(count[~keep].sum()) == 0
    prob = torch.softmax(logit.double() / T, 0) * keep
    expect = (prob / prob.sum())[keep] * STAT_ROWS
    count = count[keep]
    small = expect < 5
    if bool(small.any()):
        expect = torch.cat([expect[~small], expect[small].sum()[None]])
        count = torch.cat([count[~small], count[small].sum()[None]])
    assert float(expect.min()) >= 5
    stat = float(((count - expect) ** 2 / expect).sum())
    dof = expect.numel() - 1
    bound = float(chi2.isf(1e-4, dof))
    print(f"knobs={knobs} seed={seed}: chi-square {stat:.1f} at {dof} degrees of freedom (bound {bound:.1f})")
    assert stat < bound


@pytest.fixture(scope="module")
def tiny():
    from dmcp.models.llm import LocalLM, preset
    torch.manual_seed(0)
    return LocalLM(preset("tiny", max_batch=4, max_rows=16, max_seq=2048), device="cpu", seed=1)


def test_invalid_knobs_name_themselves(tiny):
    from dmcp.enrich.local import LocalEngine
    for kw, name in (({"top_k": -1}, "top_k"), ({"top_k": 2.5}, "top_k"), ({"top_p": 0.0}, "top_p"),
                     ({"top_p": 1.5}, "top_p"), ({"top_p": float("nan")}, "top_p"), ({"min_p": 1.0}, "min_p"),
                     ({"min_p": -0.1}, "min_p")):
        with pytest.raises(ValueError, match=name):
            LocalEngine(tiny, use_graphs=False, temperature=0.7, **kw)
        with pytest.raises(ValueError, match=name):
            LocalEngine(tiny, use_graphs=False, **kw)  # checked at temperature 0 too
        with pytest.raises(ValueError, match=name):
            reference.truncation_args(**kw)
    eng = LocalEngine(tiny, use_graphs=False, temperature=0.7, top_k=20, top_p=0.95, min_p=0.0)
    assert (eng.top_k, eng.top_p, eng.min_p) == (20, 0.95, 0.0)


def test_config_and_worker_frames_carry_the_knobs():
    from dmcp.config import Config
    from dmcp.enrich.workers import engine_spec
    c = Config()
    assert (c.local_llm_top_k, c.local_llm_top_p, c.local_llm_min_p) == (0, 1.0, 0.0)
    spec = engine_spec(c)
    assert (spec["top_k"], spec["top_p"], spec["min_p"]) == (0, 1.0, 0.0)
    cfg = Config.from_env({"LOCAL_LLM_TEMPERATURE": "0.6", "LOCAL_LLM_TOP_K": "20", "LOCAL_LLM_TOP_P": "0.95",
                           "LOCAL_LLM_MIN_P": "0.05"})
    assert (cfg.local_llm_top_k, cfg.local_llm_top_p, cfg.local_llm_min_p) == (20, 0.95, 0.05)
    spec = engine_spec(cfg)
    assert (spec["top_k"], spec["top_p"], spec["min_p"]) == (20, 0.95, 0.05)
    assert json.loads(json.dumps(spec)) == spec  # travels in a worker's init frame


def test_model_selection_paths_take_the_truncation(tiny):
    """decode_select / decode_select_gather with ``truncate`` select what
    truncated_sample selects from the step's logits; with every filter off,
    or greedy, they are the untruncated paths."""
    from dmcp.enrich.local import LocalEngine
    masks = LocalEngine(tiny, use_graphs=False).masks
    V = tiny.cfg.vocab_size
    toks, slots, pos = _i32([65, 66, 67, 68]), _i32([0, 1, 2, 3]), _i32([0, 0, 0, 0])
    midx = _i32([0, 0, 1, 0])
    cut = (3, 0.9, 0.01)
    picks = set()
    for seed in range(6):
        logits, ids = tiny.decode_select(toks, slots, pos, masks, midx, sample=(0.9, seed), truncate=cut)
        want = reference.truncated_sample(logits, masks, V, None, midx, slots, pos, 0.9, seed, *cut)
        assert torch.equal(ids, want)
        last = torch.zeros(16, dtype=torch.int32)
        logits2, ids2 = tiny.decode_select_gather(toks, _i32([-1] * 4), last, slots, pos, masks, midx,
                                                  sample=(0.9, seed), truncate=cut)
        assert torch.equal(logits2, logits) and torch.equal(ids2, want) and torch.equal(last[:4], want)
        plain = reference.masked_sample(logits, masks, V, None, midx, slots, pos, 0.9, seed)
        _, off = tiny.decode_select(toks, slots, pos, masks, midx, sample=(0.9, seed), truncate=(0, 1.0, 0.0))
        assert torch.equal(off, plain)
        picks.add((tuple(want.tolist()), tuple(plain.tolist())))
    assert any(a != b for a, b in picks)  # the truncation changed a draw
    _, greedy = tiny.decode_select(toks, slots, pos, masks, midx, sample=(0.0, 1), truncate=cut)
    assert torch.equal(greedy, reference.masked_argmax(logits, masks, V, None, midx))
    _, greedy = tiny.decode_select(toks, slots, pos, masks, midx, truncate=cut)
    assert torch.equal(greedy, reference.masked_argmax(logits, masks, V, None, midx))


def test_engine_replies_under_truncation(tiny):
    from dmcp.enrich.local import CLASS_TYPES, LocalEngine, ReplyShape
    from dmcp.enrich.types import EnrichmentInput
    inputs = [EnrichmentInput("public class S%d { void a() {} void b() {} }" % i, f"co.x.S{i}", "java", "SERVICE",
                              ["a", "b", "c"][: 1 + i % 3]) for i in range(2)]
    kw = {"reply_shape": ReplyShape(24, 16, 12, 1), "temperature": 0.8, "seed": 5}
    plain = LocalEngine(tiny, **kw).generate(inputs, "A readme")
    assert LocalEngine(tiny, top_k=0, top_p=1.0, min_p=0.0, **kw).generate(inputs, "A readme") == plain
    a = LocalEngine(tiny, top_k=4, top_p=0.9, **kw).generate(inputs, "A readme")
    assert any(x != y for x, y in zip(a, plain))
    for r, inp in zip(a, inputs):
        doc = json.loads(r)
        assert [m["methodName"] for m in doc["methods"]] == inp.method_names
        assert doc["classTypeCorrection"] is None or doc["classTypeCorrection"] in CLASS_TYPES
    greedy = LocalEngine(tiny, reply_shape=kw["reply_shape"]).generate(inputs, "A readme")
    assert LocalEngine(tiny, reply_shape=kw["reply_shape"], top_k=4, top_p=0.5).generate(inputs, "A readme") == greedy
