"""Temperature sampling on the CPU: the noise definition of
dmcp/ops/reference.py (``gumbel_bits`` / ``gumbel_noise``) against a plain-int
implementation, the statistics of ``masked_sample`` against softmax(logits /
T), its edge cases, and the ``temperature`` / ``seed`` knobs of the engine,
the configuration and the worker frames.  The gfx950 kernels draw from the
same bits (tests/test_gpu_sampling.py)."""
import json
import random

import pytest
import torch

from dmcp import ops
from dmcp.ops import reference

M32 = 0xFFFFFFFF
GOLD = 0x9E3779B1


def _fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _bits(seed, slot, position, v):
    key = _fmix32((seed & M32) ^ _fmix32((slot * GOLD + position) & M32))
    return _fmix32((key + v * GOLD) & M32)


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32)


def test_gumbel_bits_match_a_plain_int_implementation():
    rng = random.Random(5)
    V = 128256
    tuples = [(rng.getrandbits(32), rng.randrange(768), rng.randrange(8192), rng.randrange(V)) for _ in range(300)]
    tuples += [(0, 767, 8191, 128255), (M32, 767, 0, 128254), (12345, 0, 0, 0), (1, 767, 4095, 128250),
               (2 ** 31, 767, 100, 128255), (7, 1, 2 ** 20, 64)]
    for seed, slot, pos, v in tuples:
        got = reference.gumbel_bits(seed, _i32([slot, 3]), _i32([pos, 9]), V)
        assert got.shape == (2, V)
        assert int(got[0, v]) == _bits(seed, slot, pos, v), (seed, slot, pos, v)
        assert int(got[1, 5]) == _bits(seed, 3, 9, 5)
    # a seed outside uint32 is taken modulo 2^32, a negative slot as its two's complement (the kernels' cast)
    assert torch.equal(reference.gumbel_bits(2 ** 32 + 9, _i32([4]), _i32([6]), 16),
                       reference.gumbel_bits(9, _i32([4]), _i32([6]), 16))
    assert int(reference.gumbel_bits(3, _i32([-1]), _i32([2]), 8)[0, 7]) == _bits(3, M32, 2, 7)


def test_u_is_strictly_inside_the_unit_interval_in_fp32(monkeypatch):
    for bits, want in ((0, 2.0 ** -24), (M32, 1.0 - 2.0 ** -24)):
        monkeypatch.setattr(reference, "gumbel_bits",
                            lambda seed, slots, positions, vocab, b=bits: torch.full((1, 1), b, dtype=torch.int64))
        for dtype in (torch.float32, torch.float64):
            g = reference.gumbel_noise(0, _i32([0]), _i32([0]), 1, dtype)
            assert g.dtype == dtype and bool(torch.isfinite(g).all())
            u = torch.exp(-torch.exp(-g.double()))
            assert 0.0 < float(u) < 1.0 and abs(float(u) - want) < 1e-9
        u32 = torch.tensor((bits >> 9) * 2 + 1, dtype=torch.int64).to(torch.float32) * 2.0 ** -24
        assert float(u32) == want and 0.0 < float(u32) < 1.0  # exact in fp32: no rounding to 0 or 1


STAT_ROWS = 65536


@pytest.fixture(scope="module")
def stat_inputs():
    g = torch.Generator().manual_seed(0)
    logit = torch.randn(64, generator=g).to(torch.bfloat16)
    i = torch.arange(STAT_ROWS)
    return logit, (i % 768).to(torch.int32), (100 + i // 768).to(torch.int32)


@pytest.mark.parametrize("seed", [1, 20240229, 0xDEADBEEF])
@pytest.mark.parametrize("temperature", [0.5, 1.0])
def test_sample_frequencies_follow_the_softmax(stat_inputs, temperature, seed):
    """Pearson chi-square of 65,536 draws (slots i % 768, positions 100 +
    i // 768) of one bf16 logit vector over 64 ids against softmax(logits /
    T), bins of expected count < 5 merged: below the 1e-4 upper quantile."""
    from scipy.stats import chi2
    logit, slots, pos = stat_inputs
    rows = logit[None].expand(STAT_ROWS, 64).contiguous()
    ids = reference.masked_sample(rows, None, 64, None, None, slots, pos, temperature, seed)
    count = torch.bincount(ids.long(), minlength=64).double()
    expect = torch.softmax(logit.double() / temperature, 0) * STAT_ROWS
    small = expect < 5
    if bool(small.any()):
        expect = torch.cat([expect[~small], expect[small].sum()[None]])
        count = torch.cat([count[~small], count[small].sum()[None]])
    assert float(expect.min()) >= 5
    stat = float(((count - expect) ** 2 / expect).sum())
    dof = expect.numel() - 1
    bound = float(chi2.isf(1e-4, dof))
    print(f"T={temperature} seed={seed}: chi-square {stat:.1f} at {dof} degrees of freedom (bound {bound:.1f})")
    assert stat < bound


def _mask_of(allowed, V):
    words = [0] * ((V + 31) // 32)
    for v in allowed:
        words[v >> 5] |= 1 << (v & 31)
    return [w - (1 << 32) if w >= 1 << 31 else w for w in words]


def test_mask_edge_cases_and_temperature_zero():
    V = 200
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(96, 208, generator=g).to(torch.bfloat16)  # ld > V: the padding columns are never drawn
    allowed = [[7], [], [199], list(range(0, V, 3)), [31, 32, 63, 64]]
    masks = torch.tensor([_mask_of(a, V) for a in allowed], dtype=torch.int32)
    midx = _i32(i % 5 for i in range(96))
    slots, pos = _i32(range(96)), _i32(50 + i for i in range(96))
    for seed in range(8):
        ids = reference.masked_sample(logits, masks, V, None, midx, slots, pos, 1.5, seed).tolist()
        for r, v in enumerate(ids):
            a = allowed[r % 5]
            assert v in a if a else v == 0, (r, v)
            if len(a) == 1:
                assert v == a[0]
    # an output buffer is filled and returned
    out = torch.full((96,), -1, dtype=torch.int32)
    assert reference.masked_sample(logits, masks, V, out, midx, slots, pos, 1.5, 7) is out and int(out.min()) >= 0
    # per-row masks (no mask_idx), and no mask at all
    per_row = masks[midx.long()]
    assert torch.equal(reference.masked_sample(logits, per_row, V, None, None, slots, pos, 1.5, 7), out)
    free = reference.masked_sample(logits, None, V, None, None, slots, pos, 1.5, 7)
    assert int(free.max()) < V
    # padding rows (slot < 0) draw nothing
    pad = slots.clone()
    pad[::2] = -1
    got = reference.masked_sample(logits, None, V, None, None, pad, pos, 1.5, 7)
    assert got[::2].abs().sum() == 0 and torch.equal(got[1::2], free[1::2])
    # temperature 0 is the greedy op, exactly
    for mk, mi in ((masks, midx), (per_row, None), (None, None)):
        assert torch.equal(reference.masked_sample(logits, mk, V, None, mi, slots, pos, 0.0, 7),
                           reference.masked_argmax(logits, mk, V, None, mi))
    assert torch.equal(ops.masked_sample(logits, masks, V, None, midx, slots, pos, 0, 1),
                       ops.masked_argmax(logits, masks, V, None, midx))
    x = torch.randn(9, 64, generator=g).to(torch.bfloat16)
    w = torch.randn(V, 64, generator=g).to(torch.bfloat16)
    assert torch.equal(ops.lm_head_sample(x, w, masks, midx[:9], slots=slots[:9], positions=pos[:9]),
                       ops.lm_head_argmax(x, w, masks, midx[:9]))
    lg = (x.float() @ w.float().t()).to(torch.bfloat16)
    assert torch.equal(ops.lm_head_sample(x, w, masks, midx[:9], None, None, slots[:9], pos[:9], 0.8, 4),
                       ops.masked_sample(lg, masks, V, None, midx[:9], slots[:9], pos[:9], 0.8, 4))
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            reference.masked_sample(logits, masks, V, None, midx, slots, pos, bad, 1)
    for s_, p_ in ((None, pos), (slots, None), (slots.long(), pos), (slots[:5], pos)):
        with pytest.raises(ValueError):
            reference.masked_sample(logits, masks, V, None, midx, s_, p_, 0.7, 1)


def test_a_row_draws_the_same_alone_and_in_a_shuffled_batch():
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(64, 96, generator=g) * 0.5).to(torch.bfloat16)
    slots = _i32(random.Random(1).sample(range(768), 64))
    pos = _i32(random.Random(2).sample(range(4000), 64))
    batch = reference.masked_sample(logits, None, 96, None, None, slots, pos, 0.9, 42)
    perm = torch.randperm(64, generator=g)
    shuffled = reference.masked_sample(logits[perm].contiguous(), None, 96, None, None, slots[perm], pos[perm], 0.9,
                                       42)
    assert torch.equal(shuffled, batch[perm])
    for r in range(64):
        alone = reference.masked_sample(logits[r:r + 1], None, 96, None, None, slots[r:r + 1], pos[r:r + 1], 0.9, 42)
        assert int(alone) == int(batch[r])


def test_seed_and_position_change_the_draws():
    """Near-uniform distribution over 64 ids: two seeds (two positions) agree
    on ~1/64 of the rows by chance; a quarter differing is a floor only a
    constant output misses."""
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(1024, 64, generator=g) * 0.05).to(torch.bfloat16)
    slots, pos = _i32(i % 768 for i in range(1024)), _i32(10 + i // 768 for i in range(1024))
    a = reference.masked_sample(logits, None, 64, None, None, slots, pos, 1.0, 1)
    b = reference.masked_sample(logits, None, 64, None, None, slots, pos, 1.0, 2)
    c = reference.masked_sample(logits, None, 64, None, None, slots, pos + 1, 1.0, 1)
    d = reference.masked_sample(logits, None, 64, None, None, slots, pos, 1.0, 1)
    assert torch.equal(a, d)
    assert int((a != b).sum()) >= 256 and int((a != c).sum()) >= 256
    assert len(set(a.tolist())) > 32


@pytest.fixture(scope="module")
def tiny():
    from dmcp.models.llm import LocalLM, preset
    torch.manual_seed(0)
    return LocalLM(preset("tiny", max_batch=4, max_rows=16, max_seq=2048), device="cpu", seed=1)


def _inputs(n):
    from dmcp.enrich.types import EnrichmentInput
    return [EnrichmentInput("public class S%d { void a() {} void b() {} }" % i, f"co.x.S{i}", "java", "SERVICE",
                            ["a", "b", "c"][: 1 + i % 3]) for i in range(n)]


def test_engine_temperature_and_seed(tiny):
    from dmcp.enrich.local import CLASS_TYPES, LocalEngine, ReplyShape
    inputs = _inputs(5)  # > max_batch 4: a slot is recycled
    kw = {"reply_shape": ReplyShape(24, 16, 12, 1)}  # short strings: a quick test
    plain = LocalEngine(tiny, **kw).generate(inputs, "A readme")
    assert LocalEngine(tiny, temperature=0.0, seed=5, **kw).generate(inputs, "A readme") == plain
    a = LocalEngine(tiny, temperature=0.8, seed=5, **kw).generate(inputs, "A readme")
    b = LocalEngine(tiny, temperature=0.8, seed=5, **kw).generate(inputs, "A readme")
    c = LocalEngine(tiny, temperature=0.8, seed=6, **kw).generate(inputs, "A readme")
    assert a == b
    assert any(x != y for x, y in zip(a, c))
    assert any(x != y for x, y in zip(a, plain))
    for raw in (a, c):
        for r, inp in zip(raw, inputs):
            doc = json.loads(r)
            assert [m["methodName"] for m in doc["methods"]] == inp.method_names
            assert doc["classTypeCorrection"] is None or doc["classTypeCorrection"] in CLASS_TYPES
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            LocalEngine(tiny, use_graphs=False, temperature=bad)


def test_model_selection_paths_take_sample(tiny):
    """decode_select / decode_select_gather with ``sample`` draw what
    masked_sample draws from the step's logits; without it they stay greedy."""
    from dmcp.enrich.local import LocalEngine
    masks = LocalEngine(tiny, use_graphs=False).masks
    V = tiny.cfg.vocab_size
    toks, slots, pos = _i32([65, 66, 67]), _i32([0, 1, 2]), _i32([0, 0, 0])
    midx = _i32([0, 0, 1])
    logits, greedy = tiny.decode_select(toks, slots, pos, masks, midx)
    assert torch.equal(greedy, reference.masked_argmax(logits, masks, V, None, midx))
    logits2, ids = tiny.decode_select(toks, slots, pos, masks, midx, sample=(0.9, 3))
    assert torch.equal(logits2, logits)
    assert torch.equal(ids, reference.masked_sample(logits, masks, V, None, midx, slots, pos, 0.9, 3))
    last = torch.zeros(16, dtype=torch.int32)
    src = _i32([-1, -1, -1])
    _, ids3 = tiny.decode_select_gather(toks, src, last, slots, pos, masks, midx, sample=(0.9, 3))
    assert torch.equal(ids3, ids) and torch.equal(last[:3], ids)
    _, ids0 = tiny.decode_select_gather(toks, src, last, slots, pos, masks, midx, sample=(0.0, 3))
    assert torch.equal(ids0, greedy)


def test_config_and_worker_frames_carry_temperature_and_seed():
    from dmcp.config import Config
    from dmcp.enrich.workers import engine_spec
    assert (Config().local_llm_temperature, Config().local_llm_seed) == (0.0, 0)
    assert engine_spec(Config())["temperature"] == 0.0 and engine_spec(Config())["seed"] == 0
    cfg = Config.from_env({"LOCAL_LLM_TEMPERATURE": "0.7", "LOCAL_LLM_SEED": "1234"})
    assert cfg.local_llm_temperature == 0.7 and cfg.local_llm_seed == 1234
    spec = engine_spec(cfg)
    assert spec["temperature"] == 0.7 and spec["seed"] == 1234
    assert json.loads(json.dumps(spec)) == spec  # travels in a worker's init frame
