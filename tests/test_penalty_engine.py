"""The repetition / presence penalty through the model and the engine, on the
CPU (tiny preset): replies still parse, the penalty off is today's engine,
invalid settings are refused when the engine is built, a reused slot starts
from an empty history, and decode_select / decode_select_gather record first
and select with the penalised reference."""
import json

import pytest
import torch

from dmcp.ops import reference


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32)


@pytest.fixture(scope="module")
def tiny():
    from dmcp.models.llm import LocalLM, preset
    torch.manual_seed(0)
    return LocalLM(preset("tiny", max_batch=4, max_rows=16, max_seq=2048), device="cpu", seed=1)


def _inputs(n):
    from dmcp.enrich.types import EnrichmentInput
    return [EnrichmentInput("public class S%d { void a() {} void b() {} }" % i, f"co.x.S{i}", "java", "SERVICE",
                            ["a", "b", "c"][: 1 + i % 3]) for i in range(n)]


def _bits(row):
    return {32 * w + b for w, x in enumerate(row.tolist()) for b in range(32) if (x >> b) & 1}


def test_engine_replies_parse_and_off_is_todays_engine(tiny):
    from dmcp.enrich.local import CLASS_TYPES, LocalEngine, ReplyShape
    inputs = _inputs(5)  # > max_batch 4: a slot is recycled
    kw = {"reply_shape": ReplyShape(24, 16, 12, 1)}
    tiny.history = None
    plain = LocalEngine(tiny, **kw).generate(inputs, "A readme")
    off = LocalEngine(tiny, repetition_penalty=1.0, presence_penalty=0.0, **kw)
    assert off._penalty is None and "penalty" not in off._sample_kw and tiny.history is None  # no table
    assert off.generate(inputs, "A readme") == plain
    for extra in ({}, {"temperature": 0.8, "seed": 5}, {"temperature": 0.8, "seed": 5, "top_k": 20, "top_p": 0.9}):
        base = LocalEngine(tiny, **kw, **extra).generate(inputs, "A readme")
        eng = LocalEngine(tiny, repetition_penalty=1.3, presence_penalty=0.5, **kw, **extra)
        raw = eng.generate(inputs, "A readme")
        assert raw == LocalEngine(tiny, repetition_penalty=1.3, presence_penalty=0.5, **kw,
                                  **extra).generate(inputs, "A readme")  # reproducible
        assert any(x != y for x, y in zip(raw, base))  # it does act, greedy included
        for r, inp in zip(raw, inputs):
            doc = json.loads(r)
            assert [m["methodName"] for m in doc["methods"]] == inp.method_names
            assert doc["classTypeCorrection"] is None or doc["classTypeCorrection"] in CLASS_TYPES
        for s in range(tiny.num_slots):  # the lone quote is never recorded
            assert eng._quote not in _bits(tiny.history[s])


def test_invalid_settings_are_refused_when_the_engine_is_built(tiny):
    from dmcp.enrich.local import LocalEngine
    for bad in (0.0, -1.1, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="repetition_penalty"):
            LocalEngine(tiny, use_graphs=False, repetition_penalty=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), "some"):
        with pytest.raises(ValueError, match="presence_penalty"):
            LocalEngine(tiny, use_graphs=False, presence_penalty=bad)
    LocalEngine(tiny, use_graphs=False, repetition_penalty=0.9, presence_penalty=-0.2)  # both directions are valid


def test_a_reused_slot_starts_from_an_empty_history(tiny):
    """One slot, two classes without methods to fork: after the run the
    slot's row holds only tokens of the second class's reply -- the first
    class's strings were zeroed when the slot was assigned again."""
    from dmcp.enrich.local import LocalEngine, ReplyShape
    from dmcp.enrich.types import EnrichmentInput
    from dmcp.models.llm import LocalLM, preset
    torch.manual_seed(0)
    one = LocalLM(preset("tiny", max_batch=1, max_rows=16, max_seq=2048), device="cpu", seed=1)
    inputs = [EnrichmentInput("public class S%d { }" % i, f"co.x.S{i}", "java", "SERVICE", []) for i in range(2)]
    kw = {"reply_shape": ReplyShape(24, 16, 12, 1), "repetition_penalty": 1.3, "presence_penalty": 0.5,
          "fork_methods": False}
    eng = LocalEngine(one, **kw)
    marked = []
    real = reference.history_reset

    def spy(history, slots):
        marked.append((sorted(slots), _bits(history[0])))
        return real(history, slots)
    import dmcp.ops as ops
    orig = ops.history_reset
    ops.history_reset = lambda h, s: spy(h, s)
    try:
        raw = eng.generate(inputs, "A readme")
    finally:
        ops.history_reset = orig
    assert [s for s, _ in marked] == [[0], [0]]
    assert marked[0][1] == set() and marked[1][1]  # empty at first; the first reply's tokens at the second assignment
    after = _bits(one.history[0])
    second = LocalEngine(one, **kw)
    one.history.zero_()
    assert second.generate(inputs[1:], "A readme") == raw[1:]
    assert after == _bits(one.history[0]) and after  # exactly the second class's own tokens


def test_model_selection_paths_record_first_and_penalise(tiny):
    from dmcp.enrich.local import LocalEngine
    from dmcp import ops
    eng = LocalEngine(tiny, use_graphs=False, repetition_penalty=1.3, presence_penalty=0.5)
    masks, V = eng.masks, tiny.cfg.vocab_size
    theta, alpha, flags, exempt = pen = eng._penalty
    assert flags.tolist()[:2] == [1, 1] and not any(flags.tolist()[2:])
    assert _bits(exempt) == {eng._quote}
    toks, slots, pos = _i32([65, 66, eng._quote, 70]), _i32([0, 1, 2, 1]), _i32([0, 0, 0, 1])
    midx = _i32([0, 0, 1, 0])
    tiny.history.zero_()
    logits, ids = tiny.decode_select(toks, slots, pos, masks, midx, penalty=pen)
    assert [_bits(tiny.history[s]) for s in range(4)] == [{65}, {66, 70}, set(), set()]  # two rows, one slot
    p = ops.Penalty(tiny.history, slots, theta, alpha, flags)
    assert torch.equal(ids, reference.masked_argmax(logits, masks, V, None, midx, p))
    # gathered tokens are the ones recorded, before last_ids is overwritten
    tiny.history.zero_()
    last = _i32([90, 91, 92, 93] + [0] * 12)
    src = _i32([3, -1, 0, -1])
    logits, ids = tiny.decode_select_gather(toks, src, last, slots, pos, masks, midx, penalty=pen,
                                            sample=(0.9, 3), truncate=(20, 0.9, 0.0))
    assert [_bits(tiny.history[s]) for s in range(4)] == [{93}, {66, 70}, {90}, set()]
    want = reference.truncated_sample(logits, masks, V, None, midx, slots, pos, 0.9, 3, 20, 0.9, 0.0,
                                      penalty=ops.Penalty(tiny.history, slots, theta, alpha, flags))
    assert torch.equal(ids, want) and torch.equal(last[:4], ids)
    # off: nothing recorded, the unpenalised ids
    tiny.history.zero_()
    _, plain = tiny.decode_select(toks, slots, pos, masks, midx)
    _, off = tiny.decode_select(toks, slots, pos, masks, midx, penalty=(1.0, 0.0, flags, exempt))
    assert torch.equal(plain, off) and int(tiny.history.abs().sum()) == 0


def test_config_and_worker_frames_carry_the_penalties():
    from dmcp.config import Config
    from dmcp.enrich.workers import engine_spec
    assert (Config().local_llm_repetition_penalty, Config().local_llm_presence_penalty) == (1.0, 0.0)
    cfg = Config.from_env({"LOCAL_LLM_REPETITION_PENALTY": "1.1", "LOCAL_LLM_PRESENCE_PENALTY": "0.25"})
    spec = engine_spec(cfg)
    assert (spec["repetition_penalty"], spec["presence_penalty"]) == (1.1, 0.25)
    assert json.loads(json.dumps(spec)) == spec  # travels in a worker's init frame
