"""The local engine end to end on the CPU behind a ChatML chat template: a
tiny written checkpoint (no random-weights switch involved), every reply
parses, the tokens the model is fed for each class are exactly
``transformers``' ``apply_chat_template`` ids followed by the forced start of
the reply, the turn header is part of the prefix prefilled once per project,
method branches still fork from the head's KV -- and a CPU worker process
reports the mode it resolved to in its witness."""
import json

import pytest

from dmcp.enrich.backend import build_enrichment_prompt
from dmcp.enrich.local import LocalEngine
from dmcp.enrich.tokenizer import load_local_model
from tests import chat_fixtures as F
from tests.test_chat_template import _hf_ids


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return F.write_checkpoint(str(tmp_path_factory.mktemp("chat_engine") / "chatml"), F.CHATML)


def test_cpu_engine_end_to_end_behind_chatml(ckpt):
    model, tok = load_local_model(ckpt, device="cpu", max_batch=4, max_rows=32, max_seq=2048)
    assert model.checkpoint == ckpt
    eng = LocalEngine(model, tokenizer=tok, use_graphs=False, max_new_tokens=160)
    assert eng.chat_mode.startswith("template:") and eng.chat_mode.endswith("tokenizer_config.json")
    rec = F.Recorder(model)
    inputs = F.inputs()
    raw = eng.generate(inputs, F.README)
    for r, inp in zip(raw, inputs):
        doc = json.loads(r)
        assert [m["methodName"] for m in doc["methods"]] == inp.method_names
        assert isinstance(doc["description"], str)
    exp = [_hf_ids(ckpt, build_enrichment_prompt(inp, F.README).strip()) for inp in inputs]
    fed = rec.fed()
    assert len(fed) == 3 and eng.stats["prefills"] == 3
    for e in exp:  # prompt ids, then the forced first segment of the reply right after tail_ids
        (f,) = [f for f in fed if f[:len(e)] == e]
        assert len(f) > len(e) and tok.decode(f[len(e):]).startswith("{")
        assert e[-len(eng.tail_ids):] == eng.tail_ids
    # the prefix, prefilled once, begins with the turn header and is shared by the three classes
    assert len(rec.prefixes) == 1 and eng.stats["prefix_switches"] == 1 and eng.stats["unshared_prefills"] == 0
    P = len(rec.prefixes[0])
    assert rec.prefixes[0][:len(eng.head_ids)] == eng.head_ids and P > len(eng.head_ids)
    assert all(e[:P] == rec.prefixes[0] for e in exp)
    assert all(start == P for batch in rec.batches for _, _, start in batch)
    # method branches read their head's KV in place: the fork table was set
    assert eng.stats["forks"] == 3 and eng.stats["fork_branches"] >= 3
    assert rec.forks and all(end > P for _, _, end in rec.forks)
    # the raw path on the same directory: other tokens, replies still parse
    off = LocalEngine(model, tokenizer=tok, use_graphs=False, max_new_tokens=160, chat_template="off")
    rec.prefixes.clear(), rec.batches.clear()
    for r in off.generate(inputs, F.README):
        json.loads(r)
    assert rec.prefixes[0][:len(eng.head_ids)] != eng.head_ids


def test_cpu_worker_reports_the_mode_in_its_witness(ckpt):
    from dmcp.enrich.workers import GpuWorkerPool, ProcessLLMBackend
    for knob, mode in (("auto", "template:"), ("off", "raw")):
        pool = GpuWorkerPool(["cpu"], {"path": ckpt, "max_batch": 2, "max_rows": 16, "max_seq": 2048,
                                       "chat_template": knob},
                             engine={"use_graphs": False, "max_new_tokens": 128, "chat_template": knob},
                             start_timeout_s=300, env_extra={"OMP_NUM_THREADS": "2"})
        try:
            res = ProcessLLMBackend(pool).enrich_batch(F.inputs()[:2], F.README)
            assert all(r.success for r in res), [r.error_message for r in res]
            (w,) = pool.live()
            assert w.info["witness"]["chat_template"].startswith(mode)
        finally:
            pool.close()
