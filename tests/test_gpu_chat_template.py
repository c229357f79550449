"""The chat turn on the GPU: one project of three classes through the real
engine (hipGraph decode, gfx950 kernels) behind the ChatML template of a tiny
written checkpoint -- hidden 256, 2 layers, 4/2 heads, head_dim 64, max_seq
1024, 4 slots, bf16 KV.  The prompt ids are the CPU engine's, the prefix
(turn header + instructions + README) is prefilled once and the three classes
are admitted in one packed prefill, and the last-prompt-position logits stay
as close to the fp32 CPU model as the raw prompts of the same classes do.

Bound: the chat prompts add a few dozen header / trailer tokens to prompts of
several hundred, so their worst 1 - cosine against ``reference_logits`` may be
at most 2x the worst of the same three classes with
``LOCAL_LLM_CHAT_TEMPLATE=off``, measured in the same run (the margin
docs/PARITY.md uses for every new checkpoint case against its baseline)."""
import json

import pytest
import torch

from tests import chat_fixtures as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MODEL = dict(max_seq=1024, max_batch=4, max_rows=64, kv_dtype="bf16")
ENGINE = dict(max_new_tokens=128)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return F.write_checkpoint(str(tmp_path_factory.mktemp("gpu_chat") / "chatml"), F.CHATML)


def _cpu_prompts(ckpt, knob):
    """(ids, prefix_split) of the three classes from a CPU engine, and the
    fp32 last-position logits of the CPU model over each full id list."""
    from dmcp.enrich.local import LocalEngine, _Seq
    from dmcp.enrich.tokenizer import load_local_model
    model, tok = load_local_model(ckpt, device="cpu", max_seq=1024, max_batch=4, max_rows=64)
    eng = LocalEngine(model, tokenizer=tok, use_graphs=False, chat_template=knob, **ENGINE)
    out = []
    for q in (eng._seqs_for(i, inp, F.README)[0] for i, inp in enumerate(F.inputs())):
        out.append((q.prompt, q.prefix_split, model.reference_logits(q.prompt)[-1].float()))
    return eng, out


def _one_minus_cosine(model, prompts):
    """Worst 1 - cosine over the classes: the prefix prefilled once, the
    per-class parts in one packed prefill (what the engine's admission does),
    last prompt position against the fp32 CPU logits."""
    model.clear_prefix()
    split = prompts[0][1]
    assert split and all(s == split and ids[:split] == prompts[0][0][:split] for ids, s, _ in prompts)
    model.set_prefix(prompts[0][0][:split])
    got = model.prefill_batch([(ids[split:], slot, model.fork_prefix(slot))
                               for slot, (ids, _, _) in enumerate(prompts)]).float().cpu()
    model.clear_prefix()
    worst = 0.0
    for row, (_, _, ref) in zip(got, prompts):
        worst = max(worst, 1.0 - torch.nn.functional.cosine_similarity(row.double(), ref.double(), dim=0).item())
    return worst


def test_chat_project_on_the_gpu(ckpt):
    from dmcp.enrich.local import LocalEngine
    from dmcp.enrich.tokenizer import load_local_model
    from dmcp.ops import hip
    hip.lib()
    cpu_eng, chat = _cpu_prompts(ckpt, "auto")
    _, raw = _cpu_prompts(ckpt, "off")
    head, tail = cpu_eng.head_ids, cpu_eng.tail_ids
    assert len(head) > 8 and all(len(ids) < 1024 - 128 for ids, _, _ in chat)

    model, tok = load_local_model(ckpt, device="cuda", **MODEL)
    eng = LocalEngine(model, tokenizer=tok, **ENGINE)
    assert eng.graphs is not None and eng.chat_mode.startswith("template:")
    assert eng.head_ids == head and eng.tail_ids == tail
    rec = F.Recorder(model)
    inputs = F.inputs()
    replies = eng.generate(inputs, F.README)
    for r, inp in zip(replies, inputs):
        assert [m["methodName"] for m in json.loads(r)["methods"]] == inp.method_names

    # the prompt ids are the CPU engine's; the reply starts right after tail_ids
    fed = rec.fed()
    assert len(fed) == 3
    for ids, split, _ in chat:
        (f,) = [f for f in fed if f[:len(ids)] == ids]
        assert ids[-len(tail):] == tail and tok.decode(f[len(ids):]).startswith("{")
    # one prefix prefill -- ids[:prefix_split], beginning with the turn header -- and one packed admission
    split = chat[0][1]
    assert rec.prefixes == [chat[0][0][:split]] and rec.prefixes[0][:len(head)] == head and split > len(head)
    assert len(rec.batches) == 1 and len(rec.batches[0]) == 3
    assert all(start == split for _, _, start in rec.batches[0])
    assert eng.stats["prefix_switches"] == 1 and eng.stats["prefill_batches"] == 1 and eng.stats["prefills"] == 3
    assert eng.stats["unshared_prefills"] == 0 and eng.stats["forks"] == 3

    # logits at the last prompt position against the fp32 CPU model: chat within 2x of raw
    e_chat = _one_minus_cosine(model, chat)
    e_raw = _one_minus_cosine(model, raw)
    print(f"chat template 1-cos {e_chat:.3e}  raw (LOCAL_LLM_CHAT_TEMPLATE=off) 1-cos {e_raw:.3e}  "
          f"ratio {e_chat / e_raw:.2f}")
    assert e_raw > 0 and e_chat <= 2.0 * e_raw, (e_chat, e_raw)
