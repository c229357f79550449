"""The chat turn around the enrichment prompt (dmcp/enrich/chat.py, the
prompt builder of dmcp/enrich/local.py), on the CPU: the ids equal
``transformers``' ``apply_chat_template`` for three templates, the template's
BOS is the only one, untrusted source text cannot forge a turn, the shared
prefix survives, truncation cuts content only, unusable templates are refused
at start, the ``LOCAL_LLM_CHAT_TEMPLATE`` knob, and the Jinja sandbox.

The templates, the tokenizer and the checkpoints are written here
(tests/chat_fixtures.py).  The engine renders the STRIPPED prompt text (so
that a template's ``| trim`` changes nothing): ``transformers`` is given the
same stripped text, and for the trimming Llama-3 style template the raw text
too.  The tokenizer splits text with the Llama-3 / Qwen pattern, which closes
a piece at the newline run before ``Source of`` and after a turn header, so
the four separately tokenised parts spell the ids of the whole render."""
import dataclasses
import json
import os
import shutil

import pytest
import transformers

from dmcp.config import Config
from dmcp.enrich import chat
from dmcp.enrich.backend import LazyBackend, RefusedBackend, build_enrichment_prompt, create_backend
from dmcp.enrich.local import LocalEngine, _Seq, build_model
from dmcp.enrich.tokenizer import load_local_model
from dmcp.enrich.types import EnrichmentInput
from dmcp.models.llm import CheckpointUnsupported, LocalLM, check_checkpoint, preset
from tests import chat_fixtures as F

MODEL = dict(device="cpu", max_batch=4, max_rows=32, max_seq=4096)
BUDGET = 64


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("chat")
    out = {name: F.write_checkpoint(str(root / name), t) for name, t in F.TEMPLATES.items()}
    out["none"] = F.write_checkpoint(str(root / "none"), None)
    return out


@pytest.fixture(scope="module")
def loaded(ckpts):
    return {name: load_local_model(d, **MODEL) for name, d in ckpts.items()}


def _engine(loaded, name, **kw):
    model, tok = loaded[name]
    return LocalEngine(model, tokenizer=tok, use_graphs=False, **kw)


def _prompt(eng, inp, readme, budget=BUDGET):
    s = _Seq(inp, 0, [])
    return eng._prompt(s, readme, budget), s.prefix_split


def _hf_ids(d, content, template=None):
    with open(os.path.join(d, "tokenizer_config.json")) as f:
        tc = json.load(f)
    hf = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(d, "tokenizer.json"),
                                              chat_template=template or tc["chat_template"], bos_token=tc["bos_token"],
                                              eos_token=tc["eos_token"])
    out = hf.apply_chat_template([{"role": "user", "content": content}], add_generation_prompt=True,
                                 tokenize=True, enable_thinking=False)
    return list(out if isinstance(out, list) else out["input_ids"])


def _specials(tok, ids):
    return sum(i in tok.special_ids for i in ids)


# ------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", list(F.TEMPLATES))
def test_prompt_ids_equal_transformers(ckpts, loaded, name):
    """Whole prompt, and the prompt put together from the cached prefix and
    the batch-tokenised per-class part: the same ids as apply_chat_template."""
    inputs = F.inputs()[:2]
    for readme in (F.README, None):
        one = _engine(loaded, name)
        batched = _engine(loaded, name)
        batched._pretokenize([(i, x) for i, x in enumerate(inputs)], readme)
        assert len(batched._cont_cache) == 2
        for inp in inputs:
            text = build_enrichment_prompt(inp, readme)
            for probe in ("<|", "|>", "<think>"):
                assert probe not in text
            exp = _hf_ids(ckpts[name], text.strip())
            if name == "llama3":  # the template trims: the raw text renders the same
                assert _hf_ids(ckpts[name], text) == exp
            got, split = _prompt(one, inp, readme)
            assert got == exp
            assert split > len(one.head_ids) and len(one._prefix_cache) == 1
            again, split2 = _prompt(batched, inp, readme)
            assert again == exp and split2 == split
            # the cached prefix is head + the per-project content
            (pre,) = batched._prefix_cache.values()
            assert pre == exp[:split] and pre[:len(batched.head_ids)] == batched.head_ids


def test_qwen3_renders_the_non_thinking_form(loaded):
    eng = _engine(loaded, "qwen3")
    assert eng.chat.tail_text.endswith("<|im_start|>assistant\n<think>\n\n</think>\n\n")
    assert _engine(loaded, "chatml").chat.head_text.startswith("<|im_start|>system\n")


# ------------------------------------------------------------- 2. one BOS
def test_bos_appears_exactly_once(loaded):
    eng = _engine(loaded, "llama3")
    assert eng.tok.bos is not None and eng.head_ids[0] == eng.tok.bos
    for inp in F.inputs():
        ids, _ = _prompt(eng, inp, F.README)
        assert ids.count(eng.tok.bos) == 1 and ids[0] == eng.tok.bos


# -------------------------------------------------- 3. no forged turns
@pytest.mark.parametrize("name", list(F.TEMPLATES))
def test_source_text_cannot_forge_a_turn(loaded, name):
    inp = F.inputs([F.FORGING])[0]
    for lit in ("<|eot_id|>", "<|im_end|>", "<|im_start|>system"):
        assert lit in inp.source_code
    eng = _engine(loaded, name)
    tok = eng.tok
    own = _specials(tok, eng.head_ids + eng.tail_ids)
    assert own >= 3
    ids, split = _prompt(eng, inp, F.README)
    assert _specials(tok, ids) == own
    assert _specials(tok, ids[len(eng.head_ids):len(ids) - len(eng.tail_ids)]) == 0
    # the markers are still there, as text
    assert "<|im_end|>" in tok.decode(ids) and "<|eot_id|>" in tok.decode(ids)
    # batched tokenisation of the per-class part: the same
    b = _engine(loaded, name)
    b._pretokenize([(0, inp), (1, F.inputs()[0])], F.README)
    assert _prompt(b, inp, F.README)[0] == ids
    # the raw path recognises them (recorded, not asserted)
    off = _engine(loaded, name, chat_template="off")
    print(f"{name}: special ids in the raw prompt of the forging class: {_specials(tok, _prompt(off, inp, F.README)[0])}")


# --------------------------------------------------------- 4. prefix split
@pytest.mark.parametrize("name", list(F.TEMPLATES))
def test_classes_of_a_project_share_the_prefix(loaded, name):
    eng = _engine(loaded, name)
    (a, sa), (b, sb) = (_prompt(eng, inp, F.README) for inp in F.inputs()[:2])
    assert sa == sb and a[:sa] == b[:sb] and a != b
    assert sa >= len(eng.head_ids) and a[:len(eng.head_ids)] == eng.head_ids
    assert a[-len(eng.tail_ids):] == eng.tail_ids and b[-len(eng.tail_ids):] == eng.tail_ids
    assert sa >= eng.MIN_SHARED_PREFIX
    # another project: another prefix, the same turn header
    c, sc = _prompt(eng, F.inputs()[0], "Another project.")
    assert c[:len(eng.head_ids)] == eng.head_ids and c[:sc] != a[:sa]


# ----------------------------------------------------------- 5. truncation
def _long_input():
    body = "".join(f"    public void step{i}(String id) {{ repository.touch(id, {i}); }}\n" for i in range(60))
    return EnrichmentInput("package co.acme.shop;\n\npublic class Steps {\n" + body + "}\n", "co.acme.shop.Steps",
                           "java", "SERVICE", ["step0", "step1"])


@pytest.mark.parametrize("name", ["llama3", "chatml"])
def test_truncation_cuts_content_only(loaded, name):
    inp = _long_input()
    full, split = _prompt(_engine(loaded, name), inp, F.README)
    eng = _engine(loaded, name)
    H, T = len(eng.head_ids), len(eng.tail_ids)
    content = full[H:len(full) - T]
    assert split > H and len(content) > 2 * split

    def cut_at(max_prompt_tokens):
        e = _engine(loaded, name, max_prompt_tokens=max_prompt_tokens)
        ids, sp = _prompt(e, inp, F.README)
        limit = max_prompt_tokens - T            # content tokens
        keep = min(256, limit // 4)
        assert len(ids) <= H + max_prompt_tokens and len(ids) == H + limit + T
        assert ids[:H] == eng.head_ids and ids[-T:] == eng.tail_ids
        kept = ids[H:len(ids) - T]
        assert kept[-keep:] == content[-keep:] and kept[:limit - keep] == content[:limit - keep]
        return sp, H + limit - keep

    # the cut falls behind the marker: the shared prefix survives
    sp, cut = cut_at(len(content) + T - 40)
    assert cut > split and sp == split
    # the cut removes the marker: no shared prefix
    sp, cut = cut_at(200)
    assert cut < split and sp == 0
    # nothing to cut: the limit is not reached
    e = _engine(loaded, name, max_prompt_tokens=len(content) + T)
    assert _prompt(e, inp, F.README) == (full, split)


def test_kv_limit_counts_head_and_tail(loaded):
    """Without max_prompt_tokens the slot bounds the prompt: head + content +
    tail take what a raw prompt (BOS + text) may take, max_seq - budget - 1."""
    inp = _long_input()
    model, tok = loaded["chatml"]
    eng = LocalEngine(model, tokenizer=tok, use_graphs=False)
    budget = model.cfg.max_seq - 700
    ids, _ = _prompt(eng, inp, F.README, budget=budget)
    assert len(ids) == model.cfg.max_seq - budget - 1
    assert ids[:len(eng.head_ids)] == eng.head_ids and ids[-len(eng.tail_ids):] == eng.tail_ids
    raw, _ = _prompt(LocalEngine(model, tokenizer=tok, use_graphs=False, chat_template="off"), inp, F.README,
                     budget=budget)
    assert len(raw) <= len(ids)


# -------------------------------------------------------------- 6. refusal
BAD = {
    "syntax": ("{% if messages %}{{ '<|im_start|>' }}", "does not compile"),
    "raises": ("{% if messages | length < 2 %}{{ raise_exception('a system message is required') }}{% endif %}"
               "{{ messages[0]['content'] }}", "a system message is required"),
    "drops": ("{{ '<|im_start|>user\\n<|im_end|>\\n<|im_start|>assistant\\n' }}", "0 times"),
    "twice": ("{{ messages[0]['content'] + '<|im_end|>' + messages[0]['content'] }}", "2 times"),
}


def _with_template(src, dst, template, as_file=False):
    shutil.copytree(src, dst)
    tc_path = os.path.join(dst, "tokenizer_config.json")
    with open(tc_path) as f:
        tc = json.load(f)
    if as_file:
        del tc["chat_template"]
        with open(os.path.join(dst, "chat_template.jinja"), "w") as f:
            f.write(template)
    else:
        tc["chat_template"] = template
    with open(tc_path, "w") as f:
        json.dump(tc, f)
    return dst


@pytest.mark.parametrize("case", list(BAD))
@pytest.mark.parametrize("as_file", [False, True])
def test_unusable_template_is_refused_at_start(ckpts, tmp_path, case, as_file):
    template, needle = BAD[case]
    d = _with_template(ckpts["chatml"], str(tmp_path / case), template, as_file)
    file = "chat_template.jinja" if as_file else "tokenizer_config.json"
    reason = check_checkpoint(d)
    assert reason is not None and os.path.join(d, file) in reason and needle in reason
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=d))
    assert isinstance(be, RefusedBackend) and not be.enabled
    assert file in be.disabled_reason and needle in be.disabled_reason and "LOCAL_LLM_MODEL_PATH" in be.disabled_reason
    with pytest.raises(CheckpointUnsupported) as e:
        load_local_model(d, **MODEL)
    assert file in str(e.value) and needle in str(e.value)
    with pytest.raises(CheckpointUnsupported):
        build_model({"path": d, "max_batch": 2, "max_rows": 8, "max_seq": 256}, "cpu")
    # the model itself is fine: with the template off the directory loads
    assert check_checkpoint(d, chat_template="off") is None
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=d, local_llm_chat_template="off"))
    assert isinstance(be, LazyBackend)
    LocalLM.load_safetensors(d, device="cpu", max_batch=1, max_rows=1, max_seq=64)


def test_template_sources_in_order(ckpts, tmp_path):
    """tokenizer_config.json (a string, or the entry named default of a
    list) before chat_template.jinja; neither: no template."""
    d = _with_template(ckpts["chatml"], str(tmp_path / "both"), F.CHATML)
    with open(os.path.join(d, "chat_template.jinja"), "w") as f:
        f.write(F.QWEN3)
    assert chat.find_template(d) == (F.CHATML, os.path.join(d, "tokenizer_config.json"))
    with open(os.path.join(d, "tokenizer_config.json")) as f:
        tc = json.load(f)
    tc["chat_template"] = [{"name": "tool_use", "template": "x"}, {"name": "default", "template": F.LLAMA3}]
    tc["bos_token"] = {"content": "<|begin_of_text|>", "lstrip": False}
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(tc, f)
    assert chat.find_template(d)[0] == F.LLAMA3
    assert chat.load_chat_template(d).head_text.startswith("<|begin_of_text|><|start_header_id|>user")
    del tc["chat_template"]
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(tc, f)
    assert chat.find_template(d) == (F.QWEN3, os.path.join(d, "chat_template.jinja"))
    assert chat.find_template(ckpts["none"]) is None and check_checkpoint(ckpts["none"]) is None


def test_strftime_now_is_one_timestamp_per_engine(ckpts):
    import datetime
    now = datetime.datetime(2031, 5, 6, 7, 8, 9)
    t = chat.render_split("{{ strftime_now('%Y-%m-%d %H:%M:%S') }}|{{ messages[0]['content'] }}|"
                          "{{ strftime_now('%S') }}{{ {'a': '<b>'} | tojson }}", "t.jinja", now=now)
    assert t.head_text == "2031-05-06 07:08:09|" and t.tail_text == '|09{"a": "<b>"}'


# ----------------------------------------------------------------- 7. knob
def test_knob_off_auto_and_path(ckpts, loaded, tmp_path):
    inp = F.inputs()[0]
    off = _engine(loaded, "llama3", chat_template="off")
    assert off.chat_mode == "raw" and off.chat is None and off.head_ids == []
    # today's ids: BOS + the two separately encoded halves of the raw text
    text = build_enrichment_prompt(inp, F.README)
    exp, exp_split = off.tok.encode_split(text, "Source of ")
    assert exp[0] == off.tok.bos and _prompt(off, inp, F.README) == (exp, exp_split)
    auto = _engine(loaded, "llama3")
    assert auto.chat_mode == "template:" + os.path.join(ckpts["llama3"], "tokenizer_config.json")
    # a directory without a template: auto is the raw path
    none = _engine(loaded, "none")
    assert none.chat_mode == "raw"
    assert _prompt(none, inp, F.README) == none.tok.encode_split(text, "Source of ")
    # a path overrides the directory's template (the BOS / EOS texts stay the directory's)
    path = str(tmp_path / "other.jinja")
    with open(path, "w") as f:
        f.write(F.QWEN3)
    over = _engine(loaded, "chatml", chat_template=path)
    assert over.chat_mode == "template:" + path
    assert over.chat.tail_text.endswith("</think>\n\n") and over.head_ids != _engine(loaded, "chatml").head_ids
    assert _prompt(over, inp, F.README)[0] == _hf_ids(ckpts["chatml"], text.strip(), F.QWEN3)
    # ... also for a directory that has none (its tokenizer spells the markers as text)
    assert _engine(loaded, "none", chat_template=path).chat_mode == "template:" + path


def test_knob_errors_name_the_variable(loaded, tmp_path):
    with pytest.raises(ValueError, match="LOCAL_LLM_CHAT_TEMPLATE"):
        _engine(loaded, "llama3", chat_template=str(tmp_path / "missing.jinja"))
    path = str(tmp_path / "t.jinja")
    with open(path, "w") as f:
        f.write(F.CHATML)
    tiny = LocalLM(preset("tiny", max_batch=2, max_rows=16, max_seq=512), device="cpu", seed=0)
    with pytest.raises(ValueError, match="LOCAL_LLM_CHAT_TEMPLATE"):
        LocalEngine(tiny, use_graphs=False, chat_template=path)  # the byte-level vocabulary


def test_presets_are_unchanged_by_auto(tmp_path):
    tiny = LocalLM(preset("tiny", max_batch=2, max_rows=16, max_seq=2048), device="cpu", seed=0)
    inp = F.inputs()[0]
    auto, off = (LocalEngine(tiny, use_graphs=False, chat_template=m) for m in ("auto", "off"))
    assert auto.chat_mode == off.chat_mode == "raw"
    text = build_enrichment_prompt(inp, F.README)
    exp = auto.tok.encode_split(text, "Source of ")
    assert _prompt(auto, inp, F.README) == exp == _prompt(off, inp, F.README)
    assert auto.generate([inp], F.README) == off.generate([inp], F.README)
    m2, t2 = build_model({"preset": "tiny", "max_batch": 2, "max_rows": 16, "chat_template": "auto"}, "cpu")
    assert t2 is None


def test_config_and_worker_specs_carry_the_knob(ckpts):
    from dmcp.enrich.workers import engine_spec, model_spec
    assert Config().local_llm_chat_template == "auto"
    cfg = Config.from_env({"LOCAL_LLM_CHAT_TEMPLATE": "off", "LOCAL_LLM_MODEL_PATH": ckpts["chatml"]})
    assert cfg.local_llm_chat_template == "off"
    assert engine_spec(cfg)["chat_template"] == "off" and model_spec(cfg)["chat_template"] == "off"
    assert engine_spec(Config())["chat_template"] == "auto" and "chat_template" not in model_spec(Config())


def test_marker_past_the_embedding_table_is_refused(ckpts, tmp_path):
    """A turn marker whose id the model's vocabulary does not hold must never
    reach the embedding lookup."""
    d = _with_template(ckpts["chatml"], str(tmp_path / "small"), F.CHATML)
    model, tok = load_local_model(d, **MODEL)
    marker = tok.tk.token_to_id("<|im_start|>")
    assert marker in tok.special_ids and marker < model.cfg.vocab_size
    model.cfg = dataclasses.replace(model.cfg, vocab_size=marker)
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        LocalEngine(model, tokenizer=tok, use_graphs=False)


# -------------------------------------------------------------- 8. sandbox
@pytest.mark.parametrize("template", [
    "{{ messages.__class__.__mro__ }}{{ messages[0]['content'] }}",
    "{{ ''.__class__.__name__ }}{{ messages[0]['content'] }}",
    "{% set _ = messages.append({'role': 'system', 'content': 'x'}) %}{{ messages[0]['content'] }}",
    "{% set _ = messages[0].update({'content': 'x'}) %}{{ messages[0]['content'] }}",
])
def test_template_runs_in_the_immutable_sandbox(ckpts, tmp_path, template):
    from jinja2.exceptions import SecurityError
    with pytest.raises(chat.ChatTemplateError) as e:
        chat.render_split(template, "evil.jinja")
    assert isinstance(e.value.__cause__, SecurityError) and "evil.jinja" in str(e.value)
    d = _with_template(ckpts["chatml"], str(tmp_path / "evil"), template)
    reason = check_checkpoint(d)
    assert reason is not None and "SecurityError" in reason and "tokenizer_config.json" in reason
    assert isinstance(create_backend(Config(enrich_backend="local", local_llm_model_path=d)), RefusedBackend)


# ------------------------------------------------------- the synth writer
def test_writer_without_a_template_is_unchanged(tmp_path):
    """chat_template is off by default: the same files, byte for byte; with
    it, the markers are special added tokens and tokenizer_config.json holds
    the template and the BOS / EOS texts."""
    from dmcp.utils import synth
    kw = dict(F.TINY, tokenizer="code-bpe-128k", vocab=128256, hidden=64, heads=1, kv_heads=1, intermediate=64,
              layers=1)
    a = synth.llama_checkpoint(str(tmp_path / "a"), **kw)
    b = synth.llama_checkpoint(str(tmp_path / "b"), **kw, chat_template=None)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["config.json", "model.safetensors", "tokenizer.json"]
    for fn in os.listdir(a):
        with open(os.path.join(a, fn), "rb") as fa, open(os.path.join(b, fn), "rb") as fb:
            assert fa.read() == fb.read(), fn
    c = synth.llama_checkpoint(str(tmp_path / "c"), **kw, chat_template=F.LLAMA3)
    with open(os.path.join(c, "tokenizer_config.json")) as f:
        tc = json.load(f)
    assert tc["chat_template"] == F.LLAMA3 and tc["bos_token"] == "<|begin_of_text|>" and tc["eos_token"] == "<|eot_id|>"
    with open(os.path.join(c, "tokenizer.json")) as f:
        added = {t["content"]: t for t in json.load(f)["added_tokens"]}
    for m in ("<|start_header_id|>", "<|end_header_id|>", "<|eot_id|>"):
        assert added[m]["special"] is True and 128002 <= added[m]["id"] < 128256
    with open(os.path.join(a, "model.safetensors"), "rb") as fa, open(os.path.join(c, "model.safetensors"), "rb") as fc:
        assert fa.read() == fc.read()
    t = chat.load_chat_template(c)
    assert t.head_text == "<|begin_of_text|><|start_header_id|>user<|end_header_id|>\n\n"
