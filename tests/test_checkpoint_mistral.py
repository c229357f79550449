"""Mistral checkpoints, and Qwen2 ones with their sliding window switched on,
load as the models they are: the window resolution rules of
``dmcp.models.llm.checkpoint_windows`` and fp32 parity with ``transformers``.

Parity follows tests/test_checkpoint_fidelity.py's scheme: last-position
logits of ``LocalLM.reference_logits`` against the fp32 HF model loaded from
the same written directory; error = (1 - cosine, max |diff| / max |logit|),
the worst over the prompts; the plain-Llama checkpoint of the same geometry
is measured first and a windowed case may show at most 2x its error (the
window is a mask: no new arithmetic).  The same checkpoint evaluated with its
windows forced to None -- what a loader without the feature computes -- must
exceed 100x that baseline.  Prompts are 64 tokens, the window 16."""
import json
import os
import shutil

import pytest
import torch

transformers = pytest.importorskip("transformers")

from dmcp.models.llm import (CheckpointUnsupported, LocalLM, check_checkpoint, checkpoint_windows,  # noqa: E402
                             resolve_windows, windows_label)
from dmcp.utils import synth  # noqa: E402
from tests.test_checkpoint_fidelity import TINY, _edit_config, _rewrite, _unit_norms  # noqa: E402

WINDOW, PROMPT = 16, 64
CASES = {"mistral": dict(model_type="mistral", sliding_window=WINDOW),
         "qwen2_all": dict(model_type="qwen2", qkv_bias=True, sliding_window=WINDOW, max_window_layers=0),
         "qwen2_upper": dict(model_type="qwen2", qkv_bias=True, sliding_window=WINDOW, max_window_layers=1)}
EXPECT = {"mistral": (WINDOW, WINDOW), "qwen2_all": (WINDOW, WINDOW), "qwen2_upper": (0, WINDOW)}


def _write(root, name, **kw):
    d = synth.llama_checkpoint(os.path.join(str(root), name), **{**TINY, **kw})
    _rewrite(d, _unit_norms)
    return d


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("mistral")
    out = {name: _write(root, name, **kw) for name, kw in CASES.items()}
    out["plain"] = _write(root, "plain")
    return out


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (PROMPT,), generator=g).tolist() for _ in range(4)]


def _hf(path):
    mt = json.load(open(os.path.join(path, "config.json"))).get("model_type")
    cls = {"mistral": transformers.MistralForCausalLM, "qwen2": transformers.Qwen2ForCausalLM}.get(
        mt, transformers.LlamaForCausalLM)
    return cls.from_pretrained(path, dtype=torch.float32, attn_implementation="eager").eval()


def _errors(path, prompts, force_full=False):
    over = dict(layer_windows=None) if force_full else {}
    m = LocalLM.load_safetensors(path, device="cpu", max_seq=256, max_batch=1, max_rows=1, **over)
    hf = _hf(path)
    e_cos = e_abs = 0.0
    with torch.no_grad():
        for p in prompts:
            for start in (0, 100):
                pos = torch.arange(start, start + len(p))[None]
                exp = hf(input_ids=torch.tensor([p]), position_ids=pos).logits[0, -1].double()
                got = m.reference_logits(p, start_pos=start)[-1].double()
                e_cos = max(e_cos, 1.0 - torch.nn.functional.cosine_similarity(got, exp, dim=0).item())
                e_abs = max(e_abs, ((got - exp).abs().max() / exp.abs().max()).item())
    return e_cos, e_abs


@pytest.fixture(scope="module")
def baseline(ckpts, prompts):
    b = _errors(ckpts["plain"], prompts)
    print(f"baseline plain: 1-cos {b[0]:.3e}  maxabs/max {b[1]:.3e}")
    assert b[0] < 1e-6 and b[1] < 1e-3, b
    return b


@pytest.mark.parametrize("case", list(CASES))
def test_windowed_model_parity_with_transformers(ckpts, prompts, baseline, case):
    d = ckpts[case]
    assert check_checkpoint(d) is None
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=256, max_batch=1, max_rows=1)
    assert m.cfg.layer_windows == EXPECT[case] and m.windows == EXPECT[case]
    e = _errors(d, prompts)
    print(f"{case}: 1-cos {e[0]:.3e} ({e[0] / baseline[0]:.2f}x)  maxabs/max {e[1]:.3e} ({e[1] / baseline[1]:.2f}x)")
    assert e[0] <= 2 * baseline[0] and e[1] <= 2 * baseline[1], (case, e, baseline)


@pytest.mark.parametrize("case", list(CASES))
def test_without_its_windows_the_model_misses_the_gate(ckpts, prompts, baseline, case):
    """What the loader computed before windows existed: attention to every key."""
    s = _errors(ckpts[case], prompts, force_full=True)
    print(f"{case} full attention: 1-cos {s[0]:.3e} ({s[0] / baseline[0]:.1f}x)  maxabs/max {s[1]:.3e} "
          f"({s[1] / baseline[1]:.1f}x)")
    assert s[0] > 100 * baseline[0] and s[1] > 100 * baseline[1], (case, s, baseline)


def test_forward_paths_follow_the_reference(ckpts, prompts):
    """prefill_batch, forward_tokens and decode of the windowed model on the
    CPU (the fp32 reference ops over a bf16 cache) against reference_logits."""
    m = LocalLM.load_safetensors(ckpts["mistral"], device="cpu", max_seq=256, max_batch=2, max_rows=2)
    p = prompts[0]
    ref = m.reference_logits(p)
    a = m.prefill_batch([(p[:40], 0, 0), (p[:33], 1, 0)])[0].float()
    b = m.forward_tokens(torch.tensor(p[40:50], dtype=torch.int32), 0, 40).float()
    cos = torch.nn.functional.cosine_similarity
    assert cos(a, ref[39], dim=0) > 0.999 and cos(b, ref[49], dim=0) > 0.999
    for t in range(50, 54):
        out = m.decode(torch.tensor([p[t]], dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                       torch.tensor([t], dtype=torch.int32))[0].float()
        assert cos(out, ref[t], dim=0) > 0.999, t


BASE2 = dict(num_hidden_layers=2)
ACCEPT = {
    "mistral": (dict(model_type="mistral", architectures=["MistralForCausalLM"], sliding_window=16), (16, 16)),
    "mistral_no_archs": (dict(model_type="mistral", architectures=None, sliding_window=16), (16, 16)),
    "mistral_null_window": (dict(model_type="mistral", architectures=["MistralForCausalLM"]), None),
    "mistral_layer_types": (dict(model_type="mistral", architectures=["MistralForCausalLM"], sliding_window=8,
                                 layer_types=["sliding_attention", "full_attention"]), (8, 0)),
    "qwen2_off": (dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"], use_sliding_window=False,
                       sliding_window=16, max_window_layers=0), None),
    "qwen2_on": (dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"], use_sliding_window=True,
                      sliding_window=16, max_window_layers=1), (0, 16)),
    "qwen2_on_none_left": (dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"], use_sliding_window=True,
                                sliding_window=16, max_window_layers=2), None),
    "layer_types_decide": (dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"], use_sliding_window=True,
                                sliding_window=16, max_window_layers=0,
                                layer_types=["full_attention", "sliding_attention"]), (0, 16)),
    "layer_types_full": (dict(layer_types=["full_attention", "full_attention"]), None),
}
REFUSE = {
    "mistral_llama_arch": (dict(model_type="mistral"), "model_type"),
    "mistral_arch_alone": (dict(architectures=["MistralForCausalLM"]), "architectures"),
    "mistral_two_archs": (dict(model_type="mistral", architectures=["MistralForCausalLM", "LlamaForCausalLM"]),
                          "architectures"),
    "mistral_bad_window": (dict(model_type="mistral", architectures=["MistralForCausalLM"], sliding_window=-4),
                           "sliding_window"),
    "switch_without_window": (dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"],
                                   use_sliding_window=True), "use_sliding_window"),
    "switch_on_llama": (dict(use_sliding_window=True, sliding_window=16), "use_sliding_window"),
    "sliding_without_window": (dict(layer_types=["full_attention", "sliding_attention"]), "layer_types"),
    "other_layer_type": (dict(layer_types=["full_attention", "chunked_attention"], sliding_window=16),
                         "layer_types"),
    "layer_types_length": (dict(layer_types=["sliding_attention"], sliding_window=16), "layer_types"),
}


@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("rules") / "base"), **TINY)


@pytest.mark.parametrize("name", list(ACCEPT))
def test_window_resolution_accepts(base_ckpt, tmp_path, name):
    edit, want = ACCEPT[name]
    d = shutil.copytree(base_ckpt, str(tmp_path / "ck"))
    _edit_config(d, **edit)
    assert check_checkpoint(d) is None
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.cfg.layer_windows == want and m.windows == want


@pytest.mark.parametrize("name", list(REFUSE))
def test_window_resolution_refuses_with_the_key(base_ckpt, tmp_path, name):
    edit, needle = REFUSE[name]
    d = shutil.copytree(base_ckpt, str(tmp_path / "ck"))
    _edit_config(d, **edit)
    reason = check_checkpoint(d)
    assert reason is not None and needle in reason, reason
    with pytest.raises(CheckpointUnsupported, match=needle):
        LocalLM.load_safetensors(d, device="cpu")


def test_a_window_no_sequence_can_outgrow_is_full_attention(base_ckpt, tmp_path):
    d = shutil.copytree(base_ckpt, str(tmp_path / "ck"))
    _edit_config(d, model_type="mistral", architectures=["MistralForCausalLM"], sliding_window=4096)
    assert checkpoint_windows(json.load(open(os.path.join(d, "config.json"))))[0] == (4096, 4096)
    assert LocalLM.load_safetensors(d, device="cpu", max_seq=4096, max_batch=1, max_rows=1).windows is None
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=4097, max_batch=1, max_rows=1)
    assert m.windows == (4096, 4096)
    assert resolve_windows((4096, 0, 100), 200) == (0, 0, 100) and resolve_windows((4096,), 200) is None


def test_witness_and_labels(ckpts):
    from dmcp.enrich import workers
    assert windows_label((4096,) * 4) == "4096@all" and windows_label((0, 0, 7, 7)) == "7@2.."
    assert windows_label((5, 0, 5, 0)) == "5@0,2" and windows_label(None) == "none"
    m = LocalLM.load_safetensors(ckpts["qwen2_upper"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert workers._witness("cpu", m) == {"device": "cpu", "kv_dtype": "bf16", "window": "16@1.."}
    m = LocalLM.load_safetensors(ckpts["mistral"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert workers._witness("cpu", m)["window"] == "16@all"
    plain = LocalLM.load_safetensors(ckpts["plain"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert "window" not in workers._witness("cpu", plain)


def test_synth_default_config_is_unchanged(tmp_path):
    a = synth.llama_checkpoint(str(tmp_path / "a"), **TINY)
    cfg = json.load(open(os.path.join(a, "config.json")))
    assert "sliding_window" not in cfg and "model_type" not in cfg and cfg["architectures"] == ["LlamaForCausalLM"]
    with pytest.raises(ValueError, match="sliding_window"):
        synth.llama_checkpoint(str(tmp_path / "b"), **TINY, sliding_window=8)
    for knob in ("prefill_dtype", "decode_dtype"):  # the MXFP8 knobs of a mistral checkpoint behave as for llama
        m = synth.llama_checkpoint(str(tmp_path / knob), **TINY, model_type="mistral", sliding_window=8)
        got = [LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1, **{knob: "fp8"})
               for d in (a, m)]
        assert (got[0].prefill_fp8, got[0].decode_fp8) == (got[1].prefill_fp8, got[1].decode_fp8)
        assert got[1].prefill_fp8 == (knob == "prefill_dtype") and got[1].decode_fp8 == (knob == "decode_dtype")
        assert got[1].windows == (8, 8) and got[0].windows is None
