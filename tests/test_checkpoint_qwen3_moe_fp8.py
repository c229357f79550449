"""Block-scaled FP8 Qwen3 checkpoints (``quantization_config.quant_method:
"fp8"``, ``weight_block_size: [128, 128]``): what check_checkpoint accepts and
refuses -- per tensor, from the safetensors headers -- and what the loader makes
of them: experts kept in e4m3 beside their block scales (``moe_weight_dtype``
"fp8b"), every other F8 projection dequantised to bf16, and CPU logits that
match the fp32 reference forward over the dequantised weights to the tolerance
tests/test_checkpoint_qwen3_moe.py uses for its bf16 checkpoint."""
import json
import os
import shutil

import pytest
import torch

from dmcp.config import Config
from dmcp.enrich.backend import LazyBackend, RefusedBackend, create_backend
from dmcp.models.llm import CheckpointUnsupported, LocalLM, check_checkpoint
from dmcp.ops import reference
from dmcp.utils import synth

# hidden 320 / expert width 192: partial scale blocks on both axes (320 = 2.5 blocks, 192 = 1.5)
TINY = dict(layers=2, hidden=320, heads=4, kv_heads=2, head_dim=64, intermediate=512, vocab=512, tokenizer="",
            outliers=(), device="cpu", n_experts=8, experts_per_tok=2, moe_intermediate=192)
H, I, E = 320, 192, 8


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("qwen3moe_fp8"))
    return {"fp8": synth.qwen3_moe_checkpoint(os.path.join(root, "fp8"), fp8=True, **TINY),
            "bf16": synth.qwen3_moe_checkpoint(os.path.join(root, "bf16"), **TINY),
            "dense_bf16": synth.llama_checkpoint(os.path.join(root, "dense"), qk_norm=True, model_type="qwen3",
                                                 **{k: v for k, v in TINY.items()
                                                    if k not in ("n_experts", "experts_per_tok", "moe_intermediate")})}


def _rewrite(path, fn):
    from safetensors.torch import load_file, save_file
    f = os.path.join(path, "model.safetensors")
    t = load_file(f)
    fn(t)
    save_file(t, f)


def _edit_quant(path, **kv):
    """Edits ``quantization_config`` (a value None removes the key; ``_drop``: the whole object)."""
    f = os.path.join(path, "config.json")
    with open(f) as fh:
        cfg = json.load(fh)
    if kv.pop("_drop", False):
        cfg.pop("quantization_config")
    for k, v in kv.items():
        if v is None:
            cfg["quantization_config"].pop(k, None)
        else:
            cfg["quantization_config"][k] = v
    with open(f, "w") as fh:
        json.dump(cfg, fh)


def _load(d, **kw):
    return LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=2, max_rows=2, **kw)


# ------------------------------------------------------------------ accepted
def test_the_synth_fp8_checkpoint_is_accepted(ckpts):
    assert check_checkpoint(ckpts["fp8"]) is None
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=ckpts["fp8"]))
    assert isinstance(be, LazyBackend) and be.enabled and not be.built


def test_the_synth_fp8_layout(ckpts):
    """What ``fp8=True`` writes: F8_E4M3 experts and attention projections with
    ceil-divided fp32 scales, everything else bf16, quantization_config -- and
    without it the files of before, byte for byte."""
    from safetensors import safe_open
    with safe_open(os.path.join(ckpts["fp8"], "model.safetensors"), framework="pt") as f:
        heads = {k: (str(f.get_slice(k).get_dtype()), tuple(f.get_slice(k).get_shape())) for k in f.keys()}
    p = "model.layers.1."
    assert heads[p + "mlp.experts.3.gate_proj.weight"] == ("F8_E4M3", (I, H))
    assert heads[p + "mlp.experts.3.gate_proj.weight_scale_inv"] == ("F32", (2, 3))
    assert heads[p + "mlp.experts.3.down_proj.weight_scale_inv"] == ("F32", (3, 2))
    assert heads[p + "self_attn.q_proj.weight"][0] == "F8_E4M3"
    assert heads[p + "self_attn.k_proj.weight_scale_inv"] == ("F32", (1, 3))
    for n in ("model.embed_tokens.weight", "lm_head.weight", "model.norm.weight", p + "mlp.gate.weight",
              p + "input_layernorm.weight", p + "self_attn.q_norm.weight"):
        assert heads[n][0] == "BF16" and n + "_scale_inv" not in heads, n
    with open(os.path.join(ckpts["fp8"], "config.json")) as f:
        qc = json.load(f)["quantization_config"]
    assert qc == {"quant_method": "fp8", "fmt": "e4m3", "activation_scheme": "dynamic", "weight_block_size": [128, 128]}
    with open(os.path.join(ckpts["bf16"], "config.json")) as f:
        assert "quantization_config" not in json.load(f)
    assert not any(v[0].startswith("F8") for v in _heads(ckpts["bf16"]).values())


def _heads(d):
    from safetensors import safe_open
    with safe_open(os.path.join(d, "model.safetensors"), framework="pt") as f:
        return {k: (str(f.get_slice(k).get_dtype()), tuple(f.get_slice(k).get_shape())) for k in f.keys()}


def test_fmt_may_be_absent_and_a_dense_fp8_checkpoint_is_accepted(ckpts, tmp_path):
    d = shutil.copytree(ckpts["fp8"], str(tmp_path / "nofmt"))
    _edit_quant(d, fmt=None, activation_scheme=None, modules_to_not_convert=["lm_head"])
    assert check_checkpoint(d) is None
    # a non-MoE FP8 checkpoint (Qwen3-8B-FP8's layout): attention and dense-MLP projections quantised
    dense = shutil.copytree(ckpts["dense_bf16"], str(tmp_path / "dense"))

    def quantise(t):
        for n in [n for n in t if n.endswith("_proj.weight")]:
            t[n], t[n + "_scale_inv"] = reference.block_fp8_quant(t[n])
    _rewrite(dense, quantise)
    with open(os.path.join(dense, "config.json")) as f:
        cfg = json.load(f)
    cfg["quantization_config"] = {"quant_method": "fp8", "weight_block_size": [128, 128]}
    with open(os.path.join(dense, "config.json"), "w") as f:
        json.dump(cfg, f)
    assert check_checkpoint(dense) is None
    m = _load(dense)
    assert not m.moe and m.cfg.moe_weight_dtype == "bf16"
    assert all(v.dtype == torch.bfloat16 for v in m.w.values())
    from safetensors.torch import load_file
    raw = load_file(os.path.join(dense, "model.safetensors"))
    p = "model.layers.1.mlp."
    exp = torch.cat([reference.block_fp8_dequant(raw[p + n + ".weight"], raw[p + n + ".weight_scale_inv"],
                                                 torch.bfloat16) for n in ("gate_proj", "up_proj")], 0)
    g = m.norm_g["l1.ln2"].float()  # the loader folds the norm weight into the matrix that reads the normalised row
    assert torch.equal(m.w["l1.wgu"], (exp.float() * g[None, :]).to(torch.bfloat16))


# ------------------------------------------------------------------- refused
P1 = "model.layers.1."
X = P1 + "mlp.experts.2.up_proj.weight"


def _set(name, value):
    return lambda t: t.__setitem__(name, value)


REFUSALS = {
    "gptq": (dict(quant_method="gptq"), None, "quant_method"),
    "awq": (dict(quant_method="awq"), None, "quant_method"),
    "compressed_tensors": (dict(quant_method="compressed-tensors"), None, "quant_method"),
    "fmt_e5m2": (dict(fmt="e5m2"), None, "fmt"),
    "no_block_size": (dict(weight_block_size=None), None, "weight_block_size"),
    "other_block_size": (dict(weight_block_size=[64, 64]), None, "weight_block_size"),
    "static_activations": (dict(activation_scheme="static"), None, "activation_scheme"),
    "f8_without_config": (dict(_drop=True), None, "quantization_config"),
    "per_tensor_weight_scale": ({}, _set(X[:-len("weight")] + "weight_scale", torch.ones(1)), "weight_scale"),
    "per_tensor_input_scale": ({}, _set(X[:-len("weight")] + "input_scale", torch.ones(1)), "input_scale"),
    "scale_missing": ({}, lambda t: t.pop(X + "_scale_inv"), X + "_scale_inv"),
    "scale_without_f8": ({}, _set(X, torch.ones(I, H, dtype=torch.bfloat16)), X + "_scale_inv"),
    "scale_of_a_norm": ({}, _set(P1 + "input_layernorm.weight_scale_inv", torch.ones(3)),
                        P1 + "input_layernorm.weight_scale_inv"),
    "scale_shape": ({}, _set(X + "_scale_inv", torch.ones(2, 2)), X + "_scale_inv"),
    "scale_shape_floor": ({}, _set(P1 + "self_attn.o_proj.weight_scale_inv", torch.ones(2, 2)),
                          P1 + "self_attn.o_proj.weight_scale_inv"),
    "scale_dtype": ({}, _set(X + "_scale_inv", torch.ones(2, 3, dtype=torch.bfloat16)), X + "_scale_inv"),
    "f8_router": ({}, _set(P1 + "mlp.gate.weight", torch.ones(E, H).to(torch.float8_e4m3fn)), P1 + "mlp.gate.weight"),
    "f8_embedding": ({}, _set("model.embed_tokens.weight", torch.ones(512, H).to(torch.float8_e4m3fn)),
                     "model.embed_tokens.weight"),
    "f8_lm_head": ({}, _set("lm_head.weight", torch.ones(512, H).to(torch.float8_e4m3fn)), "lm_head.weight"),
    "f8_norm": ({}, _set(P1 + "input_layernorm.weight", torch.ones(H).to(torch.float8_e4m3fn)),
                P1 + "input_layernorm.weight"),
    "e5m2_tensor": ({}, _set(X, torch.ones(I, H).to(torch.float8_e5m2)), X),
    "mixed_experts": ({}, lambda t: (t.__setitem__(X, torch.ones(I, H, dtype=torch.bfloat16)),
                                     t.pop(X + "_scale_inv")), X),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_what_cannot_be_reproduced_is_refused_with_the_key(ckpts, tmp_path, name):
    cfg_edit, tensor_edit, needle = REFUSALS[name]
    d = shutil.copytree(ckpts["fp8"], str(tmp_path / "ck"))
    if cfg_edit:
        _edit_quant(d, **cfg_edit)
    if tensor_edit:
        _rewrite(d, tensor_edit)
    reason = check_checkpoint(d)
    assert reason is not None and needle in reason, reason
    with pytest.raises(CheckpointUnsupported) as e:
        LocalLM.load_safetensors(d, device="cpu")
    assert needle in str(e.value)
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=d))
    assert isinstance(be, RefusedBackend) and not be.enabled and needle in be.disabled_reason


def test_no_tensor_data_is_read(ckpts, monkeypatch):
    """check_checkpoint decides from config.json and the headers alone."""
    import safetensors
    real = safetensors.safe_open

    class Guard:
        def __init__(self, *a, **k):
            self._f = real(*a, **k)

        def __enter__(self):
            self._h = self._f.__enter__()
            return self

        def __exit__(self, *exc):
            return self._f.__exit__(*exc)

        def keys(self):
            return self._h.keys()

        def get_slice(self, k):
            sl = self._h.get_slice(k)

            class Header:
                get_shape, get_dtype = sl.get_shape, sl.get_dtype
            return Header()

        def get_tensor(self, k):
            raise AssertionError(f"check_checkpoint read the data of {k}")
    monkeypatch.setattr(safetensors, "safe_open", Guard)
    assert check_checkpoint(ckpts["fp8"], chat_template=None) is None


# -------------------------------------------------------------------- loaded
def test_a_cpu_load_keeps_the_experts_in_e4m3(ckpts):
    from safetensors.torch import load_file
    m = _load(ckpts["fp8"])
    raw = load_file(os.path.join(ckpts["fp8"], "model.safetensors"))
    assert m.moe and m.moe_w8 and m.cfg.moe_weight_dtype == "fp8b"
    for i in range(2):
        p = f"model.layers.{i}."
        gu8, gu_s, d8, d_s = (m.w[f"l{i}.{n}"] for n in ("we_gu8", "we_gu_s", "we_down8", "we_down_s"))
        assert f"l{i}.we_gu" not in m.w and f"l{i}.we_down" not in m.w
        assert gu8.dtype == d8.dtype == torch.float8_e4m3fn and gu_s.dtype == d_s.dtype == torch.float32
        assert tuple(gu8.shape) == (E, 2 * I, H) and tuple(gu_s.shape) == (E, 4, 3)
        assert tuple(d8.shape) == (E, H, I) and tuple(d_s.shape) == (E, 3, 2)
        assert all(t.is_contiguous() for t in (gu8, gu_s, d8, d_s))
        for e in (0, 3, 7):
            q = f"{p}mlp.experts.{e}."
            assert torch.equal(gu8[e, :I].view(torch.uint8), raw[q + "gate_proj.weight"].view(torch.uint8))
            assert torch.equal(gu8[e, I:].view(torch.uint8), raw[q + "up_proj.weight"].view(torch.uint8))
            assert torch.equal(d8[e].view(torch.uint8), raw[q + "down_proj.weight"].view(torch.uint8))
            assert torch.equal(gu_s[e, :2], raw[q + "gate_proj.weight_scale_inv"])
            assert torch.equal(gu_s[e, 2:], raw[q + "up_proj.weight_scale_inv"])
            assert torch.equal(d_s[e], raw[q + "down_proj.weight_scale_inv"])
        # the attention projections: dequantised to bf16 at load
        assert m.w[f"l{i}.wo"].dtype == m.w[f"l{i}.wqkv"].dtype == torch.bfloat16
        assert torch.equal(m.w[f"l{i}.wo"], reference.block_fp8_dequant(
            raw[p + "self_attn.o_proj.weight"], raw[p + "self_attn.o_proj.weight_scale_inv"], torch.bfloat16))
        assert torch.equal(m.w[f"l{i}.router"], raw[p + "mlp.gate.weight"])
    assert not any(v.dtype == torch.float8_e4m3fn for k, v in m.w.items() if "we_" not in k)


def test_cpu_logits_match_the_fp32_forward_over_dequantised_weights(ckpts):
    """forward_tokens, prefill_batch and decode (the reference ops) against
    reference_logits, whose experts are the e4m3 tensors dequantised exactly;
    the bf16 checkpoint's tolerance.  The reference forward is itself checked
    against a bf16-expert model holding the dequantised weights' fp32 values."""
    m = _load(ckpts["fp8"])
    toks = [3, 77, 140, 9, 501, 12]
    ref = m.reference_logits(toks)
    scale = max(1.0, ref.abs().max().item())
    got = m.forward_tokens(torch.tensor(toks[:5], dtype=torch.int32), 0, 0).float()
    assert (got - ref[4]).abs().max() < 0.05 * scale
    both = m.prefill_batch([(toks[:5], 0, 0), (toks[:3], 1, 0)]).float()
    assert (both[0] - ref[4]).abs().max() < 0.05 * scale and (both[1] - ref[2]).abs().max() < 0.05 * scale
    step = m.decode(torch.tensor([toks[5]], dtype=torch.int32), torch.tensor([0], dtype=torch.int32),
                    torch.tensor([5], dtype=torch.int32)).float()
    assert (step[0] - ref[5]).abs().max() < 0.05 * scale
    m.moe_rows = 3  # a prefill longer than the workspace walks its rows in chunks
    assert torch.equal(m.forward_tokens(torch.tensor(toks[:5], dtype=torch.int32), 0, 0).float(), got)
    # the same definition by another route: moe_mlp_math over the dequantised stacks
    x = torch.randn(7, H, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    w = m.w
    a = reference.moe_mlp_w8(x, w["l0.router"], w["l0.we_gu8"], w["l0.we_gu_s"], w["l0.we_down8"], w["l0.we_down_s"],
                             2, True)
    gu, dn = reference.moe_w8_dequant(w["l0.we_gu8"], w["l0.we_gu_s"], w["l0.we_down8"], w["l0.we_down_s"])
    assert torch.equal(a, reference.moe_mlp(x, w["l0.router"], gu, dn, 2, True))
    # the quantisation is visible: the bf16 checkpoint of the same draws gives other logits, close by
    ref16 = _load(ckpts["bf16"]).reference_logits(toks)
    assert not torch.equal(ref16, ref)
    assert torch.nn.functional.cosine_similarity(ref16[-1], ref[-1], dim=0) > 0.99


def test_the_bf16_checkpoint_still_loads_as_bf16(ckpts):
    m = _load(ckpts["bf16"])
    assert m.moe and not m.moe_w8 and m.cfg.moe_weight_dtype == "bf16"
    assert m.w["l0.we_gu"].dtype == torch.bfloat16 and "l0.we_gu8" not in m.w


def test_a_random_init_preset_quantises_its_experts():
    from dmcp.models.llm import preset
    kw = dict(max_batch=2, max_seq=64, max_rows=4, n_experts=4, experts_per_tok=2, moe_intermediate=64)
    m8 = LocalLM(preset("tiny", moe_weight_dtype="fp8b", **kw), device="cpu")
    m16 = LocalLM(preset("tiny", **kw), device="cpu")
    assert m8.moe_w8 and m8.w["l0.we_gu8"].dtype == torch.float8_e4m3fn and "l0.we_gu" not in m8.w
    assert tuple(m8.w["l0.we_gu_s"].shape) == (4, 2, 2) and tuple(m8.w["l0.we_down_s"].shape) == (4, 2, 1)
    gu, dn = reference.moe_w8_dequant(m8.w["l0.we_gu8"], m8.w["l0.we_gu_s"], m8.w["l0.we_down8"], m8.w["l0.we_down_s"])
    w16 = m16.w["l0.we_gu"].float()
    assert bool(((gu - w16).abs() <= 2.0 ** -4 * w16.abs().max()).all()) and not torch.equal(gu, w16)
    toks = [256, 72, 105, 33]
    ref = m8.reference_logits(toks)[-1]
    got = m8.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float()
    assert (got - ref).abs().max() < 0.05 * max(1.0, ref.abs().max().item())
    with pytest.raises(ValueError, match="moe_weight_dtype"):
        LocalLM(preset("tiny", moe_weight_dtype="int4", **kw), device="cpu")
    for knob in ("prefill_dtype", "decode_dtype"):  # the existing refusal holds for the new format too
        with pytest.raises(ValueError, match=knob):
            LocalLM(preset("tiny", moe_weight_dtype="fp8b", **kw, **{knob: "fp8"}), device="cpu")


def test_the_witness_names_the_expert_weight_format(ckpts):
    from dmcp.enrich.workers import _witness
    assert _witness("cpu", _load(ckpts["fp8"]))["moe_weights"] == "fp8b128"
    w = _witness("cpu", _load(ckpts["bf16"]))
    assert w["moe_weights"] == "bf16" and w["moe"] == "8x2"
    assert "moe_weights" not in _witness("cpu")
