"""A checkpoint directory loads as the model it is, or is refused with a reason.

The oracle is ``transformers`` (fp32 ``LlamaForCausalLM`` / ``Qwen2ForCausalLM``
loaded from the same written directory, so both sides see the same
bf16-rounded weights); the checkpoints are tiny and written by
``dmcp.utils.synth.llama_checkpoint`` with RMSNorm weights set to 1 (a folded
norm weight is rounded to bf16 once more, which is not what is measured here).
Biases are never taken from a model ``transformers`` builds itself: it
initialises Qwen2 biases to zero.

Model parity: last-position logits of ``LocalLM.reference_logits`` against the
HF model on four 200-token random prompts at positions [0, 200) and
[800, 1000); error = (1 - cosine, max |diff| / max |logit|), the worst over the
prompts.  The bound is not fixed in advance: the plain-Llama case -- the
loader as it stood before RoPE scaling and biases -- is measured first and
each new case may show at most 2x its error (the new arithmetic is another
table and one fp32 add).  A copy of each scaled / biased directory with the
``rope_scaling`` key or the bias tensors stripped -- what the earlier loader
saw -- must exceed 100x the baseline.

The plain-Llama baseline is measured per geometry: both sides sum in fp32, so
the error floor grows with the widths summed over, and the hidden-512 /
head_dim-128 plain model alone shows 1.9x (max |diff|) to 3.1x (1 - cosine)
the hidden-256 one's error.  The head_dim-128 case is therefore held to 2x the
plain head_dim-128 model; against the hidden-256 baseline it reads 2.48x /
3.76x, which says nothing about RoPE scaling.

Measured on the build host (CPU, transformers 5.15; 1 - cosine evaluated in
float64; x = multiple of the case's plain baseline):

    case                    1 - cosine          max|diff| / max|logit|
    plain (baseline)        2.80e-13            8.83e-07
    plain_hd128 (baseline)  8.68e-13            1.72e-06
    llama3_b                2.22e-13 (0.79x)    7.40e-07 (0.84x)
    linear                  1.78e-13 (0.64x)    8.17e-07 (0.93x)
    qwen2_bias              4.15e-13 (1.48x)    8.01e-07 (0.91x)
    qwen2_bias_tied         3.71e-13 (1.32x)    1.03e-06 (1.17x)
    llama_hd128_b           1.05e-12 (1.21x)    2.19e-06 (1.27x)
    stripped llama3_b       1.08e-03            5.01e-02 (56,682x)
    stripped linear         1.03e-03            4.54e-02 (51,378x)
    stripped qwen2_bias     9.76e-01            1.51e+00 (1.7e6x)
    stripped qwen2 tied     9.35e-01            2.63e+00 (3.0e6x)
    stripped llama_hd128_b  1.11e-02            1.72e-01 (1.0e5x)
"""
import json
import os
import shutil

import pytest
import torch

transformers = pytest.importorskip("transformers")

from dmcp.config import Config  # noqa: E402
from dmcp.enrich.backend import LazyBackend, RefusedBackend, create_backend  # noqa: E402
from dmcp.models.llm import CheckpointUnsupported, LocalLM, check_checkpoint  # noqa: E402
from dmcp.ops import reference  # noqa: E402
from dmcp.utils import synth  # noqa: E402

LLAMA32 = {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
           "original_max_position_embeddings": 8192}
# all three frequency bands within 1,024 positions
CASE_B = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
          "original_max_position_embeddings": 64}
LINEAR = {"rope_type": "linear", "factor": 4.0}
THETA = 500000.0
TINY = dict(layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(),
            device="cpu")
HD128 = dict(hidden=512, head_dim=128)
CASES = {
    "plain": {},
    "plain_hd128": dict(HD128),
    "llama3_b": dict(rope_scaling=CASE_B),
    "linear": dict(rope_scaling=LINEAR),
    "qwen2_bias": dict(qkv_bias=True, model_type="qwen2"),
    "qwen2_bias_tied": dict(qkv_bias=True, model_type="qwen2", tie_embeddings=True),
    "llama_hd128_b": dict(HD128, rope_scaling=CASE_B),
}
# each new case's plain-Llama model of the same geometry
BASELINE_OF = {"llama_hd128_b": "plain_hd128"}


def _rewrite(path, fn):
    """Applies ``fn`` to the tensor dict of ``path``'s safetensors file."""
    from safetensors.torch import load_file, save_file
    f = os.path.join(path, "model.safetensors")
    t = load_file(f)
    fn(t)
    save_file(t, f)


def _edit_config(path, **kv):
    f = os.path.join(path, "config.json")
    with open(f) as fh:
        cfg = json.load(fh)
    for k, v in kv.items():
        if v is None:
            cfg.pop(k, None)
        else:
            cfg[k] = v
    with open(f, "w") as fh:
        json.dump(cfg, fh)


def _unit_norms(t):
    for k in t:
        if k.endswith("layernorm.weight") or k == "model.norm.weight":
            t[k] = torch.ones_like(t[k])


def _write(root, name, **kw):
    d = synth.llama_checkpoint(os.path.join(str(root), name), **{**TINY, **kw})
    _rewrite(d, _unit_norms)
    return d


def _hf(path):
    with open(os.path.join(path, "config.json")) as f:
        qwen = json.load(f).get("model_type") == "qwen2"
    cls = transformers.Qwen2ForCausalLM if qwen else transformers.LlamaForCausalLM
    return cls.from_pretrained(path, dtype=torch.float32).eval()


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("fidelity")
    return {name: _write(root, name, **kw) for name, kw in CASES.items()}


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (200,), generator=g).tolist() for _ in range(4)]


_HF_LOGITS = {}


def _hf_logits(path, prompts):
    """HF fp32 last-position logits per (prompt, start); computed once per directory."""
    if path not in _HF_LOGITS:
        m = _hf(path)
        out = {}
        with torch.no_grad():
            for i, p in enumerate(prompts):
                for start in (0, 800):
                    ids = torch.tensor([p])
                    pos = torch.arange(start, start + len(p))[None]
                    out[i, start] = m(input_ids=ids, position_ids=pos).logits[0, -1].float()
        _HF_LOGITS[path] = out
    return _HF_LOGITS[path]


def _errors(local_dir, hf_dir, prompts):
    """(1 - cosine, max |diff| / max |logit|): the worst over prompts and offsets."""
    m = LocalLM.load_safetensors(local_dir, device="cpu", max_seq=1024, max_batch=1, max_rows=1)
    ref = _hf_logits(hf_dir, prompts)
    e_cos = e_abs = 0.0
    for (i, start), exp in ref.items():
        got = m.reference_logits(prompts[i], start_pos=start)[-1].double()
        e = exp.double()
        e_cos = max(e_cos, 1.0 - torch.nn.functional.cosine_similarity(got, e, dim=0).item())
        e_abs = max(e_abs, ((got - e).abs().max() / e.abs().max()).item())
    return e_cos, e_abs


@pytest.fixture(scope="module")
def baselines(ckpts, prompts):
    """The plain-Llama cases: the loader's code path as it was, against HF."""
    out = {}
    for name in ("plain", "plain_hd128"):
        b = out[name] = _errors(ckpts[name], ckpts[name], prompts)
        print(f"baseline {name}: 1-cos {b[0]:.3e}  maxabs/max {b[1]:.3e}")
        assert b[0] < 1e-6 and b[1] < 1e-3, b  # fp32 against fp32: anything larger is a different model
    return out


# ------------------------------------------------------------- 1. inv_freq
def _table_freq(head_dim, scaling):
    """Frequencies implied by the table: the angle of position 1."""
    cs = reference.rope_tables(4, head_dim, THETA, scaling=scaling).double()
    return torch.atan2(cs[1, :, 1], cs[1, :, 0])


@pytest.mark.parametrize("scaling", [LLAMA32, CASE_B], ids=["llama3.2", "case_b"])
def test_inv_freq_matches_transformers(tmp_path, scaling):
    d = _write(tmp_path, "m", rope_scaling=scaling)
    hf = _hf(d).model.rotary_emb.inv_freq.double()
    torch.testing.assert_close(reference.rope_inv_freq(64, THETA, scaling), hf, rtol=1e-6, atol=0)
    torch.testing.assert_close(_table_freq(64, scaling), hf, rtol=1e-6, atol=0)
    plain = reference.rope_inv_freq(64, THETA)
    changed = int(((hf / plain - 1).abs() > 1e-3).sum())
    print("pairs whose frequency the scaling changes:", changed, "of 32")
    if scaling is LLAMA32:
        assert changed == 17
    else:  # every band occurs: unchanged, divided by the factor, interpolated
        ratio = plain / hf
        assert (ratio - 1).abs().min() < 1e-6 and (ratio - 8).abs().min() < 1e-5
        assert ((ratio > 1.01) & (ratio < 7.99)).any()
    assert LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1).cfg.rope_scaling == \
        reference.rope_scaling_key(scaling)


def test_linear_scaling_divides_every_frequency():
    plain = reference.rope_inv_freq(64, THETA)
    torch.testing.assert_close(reference.rope_inv_freq(64, THETA, LINEAR), plain / 4, rtol=1e-6, atol=0)
    torch.testing.assert_close(_table_freq(64, LINEAR), plain / 4, rtol=1e-6, atol=0)


def test_no_scaling_is_the_unchanged_table():
    a = reference.rope_tables(128, 64, THETA)
    assert torch.equal(a, reference.rope_tables(128, 64, THETA, scaling=None))
    assert torch.equal(a, reference.rope_tables(128, 64, THETA, scaling={"rope_type": "default"}))
    half = 32
    inv = 1.0 / (THETA ** (torch.arange(0, half, dtype=torch.float64) / half))
    ang = torch.arange(128, dtype=torch.float64)[:, None] * inv[None, :]
    assert torch.equal(a, torch.stack([ang.cos(), ang.sin()], dim=-1).to(torch.float32))


# ---------------------------------------------------------- 2. model parity
@pytest.mark.parametrize("case", [c for c in CASES if not c.startswith("plain")])
def test_model_parity_with_transformers(ckpts, prompts, baselines, case, tmp_path):
    """Each new case within 2x the plain-Llama error; the same directory as
    the earlier loader saw it (scaling key / bias tensors dropped) beyond 100x.
    The figures are in the module docstring and docs/PARITY.md."""
    baseline = baselines[BASELINE_OF.get(case, "plain")]
    d = ckpts[case]
    e = _errors(d, d, prompts)
    print(f"{case}: 1-cos {e[0]:.3e} ({e[0] / baseline[0]:.2f}x)  maxabs/max {e[1]:.3e} ({e[1] / baseline[1]:.2f}x)")
    # what the loader saw before this feature
    old = shutil.copytree(d, str(tmp_path / "stripped"))
    if "rope_scaling" in CASES[case]:
        _edit_config(old, rope_scaling=None)
    else:
        _rewrite(old, lambda t: [t.pop(k) for k in list(t) if k.endswith("_proj.bias")])
        _edit_config(old, attention_bias=None)
    s = _errors(old, d, prompts)
    print(f"{case} stripped: 1-cos {s[0]:.3e} ({s[0] / baseline[0]:.1f}x)  maxabs/max {s[1]:.3e} "
          f"({s[1] / baseline[1]:.1f}x)")
    assert e[0] <= 2 * baseline[0] and e[1] <= 2 * baseline[1], (case, e, baseline)
    assert s[0] > 100 * baseline[0] and s[1] > 100 * baseline[1], (case, s, baseline)


def test_loaded_bias_layout(ckpts):
    from safetensors.torch import load_file
    d = ckpts["qwen2_bias"]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(d, "model.safetensors"))
    assert m.has_bias
    for i in range(2):
        p = f"model.layers.{i}.self_attn."
        b = m.w[f"l{i}.bqkv"]
        assert b.dtype == torch.bfloat16 and b.shape == (m.cfg.qkv_dim,)
        assert torch.equal(b, torch.cat([raw[p + "q_proj.bias"], raw[p + "k_proj.bias"], raw[p + "v_proj.bias"]]))
        assert b.float().std() > 1.0  # N(0, 2^2): dropping it is unmistakable
    plain = LocalLM.load_safetensors(ckpts["plain"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert not plain.has_bias and not any(k.endswith("bqkv") for k in plain.w)
    from dmcp.models.llm import preset
    assert not any(k.endswith("bqkv") for k in LocalLM(preset("tiny"), device="cpu").w)


def test_synth_defaults_write_the_same_tensors(tmp_path):
    """The new options draw after every existing draw: the shared tensors of
    a biased checkpoint equal the default one's (same seed)."""
    from safetensors.torch import load_file
    a = load_file(os.path.join(synth.llama_checkpoint(str(tmp_path / "a"), **TINY), "model.safetensors"))
    b = load_file(os.path.join(synth.llama_checkpoint(str(tmp_path / "b"), **TINY, qkv_bias=True,
                                                       model_type="qwen2"), "model.safetensors"))
    assert set(b) - set(a) == {f"model.layers.{i}.self_attn.{n}_proj.bias" for i in range(2) for n in "qkv"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    with open(os.path.join(str(tmp_path / "a"), "config.json")) as f:
        assert set(json.load(f)) == {"vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads",
                                     "num_key_value_heads", "intermediate_size", "rms_norm_eps", "rope_theta",
                                     "architectures"}


# ------------------------------------------------------------ 3. validation
def _add_tensor(name, shape=(4,)):
    return lambda t: t.__setitem__(name, torch.zeros(shape, dtype=torch.bfloat16))


REFUSALS = {
    "model_type": (dict(model_type="mistral"), None, "model_type"),
    "architectures": (dict(architectures=["MistralForCausalLM"]), None, "architectures"),
    "hidden_act": (dict(hidden_act="gelu"), None, "hidden_act"),
    "mlp_bias": (dict(mlp_bias=True), None, "mlp_bias"),
    "o_proj_bias": ({}, _add_tensor("model.layers.0.self_attn.o_proj.bias"), "model.layers.0.self_attn.o_proj.bias"),
    "mlp_bias_tensor": ({}, _add_tensor("model.layers.1.mlp.gate_proj.bias"), "model.layers.1.mlp.gate_proj.bias"),
    "sliding_window": (dict(use_sliding_window=True), None, "use_sliding_window"),
    "rope_yarn": (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), None, "yarn"),
    "rope_dynamic_legacy_key": (dict(rope_scaling={"type": "dynamic", "factor": 2.0}), None, "dynamic"),
    "rope_longrope_parameters": (dict(rope_parameters={"rope_type": "longrope", "rope_theta": 1e4}), None,
                                 "longrope"),
    "kv_heads": (dict(num_key_value_heads=3), None, "num_key_value_heads"),
    "q_norm": ({}, _add_tensor("model.layers.0.self_attn.q_norm.weight"), "model.layers.0.self_attn.q_norm.weight"),
}


@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("valid") / "base"), **TINY)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_unsupported_checkpoints_are_refused_with_the_key(base_ckpt, tmp_path, name):
    cfg_edit, tensor_edit, needle = REFUSALS[name]
    d = shutil.copytree(base_ckpt, str(tmp_path / "ck"))
    if cfg_edit:
        _edit_config(d, **cfg_edit)
    if tensor_edit:
        _rewrite(d, tensor_edit)
    reason = check_checkpoint(d)
    assert reason is not None and needle in reason, reason
    with pytest.raises(CheckpointUnsupported) as e:
        LocalLM.load_safetensors(d, device="cpu")
    assert needle in str(e.value)
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=d))
    assert isinstance(be, RefusedBackend) and not be.enabled
    assert needle in be.disabled_reason and "LOCAL_LLM_MODEL_PATH" in be.disabled_reason


def test_supported_checkpoints_are_accepted(base_ckpt, ckpts, tmp_path):
    assert check_checkpoint(base_ckpt) is None  # the unchanged default writer's directory
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=base_ckpt))
    assert isinstance(be, LazyBackend) and be.enabled and not be.built
    for d in ckpts.values():
        assert check_checkpoint(d) is None, d
    # rotary_emb.inv_freq buffers (older exports) are the only ignorable tensors
    d = shutil.copytree(base_ckpt, str(tmp_path / "inv"))
    _rewrite(d, _add_tensor("model.layers.0.self_attn.rotary_emb.inv_freq", (32,)))
    assert check_checkpoint(d) is None
    # the newer rope_parameters form, carrying theta
    d = shutil.copytree(base_ckpt, str(tmp_path / "params"))
    _edit_config(d, rope_theta=None, rope_parameters={**CASE_B, "rope_theta": 12345.0})
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.cfg.rope_theta == 12345.0 and m.cfg.rope_scaling == reference.rope_scaling_key(CASE_B)
    # the legacy key "type"
    d = shutil.copytree(base_ckpt, str(tmp_path / "legacy"))
    _edit_config(d, rope_scaling={"type": "linear", "factor": 4.0})
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.cfg.rope_scaling == reference.rope_scaling_key(LINEAR) and hash(m.cfg) is not None


def test_check_reads_no_tensor_data(base_ckpt, tmp_path):
    """Headers only: the check passes on a file whose tensor bytes are cut off."""
    d = shutil.copytree(base_ckpt, str(tmp_path / "cut"))
    f = os.path.join(d, "model.safetensors")
    with open(f, "rb") as fh:
        n = int.from_bytes(fh.read(8), "little")
        head = fh.read(n)
    size = os.path.getsize(f)
    with open(f, "wb") as fh:  # same length, tensor bytes zeroed
        fh.write(n.to_bytes(8, "little") + head)
        fh.truncate(size)
    assert check_checkpoint(d) is None


@pytest.mark.parametrize("knob", ["prefill_dtype", "decode_dtype"])
def test_fp8_gemms_with_biases_are_refused_by_name(ckpts, knob):
    with pytest.raises(ValueError) as e:
        LocalLM.load_safetensors(ckpts["qwen2_bias"], device="cpu", max_seq=64, max_batch=1, max_rows=1,
                                 **{knob: "fp8"})
    assert knob in str(e.value) and not isinstance(e.value, CheckpointUnsupported)


# ------------------------------------------------------------ 4. references
@pytest.mark.parametrize("op", ["fused_rope_kv", "wgemm_rope_kv", "tgemm_rope_kv"])
@pytest.mark.parametrize("kv", [torch.float32, torch.uint8], ids=["wide", "fp8"])
def test_reference_qkv_ops_apply_the_bias_before_rope(op, kv):
    Hq, Hkv, D, K, M, S, MAXS, eps = 4, 2, 64, 128, 5, 3, 32, 1e-5
    g = torch.Generator().manual_seed(3)
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    b = (2.0 * torch.randn(N, generator=g)).to(torch.bfloat16)
    pos = torch.tensor([0, 31, 7, 8, 9], dtype=torch.int32)
    slot = torch.tensor([0, 1, -1, 2, 0], dtype=torch.int32)
    cs = reference.rope_tables(MAXS, D, THETA, scaling=CASE_B)
    kc, vc = torch.zeros(S, Hkv, MAXS, D, dtype=kv), torch.zeros(S, Hkv, MAXS, D, dtype=kv)
    kr, vr = kc.clone(), vc.clone()
    xin = x.float()
    if op == "fused_rope_kv":
        xin = xin * torch.rsqrt(xin.pow(2).mean(-1, keepdim=True) + eps)
        q = reference.fused_rope_kv(x, w, eps, pos, slot, cs, kc, vc, Hq, bias=b)
    else:
        q = getattr(reference, op)(x, w, pos, slot, cs, kc, vc, Hq, None, bias=b)
    exp = reference.rope_kv(torch.nn.functional.linear(xin, w.float(), b.float()), pos, slot, cs, kr, vr, Hq)
    torch.testing.assert_close(q.float(), exp, atol=2e-2, rtol=2 ** -7)  # q is rounded to bf16
    tol = dict(atol=2e-2, rtol=0.13) if kv == torch.uint8 else dict(atol=2e-2, rtol=2 ** -7)
    torch.testing.assert_close(reference.kv_float(kc), reference.kv_float(kr), **tol)
    torch.testing.assert_close(reference.kv_float(vc), reference.kv_float(vr), **tol)
    assert not reference.kv_float(kc)[:, :, 7].any() and reference.kv_float(kc)[1, :, 31].any()
    # the bias matters, and None is the old result
    q0 = (reference.fused_rope_kv(x, w, eps, pos, slot, cs, kc.clone(), vc.clone(), Hq) if op == "fused_rope_kv"
          else getattr(reference, op)(x, w, pos, slot, cs, kc.clone(), vc.clone(), Hq, None))
    assert (q0.float() - q.float()).abs().max() > 1.0
