"""Qwen3 checkpoints: the per-head q / k RMSNorm against ``transformers``.

The oracle is fp32 ``Qwen3ForCausalLM`` loaded from the directory the loader
reads, as tests/test_checkpoint_fidelity.py does for Llama and Qwen2.  Layer
and final norm weights are 1 (the loader folds them into bf16 matrices, which
is not what is measured here); ``q_norm`` / ``k_norm`` weights stay as drawn
(1 +- 0.25): they are not folded and are what is measured.

Each Qwen3 case may show at most 2x the error of the plain-Llama model of the
same geometry, measured in the same run (one more fp32 norm per head: the
order of arithmetic of the bias cases that got 2x); the same directory with
the norm tensors stripped and ``model_type`` ``llama`` -- what a loader
ignoring them would compute -- must exceed 100x.

Measured (CPU, fp32; 1 - cosine, max |diff| / max |logit| of the last-position
logits; worst of four 200-token prompts at positions [0, 200) and [800, 1000)):

    case                     1 - cos             max|diff| / max|logit|
    llama hd64 (baseline)    2.80e-13            8.83e-07
    llama hd128 (baseline)   2.42e-13            7.55e-07
    qwen3 hd64               2.39e-13 (0.85x)    9.16e-07 (1.04x)
    qwen3 hd128              2.68e-13 (1.11x)    7.88e-07 (1.04x)
    stripped qwen3 hd64      7.84e-02            4.19e-01 (4.7e5x)
    stripped qwen3 hd128     1.41e-01            5.35e-01 (7.1e5x)

With the RoPE table's angles taken in float64 (as for un-normed models) the
two Qwen3 cases measured 8.4x / 2.6x and 43.6x / 6.6x their baselines: fp32
``transformers`` rounds position x inv_freq to fp32 (3e-5 rad at position
1,000), and unit-RMS q / k heads turn that into attention-logit differences
an un-normed model's small q / k do not show.  A QK-norm model's table is
therefore built in fp32 like its own code's (``rope_tables(fp32_angles=True)``).
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

TINY = dict(layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(),
            device="cpu")
QWEN3 = dict(qk_norm=True, model_type="qwen3")
# hidden 256 with 4 heads of 128: heads x head_dim = 512 is not the hidden size (Qwen3-0.6B's shape in small)
CASES = {
    "llama_hd64": dict(head_dim=64),
    "llama_hd128": dict(head_dim=128),
    "qwen3_hd64": dict(QWEN3, head_dim=64),
    "qwen3_hd128": dict(QWEN3, head_dim=128),
}
BASELINE_OF = {"qwen3_hd64": "llama_hd64", "qwen3_hd128": "llama_hd128"}
QK = ("q_norm.weight", "k_norm.weight")


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
        qwen3 = json.load(f).get("model_type") == "qwen3"
    cls = transformers.Qwen3ForCausalLM if qwen3 else transformers.LlamaForCausalLM
    return cls.from_pretrained(path, dtype=torch.float32).eval()


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("qwen3")
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
    """The plain-Llama models of the two geometries, against HF."""
    out = {}
    for name in ("llama_hd64", "llama_hd128"):
        b = out[name] = _errors(ckpts[name], ckpts[name], prompts)
        print(f"baseline {name}: 1-cos {b[0]:.3e}  maxabs/max {b[1]:.3e}")
        assert b[0] < 1e-6 and b[1] < 1e-3, b  # fp32 against fp32: anything larger is a different model
    return out


# ---------------------------------------------------------- 1. model parity
@pytest.mark.parametrize("case", sorted(BASELINE_OF))
def test_qwen3_parity_with_transformers(ckpts, prompts, baselines, case, tmp_path):
    baseline = baselines[BASELINE_OF[case]]
    d = ckpts[case]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.has_qk_norm and m.cfg.head_dim == CASES[case]["head_dim"] and m.cfg.rope_theta == 1e6
    assert (m.cfg.n_heads * m.cfg.head_dim != m.cfg.hidden) == (case == "qwen3_hd128")
    e = _errors(d, d, prompts)
    print(f"{case}: 1-cos {e[0]:.3e} ({e[0] / baseline[0]:.2f}x)  maxabs/max {e[1]:.3e} ({e[1] / baseline[1]:.2f}x)")
    # what a loader that ignored the norm tensors would have produced
    old = shutil.copytree(d, str(tmp_path / "stripped"))
    _rewrite(old, lambda t: [t.pop(k) for k in list(t) if k.endswith(QK)])
    _edit_config(old, model_type="llama", architectures=["LlamaForCausalLM"], layer_types=None)
    assert check_checkpoint(old) is None
    s = _errors(old, d, prompts)
    print(f"{case} stripped: 1-cos {s[0]:.3e} ({s[0] / baseline[0]:.1f}x)  maxabs/max {s[1]:.3e} "
          f"({s[1] / baseline[1]:.1f}x)")
    assert e[0] <= 2 * baseline[0] and e[1] <= 2 * baseline[1], (case, e, baseline)
    assert s[0] > 100 * baseline[0] and s[1] > 100 * baseline[1], (case, s, baseline)


def test_loaded_qk_norm_layout(ckpts):
    from safetensors.torch import load_file
    d = ckpts["qwen3_hd128"]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(d, "model.safetensors"))
    for i in range(2):
        p = f"model.layers.{i}.self_attn."
        assert torch.equal(m.w[f"l{i}.qnorm"], raw[p + "q_norm.weight"]) and m.w[f"l{i}.qnorm"].shape == (128,)
        assert torch.equal(m.w[f"l{i}.knorm"], raw[p + "k_norm.weight"])
        assert m.w[f"l{i}.qnorm"].dtype == torch.bfloat16 and not torch.equal(m.w[f"l{i}.qnorm"], m.w[f"l{i}.knorm"])
        assert m._qk_norm(i) == (m.w[f"l{i}.qnorm"], m.w[f"l{i}.knorm"], m.cfg.eps)
    plain = LocalLM.load_safetensors(ckpts["llama_hd128"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert not plain.has_qk_norm and plain._qk_norm(0) is None
    assert not any(k.endswith(("qnorm", "knorm")) for k in plain.w)


def test_synth_qk_norm_draws_after_every_other_tensor(tmp_path):
    from safetensors.torch import load_file
    a = load_file(os.path.join(synth.llama_checkpoint(str(tmp_path / "a"), **TINY), "model.safetensors"))
    d = synth.llama_checkpoint(str(tmp_path / "b"), **TINY, **QWEN3)
    b = load_file(os.path.join(d, "model.safetensors"))
    assert set(b) - set(a) == {f"model.layers.{i}.self_attn.{n}" for i in range(2) for n in QK}
    assert all(torch.equal(a[k], b[k]) for k in a)
    w = b["model.layers.1.self_attn.k_norm.weight"].float()
    assert w.shape == (64,) and 0.1 < w.std().item() < 0.4 and abs(w.mean().item() - 1) < 0.15
    with open(os.path.join(d, "config.json")) as f:
        cfg = json.load(f)
    assert cfg["model_type"] == "qwen3" and cfg["architectures"] == ["Qwen3ForCausalLM"] and cfg["head_dim"] == 64
    assert cfg["layer_types"] == ["full_attention"] * 2 and cfg["attention_bias"] is False
    assert cfg["use_sliding_window"] is False and cfg["rope_theta"] == 1e6


# ------------------------------------------------------------ 2. validation
def _drop(name):
    return lambda t: t.pop(name)


def _set_tensor(name, shape):
    return lambda t: t.__setitem__(name, torch.ones(shape, dtype=torch.bfloat16))


L0 = "model.layers.0.self_attn."
L1 = "model.layers.1.self_attn."
REFUSALS = {
    "only_q_norm": ({}, _drop(L1 + "k_norm.weight"), L1 + "k_norm.weight"),
    "only_k_norm": ({}, _drop(L0 + "q_norm.weight"), L0 + "q_norm.weight"),
    "q_norm_length": ({}, _set_tensor(L0 + "q_norm.weight", (32,)), L0 + "q_norm.weight"),
    "k_norm_per_head": ({}, _set_tensor(L1 + "k_norm.weight", (2, 64)), L1 + "k_norm.weight"),
    "layer_types": (dict(layer_types=["full_attention", "sliding_attention"]), None, "layer_types"),
    "sliding_window": (dict(use_sliding_window=True), None, "use_sliding_window"),
    "bias_missing": (dict(attention_bias=True), _set_tensor(L0 + "q_proj.bias", (256,)), "bias"),
    "moe": (dict(model_type="qwen3_moe"), None, "model_type"),
    "arch": (dict(architectures=["Qwen3MoeForCausalLM"]), None, "architectures"),
}


@pytest.fixture(scope="module")
def base_ckpt(tmp_path_factory):
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("valid") / "qwen3"), **TINY, **QWEN3)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_malformed_qwen3_checkpoints_are_refused_with_the_key(base_ckpt, tmp_path, name):
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


@pytest.mark.parametrize("model_type", ["llama", "qwen2", None])
def test_q_norm_outside_qwen3_stays_refused(base_ckpt, tmp_path, model_type):
    """The norm tensors are consumed for ``model_type`` qwen3 only."""
    d = shutil.copytree(base_ckpt, str(tmp_path / "ck"))
    arch = {"llama": ["LlamaForCausalLM"], "qwen2": ["Qwen2ForCausalLM"], None: None}[model_type]
    _edit_config(d, model_type=model_type, architectures=arch, layer_types=None)
    reason = check_checkpoint(d)
    assert reason is not None and "_norm.weight is not consumed" in reason, reason


def test_wellformed_qwen3_is_accepted(base_ckpt, ckpts, tmp_path):
    assert check_checkpoint(base_ckpt) is None
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=base_ckpt))
    assert isinstance(be, LazyBackend) and be.enabled and not be.built
    for d in ckpts.values():
        assert check_checkpoint(d) is None, d
    # biases with attention_bias true, tied embeddings, no layer_types key
    d = synth.llama_checkpoint(str(tmp_path / "biased"), **TINY, **QWEN3, qkv_bias=True, tie_embeddings=True)
    _edit_config(d, layer_types=None)
    assert check_checkpoint(d) is None
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.has_qk_norm and m.has_bias and m.w["lm_head"] is not None


def test_check_reads_no_tensor_data(base_ckpt, tmp_path):
    """Headers only, the norm shapes included: the check passes on a file whose tensor bytes are zeroed."""
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
def test_fp8_gemms_with_qk_norm_are_refused_by_name(ckpts, knob):
    with pytest.raises(ValueError) as e:
        LocalLM.load_safetensors(ckpts["qwen3_hd64"], device="cpu", max_seq=64, max_batch=1, max_rows=1,
                                 **{knob: "fp8"})
    assert knob in str(e.value) and "norm" in str(e.value) and not isinstance(e.value, CheckpointUnsupported)
    m = LocalLM.load_safetensors(ckpts["qwen3_hd64"], device="cpu", max_seq=64, max_batch=1, max_rows=1,
                                 prefill_dtype="auto")
    assert not m.prefill_fp8 and m.cfg.prefill_dtype == "bf16"


# ------------------------------------------------------------ 3. references
@pytest.mark.parametrize("op", ["rope_kv", "fused_rope_kv", "wgemm_rope_kv", "tgemm_rope_kv"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kv", [torch.float32, torch.uint8], ids=["wide", "fp8"])
def test_reference_qkv_ops_norm_then_rope(op, D, kv):
    """``qk_norm`` on each reference QKV op is norm-then-``apply_rope`` by
    hand, on the projection rounded where the op rounds it; v and the cache
    rows no row addresses are untouched."""
    Hq, Hkv, K, M, S, MAXS, eps, neps = 4, 2, 128, 5, 3, 32, 1e-5, 1e-6
    g = torch.Generator().manual_seed(3)
    N = (Hq + 2 * Hkv) * D
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
    b = (2.0 * torch.randn(N, generator=g)).to(torch.bfloat16)
    qw = (1.0 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16)
    kw = (1.0 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16)
    qw[3], kw[D - 2] = 8.0, 8.0
    pos = torch.tensor([0, 31, 7, 8, 9], dtype=torch.int32)
    slot = torch.tensor([0, 1, -1, 2, 0], dtype=torch.int32)
    cs = reference.rope_tables(MAXS, D, 1e6)
    kc, vc = torch.full((S, Hkv, MAXS, D), 0.5).to(kv), torch.full((S, Hkv, MAXS, D), 0.5).to(kv)
    k0 = kc.clone()
    xin = x.float()
    if op == "fused_rope_kv":
        xin = xin * torch.rsqrt(xin.pow(2).mean(-1, keepdim=True) + eps)
    proj = torch.nn.functional.linear(xin, w.float(), b.float())
    if op != "fused_rope_kv":
        proj = proj.to(torch.bfloat16)  # the row the reduction / F.linear rounds
    call = {"rope_kv": lambda **k: reference.rope_kv(proj, pos, slot, cs, kc, vc, Hq, **k),
            "fused_rope_kv": lambda **k: reference.fused_rope_kv(x, w, eps, pos, slot, cs, kc, vc, Hq, bias=b, **k),
            }.get(op, lambda **k: getattr(reference, op)(x, w, pos, slot, cs, kc, vc, Hq, None, bias=b, **k))
    q = call(qk_norm=(qw, kw, neps))
    # by hand
    heads = proj.float().view(M, Hq + 2 * Hkv, D)

    def norm(t, wt):
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + neps) * wt.float()
    q_exp = reference.apply_rope(norm(heads[:, :Hq], qw), pos, cs)
    k_exp = reference.apply_rope(norm(heads[:, Hq:Hq + Hkv], kw), pos, cs)
    v_exp = heads[:, Hq + Hkv:]
    torch.testing.assert_close(q.float(), q_exp, atol=2e-2, rtol=2 ** -7)  # q is rounded to bf16
    tol = dict(atol=2e-2, rtol=0.13) if kv == torch.uint8 else dict(atol=2e-2, rtol=2 ** -7)
    kf, vf = reference.kv_float(kc), reference.kv_float(vc)
    for t in range(M):
        s, p = int(slot[t]), int(pos[t])
        if s < 0:
            continue
        torch.testing.assert_close(kf[s, :, p], k_exp[t], **tol)
        torch.testing.assert_close(vf[s, :, p], v_exp[t], **tol)  # v: the projection, no norm
    written = torch.zeros(S, MAXS, dtype=torch.bool)
    written[slot[slot >= 0].long(), pos[slot >= 0].long()] = True
    keep = ~written[:, None, :, None].expand_as(kc)
    assert torch.equal(kc[keep], k0[keep]) and torch.equal(vc[keep], k0[keep]) and int(written.sum()) == 4
    # the norm matters, a q / k weight swap shows, and None is the call without the keyword
    q_none = call(qk_norm=None)
    assert torch.equal(q_none, call())
    assert (q_none.float() - q.float()).abs().max() > 1.0
    assert (call(qk_norm=(kw, qw, neps)).float() - q.float()).abs().max() > 1.0
