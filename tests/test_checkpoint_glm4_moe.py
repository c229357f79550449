"""GLM-4.5 checkpoints (``model_type: glm4_moe``): the sigmoid router with its
selection bias and scaling factor, shared experts, leading dense layers and
the partial rotary embedding against ``transformers``, as
tests/test_checkpoint_qwen3_moe.py does for Qwen3-MoE.

The oracle is fp32 ``Glm4MoeForCausalLM`` loaded from the directory the loader
reads (hub layout: ``mlp.gate.weight``, ``mlp.gate.e_score_correction_bias``,
``mlp.experts.{e}.*``, ``mlp.shared_experts.*``).  Each case may show at most
2x the error of a dense checkpoint of the same geometry that the project
already loads, measured in the same run -- Qwen2 (q/k/v biases) for the biased
cases, Qwen3 where ``use_qk_norm`` -- and what a loader that ignored the bias,
the scaling factor, the shared experts, their slice order or the partial
rotary factor, or put every expert one place further, would compute must
exceed 100x.

Measured (CPU, fp32; 1 - cosine, max |diff| / max |logit| of the last-position
logits; worst of four 200-token prompts at positions [0, 200) and [800, 1000));
the figures are printed by the tests and copied to docs/PARITY.md.
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
from dmcp.utils import synth  # noqa: E402
from tests.test_checkpoint_qwen3 import _edit_config, _rewrite, _unit_norms  # noqa: E402
from tests.test_checkpoint_qwen3_moe import _rotate_experts  # noqa: E402

TINY = dict(layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(),
            device="cpu")
E8 = dict(n_experts=8, experts_per_tok=2, moe_intermediate=128)
# name -> (writer keywords, dense baseline, the wrong loaders to show)
CASES = {
    "glm_hd64_e8k2_s1_lead1": (dict(head_dim=64, **E8, n_shared=1, dense_lead=1), "qwen2_hd64",
                               # (its one routed layer is the last: only the four last-position rows'
                               # routing reaches the logits, too few for the bias to show; the cases
                               # whose first layer is routed show it)
                               ("scale_ignored", "shared_dropped", "rotary_ignored", "experts_rotated")),
    "glm_hd128_e16k4_s2_lead0": (dict(head_dim=128, n_experts=16, experts_per_tok=4, moe_intermediate=64, n_shared=2,
                                      dense_lead=0), "qwen2_hd128",
                                 ("bias_ignored", "shared_dropped", "shared_swapped", "rotary_ignored",
                                  "experts_rotated")),
    "glm_no_renorm": (dict(head_dim=64, **E8, norm_topk=False), "qwen2_hd64", ("renorm_ignored",)),
    "glm_scale_2p5": (dict(head_dim=64, **E8, route_scale=2.5), "qwen2_hd64", ("scale_ignored",)),
    "glm_full_rotary": (dict(head_dim=64, **E8, partial_rotary=1.0), "qwen2_hd64", ("rotary_ignored",)),
    "glm_rotary_in_rope_parameters": (dict(head_dim=64, **E8, rotary_in_rope_parameters=True), "qwen2_hd64", ()),
    "glm_rotary_default": (dict(head_dim=64, **E8, partial_rotary=None), "qwen2_hd64", ()),
    "glm_qk_norm": (dict(head_dim=64, **E8, qk_norm=True, qkv_bias=False), "qwen3_hd64", ("rotary_ignored",)),
    "glm_mtp_layer": (dict(head_dim=64, **E8, mtp_layers=1), "qwen2_hd64", ()),
    "glm_s0_lead0": (dict(head_dim=64, **E8, n_shared=0, dense_lead=0), "qwen2_hd64",
                     ("bias_ignored", "experts_rotated")),
}
DENSE = {"qwen2_hd64": dict(head_dim=64, qkv_bias=True, model_type="qwen2"),
         "qwen2_hd128": dict(head_dim=128, qkv_bias=True, model_type="qwen2"),
         "qwen3_hd64": dict(head_dim=64, qk_norm=True, model_type="qwen3")}
BASE = "glm_hd64_e8k2_s1_lead1"


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("glm4moe")
    out = {}
    for name, kw in DENSE.items():
        out[name] = synth.llama_checkpoint(os.path.join(str(root), name), **TINY, **kw)
    for name, (kw, _, _) in CASES.items():
        out[name] = synth.glm4_moe_checkpoint(os.path.join(str(root), name), **TINY, **kw)
    for d in out.values():
        _rewrite(d, _unit_norms)
    return out


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 512, (200,), generator=g).tolist() for _ in range(4)]


_HF = {}


def _hf_logits(path, prompts):
    if path not in _HF:
        with open(os.path.join(path, "config.json")) as f:
            mt = json.load(f)["model_type"]
        cls = {"glm4_moe": transformers.Glm4MoeForCausalLM, "qwen2": transformers.Qwen2ForCausalLM,
               "qwen3": transformers.Qwen3ForCausalLM}[mt]
        m = cls.from_pretrained(path, dtype=torch.float32).eval()
        out = {}
        with torch.no_grad():
            for i, p in enumerate(prompts):
                for start in (0, 800):
                    pos = torch.arange(start, start + len(p))[None]
                    out[i, start] = m(input_ids=torch.tensor([p]), position_ids=pos).logits[0, -1].float()
        _HF[path] = out
    return _HF[path]


def _errors(local_dir, hf_dir, prompts):
    m = LocalLM.load_safetensors(local_dir, device="cpu", max_seq=1024, max_batch=1, max_rows=1)
    e_cos = e_abs = 0.0
    for (i, start), exp in _hf_logits(hf_dir, prompts).items():
        got = m.reference_logits(prompts[i], start_pos=start)[-1].double()
        e = exp.double()
        e_cos = max(e_cos, 1.0 - torch.nn.functional.cosine_similarity(got, e, dim=0).item())
        e_abs = max(e_abs, ((got - e).abs().max() / e.abs().max()).item())
    return e_cos, e_abs


@pytest.fixture(scope="module")
def baselines(ckpts, prompts):
    out = {}
    for name in DENSE:
        b = out[name] = _errors(ckpts[name], ckpts[name], prompts)
        print(f"baseline {name}: 1-cos {b[0]:.3e}  maxabs/max {b[1]:.3e}")
        assert b[0] < 1e-6 and b[1] < 1e-3, b
    return out


def _zero(suffix):
    def fn(t):
        for k in t:
            if k.endswith(suffix):
                t[k] = torch.zeros_like(t[k])
    return fn


def _swap_shared_down(t):
    """The down projection's two slices change places, gate and up stay: what a
    loader that paired slice s of gate / up with another slice of down computes."""
    for k in t:
        if k.endswith("shared_experts.down_proj.weight"):
            half = t[k].shape[1] // 2
            t[k] = torch.cat([t[k][:, half:], t[k][:, :half]], 1).contiguous()


def _wrong_loader(what, d, kw):
    """Turns the copy ``d`` into the checkpoint a loader with that mistake would have read."""
    if what == "bias_ignored":
        _rewrite(d, _zero("e_score_correction_bias"))
    elif what == "scale_ignored":  # any other factor: the case's own, or 2.5 where that is 1
        _edit_config(d, routed_scaling_factor=1.0 if kw.get("route_scale", 1.0) != 1.0 else 2.5)
    elif what == "renorm_ignored":
        _edit_config(d, norm_topk_prob=not kw.get("norm_topk", True))
    elif what == "shared_dropped":
        _rewrite(d, _zero("shared_experts.down_proj.weight"))
    elif what == "shared_swapped":
        _rewrite(d, _swap_shared_down)
    elif what == "rotary_ignored":  # the other rotary width
        _edit_config(d, partial_rotary_factor=1.0 if kw.get("partial_rotary", 0.5) != 1.0 else 0.5)
    elif what == "experts_rotated":
        _rewrite(d, _rotate_experts)
    else:
        raise AssertionError(what)


@pytest.mark.parametrize("case", sorted(CASES))
def test_glm4_moe_parity_with_transformers(ckpts, prompts, baselines, case, tmp_path):
    kw, dense, wrong = CASES[case]
    base = baselines[dense]
    d = ckpts[case]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    c = m.cfg
    S, lead = kw.get("n_shared", 1), kw.get("dense_lead", 1)
    pr = kw.get("partial_rotary", 0.5) or 0.5
    assert m.moe and m.moe_sig and c.layers == 2 and m.has_qk_norm == kw.get("qk_norm", False)
    assert (c.n_experts, c.experts_per_tok, c.moe_intermediate, c.norm_topk, c.moe_score, c.moe_route_scale,
            c.moe_shared, c.dense_lead, c.rotary_dim) == \
        (kw["n_experts"], kw["experts_per_tok"], kw["moe_intermediate"], kw.get("norm_topk", True), "sigmoid",
         kw.get("route_scale", 1.0), S, lead, 0 if pr == 1.0 else int(c.head_dim * pr))
    assert m.w["l1.we_gu"].shape == (c.n_experts + S, 2 * c.moe_intermediate, 256) and "l1.wgu" not in m.w
    assert m.w["l1.router_bias"].dtype == torch.float32 and not any(k.startswith("l2.") for k in m.w)
    assert ("l0.wgu" in m.w) == (lead == 1) and ("l0.router" in m.w) == (lead == 0)
    e = _errors(d, d, prompts)
    print(f"{case}: 1-cos {e[0]:.3e} ({e[0] / base[0]:.2f}x)  maxabs/max {e[1]:.3e} ({e[1] / base[1]:.2f}x)")
    stripped = {}
    for what in wrong:
        old = shutil.copytree(d, str(tmp_path / what))
        _wrong_loader(what, old, kw)
        assert check_checkpoint(old) is None
        s = stripped[what] = _errors(old, d, prompts)
        print(f"{case} {what}: 1-cos {s[0]:.3e} ({s[0] / base[0]:.1f}x)  maxabs/max {s[1]:.3e} "
              f"({s[1] / base[1]:.1f}x)")
    assert e[0] <= 2 * base[0] and e[1] <= 2 * base[1], (case, e, base)
    for what, s in stripped.items():
        assert s[0] > 100 * base[0] and s[1] > 100 * base[1], (case, what, s, base)


def test_the_synthetic_bias_changes_selections(ckpts):
    """The writer's correction bias is large enough to matter: on the rows of a
    prompt, the chosen set differs from the unbiased one on a quarter or more."""
    from dmcp.ops import reference
    m = LocalLM.load_safetensors(ckpts[BASE], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    g = torch.Generator().manual_seed(3)
    h = torch.randn(400, 256, generator=g)
    wr, b = m.w["l1.router"].float(), m.w["l1.router_bias"]
    a = reference.moe_route_sig_math(h, wr, b, 2, True)[0].sort(1).values
    z = reference.moe_route_sig_math(h, wr, torch.zeros_like(b), 2, True)[0].sort(1).values
    assert (a != z).any(1).float().mean().item() >= 0.25


def test_loaded_layout(ckpts):
    """Router bias in fp32, the shared slices behind the routed experts, the
    dense lead layer's MLP, and q / k rows in the whole-head rotation's order."""
    from safetensors.torch import load_file
    from dmcp.ops import reference
    d = ckpts["glm_hd128_e16k4_s2_lead0"]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(d, "model.safetensors"))
    E, inter, S, D = 16, 64, 2, 128
    perm = reference.partial_rotary_perm(D, 64)
    for i in range(2):
        p = f"model.layers.{i}.mlp."
        assert torch.equal(m.w[f"l{i}.router"], raw[p + "gate.weight"])
        assert torch.equal(m.w[f"l{i}.router_bias"], raw[p + "gate.e_score_correction_bias"])
        for e in (0, 7, 15):
            assert torch.equal(m.w[f"l{i}.we_gu"][e, :inter], raw[f"{p}experts.{e}.gate_proj.weight"])
            assert torch.equal(m.w[f"l{i}.we_gu"][e, inter:], raw[f"{p}experts.{e}.up_proj.weight"])
            assert torch.equal(m.w[f"l{i}.we_down"][e], raw[f"{p}experts.{e}.down_proj.weight"])
        for s in range(S):
            sl = slice(s * inter, (s + 1) * inter)
            assert torch.equal(m.w[f"l{i}.we_gu"][E + s, :inter], raw[p + "shared_experts.gate_proj.weight"][sl])
            assert torch.equal(m.w[f"l{i}.we_gu"][E + s, inter:], raw[p + "shared_experts.up_proj.weight"][sl])
            assert torch.equal(m.w[f"l{i}.we_down"][E + s], raw[p + "shared_experts.down_proj.weight"][:, sl])
        assert m.w[f"l{i}.we_gu"].is_contiguous() and m.w[f"l{i}.we_down"].is_contiguous()
        a = f"model.layers.{i}.self_attn."
        q = raw[a + "q_proj.weight"].view(4, D, 256)[:, perm].reshape(4 * D, 256)
        k = raw[a + "k_proj.weight"].view(2, D, 256)[:, perm].reshape(2 * D, 256)
        assert torch.equal(m.w[f"l{i}.wqkv"], torch.cat([q, k, raw[a + "v_proj.weight"]], 0))
        bq = raw[a + "q_proj.bias"].view(4, D)[:, perm].reshape(-1)
        bk = raw[a + "k_proj.bias"].view(2, D)[:, perm].reshape(-1)
        assert torch.equal(m.w[f"l{i}.bqkv"], torch.cat([bq, bk, raw[a + "v_proj.bias"]], 0))
    assert bool((m.cos_sin[:, 32:, 0] == 1).all()) and bool((m.cos_sin[:, 32:, 1] == 0).all())
    n = LocalLM.load_safetensors(ckpts["glm_qk_norm"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(ckpts["glm_qk_norm"], "model.safetensors"))
    p64 = reference.partial_rotary_perm(64, 32)
    assert torch.equal(n.w["l1.qnorm"], raw["model.layers.1.self_attn.q_norm.weight"][p64])
    assert torch.equal(n.w["l1.knorm"], raw["model.layers.1.self_attn.k_norm.weight"][p64])
    lead = LocalLM.load_safetensors(ckpts[BASE], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(ckpts[BASE], "model.safetensors"))
    assert torch.equal(lead.w["l0.wgu"], torch.cat([raw["model.layers.0.mlp.gate_proj.weight"],
                                                    raw["model.layers.0.mlp.up_proj.weight"]], 0))


def test_wellformed_is_accepted(ckpts):
    for name in CASES:
        assert check_checkpoint(ckpts[name]) is None, name
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=ckpts[BASE]))
    assert isinstance(be, LazyBackend) and be.enabled and not be.built


P1 = "model.layers.1.mlp."
BIAS = P1 + "gate.e_score_correction_bias"
SH = P1 + "shared_experts."


def _pop_shared(t):
    for n in ("gate_proj", "up_proj", "down_proj"):
        t.pop(f"{SH}{n}.weight")


REFUSALS = {
    "n_group": (dict(n_group=2), None, "n_group"),
    "topk_group": (dict(topk_group=2), None, "topk_group"),
    "quantization_config": (dict(quantization_config={"quant_method": "fp8", "fmt": "e4m3",
                                                      "activation_scheme": "dynamic",
                                                      "weight_block_size": [128, 128]}), None, "quantization_config"),
    "missing_bias": ({}, lambda t: t.pop(BIAS), BIAS),
    "bias_shape": ({}, lambda t: t.__setitem__(BIAS, torch.zeros(4)), BIAS),
    "missing_shared": ({}, lambda t: t.pop(SH + "up_proj.weight"), SH + "up_proj.weight"),
    "shared_without_tensors": ({}, _pop_shared, SH + "down_proj.weight"),
    "tensors_without_shared": (dict(n_shared_experts=0), None, SH),
    "shared_width": (dict(n_shared_experts=2), None, SH + "down_proj.weight"),
    "shared_shape": ({}, lambda t: t.__setitem__(SH + "gate_proj.weight", torch.ones(128, 128, dtype=torch.bfloat16)),
                     SH + "gate_proj.weight"),
    "geometry": (dict(moe_intermediate_size=96), None, "moe_intermediate_size"),
    "too_many_experts": (dict(n_routed_experts=256), None, "n_routed_experts"),
    "k_over_e": (dict(num_experts_per_tok=9), None, "num_experts_per_tok"),
    "no_expert_count": (dict(n_routed_experts=None), None, "n_routed_experts"),
    "dense_lead_range": (dict(first_k_dense_replace=3), None, "first_k_dense_replace"),
    "dense_lead_mismatch": (dict(first_k_dense_replace=0), None, "model.layers.0.mlp."),
    "scale_zero": (dict(routed_scaling_factor=0.0), None, "routed_scaling_factor"),
    "rotary_odd": (dict(partial_rotary_factor=0.3), None, "partial_rotary_factor"),
    "rotary_over": (dict(partial_rotary_factor=1.5), None, "partial_rotary_factor"),
    "qk_norm_without_tensors": (dict(use_qk_norm=True), None, "_norm.weight"),
    "missing_expert": ({}, lambda t: t.pop(P1 + "experts.5.up_proj.weight"), P1 + "experts.5.up_proj.weight"),
    "stray_layer": ({}, lambda t: t.__setitem__("model.layers.2.eh_proj.weight", torch.ones(4, 4)),
                    "model.layers.2.eh_proj.weight"),
    "mtp_count": (dict(num_nextn_predict_layers=-1), None, "num_nextn_predict_layers"),
    "hidden_act": (dict(hidden_act="gelu"), None, "hidden_act"),
    "other_arch": (dict(architectures=["Qwen3MoeForCausalLM"]), None, "architectures"),
    "o_proj_bias": ({}, lambda t: t.__setitem__("model.layers.1.self_attn.o_proj.bias", torch.ones(256)),
                    "model.layers.1.self_attn.o_proj.bias"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_malformed_glm_checkpoints_are_refused_with_the_key(ckpts, tmp_path, name, monkeypatch):
    cfg_edit, tensor_edit, needle = REFUSALS[name]
    d = shutil.copytree(ckpts[BASE], str(tmp_path / "ck"))
    if cfg_edit:
        _edit_config(d, **cfg_edit)
    if tensor_edit:
        _rewrite(d, tensor_edit)
    reason = check_checkpoint(d)
    assert reason is not None and needle in reason, reason
    with pytest.raises(CheckpointUnsupported) as e:
        LocalLM.load_safetensors(d, device="cpu")
    assert needle in str(e.value)
    # refused at configuration time: a backend without workers, nothing to build
    import multiprocessing.context as mpc
    for ctx in (mpc.SpawnContext, mpc.ForkContext, mpc.ForkServerContext):
        monkeypatch.setattr(ctx, "Process", lambda *a, **k: pytest.fail("a worker process was started"))
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=d))
    assert isinstance(be, RefusedBackend) and not be.enabled
    assert needle in be.disabled_reason and "LOCAL_LLM_MODEL_PATH" in be.disabled_reason


def test_the_quantised_refusal_says_what_is_missing(ckpts, tmp_path):
    d = shutil.copytree(ckpts[BASE], str(tmp_path / "ck"))
    _edit_config(d, **REFUSALS["quantization_config"][0])
    assert "sigmoid router" in check_checkpoint(d) and "bf16" in check_checkpoint(d)


def test_an_appended_mtp_layer_is_skipped_and_only_that(ckpts, tmp_path):
    d = ckpts["glm_mtp_layer"]
    from safetensors.torch import load_file
    raw = load_file(os.path.join(d, "model.safetensors"))
    assert "model.layers.2.eh_proj.weight" in raw and "model.layers.2.mlp.experts.0.up_proj.weight" in raw
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert m.cfg.layers == 2
    # the same tensors without the config key are strays; so is a second extra layer
    a = shutil.copytree(d, str(tmp_path / "a"))
    _edit_config(a, num_nextn_predict_layers=0)
    assert "model.layers.2." in check_checkpoint(a) and "not consumed" in check_checkpoint(a)
    b = shutil.copytree(d, str(tmp_path / "b"))
    _rewrite(b, lambda t: t.__setitem__("model.layers.3.enorm.weight", torch.ones(256)))
    assert "model.layers.3.enorm.weight" in check_checkpoint(b)


def test_a_qwen3_moe_directory_with_shared_experts_stays_refused(tmp_path):
    d = synth.qwen3_moe_checkpoint(str(tmp_path / "q"), head_dim=64, **E8, **TINY)
    name = "model.layers.1.mlp.shared_expert.gate_proj.weight"
    _rewrite(d, lambda t: t.__setitem__(name, torch.ones(128, 256, dtype=torch.bfloat16)))
    reason = check_checkpoint(d)
    assert name in reason and "only Qwen3-MoE's routed experts are loaded" in reason
    _rewrite(d, lambda t: (t.pop(name), t.__setitem__("model.layers.1.mlp.shared_experts.gate_proj.weight",
                                                      torch.ones(128, 256, dtype=torch.bfloat16))))
    assert "shared_experts.gate_proj.weight" in check_checkpoint(d)


@pytest.mark.parametrize("knob", ["prefill_dtype", "decode_dtype"])
def test_fp8_gemms_with_a_glm_model_are_refused_by_name(ckpts, knob):
    with pytest.raises(ValueError) as e:
        LocalLM.load_safetensors(ckpts[BASE], device="cpu", max_seq=64, max_batch=1, max_rows=1, **{knob: "fp8"})
    assert knob in str(e.value) and not isinstance(e.value, CheckpointUnsupported)
    m = LocalLM.load_safetensors(ckpts[BASE], device="cpu", max_seq=64, max_batch=1, max_rows=1, prefill_dtype="auto")
    assert not m.prefill_fp8 and m.cfg.prefill_dtype == "bf16"


@pytest.mark.parametrize("case", [BASE, "glm_hd128_e16k4_s2_lead0", "glm_qk_norm"])
def test_bf16_forward_paths_agree_with_the_fp32_model(ckpts, case):
    """forward_tokens, prefill_batch and decode on the CPU (the reference ops) against reference_logits."""
    m = LocalLM.load_safetensors(ckpts[case], device="cpu", max_seq=64, max_batch=2, max_rows=2)
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
