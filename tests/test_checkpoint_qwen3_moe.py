"""Qwen3-MoE checkpoints (``model_type: qwen3_moe``): the routed expert MLP
against ``transformers``, as tests/test_checkpoint_qwen3.py does for the dense
Qwen3 model.

The oracle is fp32 ``Qwen3MoeForCausalLM`` loaded from the directory the
loader reads (hub layout: ``mlp.gate.weight``, ``mlp.experts.{e}.*``).  Each
case may show at most 2x the error of the dense Qwen3 model of the same
geometry, measured in the same run (the project's rule for a loaded
architecture); what a loader that ignored ``norm_topk_prob`` or put every
expert one place further would compute must exceed 100x.

Measured (CPU, fp32; 1 - cosine, max |diff| / max |logit| of the last-position
logits; worst of four 200-token prompts at positions [0, 200) and [800, 1000));
the figures are printed by the tests.
"""
import json
import os
import shutil

import pytest
import torch

transformers = pytest.importorskip("transformers")

from dmcp.config import Config  # noqa: E402
from dmcp.enrich.backend import LazyBackend, RefusedBackend, create_backend  # noqa: E402
from dmcp.models.llm import CheckpointUnsupported, LocalLM, check_checkpoint, preset  # noqa: E402
from dmcp.utils import synth  # noqa: E402
from tests.test_checkpoint_qwen3 import _edit_config, _rewrite, _unit_norms  # noqa: E402

TINY = dict(layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(),
            device="cpu")
# name -> (writer keywords, dense baseline)
CASES = {
    "moe_hd64_e8k2": (dict(head_dim=64, n_experts=8, experts_per_tok=2, moe_intermediate=128), "dense_hd64"),
    "moe_hd128_e16k4": (dict(head_dim=128, n_experts=16, experts_per_tok=4, moe_intermediate=64), "dense_hd128"),
    "moe_no_renorm": (dict(head_dim=64, n_experts=8, experts_per_tok=2, moe_intermediate=128, norm_topk=False),
                      "dense_hd64"),
    "moe_tied": (dict(head_dim=64, n_experts=8, experts_per_tok=2, moe_intermediate=128, tie_embeddings=True,
                      experts_key="num_local_experts"), "dense_hd64"),
}
DENSE = {"dense_hd64": dict(head_dim=64), "dense_hd128": dict(head_dim=128)}


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    root = tmp_path_factory.mktemp("qwen3moe")
    out = {}
    for name, kw in DENSE.items():
        out[name] = synth.llama_checkpoint(os.path.join(str(root), name), **TINY, qk_norm=True, model_type="qwen3", **kw)
    for name, (kw, _) in CASES.items():
        out[name] = synth.qwen3_moe_checkpoint(os.path.join(str(root), name), **TINY, **kw)
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
            moe = json.load(f)["model_type"] == "qwen3_moe"
        cls = transformers.Qwen3MoeForCausalLM if moe else transformers.Qwen3ForCausalLM
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


def _rotate_experts(t):
    """Expert e's three matrices move to expert e + 1 (the router stays)."""
    names = sorted(k for k in t if ".mlp.experts." in k)
    n = 1 + max(int(k.split(".experts.")[1].split(".")[0]) for k in names)
    old = {k: t[k] for k in names}
    for k in names:
        head, rest = k.split(".experts.")
        e, tail = rest.split(".", 1)
        t[f"{head}.experts.{(int(e) + 1) % n}.{tail}"] = old[k]


@pytest.mark.parametrize("case", sorted(CASES))
def test_qwen3_moe_parity_with_transformers(ckpts, prompts, baselines, case, tmp_path):
    kw, dense = CASES[case]
    base = baselines[dense]
    d = ckpts[case]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    c = m.cfg
    assert m.moe and m.has_qk_norm and (c.n_experts, c.experts_per_tok, c.moe_intermediate, c.norm_topk) == \
        (kw["n_experts"], kw["experts_per_tok"], kw["moe_intermediate"], kw.get("norm_topk", True))
    assert m.w["l1.we_gu"].shape == (c.n_experts, 2 * c.moe_intermediate, 256) and "l1.wgu" not in m.w
    e = _errors(d, d, prompts)
    print(f"{case}: 1-cos {e[0]:.3e} ({e[0] / base[0]:.2f}x)  maxabs/max {e[1]:.3e} ({e[1] / base[1]:.2f}x)")
    stripped = {}
    for what in ("renorm_ignored", "experts_rotated"):
        old = shutil.copytree(d, str(tmp_path / what))
        if what == "renorm_ignored":
            _edit_config(old, norm_topk_prob=not kw.get("norm_topk", True))
        else:
            _rewrite(old, _rotate_experts)
        assert check_checkpoint(old) is None
        s = stripped[what] = _errors(old, d, prompts)
        print(f"{case} {what}: 1-cos {s[0]:.3e} ({s[0] / base[0]:.1f}x)  maxabs/max {s[1]:.3e} "
              f"({s[1] / base[1]:.1f}x)")
    assert e[0] <= 2 * base[0] and e[1] <= 2 * base[1], (case, e, base)
    for what, s in stripped.items():
        assert s[0] > 100 * base[0] and s[1] > 100 * base[1], (case, what, s, base)


def test_loaded_expert_layout(ckpts):
    from safetensors.torch import load_file
    d = ckpts["moe_hd64_e8k2"]
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    raw = load_file(os.path.join(d, "model.safetensors"))
    for i in range(2):
        p = f"model.layers.{i}.mlp."
        assert torch.equal(m.w[f"l{i}.router"], raw[p + "gate.weight"])
        for e in (0, 3, 7):
            assert torch.equal(m.w[f"l{i}.we_gu"][e, :128], raw[f"{p}experts.{e}.gate_proj.weight"])
            assert torch.equal(m.w[f"l{i}.we_gu"][e, 128:], raw[f"{p}experts.{e}.up_proj.weight"])
            assert torch.equal(m.w[f"l{i}.we_down"][e], raw[f"{p}experts.{e}.down_proj.weight"])
        assert m.w[f"l{i}.we_gu"].dtype == torch.bfloat16 and m.w[f"l{i}.we_gu"].is_contiguous()
    with open(os.path.join(ckpts["moe_tied"], "config.json")) as f:
        cfg = json.load(f)
    assert "num_experts" not in cfg and cfg["num_local_experts"] == 8


def test_wellformed_is_accepted(ckpts):
    for name in CASES:
        assert check_checkpoint(ckpts[name]) is None, name
    be = create_backend(Config(enrich_backend="local", local_llm_model_path=ckpts["moe_hd64_e8k2"]))
    assert isinstance(be, LazyBackend) and be.enabled and not be.built


P1 = "model.layers.1.mlp."
REFUSALS = {
    "mlp_only_layers": (dict(mlp_only_layers=[0]), None, "mlp_only_layers"),
    "sparse_step": (dict(decoder_sparse_step=2), None, "decoder_sparse_step"),
    "shared_expert": ({}, lambda t: t.__setitem__(P1 + "shared_expert.gate_proj.weight",
                                                  torch.ones(128, 256, dtype=torch.bfloat16)),
                      P1 + "shared_expert.gate_proj.weight"),
    "shared_expert_gate": ({}, lambda t: t.__setitem__(P1 + "shared_expert_gate.weight",
                                                       torch.ones(1, 256, dtype=torch.bfloat16)),
                           P1 + "shared_expert_gate.weight"),
    "missing_expert": ({}, lambda t: t.pop(P1 + "experts.5.up_proj.weight"), P1 + "experts.5.up_proj.weight"),
    "missing_router": ({}, lambda t: t.pop(P1 + "gate.weight"), P1 + "gate.weight"),
    "geometry": (dict(moe_intermediate_size=96), None, "moe_intermediate_size"),
    "too_many_experts": (dict(num_experts=300), None, "num_experts"),
    "k_over_e": (dict(num_experts_per_tok=9), None, "num_experts_per_tok"),
    "no_expert_count": (dict(num_experts=None), None, "num_experts"),
    "expert_shape": ({}, lambda t: t.__setitem__(P1 + "experts.2.down_proj.weight",
                                                 torch.ones(256, 64, dtype=torch.bfloat16)),
                     P1 + "experts.2.down_proj.weight"),
    "router_shape": ({}, lambda t: t.__setitem__(P1 + "gate.weight", torch.ones(4, 256, dtype=torch.bfloat16)),
                     P1 + "gate.weight"),
    "qwen2_moe": (dict(model_type="qwen2_moe", architectures=["Qwen2MoeForCausalLM"]), None, "model_type"),
    "mixtral": (dict(model_type="mixtral", architectures=["MixtralForCausalLM"]), None, "model_type"),
    "dense_arch": (dict(architectures=["Qwen3ForCausalLM"]), None, "architectures"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_malformed_moe_checkpoints_are_refused_with_the_key(ckpts, tmp_path, name):
    cfg_edit, tensor_edit, needle = REFUSALS[name]
    d = shutil.copytree(ckpts["moe_hd64_e8k2"], str(tmp_path / "ck"))
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


def test_a_wrong_expert_shape_is_named_with_the_config_keys(ckpts, tmp_path):
    d = shutil.copytree(ckpts["moe_hd64_e8k2"], str(tmp_path / "ck"))
    _rewrite(d, REFUSALS["expert_shape"][1])
    reason = check_checkpoint(d)
    assert "[256, 64]" in reason and "[256, 128]" in reason and "moe_intermediate_size" in reason, reason


def test_the_mapped_files_are_closed_after_the_load(ckpts, monkeypatch):
    """The routed model reads its tensors one at a time from the mapped
    files; they are closed when the load returns, and when it fails."""
    from dmcp.models import llm
    seen = []

    class Spy(llm._LazyTensors):
        def __init__(self, files):
            super().__init__(files)
            seen.append(self)

    monkeypatch.setattr(llm, "_LazyTensors", Spy)
    LocalLM.load_safetensors(ckpts["moe_hd64_e8k2"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert len(seen) == 1 and "model.norm.weight" not in seen[0]
    with pytest.raises(KeyError):
        seen[0]["model.norm.weight"]
    with llm._LazyTensors([os.path.join(ckpts["moe_hd64_e8k2"], "model.safetensors")]) as raw:
        assert "model.norm.weight" in raw and raw["model.norm.weight"].shape == (256,)
    assert "model.norm.weight" not in raw


def test_worker_witness_names_the_routed_mlp(ckpts):
    """moe=<experts>x<per token> for a routed model, no such key for a dense one."""
    from dmcp.enrich.workers import _witness
    moe = LocalLM.load_safetensors(ckpts["moe_hd128_e16k4"], device="cpu", max_seq=64, max_batch=1, max_rows=1)
    assert _witness("cpu", moe)["moe"] == "16x4"
    assert "moe" not in _witness("cpu", LocalLM(preset("tiny", max_batch=1, max_seq=64, max_rows=1), device="cpu"))
    assert "moe" not in _witness("cpu")


@pytest.mark.parametrize("knob", ["prefill_dtype", "decode_dtype"])
def test_fp8_gemms_with_a_moe_model_are_refused_by_name(ckpts, knob):
    with pytest.raises(ValueError) as e:
        LocalLM.load_safetensors(ckpts["moe_hd64_e8k2"], device="cpu", max_seq=64, max_batch=1, max_rows=1,
                                 **{knob: "fp8"})
    # (a Qwen3-MoE checkpoint also has q/k norms, whose rule fires first; the routed MLP's own message is
    # tests/test_hip_dry_launch_moe.py::test_a_moe_preset_runs_the_op_on_every_path's)
    assert knob in str(e.value) and not isinstance(e.value, CheckpointUnsupported)
    m = LocalLM.load_safetensors(ckpts["moe_hd64_e8k2"], device="cpu", max_seq=64, max_batch=1, max_rows=1,
                                 prefill_dtype="auto")
    assert not m.prefill_fp8 and m.cfg.prefill_dtype == "bf16"


def test_bf16_forward_paths_agree_with_the_fp32_model(ckpts):
    """forward_tokens, prefill_batch and decode on the CPU (the reference ops) against reference_logits."""
    m = LocalLM.load_safetensors(ckpts["moe_hd64_e8k2"], device="cpu", max_seq=64, max_batch=2, max_rows=2)
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
