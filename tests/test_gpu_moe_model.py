"""A written Qwen3-MoE checkpoint through ``LocalLM`` on the GPU: batched
prefill, then decode steps on the fused (4 rows), the weight-streaming (40)
and the large-tile (600) path, against the fp32 CPU model -- with the cosine
and top-1 gates tests/test_gpu_qk_norm.py applies to the dense Qwen3 model,
which is measured on the same prompts in the same run -- for bf16 and
per-row scaled fp8 KV; the engine over that checkpoint; and the dense
model's captured graphs, which must not have grown."""
import json

import pytest
import torch

from tests.test_gpu_qk_norm import _check_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

GEOM = dict(layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(7,),
            device="cpu")
MOE = dict(n_experts=8, experts_per_tok=2, moe_intermediate=128)
ROWS = (4, 40, 600)


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    from dmcp.utils import synth
    root = tmp_path_factory.mktemp("moe_tiny")
    out = {}
    for hd in (64, 128):
        out["moe", hd] = synth.qwen3_moe_checkpoint(str(root / f"moe{hd}"), head_dim=hd, **GEOM, **MOE)
        out["dense", hd] = synth.llama_checkpoint(str(root / f"dense{hd}"), head_dim=hd, qk_norm=True,
                                                  model_type="qwen3", **GEOM)
    return out


_REF = {}


def _reference(path):
    """fp32 logits of the CPU model for three sequences: uneven prompts + the
    token stream each slot's decode rows append (once per directory)."""
    from dmcp.models.llm import LocalLM
    if path not in _REF:
        cpu = LocalLM.load_safetensors(path, device="cpu", max_seq=512, max_batch=1, max_rows=1)
        g = torch.Generator().manual_seed(9)
        prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (37, 60, 91)]
        n_stream = sum(-(-r // 3) for r in ROWS)
        streams = [torch.randint(0, 512, (n_stream,), generator=g).tolist() for _ in range(3)]
        _REF[path] = prompts, streams, [cpu.reference_logits(p + s) for p, s in zip(prompts, streams)]
    return _REF[path]


def _run(path, kv, bound, what, moe):
    from dmcp.models.llm import LocalLM
    prompts, streams, ref = _reference(path)
    m = LocalLM.load_safetensors(path, device="cuda", max_seq=512, max_batch=8, max_rows=600, kv_dtype=kv)
    assert m.use_fused and m.use_wgemm and m.use_tgemm and m.has_qk_norm and m.moe == moe
    assert (m.moe_ws is not None) == moe
    got = m.prefill_batch([(p, s, 0) for s, p in enumerate(prompts)])
    _check_rows(got, torch.stack([ref[s][len(p) - 1] for s, p in enumerate(prompts)]), bound, f"{what} prefill {kv}")
    done = [0, 0, 0]  # stream tokens each slot has consumed
    for rows in ROWS:
        sl = [r % 3 for r in range(rows)]
        off = [done[r % 3] + r // 3 for r in range(rows)]
        tk = torch.tensor([streams[s][j] for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        ps = torch.tensor([len(prompts[s]) + j for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        logits = m.decode(tk, torch.tensor(sl, dtype=torch.int32, device="cuda"), ps)
        exp = torch.stack([ref[s][len(prompts[s]) + j] for s, j in zip(sl, off)])
        _check_rows(logits, exp, bound, f"{what} decode {rows} rows {kv}")
        for s in range(3):
            done[s] += sum(1 for x in sl if x == s)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kv,bound", [("bf16", 0.999), ("fp8s", 0.99)])
def test_moe_checkpoint_decodes_on_every_path(ckpts, hd, kv, bound):
    """The dense Qwen3 model of the same geometry first (the figures to read
    the routed model's against), then the routed one under the same gates."""
    _run(ckpts["dense", hd], kv, bound, f"dense hd{hd}", False)
    _run(ckpts["moe", hd], kv, bound, f"moe hd{hd}", True)


def test_engine_over_the_moe_checkpoint(ckpts):
    from dmcp.enrich.local import LocalEngine
    from dmcp.enrich.types import EnrichmentInput
    from dmcp.models.llm import LocalLM
    m = LocalLM.load_safetensors(ckpts["moe", 64], device="cuda", max_seq=2048, max_batch=8, max_rows=16)
    eng = LocalEngine(m)
    inputs = [EnrichmentInput("public class S%d { void a() {} void b() {} }" % i, f"co.x.S{i}", "java", "SERVICE",
                              ["a", "b", "c"][: 1 + i % 3]) for i in range(3)]
    raw = eng.generate(inputs, "A readme")
    for r, inp in zip(raw, inputs):
        doc = json.loads(r)
        assert [x["methodName"] for x in doc["methods"]] == inp.method_names
    assert eng.stats["prefills"] == 3 and eng.stats["decode_steps"] > 0


def test_dense_graphs_have_the_kernel_nodes_they_had():
    """A dense model allocates no routed-MLP workspace and captures none of
    its kernels.  Its 4-row step (``_decode_fused``, bf16 KV, shared prefix,
    one key split at max_seq 256) is, launch for launch: embed + first norm,
    then per layer QKV + RoPE + append, the prefix partials, the per-row
    attention (which also merges when there is one split), O + residual,
    gate/up + SwiGLU, down + residual, then the LM head and the masked
    arg-max -- 3 + 6 per layer, the count the step had before the routed MLP
    existed.  The routed model's step has the explicit norm and the op's six
    launches where the dense one has gate/up and down: five kernel nodes
    more per layer, and nothing else differs."""
    from dmcp.models.llm import DecodeGraphs, LocalLM, preset
    dense = LocalLM(preset("tiny", max_batch=8, max_seq=256, max_rows=16), device="cuda")
    assert dense.moe_ws is None and not dense.moe and dense.shared_prefix and dense.cfg.kv_dtype == "bf16"
    moe = LocalLM(preset("tiny", max_batch=8, max_seq=256, max_rows=16, **MOE), device="cuda")
    masks = torch.full((1, (dense.cfg.vocab_size + 31) // 32), -1, dtype=torch.int32, device="cuda")
    counts = {}
    for name, m in (("dense", dense), ("moe", moe)):
        g = DecodeGraphs(m, masks, buckets=(4,))
        g._capture(4)
        counts[name] = g.graphs[4].kernels
    print("kernel nodes of the 4-row step:", counts)
    layers = dense.cfg.layers
    assert counts["dense"] > 0 and counts["moe"] > 0, "the runtime reports no kernel nodes"
    assert counts["dense"] == 3 + layers * 6
    assert counts["moe"] == 3 + layers * (4 + 1 + 6)
