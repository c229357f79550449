"""A written block-scaled FP8 Qwen3-MoE checkpoint through ``LocalLM`` on the
GPU: batched prefill and decode steps on the fused (4 rows), the
weight-streaming (40) and the large-tile (600) path against the fp32 CPU
forward over the dequantised weights, under the logit-cosine gates
tests/test_gpu_moe_model.py applies to the bf16 checkpoint (the arithmetic
differs only by exact weights and an fp32 scale); a chunked prefill against the
unchunked one; the captured step's kernel nodes against the bf16 routed
model's; the engine; the worker witness."""
import json

import pytest
import torch

from tests.test_gpu_moe_model import GEOM, MOE, ROWS
from tests.test_gpu_qk_norm import _check_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from dmcp.utils import synth
    return synth.qwen3_moe_checkpoint(str(tmp_path_factory.mktemp("moe_fp8") / "moe64"), head_dim=64, fp8=True,
                                      **GEOM, **MOE)


_REF = {}


def _reference(path):
    """fp32 logits of the CPU model (experts dequantised exactly) for three
    sequences: uneven prompts + the token stream each slot's decode rows append."""
    from dmcp.models.llm import LocalLM
    if path not in _REF:
        cpu = LocalLM.load_safetensors(path, device="cpu", max_seq=512, max_batch=1, max_rows=1)
        assert cpu.moe_w8
        g = torch.Generator().manual_seed(9)
        prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (37, 60, 91)]
        n_stream = sum(-(-r // 3) for r in ROWS)
        streams = [torch.randint(0, 512, (n_stream,), generator=g).tolist() for _ in range(3)]
        _REF[path] = prompts, streams, [cpu.reference_logits(p + s) for p, s in zip(prompts, streams)]
    return _REF[path]


@pytest.mark.parametrize("kv,bound", [("bf16", 0.999), ("fp8s", 0.99)])
def test_fp8_checkpoint_decodes_on_every_path(ckpt, kv, bound):
    from dmcp.models.llm import LocalLM
    prompts, streams, ref = _reference(ckpt)
    m = LocalLM.load_safetensors(ckpt, device="cuda", max_seq=512, max_batch=8, max_rows=600, kv_dtype=kv)
    assert m.use_fused and m.use_wgemm and m.use_tgemm and m.has_qk_norm and m.moe and m.moe_w8
    assert m.cfg.moe_weight_dtype == "fp8b" and m.moe_ws is not None
    assert m.w["l0.we_gu8"].dtype == torch.float8_e4m3fn and m.w["l0.we_gu8"].is_cuda and "l0.we_gu" not in m.w
    assert m.w["l0.wqkv"].dtype == torch.bfloat16
    got = m.prefill_batch([(p, s, 0) for s, p in enumerate(prompts)])
    _check_rows(got, torch.stack([ref[s][len(p) - 1] for s, p in enumerate(prompts)]), bound, f"moe fp8b prefill {kv}")
    done = [0, 0, 0]
    for rows in ROWS:
        sl = [r % 3 for r in range(rows)]
        off = [done[r % 3] + r // 3 for r in range(rows)]
        tk = torch.tensor([streams[s][j] for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        ps = torch.tensor([len(prompts[s]) + j for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        logits = m.decode(tk, torch.tensor(sl, dtype=torch.int32, device="cuda"), ps)
        exp = torch.stack([ref[s][len(prompts[s]) + j] for s, j in zip(sl, off)])
        _check_rows(logits, exp, bound, f"moe fp8b decode {rows} rows {kv}")
        for s in range(3):
            done[s] += sum(1 for x in sl if x == s)


def test_a_chunked_prefill_equals_the_unchunked_one(ckpt):
    """More rows than ``moe_rows`` walk the op in chunks; every output element
    keeps its summation order, so the logits are the same bits."""
    from dmcp.models.llm import LocalLM
    m = LocalLM.load_safetensors(ckpt, device="cuda", max_seq=512, max_batch=2, max_rows=16)
    toks = torch.randint(0, 512, (300,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    assert m.moe_rows >= 300
    whole = m.forward_tokens(toks, 0, 0).clone()
    m.moe_rows = 70  # four chunks of 70 and one of 20 on the GEMMs' 32-row tile; the whole prefill ran on the 128-row one
    chunked = m.forward_tokens(toks, 1, 0)
    assert torch.equal(whole, chunked)


def test_the_captured_step_has_the_bf16_routed_models_kernel_nodes():
    from dmcp.models.llm import DecodeGraphs, LocalLM, preset
    kw = dict(max_batch=8, max_seq=256, max_rows=16, **MOE)
    counts = {}
    for name in ("bf16", "fp8b"):
        m = LocalLM(preset("tiny", moe_weight_dtype=name, **kw), device="cuda")
        assert m.moe_w8 == (name == "fp8b")
        masks = torch.full((1, (m.cfg.vocab_size + 31) // 32), -1, dtype=torch.int32, device="cuda")
        g = DecodeGraphs(m, masks, buckets=(4,))
        g._capture(4)
        counts[name] = g.graphs[4].kernels
        layers = m.cfg.layers
    print("kernel nodes of the 4-row step:", counts)
    assert counts["bf16"] > 0, "the runtime reports no kernel nodes"
    assert counts["fp8b"] == counts["bf16"] == 3 + layers * (4 + 1 + 6)


def test_engine_and_witness_over_the_fp8_checkpoint(ckpt):
    from dmcp.enrich.local import LocalEngine
    from dmcp.enrich.types import EnrichmentInput
    from dmcp.enrich.workers import _witness
    from dmcp.models.llm import LocalLM
    m = LocalLM.load_safetensors(ckpt, device="cuda", max_seq=2048, max_batch=8, max_rows=16)
    wit = _witness("cuda:0", m)
    assert wit["moe_weights"] == "fp8b128" and wit["moe"] == "8x2" and wit["hipops_abi"] == 20, wit
    eng = LocalEngine(m)
    inputs = [EnrichmentInput("public class S%d { void a() {} void b() {} }" % i, f"co.x.S{i}", "java", "SERVICE",
                              ["a", "b", "c"][: 1 + i % 3]) for i in range(3)]
    raw = eng.generate(inputs, "A readme")
    for r, inp in zip(raw, inputs):
        doc = json.loads(r)
        assert [x["methodName"] for x in doc["methods"]] == inp.method_names
    assert eng.stats["prefills"] == 3 and eng.stats["decode_steps"] > 0
