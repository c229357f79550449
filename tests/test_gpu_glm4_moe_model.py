"""A written GLM-4.5 checkpoint through ``LocalLM`` on the GPU, as
tests/test_gpu_moe_model.py does for Qwen3-MoE: three layers (one dense lead,
two routed), 8 experts, 2 per token, one shared expert, partial rotary 0.5,
q/k/v biases, bf16 KV -- batched prefill, then decode steps on the fused (4
rows), the weight-streaming (40) and the large-tile (600) path, against the
fp32 CPU model under the gates that file asserts for Qwen3-MoE at those row
counts (cosine 0.999 for bf16 KV, top-1 on every decisive row).  The Qwen3-MoE
model of the same three-layer geometry is measured on the same prompts in the
same run and printed, the figures to read this model's against."""
import pytest
import torch

from tests.test_gpu_moe_model import ROWS, _reference
from tests.test_gpu_qk_norm import _check_rows

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

GEOM = dict(layers=3, hidden=256, heads=4, kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(7,),
            device="cpu")
MOE = dict(n_experts=8, experts_per_tok=2, moe_intermediate=128)
BOUND = 0.999  # tests/test_gpu_moe_model.py's gate for bf16 KV


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    from dmcp.utils import synth
    root = tmp_path_factory.mktemp("glm_tiny")
    return {"glm": synth.glm4_moe_checkpoint(str(root / "glm"), head_dim=64, n_shared=1, dense_lead=1,
                                             partial_rotary=0.5, qkv_bias=True, route_scale=2.5, **GEOM, **MOE),
            "qwen3_moe": synth.qwen3_moe_checkpoint(str(root / "q3moe"), head_dim=64, **GEOM, **MOE)}


def _paths(m, prompts, streams, ref):
    """(what, logits, fp32 logits) of the batched prefill, then of decode steps
    of 4 (fused), 40 (weight-streaming, 32-row MoE tile) and 600 rows (large
    tile, 128-row MoE tile), as tests/test_gpu_moe_model.py walks them."""
    got = m.prefill_batch([(p, s, 0) for s, p in enumerate(prompts)])
    yield "prefill", got, torch.stack([ref[s][len(p) - 1] for s, p in enumerate(prompts)])
    done = [0, 0, 0]  # stream tokens each slot has consumed
    for rows in ROWS:
        sl = [r % 3 for r in range(rows)]
        off = [done[r % 3] + r // 3 for r in range(rows)]
        tk = torch.tensor([streams[s][j] for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        ps = torch.tensor([len(prompts[s]) + j for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        logits = m.decode(tk, torch.tensor(sl, dtype=torch.int32, device="cuda"), ps)
        yield f"decode {rows} rows", logits, torch.stack([ref[s][len(prompts[s]) + j] for s, j in zip(sl, off)])
        for s in range(3):
            done[s] += sum(1 for x in sl if x == s)


def test_glm_checkpoint_decodes_on_every_path(ckpts):
    from dmcp.models.llm import LocalLM
    from dmcp.ops import hip
    # the Qwen3-MoE model of the same three-layer geometry: measured and printed, the figures to read the
    # GLM model's against (its own gates are tests/test_gpu_moe_model.py's, at that file's geometry)
    q = LocalLM.load_safetensors(ckpts["qwen3_moe"], device="cuda", max_seq=512, max_batch=8, max_rows=600)
    for what, got, exp in _paths(q, *_reference(ckpts["qwen3_moe"])):
        cos = torch.nn.functional.cosine_similarity(got.float().cpu(), exp.float().cpu(), dim=-1)
        print(f"qwen3-moe (3 layers) {what} bf16: min cosine {cos.min().item():.5f}, rows below {BOUND}: "
              f"{int((cos < BOUND).sum())}/{len(cos)}")
    del q
    path = ckpts["glm"]
    m = LocalLM.load_safetensors(path, device="cuda", max_seq=512, max_batch=8, max_rows=600, kv_dtype="bf16")
    c = m.cfg
    assert m.moe and m.moe_sig and m.has_bias and not m.has_qk_norm and m.moe_ws is not None
    assert (c.dense_lead, c.moe_shared, c.rotary_dim, c.moe_route_scale, c.layers) == (1, 1, 32, 2.5, 3)
    assert m.use_fused and m.use_wgemm and m.use_tgemm
    assert "l0.wgu" in m.w and m.w["l1.we_gu"].shape == (9, 256, 256)
    assert {hip.moe_row_tile(r, 9, 3) for r in ROWS} == {32, 128}
    for what, got, exp in _paths(m, *_reference(path)):
        _check_rows(got, exp, BOUND, f"glm {what} bf16")


def test_glm_decode_graph_replays_the_eager_step(ckpts):
    """The captured 4-row step (one stream) equals the eager step bit for bit,
    and holds the dense layer's six kernel nodes plus the routed layers' eleven."""
    from dmcp.models.llm import DecodeGraphs, LocalLM
    m = LocalLM.load_safetensors(ckpts["glm"], device="cuda", max_seq=256, max_batch=8, max_rows=16)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (9, 14, 5, 11)]
    m.prefill_batch([(p, s, 0) for s, p in enumerate(prompts)])
    tk = torch.tensor([5, 6, 7, 8], dtype=torch.int32, device="cuda")
    sl = torch.arange(4, dtype=torch.int32, device="cuda")
    ps = torch.tensor([len(p) for p in prompts], dtype=torch.int32, device="cuda")
    eager = m.decode(tk, sl, ps).clone()
    masks = torch.full((1, (m.cfg.vocab_size + 31) // 32), -1, dtype=torch.int32, device="cuda")
    graphs = DecodeGraphs(m, masks, buckets=(4,))
    graphs._capture(4)
    # the bias-taking fused QKV is one launch, so a layer is 6 launches dense and 4 + 1 + 6 routed
    assert graphs.graphs[4].kernels == 3 + 6 + 2 * (4 + 1 + 6)
    # the same rows again (the K/V they append is what the eager step appended)
    logits, ids = graphs.run([5, 6, 7, 8], [0, 1, 2, 3], [len(p) for p in prompts], [0, 0, 0, 0])
    assert torch.equal(ids.long(), eager.float().argmax(-1))
    assert logits is None or torch.equal(logits, eager)
