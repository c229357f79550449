"""The q/k/v projection bias through every hand-written QKV path (the fused
epilogue of csrc/fused_gemm.hip, the split-K reduction of csrc/wgemm.hip that
serves the weight-streaming and the large-tile GEMM) against the fp32
references of ``dmcp.ops.reference`` -- which tests/test_checkpoint_fidelity.py
pins to ``transformers`` -- and a Qwen2-style checkpoint (biases + llama3 RoPE
scaling) decoded on each path against the fp32 CPU model."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

K, MAXS, S = 256, 64, 3
GEOMS = [(4, 2, 64), (2, 1, 128)]  # (Hq, Hkv, D): qkv width 512, a multiple of the large tile's 256
CASE_B = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
          "original_max_position_embeddings": 64}
# (op, rows, forced split-K count): 96 rows at K = 256 plan one slice, so the
# two-slice reduction is forced; the large-tile plan chooses its own
OPS = [("fused_rope_kv", 1, 0), ("fused_rope_kv", 16, 0), ("wgemm_rope_kv", 17, 0), ("wgemm_rope_kv", 96, 2),
       ("tgemm_rope_kv", 513, 0)]


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _inputs(M, Hq, Hkv, D):
    from dmcp.ops import reference
    N = (Hq + 2 * Hkv) * D
    x, w = _bf(M, K, seed=21), _bf(N, K, seed=22, scale=0.05)
    b = _bf(N, seed=23, scale=2.0)
    # one (slot, position) per row (rows of a large step wrap a bigger cache), 0 and the last position included
    maxs = max(MAXS, -(-M // S))
    pos = torch.tensor([(maxs - 1 - m // S) if m % 2 else m // S for m in range(M)], dtype=torch.int32)
    slot = torch.tensor([m % S for m in range(M)], dtype=torch.int32)
    if M > 1:
        slot[M // 2] = -1  # a padding row: q written, nothing appended
        pos[1] = maxs - 1
    seen = {(int(s), int(p)) for s, p in zip(slot, pos) if s >= 0}
    assert len(seen) == int((slot >= 0).sum()) and int(pos[0]) == 0
    cs = reference.rope_tables(maxs, D, 500000.0, device="cuda", scaling=CASE_B)
    return x, w, b, pos.cuda(), slot.cuda(), cs, maxs


def _run(mod, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits):
    M, N = x.shape[0], w.shape[0]
    if op == "fused_rope_kv":
        return mod.fused_rope_kv(x, w, 1e-5, pos, slot, cs, kc, vc, Hq, bias=b)
    ws = torch.empty(16 * M * N, dtype=torch.float32, device="cuda")
    return getattr(mod, op)(x, w, pos, slot, cs, kc, vc, Hq, ws, splits=splits, bias=b)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
@pytest.mark.parametrize("op,M,splits", OPS)
def test_qkv_bias_matches_the_fp32_reference(hip, op, M, splits, Hq, Hkv, D, kv):
    """q, the appended K / V rows and every untouched cache row, within the
    tolerances of the op's existing no-bias test (the rounding points are the same)."""
    from dmcp.ops import reference
    from dmcp.ops.reference import kv_float
    x, w, b, pos, slot, cs, maxs = _inputs(M, Hq, Hkv, D)
    dt = torch.uint8 if kv == "fp8" else torch.bfloat16
    fill = 0x38 if kv == "fp8" else 1.0  # a non-zero pattern: an unwritten row must keep it
    kc = torch.full((S, Hkv, maxs, D), fill, dtype=dt, device="cuda")
    vc = kc.clone()
    kr, vr = kc.clone(), vc.clone()
    if op != "fused_rope_kv":
        assert (splits or (hip.wgemm_plan if op[0] == "w" else hip.tgemm_plan)(M, w.shape[0], K)[0]) >= 1
    q = _run(hip, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits)
    qr = _run(reference, op, x, w, b, pos, slot, cs, kr, vr, Hq, splits)
    torch.testing.assert_close(q.float(), qr.float(), atol=3e-2, rtol=3e-2)
    tol = dict(atol=3e-2, rtol=0.13) if kv == "fp8" else dict(atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(kv_float(kc), kv_float(kr), **tol)
    torch.testing.assert_close(kv_float(vc), kv_float(vr), **tol)
    written = torch.zeros((S, maxs), dtype=torch.bool, device="cuda")
    ok = slot >= 0
    written[slot[ok].long(), pos[ok].long()] = True
    keep = ~written[:, None, :, None].expand_as(kc)
    assert bool((kc[keep] == fill).all()) and bool((vc[keep] == fill).all())  # no other cache row changed
    # the bias is what is being compared: without it q is far off
    q0 = _run(reference, op, x, w, None, pos, slot, cs, kr.clone(), vr.clone(), Hq, splits)
    assert (q0.float() - qr.float()).abs().max().item() > 1.0


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("op,M,splits", OPS)
def test_no_bias_and_zero_bias_are_bit_identical(hip, op, M, splits, kv):
    """bias=None launches the kernels' earlier arithmetic; an all-zero bias
    gives the same bytes (x + 0 == x), and both are what the existing no-bias
    tests expect."""
    from dmcp.ops import reference
    from dmcp.ops.reference import kv_float
    Hq, Hkv, D = GEOMS[0]
    x, w, _, pos, slot, cs, maxs = _inputs(M, Hq, Hkv, D)
    dt = torch.uint8 if kv == "fp8" else torch.bfloat16
    outs = []
    for b in (None, torch.zeros(w.shape[0], dtype=torch.bfloat16, device="cuda")):
        kc = torch.zeros((S, Hkv, maxs, D), dtype=dt, device="cuda")
        vc = torch.zeros_like(kc)
        outs.append((_run(hip, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits), kc, vc))
    for a, z in zip(*outs):
        assert torch.equal(a, z)
    kr = torch.zeros((S, Hkv, maxs, D), dtype=dt, device="cuda")
    vr = torch.zeros_like(kr)
    qr = _run(reference, op, x, w, None, pos, slot, cs, kr, vr, Hq, splits)
    torch.testing.assert_close(outs[0][0].float(), qr.float(), atol=3e-2, rtol=3e-2)
    tol = dict(atol=3e-2, rtol=0.13) if kv == "fp8" else dict(atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(kv_float(outs[0][1]), kv_float(kr), **tol)
    torch.testing.assert_close(kv_float(outs[0][2]), kv_float(vr), **tol)


def test_bias_validation(hip):
    Hq, Hkv, D = GEOMS[0]
    x, w, b, pos, slot, cs, maxs = _inputs(4, Hq, Hkv, D)
    kc = torch.zeros((S, Hkv, maxs, D), dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    ws = torch.empty(16 * 4 * w.shape[0], dtype=torch.float32, device="cuda")
    for bad in (b[:-8].contiguous(), b.float(), b.cpu()):
        with pytest.raises(hip.HipOpsError):
            hip.fused_rope_kv(x, w, 1e-5, pos, slot, cs, kc, vc, Hq, bias=bad)
        with pytest.raises(hip.HipOpsError):
            hip.wgemm_rope_kv(x, w, pos, slot, cs, kc, vc, Hq, ws, bias=bad)
        with pytest.raises(hip.HipOpsError):
            hip.tgemm_rope_kv(x, w, pos, slot, cs, kc, vc, Hq, ws, bias=bad)


# ------------------------------------------------------------------ model level
def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.float().flatten(), b.float().flatten(), dim=0).item()


def _check_rows(got, ref, bound, what):
    """Per-row logit cosine >= the full-checkpoint decode test's margin, and
    top-1 agreement on every decisive row (fp32 top-2 gap above twice the
    row's largest logit error, the rule of tests/test_gpu_pgemm.py)."""
    got, ref = got.float().cpu(), ref.float().cpu()
    coss = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    top2 = ref.topk(2, dim=-1).values
    decisive = (top2[:, 0] - top2[:, 1]) > 2 * (got - ref).abs().max(-1).values
    same = got.argmax(-1) == ref.argmax(-1)
    print(f"{what}: min cosine {coss.min().item():.5f}, decisive rows {int(decisive.sum())}/{len(coss)}, "
          f"top-1 agreement {same.float().mean().item():.3f}")
    assert coss.min().item() >= bound, (what, coss.min().item())
    assert bool(same[decisive].all()), what


@pytest.fixture(scope="module")
def tiny_ckpt(tmp_path_factory):
    from dmcp.utils import synth
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("qwen_tiny")), layers=2, hidden=256, heads=4,
                                  kv_heads=2, intermediate=512, vocab=512, tokenizer="", outliers=(7,),
                                  rope_scaling=CASE_B, qkv_bias=True, model_type="qwen2", device="cpu")


@pytest.fixture(scope="module")
def tiny_ref(tiny_ckpt):
    """fp32 logits of the CPU model for three sequences: uneven prompts + the
    token stream each slot's decode rows append (computed once, shared)."""
    from dmcp.models.llm import LocalLM
    cpu = LocalLM.load_safetensors(tiny_ckpt, device="cpu", max_seq=512, max_batch=1, max_rows=1)
    assert cpu.has_bias and cpu.cfg.rope_scaling is not None
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (37, 60, 91)]
    streams = [torch.randint(0, 512, (176,), generator=g).tolist() for _ in range(3)]
    logits = [cpu.reference_logits(p + s) for p, s in zip(prompts, streams)]
    return prompts, streams, logits


@pytest.mark.parametrize("kv,bound", [("bf16", 0.999), ("fp8", 0.99)])
def test_biased_checkpoint_decodes_on_every_qkv_path(hip, tiny_ckpt, tiny_ref, kv, bound):
    """Prefill (hipBLASLt + rope_kv), then one decode step each on the fused
    (8 rows), weight-streaming (40) and large-tile (520) QKV kernels; rows of
    a step extend the three slots at consecutive positions."""
    from dmcp.models.llm import LocalLM
    prompts, streams, ref = tiny_ref
    m = LocalLM.load_safetensors(tiny_ckpt, device="cuda", max_seq=512, max_batch=8, max_rows=520, kv_dtype=kv)
    assert m.use_fused and m.use_wgemm and m.use_tgemm and m.has_bias
    got = m.prefill_batch([(p, s, 0) for s, p in enumerate(prompts)])
    _check_rows(got, torch.stack([ref[s][len(p) - 1] for s, p in enumerate(prompts)]), bound, f"prefill {kv}")
    for rows in (8, 40, 520):
        sl = [r % 3 for r in range(rows)]
        off = [r // 3 for r in range(rows)]
        tk = torch.tensor([streams[s][j] for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        ps = torch.tensor([len(prompts[s]) + j for s, j in zip(sl, off)], dtype=torch.int32, device="cuda")
        logits = m.decode(tk, torch.tensor(sl, dtype=torch.int32, device="cuda"), ps)
        exp = torch.stack([ref[s][len(prompts[s]) + j] for s, j in zip(sl, off)])
        _check_rows(logits, exp, bound, f"decode {rows} rows {kv}")


def test_qwen25_coder_geometry_loads_and_decodes(hip, tmp_path):
    """Qwen2.5-Coder-1.5B's geometry (2 layers of it): nothing refused, every
    hand-written decode path on, a 40-row step within the bf16 margin."""
    from dmcp.models.llm import LocalLM, check_checkpoint
    from dmcp.utils import synth
    d = synth.llama_checkpoint(str(tmp_path / "qwen15"), layers=2, hidden=1536, heads=12, kv_heads=2,
                               intermediate=8960, vocab=151936, tokenizer="", outliers=(7, 300, 1029),
                               qkv_bias=True, model_type="qwen2", tie_embeddings=True, head_dim=128)
    assert check_checkpoint(d) is None
    m = LocalLM.load_safetensors(d, device="cuda", max_seq=256, max_batch=64, max_rows=520, kv_dtype="bf16")
    assert m.use_wgemm and m.use_tgemm and m.fused_head and m.has_bias and not m.prefill_fp8
    assert m.cfg.head_dim == 128 and m.cfg.qkv_dim == 2048
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, 151936, (24,), generator=g).tolist()
    nxt = torch.randint(0, 151936, (40,), generator=g).tolist()
    for s in range(0, 40, 8):
        m.prefill_batch([(prompt, s + i, 0) for i in range(8)])
    tk = torch.tensor(nxt, dtype=torch.int32, device="cuda")
    sl = torch.arange(40, dtype=torch.int32, device="cuda")
    ps = torch.full((40,), len(prompt), dtype=torch.int32, device="cuda")
    logits = m.decode(tk, sl, ps)
    cpu = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=1, max_rows=1)
    rows = (0, 17, 39)
    exp = torch.stack([cpu.reference_logits(prompt + [nxt[r]])[-1] for r in rows])
    _check_rows(logits[list(rows)], exp, 0.999, "qwen2.5-coder-1.5b geometry, 40 rows")
