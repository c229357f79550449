"""Qwen3's per-head q / k RMSNorm through every hand-written QKV path: the
norm-taking RoPE + append (csrc/dmcp_kernels.hip), the split-K reduction
(csrc/splitk_reduce.hip) behind the weight-streaming and the large-tile GEMM,
and the small-row pair fused_linear_norm + rope_kv -- against the fp32
references of ``dmcp.ops.reference`` (which tests/test_checkpoint_qwen3.py
pins to ``transformers``), and a Qwen3-style checkpoint decoded on each path
against the fp32 CPU model.

The tolerances are those of tests/test_gpu_qkv_bias.py: the norm adds no
rounding point (bf16 row -> norm and RoPE in fp32 -> one rounding)."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

K, MAXS, S = 256, 64, 3
EPS = 1e-6
# (Hq, Hkv, D): (Hq + Hkv) D / 8 RoPE units of D / 8 lanes a head -- 48 (a
# partial first wave) twice, and 320 (a second trip of the 256-thread loop
# with a partial tail); qkv widths 512, 512 and 3,072: multiples of the large
# tile's 256
GEOMS = [(4, 2, 64), (2, 1, 128), (32, 8, 64)]
# (op, rows, forced split-K count), as tests/test_gpu_qkv_bias.py
OPS = [("rope_kv", 1, 0), ("rope_kv", 16, 0), ("wgemm_rope_kv", 17, 0), ("wgemm_rope_kv", 96, 2),
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
    cs = reference.rope_tables(maxs, D, 1000000.0, device="cuda")
    return x, w, b, pos.cuda(), slot.cuda(), cs, maxs


def _norm(D):
    """q / k norm weights at 1 +- 0.25 with one channel at 8 each, different
    channels in different halves: a q / k swap or an off-by-group error shows."""
    g = torch.Generator(device="cuda").manual_seed(31)
    qw = 1.0 + 0.25 * torch.randn(D, generator=g, device="cuda")
    kw = 1.0 + 0.25 * torch.randn(D, generator=g, device="cuda")
    qw[5] = 8.0
    kw[D // 2 + 9] = 8.0
    return qw.to(torch.bfloat16), kw.to(torch.bfloat16), EPS


def _run(mod, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits, **kw):
    from dmcp.ops import reference
    M, N = x.shape[0], w.shape[0]
    if op == "rope_kv":  # the bf16 QKV row hipBLASLt's F.linear hands it
        qkv = reference._linear_f32(x, w, b).to(torch.bfloat16)
        return mod.rope_kv(qkv, pos, slot, cs, kc, vc, Hq, **kw)
    ws = torch.empty(16 * M * N, dtype=torch.float32, device="cuda")
    return getattr(mod, op)(x, w, pos, slot, cs, kc, vc, Hq, ws, splits=splits, bias=b, **kw)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
@pytest.mark.parametrize("op,M,splits", OPS)
def test_qk_norm_matches_the_fp32_reference(hip, op, M, splits, Hq, Hkv, D, bias, kv):
    """q, the appended K / V rows and every untouched cache row."""
    from dmcp.ops import reference
    from dmcp.ops.reference import kv_float
    x, w, b, pos, slot, cs, maxs = _inputs(M, Hq, Hkv, D)
    b = b if bias else None
    qkn = _norm(D)
    dt = torch.uint8 if kv == "fp8" else torch.bfloat16
    fill = 0x38 if kv == "fp8" else 1.0  # a non-zero pattern: an unwritten row must keep it
    kc = torch.full((S, Hkv, maxs, D), fill, dtype=dt, device="cuda")
    vc = kc.clone()
    kr, vr = kc.clone(), vc.clone()
    q = _run(hip, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits, qk_norm=qkn)
    qr = _run(reference, op, x, w, b, pos, slot, cs, kr, vr, Hq, splits, qk_norm=qkn)
    print(f"{op} M={M} ({Hq},{Hkv},{D}) bias={bias} {kv}: max |q - ref| "
          f"{(q.float() - qr.float()).abs().max().item():.4f}, max |k - ref| "
          f"{(kv_float(kc) - kv_float(kr)).abs().max().item():.4f}")
    torch.testing.assert_close(q.float(), qr.float(), atol=3e-2, rtol=3e-2)
    tol = dict(atol=3e-2, rtol=0.13) if kv == "fp8" else dict(atol=3e-2, rtol=3e-2)
    torch.testing.assert_close(kv_float(kc), kv_float(kr), **tol)
    torch.testing.assert_close(kv_float(vc), kv_float(vr), **tol)
    written = torch.zeros((S, maxs), dtype=torch.bool, device="cuda")
    ok = slot >= 0
    written[slot[ok].long(), pos[ok].long()] = True
    keep = ~written[:, None, :, None].expand_as(kc)
    assert bool((kc[keep] == fill).all()) and bool((vc[keep] == fill).all())  # no other cache row changed
    # the norm is what is being compared: without it q is far off
    q0 = _run(reference, op, x, w, b, pos, slot, cs, kr.clone(), vr.clone(), Hq, splits)
    assert (q0.float() - qr.float()).abs().max().item() > 1.0


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("op,M,splits", [("rope_kv", 16, 0), ("wgemm_rope_kv", 96, 2), ("tgemm_rope_kv", 513, 0)])
def test_qk_norm_none_is_the_call_without_the_keyword(hip, op, M, splits, kv):
    """qk_norm=None launches the no-norm kernels: q and both caches are
    byte-identical to a call that does not pass the keyword."""
    Hq, Hkv, D = GEOMS[0]
    x, w, b, pos, slot, cs, maxs = _inputs(M, Hq, Hkv, D)
    dt = torch.uint8 if kv == "fp8" else torch.bfloat16
    outs = []
    for kw in ({}, {"qk_norm": None}):
        kc = torch.zeros((S, Hkv, maxs, D), dtype=dt, device="cuda")
        vc = torch.zeros_like(kc)
        outs.append((_run(hip, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits, **kw), kc, vc))
    for a, z in zip(*outs):
        assert torch.equal(a, z)
    assert bool(outs[0][1].any()) and bool(outs[0][2].any())


def test_qk_norm_validation(hip):
    """Bad norm weights are refused on the host, before any launch."""
    Hq, Hkv, D = GEOMS[0]
    x, w, b, pos, slot, cs, maxs = _inputs(4, Hq, Hkv, D)
    kc = torch.zeros((S, Hkv, maxs, D), dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    ws = torch.empty(16 * 4 * w.shape[0], dtype=torch.float32, device="cuda")
    qkv = torch.zeros((4, w.shape[0]), dtype=torch.bfloat16, device="cuda")
    qw, kw, eps = _norm(D)
    wide = torch.ones(2 * D, dtype=torch.bfloat16, device="cuda")
    for bad in ((qw[:-8].contiguous(), kw, eps), (qw, kw.float(), eps), (qw.cpu(), kw, eps), (qw, wide[::2], eps),
                (qw, kw)):
        with pytest.raises(hip.HipOpsError):
            hip.rope_kv(qkv, pos, slot, cs, kc, vc, Hq, qk_norm=bad)
        with pytest.raises(hip.HipOpsError):
            hip.wgemm_rope_kv(x, w, pos, slot, cs, kc, vc, Hq, ws, qk_norm=bad)
        with pytest.raises(hip.HipOpsError):
            hip.tgemm_rope_kv(x, w, pos, slot, cs, kc, vc, Hq, ws, qk_norm=bad)
    assert not bool(kc.any()) and not bool(vc.any())
    # a head size the lane groups do not cover
    k32 = torch.zeros((S, 2, maxs, 32), dtype=torch.bfloat16, device="cuda")
    w32 = torch.ones(32, dtype=torch.bfloat16, device="cuda")
    cs32 = cs[:, :16].contiguous()
    with pytest.raises(hip.HipOpsError):
        hip.rope_kv(torch.zeros((4, 8 * 32), dtype=torch.bfloat16, device="cuda"), pos, slot, cs32, k32, k32.clone(),
                    4, qk_norm=(w32, w32, eps))
    # the fused QKV tile takes none: an error, not a norm silently dropped
    with pytest.raises(hip.HipOpsError):
        hip.fused_rope_kv(x, w, 1e-5, pos, slot, cs, kc, vc, Hq, qk_norm=(qw, kw, eps))


# ------------------------------------------------------------------ model level
def _check_rows(got, ref, bound, what):
    """tests/test_gpu_qkv_bias.py's rule: per-row logit cosine >= ``bound``
    and top-1 agreement on every decisive row (fp32 top-2 gap above twice the
    row's largest logit error)."""
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
    return synth.llama_checkpoint(str(tmp_path_factory.mktemp("qwen3_tiny")), layers=2, hidden=256, heads=4,
                                  kv_heads=2, head_dim=128, intermediate=512, vocab=512, tokenizer="",
                                  outliers=(7,), qk_norm=True, model_type="qwen3", device="cpu")


@pytest.fixture(scope="module")
def tiny_ref(tiny_ckpt):
    """fp32 logits of the CPU model for three sequences: uneven prompts + the
    token stream each slot's decode rows append (computed once, shared)."""
    from dmcp.models.llm import LocalLM
    cpu = LocalLM.load_safetensors(tiny_ckpt, device="cpu", max_seq=512, max_batch=1, max_rows=1)
    assert cpu.has_qk_norm and cpu.cfg.head_dim == 128 and cpu.cfg.rope_theta == 1e6
    assert cpu.cfg.n_heads * cpu.cfg.head_dim != cpu.cfg.hidden
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (37, 60, 91)]
    streams = [torch.randint(0, 512, (176,), generator=g).tolist() for _ in range(3)]
    logits = [cpu.reference_logits(p + s) for p, s in zip(prompts, streams)]
    return prompts, streams, logits


@pytest.mark.parametrize("kv,bound", [("bf16", 0.999), ("fp8", 0.99)])
def test_qwen3_checkpoint_decodes_on_every_qkv_path(hip, tiny_ckpt, tiny_ref, kv, bound):
    """Prefill (hipBLASLt + rope_kv), then one decode step each on the
    small-row pair fused_linear_norm + rope_kv (8 rows), the weight-streaming
    (40) and the large-tile (520) QKV reduction; rows of a step extend the
    three slots at consecutive positions."""
    from dmcp.models.llm import LocalLM
    prompts, streams, ref = tiny_ref
    m = LocalLM.load_safetensors(tiny_ckpt, device="cuda", max_seq=512, max_batch=8, max_rows=520, kv_dtype=kv)
    assert m.use_fused and m.use_wgemm and m.use_tgemm and m.has_qk_norm and not m.prefill_fp8
    assert m.qkv_buf is not None and tuple(m.qkv_buf.shape) == (m.fused_max_rows, m.cfg.qkv_dim)
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


def test_qwen3_small_row_step_is_capturable(hip, tiny_ckpt):
    """The two-launch small-row QKV inside a captured step: the replay's ids
    are the eager step's (the QKV row buffer is preallocated)."""
    from dmcp.models.llm import LocalLM
    m = LocalLM.load_safetensors(tiny_ckpt, device="cuda", max_seq=128, max_batch=8, max_rows=64)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, 512, (20,), generator=g).tolist()
    m.prefill_batch([(prompt, s, 0) for s in range(8)])
    tk = torch.randint(0, 512, (8,), generator=g).to(dtype=torch.int32, device="cuda")
    sl = torch.arange(8, dtype=torch.int32, device="cuda")
    ps = torch.full((8,), len(prompt), dtype=torch.int32, device="cuda")
    eager = m.decode(tk, sl, ps).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.decode(tk, sl, ps)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.decode(tk, sl, ps)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_qwen3_06b_geometry_loads_and_decodes(hip, tmp_path):
    """Qwen3-0.6B's geometry (2 layers of it; heads x head_dim = 2,048 over a
    hidden size of 1,024): nothing refused, every hand-written decode path
    on, a 40-row step within the bf16 margin."""
    from dmcp.models.llm import LocalLM, check_checkpoint
    from dmcp.utils import synth
    d = synth.llama_checkpoint(str(tmp_path / "qwen3_06"), layers=2, hidden=1024, heads=16, kv_heads=8,
                               intermediate=3072, vocab=151936, tokenizer="", outliers=(7, 300),
                               qk_norm=True, model_type="qwen3", tie_embeddings=True, head_dim=128)
    assert check_checkpoint(d) is None
    m = LocalLM.load_safetensors(d, device="cuda", max_seq=256, max_batch=64, max_rows=520, kv_dtype="bf16")
    assert m.use_fused and m.use_wgemm and m.use_tgemm and m.fused_head and m.has_qk_norm and not m.prefill_fp8
    assert m.cfg.head_dim == 128 and m.cfg.qkv_dim == 4096 and m.cfg.hidden == 1024
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
    _check_rows(logits[list(rows)], exp, 0.999, "qwen3-0.6b geometry, 40 rows")
