"""The per-row scaled fp8 KV cache (kv_dtype fp8s) on the GPU: every writer
(rope_kv, the split-K reduction behind wgemm_rope_kv / tgemm_rope_kv, kv_fork)
against ``dmcp.ops.reference``, every reader (decode attention with its fork
table and shared prefix, prefill attention dense and varlen) on the scaled
needle cases of tests/needles_scaled.py, and a K-biased checkpoint through the
engine's four step sizes.

Writers.  The exponent bytes must equal the reference's.  A cache byte may
differ only where the kernel's fp32 value (its own summation order, fused
multiply-adds in the rotation) lands one bf16 step from the reference's before
the rounding to bf16: the decoded values then differ by at most one e4m3 step
of the element's own binade (the subnormal step of the row's scale under it)
-- what rtol 0.13 allows in the unscaled fp8 tests of the same kernels
(tests/test_gpu_qk_norm.py).  One bf16 step is 1/16 of an e4m3 step, so at most
1/16 of the elements whose pre-round values differ can cross an e4m3 rounding
boundary: BYTE_SHARE = 1/16.  The reference alone (its fp32 sum against an
fp64 one) stays inside the same share, checked below."""
import pytest
import torch

from tests import needles, needles_scaled

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

K, MAXS, S = 256, 64, 3
EPS = 1e-6
GEOMS = [(4, 2, 64), (2, 1, 128), (32, 8, 64)]  # 48, 48 and 320 RoPE units (tests/test_gpu_qk_norm.py)
OPS = [("rope_kv", 1, 0), ("rope_kv", 17, 0), ("wgemm_rope_kv", 17, 0), ("wgemm_rope_kv", 96, 2),
       ("tgemm_rope_kv", 513, 0)]
BYTE_SHARE = 1.0 / 16


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


def _bf(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, generator=g, device="cuda") * scale).to(torch.bfloat16)


def _inputs(M, Hq, Hkv, D):
    """Rows whose projections span 1e-3 .. 3,000 (a magnitude per row), a bias
    of +-2, the last V head all zero (weights and bias), one (slot, position)
    per row with position 0 and the last one included, one padding row and one
    row past the cache."""
    from dmcp.ops import reference
    N = (Hq + 2 * Hkv) * D
    g = torch.Generator(device="cuda").manual_seed(20)
    mag = torch.logspace(-3, 3.5, M, device="cuda")[torch.randperm(M, generator=g, device="cuda")] if M > 1 \
        else torch.tensor([3000.0], device="cuda")
    x = (_bf(M, K, seed=21).float() * mag[:, None] / 4).to(torch.bfloat16)
    w = _bf(N, K, seed=22, scale=0.25)
    b = _bf(N, seed=23, scale=2.0)
    w[N - D:] = 0
    b[N - D:] = 0
    maxs = max(MAXS, -(-M // S))
    pos = torch.tensor([(maxs - 1 - m // S) if m % 2 else m // S for m in range(M)], dtype=torch.int32)
    slot = torch.tensor([m % S for m in range(M)], dtype=torch.int32)
    if M > 4:
        slot[M // 2] = -1
        pos[1] = maxs - 1
        pos[3] = maxs  # past the cache: writes neither bytes nor an exponent
    cs = reference.rope_tables(maxs, D, 1000000.0, device="cuda")
    return x, w, b, pos.cuda(), slot.cuda(), cs, maxs


def _run(mod, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits, **kw):
    from dmcp.ops import reference
    M, N = x.shape[0], w.shape[0]
    if op == "rope_kv":
        qkv = reference._linear_f32(x, w, b).to(torch.bfloat16)
        return mod.rope_kv(qkv, pos, slot, cs, kc, vc, Hq, **kw)
    ws = torch.empty(16 * M * N, dtype=torch.float32, device="cuda")
    return getattr(mod, op)(x, w, pos, slot, cs, kc, vc, Hq, ws, splits=splits, bias=b, **kw)


def _norm(D):
    g = torch.Generator(device="cuda").manual_seed(31)
    qw = 1.0 + 0.25 * torch.randn(D, generator=g, device="cuda")
    kw = 1.0 + 0.25 * torch.randn(D, generator=g, device="cuda")
    return qw.to(torch.bfloat16), kw.to(torch.bfloat16), EPS


@pytest.mark.parametrize("qkn", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
@pytest.mark.parametrize("op,M,splits", OPS)
def test_scaled_writers_match_the_reference(hip, op, M, splits, Hq, Hkv, D, bias, qkn):
    from dmcp.ops import reference
    x, w, b, pos, slot, cs, maxs = _inputs(M, Hq, Hkv, D)
    b = b if bias else None
    kw = {"qk_norm": _norm(D)} if qkn else {}
    fill, sfill = 0x38, 99  # unwritten rows keep their bytes and their exponent
    tabs = []
    for mod in (hip, reference):
        kc = torch.full((S, Hkv, maxs, D), fill, dtype=torch.uint8, device="cuda")
        vc = kc.clone()
        ks = torch.full((S, Hkv, maxs), sfill, dtype=torch.uint8, device="cuda")
        vs = ks.clone()
        q = _run(mod, op, x, w, b, pos, slot, cs, kc, vc, Hq, splits, kv_scale=(ks, vs), **kw)
        tabs.append((q, kc, vc, ks, vs))
    (q, kc, vc, ks, vs), (qr, kr, vr, ksr, vsr) = tabs
    torch.testing.assert_close(q.float(), qr.float(), atol=3e-2, rtol=3e-2)
    ok = (slot >= 0) & (pos < maxs)
    written = torch.zeros((S, maxs), dtype=torch.bool, device="cuda")
    written[slot[ok].long(), pos[ok].long()] = True
    wr = written[:, None, :].expand_as(ks)
    assert bool((ks[~wr] == sfill).all()) and bool((vs[~wr] == sfill).all())
    assert bool((kc[~wr] == fill).all()) and bool((vc[~wr] == fill).all())
    assert bool(wr.any())
    share = {}
    for name, c, s, cr, sr in (("k", kc, ks, kr, ksr), ("v", vc, vs, vr, vsr)):
        nbad = int((s[wr] != sr[wr]).sum())
        share[name] = float((c[wr] != cr[wr]).float().mean())
        # one e4m3 step of the ELEMENT's binade (2^-3 of it; the larger of the two decoded values decides),
        # at least the subnormal step of the row's scale
        dv, dr = reference.kv_decode_scaled(c, s), reference.kv_decode_scaled(cr, sr)
        binade = torch.exp2(torch.floor(torch.log2(torch.maximum(dv.abs(), dr.abs()).clamp_min(1e-38))))
        step = torch.maximum(binade / 8, reference._pow2(sr.to(torch.int32) - 127).float()[..., None] * 2.0 ** -9)
        diff = (dv - dr).abs()
        print(f"{op} M={M} ({Hq},{Hkv},{D}) bias={bias} qkn={qkn} {name}: exponent bytes differing {nbad}, "
              f"cache bytes differing {share[name]:.5f}, max diff / step {float((diff / step)[wr].max()):.3f}")
        assert nbad == 0, f"{name}: {nbad} exponent bytes differ from the reference"
        assert bool((diff <= step)[wr].all())
        assert share[name] <= BYTE_SHARE
    # the all-zero V head: exponent 0, zero bytes
    assert bool((vs[:, -1][written] == 127).all()) and bool((vc[:, -1][written] == 0).all())
    if op == "rope_kv":  # the same bf16 row in, the same fp32 rotation: V is a pure re-encode
        assert torch.equal(vc, vr)
    # magnitudes beyond the unit-scale range are really in the rows (V: a QK-norm levels K)
    if M >= 17 and Hkv > 1:  # (with one kv head the only V head is the all-zero one)
        assert int(vs[wr].max()) > 127 + 1 and int(vs[wr].min()) < 127 - 4


def test_reference_alone_is_inside_the_byte_share():
    """fp32 against fp64 summation of the same projection, both through the
    reference encoder: the bytes that flip stay under BYTE_SHARE."""
    from dmcp.ops import reference
    x, w, b, *_ = _inputs(96, 4, 2, 64)
    y32 = reference._linear_f32(x, w, b).to(torch.bfloat16)
    y64 = (x.double() @ w.double().t() + b.double()).to(torch.bfloat16)
    q32, s32 = reference.kv_encode_scaled(y32.view(96, -1, 64))
    q64, s64 = reference.kv_encode_scaled(y64.view(96, -1, 64))
    share = float((q32 != q64).float().mean())
    print(f"reference fp32 vs fp64 sum: cache bytes differing {share:.5f}")
    assert share <= BYTE_SHARE


def test_kv_fork_moves_the_exponents(hip):
    L, Sn, H, T, D = 2, 5, 2, 64, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    kc = torch.randint(0, 120, (L, Sn, H, T, D), generator=g, device="cuda", dtype=torch.uint8)
    vc = torch.randint(0, 120, (L, Sn, H, T, D), generator=g, device="cuda", dtype=torch.uint8)
    ks = torch.randint(100, 140, (L, Sn, H, T), generator=g, device="cuda", dtype=torch.uint8)
    vs = torch.randint(100, 140, (L, Sn, H, T), generator=g, device="cuda", dtype=torch.uint8)
    exp = [t.clone() for t in (kc, vc, ks, vs)]
    for t in exp:
        t[:, [3, 0], :, 5:38] = t[:, 1, :, 5:38].unsqueeze(1)
    hip.kv_fork(kc, vc, 1, [3, 0], 5, 38, kv_scale=(ks, vs))
    for got, want in zip((kc, vc, ks, vs), exp):
        assert torch.equal(got, want)


def test_bad_scale_tables_are_refused(hip):
    Hq, Hkv, D = GEOMS[0]
    x, w, b, pos, slot, cs, maxs = _inputs(8, Hq, Hkv, D)
    kc = torch.zeros((S, Hkv, maxs, D), dtype=torch.uint8, device="cuda")
    vc = torch.zeros_like(kc)
    ks = torch.zeros((S, Hkv, maxs), dtype=torch.uint8, device="cuda")
    qkv = torch.zeros((8, w.shape[0]), dtype=torch.bfloat16, device="cuda")
    for bad in ((ks, ks[:, :, :-1].contiguous()), (ks.int(), ks), (ks.cpu(), ks), (ks,), (ks, ks.transpose(0, 1))):
        with pytest.raises(hip.HipOpsError):
            hip.rope_kv(qkv, pos, slot, cs, kc, vc, Hq, kv_scale=bad)
    with pytest.raises(hip.HipOpsError):  # bf16 caches have no scaled form
        hip.rope_kv(qkv, pos, slot, cs, kc.bfloat16(), vc.bfloat16(), Hq, kv_scale=(ks, ks.clone()))
    with pytest.raises(hip.HipOpsError):
        hip.fused_rope_kv(x, w, 1e-5, pos, slot, cs, kc, vc, Hq, kv_scale=(ks, ks.clone()))
    assert not bool(kc.any()) and not bool(ks.any())


# ------------------------------------------------------------------ readers
# (the cases: tests/needles_scaled.py, where the CPU mutant test takes them from too)
OWN, PREFIX = needles_scaled.OWN, needles_scaled.PREFIX
PLANS = [(64, 1), (64, 3), (256, None)]


@pytest.mark.parametrize("si", range(len(needles_scaled.DECODE_SEQS)))
@pytest.mark.parametrize("D,Hq,Hkv", needles_scaled.RGEOMS)
def test_decode_scaled_needles(hip, D, Hq, Hkv, si):
    from dmcp.ops import SharedPrefix
    seq = needles_scaled.DECODE_SEQS[si]
    worst = 0.0
    for pairs in (False, True):
        c, kc, vc, ks, vs = needles_scaled.to("cuda", *needles_scaled.decode_case(D, Hq, Hkv, si, pairs))
        exp, bound = c.decode_expected()
        c.check_single_needles(exp)
        slot, lens, pre, fork = c.decode_inputs()
        if pre is not None:
            ps = c.seqs_prefix_slot()
            pre = SharedPrefix(kc[ps], vc[ps], pre.length, pre.rows, ks[ps], vs[ps])
        for chunk, splits in PLANS:
            got = hip.decode_attention(c.q, kc, vc, slot, lens, c.scale, chunk=chunk, prefix=pre, splits=splits,
                                       fork=fork, kv_scale=(ks, vs))
            worst = max(worst, needles.assert_within_bound(got, exp, bound, f"{seq} chunk {chunk} splits {splits}"))
    print(f"\nneedle error/bound [decode fp8s] = {worst:.4f}")


@pytest.mark.parametrize("T,start,P", needles_scaled.PREFILL_CASES)
@pytest.mark.parametrize("D,Hq,Hkv", needles_scaled.RGEOMS)
def test_prefill_scaled_needles(hip, D, Hq, Hkv, T, start, P):
    c, kc, vc, ks, vs = needles_scaled.to("cuda", *needles_scaled.prefill_case(D, Hq, Hkv, T, start, P))
    exp, bound = c.prefill_expected()
    c.check_single_needles(exp)
    worst = 0.0
    for variant in hip.PREFILL_VARIANTS[D]:
        for nsplit in (1, 3):
            got = hip.prefill_attention(c.q, kc, vc, OWN, start, PREFIX if P else None, P, c.scale, variant=variant,
                                        nsplit=nsplit, kv_scale=(ks, vs))
            worst = max(worst, needles.assert_within_bound(got, exp, bound, f"variant {variant} nsplit {nsplit}"))
    print(f"\nneedle error/bound [prefill fp8s] = {worst:.4f}")


@pytest.mark.parametrize("D,Hq,Hkv", needles_scaled.RGEOMS)
def test_prefill_varlen_scaled_needles(hip, D, Hq, Hkv):
    c, kc, vc, ks, vs = needles_scaled.to("cuda", *needles_scaled.varlen_case(D, Hq, Hkv))
    offsets, slots, starts, ps, plens = c.prefill_tables()
    assert ps == needles_scaled.VARLEN_PSLOT
    exp, bound = c.prefill_expected()
    c.check_single_needles(exp)
    got = hip.prefill_attention_varlen(c.q, kc, vc, offsets, slots, starts, ps, plens, c.scale, kv_scale=(ks, vs))
    print(f"\nneedle error/bound [varlen fp8s] = {needles.assert_within_bound(got, exp, bound, 'varlen'):.4f}")


# ------------------------------------------------------------------ model
def test_biased_checkpoint_on_every_step_size(tmp_path):
    """A Qwen2-layout checkpoint whose K bias takes K rows past 448, on the GPU
    engine with fp8 and fp8s caches against the fp32 reference logits: prefill,
    a <= 16-row step, a 17-512-row step and a > 512-row step.  fp8s must be
    closer to the reference than fp8 on every one, over all rows of the step
    (each row feeds its own next token: tests/kv_scaled_model.py)."""
    from tests.kv_scaled_model import biased_checkpoint, step_errors
    ckpt = biased_checkpoint(str(tmp_path / "qwen2-kbias"), head_dim=64)
    rows = (16, 96, 600)
    errs = {kv: step_errors(ckpt, kv, "cuda", rows=rows) for kv in ("fp8", "fp8s")}
    # the same checkpoint with the bias scaled down until nothing saturates: what e4m3 can do
    base = step_errors(biased_checkpoint(str(tmp_path / "unsaturated"), k_bias_scale=10.0), "fp8", "cuda", rows=rows)
    for step in errs["fp8"]:
        print(f"{step}: max |logit - fp32| fp8 {errs['fp8'][step]:.4f} fp8s {errs['fp8s'][step]:.4f} "
              f"fp8 unsaturated {base[step]:.4f}")
    for step in errs["fp8"]:
        assert errs["fp8s"][step] < errs["fp8"][step], step
        assert errs["fp8s"][step] <= 2 * base[step], step


def test_small_steps_without_a_bias_take_the_two_launch_qkv():
    """No bias: the <= 16-row step of an fp8s model is fused_linear_norm +
    the scaled rope_kv.  Prefill and an 8-row step against the fp32 reference,
    with smoke()'s tolerance."""
    from dmcp.models.llm import LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=16, max_seq=256, kv_dtype="fp8s"), device="cuda:0")
    assert m.use_fused and m.qkv_buf is not None
    toks = [256] + list(b"public class OrderService {")
    n = len(toks)
    ref = m.reference_logits(toks + [65]).float().cpu()
    got = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float().cpu()
    assert float((got - ref[n - 1]).abs().max()) < 0.05 * max(1.0, float(ref[n - 1].abs().max()))
    m.fork_kv(0, list(range(1, 8)), 0, n)
    dev = "cuda:0"
    lg = m.decode(torch.full((8,), 65, dtype=torch.int32, device=dev), torch.arange(8, dtype=torch.int32, device=dev),
                  torch.full((8,), n, dtype=torch.int32, device=dev)).float().cpu()
    assert float((lg - ref[n][None]).abs().max()) < 0.05 * max(1.0, float(ref[n].abs().max()))
