"""The Python side of the gfx950 op wrappers (dmcp/ops/hip.py) run on the CPU
against a recording stand-in for the kernel library: every argument check,
workspace size and launch argument list of the GPU path executes here (a
wrapper's own bug -- an unbound name, a wrong argument count -- would
otherwise surface only on the GPU box).  The kernels themselves are checked
against fp32 by the ``gpu`` tests."""
import pytest
import torch


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def dry(monkeypatch):
    from dmcp.ops import hip
    fake = _FakeLib()
    real_req = hip._req

    def req(t, dtype, name):  # the dtype / layout checks, without the device check
        if t.dtype != dtype:
            raise hip.HipOpsError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise hip.HipOpsError(f"{name}: tensor must be contiguous")
    monkeypatch.setattr(hip, "_req", req)
    monkeypatch.setattr(hip, "_stream", lambda: None)
    monkeypatch.setattr(hip, "lib", lambda: fake)
    assert real_req is not req
    return hip, fake


def _bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


@pytest.mark.parametrize("with_prefix", [False, True])
@pytest.mark.parametrize("with_fork", [False, True])
def test_decode_attention_launch_arguments(dry, with_prefix, with_fork):
    hip, fake = dry
    from dmcp.ops.reference import SharedPrefix
    B, Hq, Hkv, D, MAXS, S = 40, 32, 8, 64, 1024, 9
    q = _bf(B, Hq, D)
    kc, vc = _bf(S, Hkv, MAXS, D), _bf(S, Hkv, MAXS, D)
    slot = torch.zeros(B, dtype=torch.int32)
    lens = torch.ones(B, dtype=torch.int32)
    fork = torch.zeros(S, 2, dtype=torch.int32) if with_fork else None
    pre = SharedPrefix(kc[S - 1], vc[S - 1], torch.tensor([7], dtype=torch.int32)) if with_prefix else None
    out = hip.decode_attention(q, kc, vc, slot, lens, 0.125, prefix=pre, splits=3, fork=fork)
    name, args = fake.calls[-1]
    assert name == "dmcp_decode_attention" and len(args) == 25 and out.shape == q.shape
    ps = hip.prefix_mfma_splits(B, Hq // Hkv, Hkv) if with_prefix else 0
    assert args[20] == ps
    if with_prefix:  # a workspace without room for the prefix partials is refused, never overrun
        ws = hip.decode_workspace(B, Hq, Hkv, D, MAXS, "cpu", prefix_slots=0)
        with pytest.raises(hip.HipOpsError):
            hip.decode_attention(q, kc, vc, slot, lens, 0.125, workspace=ws, prefix=pre, splits=3, fork=fork)


def test_prefill_varlen_launch_arguments(dry):
    hip, fake = dry
    Hq, Hkv, D, MAXS, S = 32, 8, 64, 4096, 8
    offsets, slots, starts = [0, 100, 300], [1, 2], [1119, 1119]
    q = _bf(300, Hq, D)
    kc, vc = _bf(S, Hkv, MAXS, D), _bf(S, Hkv, MAXS, D)
    for _ in range(2):  # the second call reuses the work list built by the first
        hip.prefill_attention_varlen(q, kc, vc, offsets, slots, starts, 0, [1119, 1119], 0.125)
        name, args = fake.calls[-1]
        assert name == "dmcp_prefill_varlen" and len(args) == 17
    assert args[8] == sum(-(-T * 4 // hip.VARLEN_COLS) for T in (100, 200))


@pytest.mark.parametrize("M", [40, 320, 610])
def test_decode_gemm_wrappers_launch(dry, M):
    """The decode step's fused GEMM wrappers (weight-streaming up to 512 rows,
    large-tile above) with Llama-3.2-1B projection shapes."""
    hip, fake = dry
    H, I, Hq, Hkv, D, MAXS = 2048, 8192, 32, 8, 64, 1024
    Q = (Hq + 2 * Hkv) * D
    x = _bf(M, H)
    pos = torch.zeros(M, dtype=torch.int32)
    slot = torch.zeros(M, dtype=torch.int32)
    cs = torch.zeros(MAXS, D // 2, 2, dtype=torch.float32)
    kc, vc = torch.zeros(4, Hkv, MAXS, D, dtype=torch.uint8), torch.zeros(4, Hkv, MAXS, D, dtype=torch.uint8)
    resid, nw = _bf(M, H), _bf(H)
    V = 128256
    masks = torch.zeros(2, (V + 31) // 32, dtype=torch.int32)
    midx = torch.zeros(M, dtype=torch.int32)
    if M <= hip.WGEMM_MAX_ROWS:
        ws = hip.wgemm_workspace(M, Q, "cpu")
        hip.wgemm_rope_kv(x, _bf(Q, H), pos, slot, cs, kc, vc, Hq, ws)
        hip.wgemm_resid_norm(x, _bf(H, H), resid, nw, 1e-5, ws)
        hip.wgemm_resid_norm(_bf(M, I), _bf(H, I), resid, nw, 1e-5, ws)
        hip.wgemm_swiglu(x, _bf(2 * I, H))
        hip.lm_head_argmax(x, _bf(V, H), masks, midx, workspace=hip.lm_head_workspace(V, "cpu", M))
    if M > 256 or M <= hip.TGEMM_MAX_ROWS:
        tw = torch.empty(16 * M * Q, dtype=torch.float32)
        hip.tgemm_rope_kv(x, _bf(Q, H), pos, slot, cs, kc, vc, Hq, tw)
        hip.tgemm_resid_norm(x, _bf(H, H), resid, nw, 1e-5, tw)
        hip.tgemm_swiglu(x, _bf(2 * I, H))
        hip.tgemm_lm_head_argmax(x, _bf(V, H), masks, midx, workspace=torch.empty(2 * (V // 64) * M,
                                                                                   dtype=torch.float32))
    assert fake.calls and all(isinstance(n, str) for n, _ in fake.calls)


# (Hq, Hkv, D, K): a small projection and Llama-3.2-1B's
_PROJ = {"small": (4, 2, 64, 256), "llama1b": (32, 8, 64, 2048)}
# family -> (GEMM entry point, index of M in its argument list: M, N, K, S follow each other)
_GEMM = {"wgemm": ("dmcp_wgemm", 4), "tgemm": ("dmcp_tgemm", 4), "wgemm_mx": ("dmcp_wgemm_mx", 7)}
_FAMILY_ROWS = [(f, M) for f, rows in (("wgemm", (1, 17, 96, 320)), ("tgemm", (96, 520, 1024)),
                                       ("wgemm_mx", (96, 520, 1024))) for M in rows]


def _operands(family, M, N, K):
    if family == "wgemm_mx":
        return (torch.zeros(M, K, dtype=torch.uint8), torch.zeros(M, K // 32, dtype=torch.uint8),
                torch.zeros(N, K, dtype=torch.uint8), torch.zeros(N, dtype=torch.float32))
    return _bf(M, K), _bf(N, K)


def _plan(hip, family, M, N, K):
    return {"wgemm": hip.wgemm_plan, "tgemm": hip.tgemm_plan, "wgemm_mx": hip.wmx_plan}[family](M, N, K)[0]


def _rope_inputs(M, Hkv, D, kv_dtype):
    pos = torch.zeros(M, dtype=torch.int32)
    slot = torch.zeros(M, dtype=torch.int32)
    cs = torch.zeros(128, D // 2, 2, dtype=torch.float32)
    kc, vc = torch.zeros(3, Hkv, 128, D, dtype=kv_dtype), torch.zeros(3, Hkv, 128, D, dtype=kv_dtype)
    return pos, slot, cs, kc, vc


def _gemm_then(fake, family, reduction):
    """The recorded calls are exactly the family's GEMM then ``reduction``;
    returns the GEMM's (M, N, K, S) and the reduction's arguments."""
    gemm, at = _GEMM[family]
    assert [n for n, _ in fake.calls] == [gemm, reduction]
    return fake.calls[0][1][at:at + 4], fake.calls[1][1]


@pytest.mark.parametrize("proj", sorted(_PROJ))
@pytest.mark.parametrize("family,M", _FAMILY_ROWS)
def test_splitk_consumers_call_sequence(dry, family, M, proj):
    """Each fused wrapper is its family's partials GEMM followed by the one
    split-K reduction, both given the same S / M / N."""
    hip, fake = dry
    Hq, Hkv, D, K = _PROJ[proj]
    Q = (Hq + 2 * Hkv) * D
    mx = family == "wgemm_mx"
    ws = torch.empty(16 * M * max(Q, K), dtype=torch.float32)
    for kv_dtype, with_bias in ((torch.bfloat16, False), (torch.uint8, True)):
        planned = _plan(hip, family, M, Q, K)
        kw = {} if mx else {"splits": 2 if planned == 1 else 0}
        S = kw.get("splits") or planned
        bias = None if mx or not with_bias else _bf(Q)
        if bias is not None:
            kw["bias"] = bias
        pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, kv_dtype)
        del fake.calls[:]
        q = getattr(hip, f"{family}_rope_kv")(*_operands(family, M, Q, K), pos, slot, cs, kc, vc, Hq, ws, **kw)
        dims, red = _gemm_then(fake, family, "dmcp_reduce_rope_kv")
        assert dims == (M, Q, K, S) and tuple(q.shape) == (M, Hq, D)
        assert (red[1], red[8], red[9], red[10], red[11]) == (S, M, Hq, Hkv, D)
        assert red[15] == int(kv_dtype == torch.uint8)
        assert (red[17].value is None) == (bias is None)
    # O projection [K, K] + residual + RMSNorm: bf16 output, and MXFP8 where the MX family's N allows it
    resid, nw = _bf(M, K), _bf(K)
    planned = _plan(hip, family, M, K, K)
    kw = {} if mx else {"splits": 2 if planned == 1 else 0}
    S = kw.get("splits") or planned
    for to_mx in ((False, True) if mx and K % 2048 == 0 else (False,)):
        if mx:
            kw["mx"] = to_mx
        del fake.calls[:]
        getattr(hip, f"{family}_resid_norm")(*_operands(family, M, K, K), resid, nw, 1e-5, ws, **kw)
        dims, red = _gemm_then(fake, family, "dmcp_reduce_resid_norm_mx" if to_mx else "dmcp_reduce_resid_norm")
        assert dims == (M, K, K, S) and red[1] == S
        assert (red[6], red[7]) == (M, K) if to_mx else (red[5], red[6]) == (M, K)


@pytest.mark.parametrize("family", sorted(_GEMM))
def test_splitk_consumers_refuse_before_launch(dry, family):
    """A bad workspace, K split, pos or bias raises before anything is launched."""
    hip, fake = dry
    Hq, Hkv, D, K = _PROJ["small"]
    Q, M = (Hq + 2 * Hkv) * D, 96
    mx = family == "wgemm_mx"
    pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, torch.bfloat16)
    qkv, o = _operands(family, M, Q, K), _operands(family, M, K, K)
    resid, nw = _bf(M, K), _bf(K)
    ws = torch.empty(16 * M * Q, dtype=torch.float32)
    rope_kv, resid_norm = getattr(hip, f"{family}_rope_kv"), getattr(hip, f"{family}_resid_norm")
    partials = getattr(hip, f"{family}_partials")
    rn_kw = {"mx": False} if mx else {}
    small = torch.empty(_plan(hip, family, M, Q, K) * M * Q - 1, dtype=torch.float32)
    refused = [lambda: rope_kv(*qkv, pos, slot, cs, kc, vc, Hq, small),
               lambda: resid_norm(*o, resid, nw, 1e-5, torch.empty(M * K - 1, dtype=torch.float32), **rn_kw),
               lambda: rope_kv(*qkv, pos[:-1], slot, cs, kc, vc, Hq, ws),
               # K = 256 is 4 stages: wgemm / wmx need K % (64 S) == 0, tgemm non-empty slices of whole stages
               lambda: partials(*qkv, ws, splits=3),
               lambda: partials(*qkv, ws, splits=5)]
    if not mx:
        refused += [lambda: rope_kv(*qkv, pos, slot, cs, kc, vc, Hq, ws, splits=3),
                    lambda: resid_norm(*o, resid, nw, 1e-5, ws, splits=3),
                    lambda: rope_kv(*qkv, pos, slot, cs, kc, vc, Hq, ws, bias=_bf(Q - 1))]
    for call in refused:
        with pytest.raises(hip.HipOpsError):
            call()
        assert not fake.calls
    if family == "tgemm":  # its own rule: 2 and 4 slices of the 4 stages are fine, 3 would leave the last one empty
        assert partials(*qkv, ws, splits=4) == 4 and fake.calls
