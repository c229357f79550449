"""The ``qk_norm`` keyword of the QKV wrappers (dmcp/ops/hip.py) on the CPU
against the recording stand-in of tests/test_hip_dry_launch.py: with a norm
the wrappers call the norm-taking entry points with their argument lists,
without one the earlier entry points with the earlier lists, and bad norm
weights are refused before anything is launched."""
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


def _rope_inputs(M, Hkv, D, kv_dtype):
    pos = torch.zeros(M, dtype=torch.int32)
    slot = torch.zeros(M, dtype=torch.int32)
    cs = torch.zeros(128, D // 2, 2, dtype=torch.float32)
    kc, vc = torch.zeros(3, Hkv, 128, D, dtype=kv_dtype), torch.zeros(3, Hkv, 128, D, dtype=kv_dtype)
    return pos, slot, cs, kc, vc


GEOMS = [(4, 2, 64), (2, 1, 128)]
K = 256
EPS = 1e-6


def test_abi_version_is_20():
    import os
    import re
    from dmcp.ops import hip
    assert hip.ABI_VERSION == 20
    src = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "dmcp_kernels.hip")).read()
    assert re.search(r"int dmcp_abi_version\(\) \{ return 20; \}", src)


@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
@pytest.mark.parametrize("kv_dtype", [torch.bfloat16, torch.uint8])
def test_rope_kv_entry_points(dry, Hq, Hkv, D, kv_dtype):
    hip, fake = dry
    M, N = 16, (Hq + 2 * Hkv) * D
    pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, kv_dtype)
    qw, kw = _bf(D), _bf(D)
    q = hip.rope_kv(_bf(M, N), pos, slot, cs, kc, vc, Hq, qk_norm=(qw, kw, EPS))
    (name, args), = fake.calls
    assert name == "dmcp_rope_kv_norm" and len(args) == 19 and tuple(q.shape) == (M, Hq, D)
    assert args[7:15] == (M, Hq, Hkv, D, 128, 128, 3, int(kv_dtype == torch.uint8))
    assert (args[16].value, args[17].value, args[18]) == (qw.data_ptr(), kw.data_ptr(), EPS)
    for kwargs in ({}, {"qk_norm": None}):
        del fake.calls[:]
        hip.rope_kv(_bf(M, N), pos, slot, cs, kc, vc, Hq, **kwargs)
        (name, old), = fake.calls
        assert name == "dmcp_rope_kv" and len(old) == 16 and old[7:15] == args[7:15]


@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
@pytest.mark.parametrize("family,M", [("wgemm", 40), ("wgemm", 320), ("tgemm", 610)])
def test_splitk_rope_kv_entry_points(dry, family, M, Hq, Hkv, D):
    hip, fake = dry
    N = (Hq + 2 * Hkv) * D
    gemm = {"wgemm": "dmcp_wgemm", "tgemm": "dmcp_tgemm"}[family]
    op = getattr(hip, f"{family}_rope_kv")
    ws = torch.empty(16 * M * N, dtype=torch.float32)
    qw, kw = _bf(D), _bf(D)
    for kv_dtype, bias in ((torch.bfloat16, None), (torch.uint8, _bf(N))):
        pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, kv_dtype)
        del fake.calls[:]
        q = op(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, bias=bias, qk_norm=(qw, kw, EPS))
        assert [n for n, _ in fake.calls] == [gemm, "dmcp_reduce_rope_kv_norm"] and tuple(q.shape) == (M, Hq, D)
        red = fake.calls[1][1]
        assert len(red) == 21 and red[1] >= 1
        assert red[8:16] == (M, Hq, Hkv, D, 128, 128, 3, int(kv_dtype == torch.uint8))
        assert (red[17].value is None) == (bias is None)  # the norm-taking reduction still takes the bias
        assert (red[18].value, red[19].value, red[20]) == (qw.data_ptr(), kw.data_ptr(), EPS)
        for kwargs in ({}, {"qk_norm": None}):
            del fake.calls[:]
            op(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, bias=bias, **kwargs)
            assert [n for n, _ in fake.calls] == [gemm, "dmcp_reduce_rope_kv"]
            old = fake.calls[1][1]
            assert len(old) == 18 and old[8:16] == red[8:16] and old[1] == red[1]
            same = (0, 2, 3, 4, 6, 7)  # workspace, pos, slot, cos_sin, k / v cache (q_out is a new tensor per call)
            assert [old[i].value for i in same] == [red[i].value for i in same]
            assert (old[17].value is None) == (bias is None)


def test_bad_norm_weights_are_refused_before_any_launch(dry):
    hip, fake = dry
    Hq, Hkv, D = GEOMS[0]
    M, N = 40, (Hq + 2 * Hkv) * D
    pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, torch.bfloat16)
    ws = torch.empty(16 * M * N, dtype=torch.float32)
    good = _bf(D)
    bad = [(good, _bf(D - 8), EPS),                       # wrong length
           (_bf(2 * D), good, EPS),
           (good, torch.zeros(D, dtype=torch.float32), EPS),  # wrong dtype
           (_bf(D, 2)[:, 0], good, EPS),                 # not contiguous
           (good, good),                                  # no eps
           (good, None, EPS)]
    for qkn in bad:
        with pytest.raises(hip.HipOpsError):
            hip.rope_kv(_bf(M, N), pos, slot, cs, kc, vc, Hq, qk_norm=qkn)
        with pytest.raises(hip.HipOpsError):
            hip.wgemm_rope_kv(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, qk_norm=qkn)
        with pytest.raises(hip.HipOpsError):
            hip.tgemm_rope_kv(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, qk_norm=qkn)
        assert not fake.calls
    # head sizes outside {64, 128}: the lane groups of a head would not be whole
    for D2 in (32, 96, 256):
        Hq2, Hkv2 = 2, 1
        pos, slot, cs, kc, vc = _rope_inputs(M, Hkv2, D2, torch.bfloat16)
        N2 = (Hq2 + 2 * Hkv2) * D2
        with pytest.raises(hip.HipOpsError, match="head_dim"):
            hip.rope_kv(_bf(M, N2), pos, slot, cs, kc, vc, Hq2, qk_norm=(_bf(D2), _bf(D2), EPS))
        if N2 % 64 == 0:
            with pytest.raises(hip.HipOpsError, match="head_dim"):
                hip.wgemm_rope_kv(_bf(M, K), _bf(N2, K), pos, slot, cs, kc, vc, Hq2,
                                  torch.empty(16 * M * N2, dtype=torch.float32), qk_norm=(_bf(D2), _bf(D2), EPS))
        assert not fake.calls
    # the fused small-row QKV kernel takes no norm: refused, never dropped
    pos, slot, cs, kc, vc = _rope_inputs(8, Hkv, D, torch.bfloat16)
    with pytest.raises(hip.HipOpsError, match="qk_norm"):
        hip.fused_rope_kv(_bf(8, K), _bf(N, K), 1e-5, pos, slot, cs, kc, vc, Hq, qk_norm=(good, good, EPS))
    assert not fake.calls
    hip.fused_rope_kv(_bf(8, K), _bf(N, K), 1e-5, pos, slot, cs, kc, vc, Hq)
    assert [n for n, _ in fake.calls] == ["dmcp_fused_gemm"] and len(fake.calls[0][1]) == 25
