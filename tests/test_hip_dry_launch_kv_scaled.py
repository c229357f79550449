"""The ``kv_scale`` keyword of the KV wrappers (dmcp/ops/hip.py) on the CPU
against a recording stand-in for the library: None calls the earlier entry
point with the earlier argument list, a pair of exponent tables the ``_scaled``
one, bad tables are refused before anything is launched, and a model with an
fp8 or bf16 cache allocates no table."""
import pytest
import torch

from tests.test_hip_dry_launch_qk_norm import _bf, _FakeLib, _rope_inputs, dry  # noqa: F401

K, EPS = 256, 1e-6
GEOMS = [(4, 2, 64), (2, 1, 128)]


def _tables(kc):
    return torch.zeros(kc.shape[:-1], dtype=torch.uint8), torch.zeros(kc.shape[:-1], dtype=torch.uint8)


@pytest.mark.parametrize("Hq,Hkv,D", GEOMS)
def test_rope_kv(dry, Hq, Hkv, D):  # noqa: F811
    hip, fake = dry
    M, N = 16, (Hq + 2 * Hkv) * D
    pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, torch.uint8)
    ks, vs = _tables(kc)
    for kwargs in ({}, {"kv_scale": None}):
        del fake.calls[:]
        hip.rope_kv(_bf(M, N), pos, slot, cs, kc, vc, Hq, **kwargs)
        (name, old), = fake.calls
        assert name == "dmcp_rope_kv" and len(old) == 16
    qw, kw = _bf(D), _bf(D)
    for norm in (None, (qw, kw, EPS)):
        del fake.calls[:]
        hip.rope_kv(_bf(M, N), pos, slot, cs, kc, vc, Hq, qk_norm=norm, kv_scale=(ks, vs))
        (name, args), = fake.calls
        assert name == "dmcp_rope_kv_scaled" and len(args) == 20
        assert args[7:14] == (M, Hq, Hkv, D, 128, 128, 3)
        assert (args[15].value, args[16].value) == ((qw.data_ptr(), kw.data_ptr()) if norm else (None, None))
        assert (args[18].value, args[19].value) == (ks.data_ptr(), vs.data_ptr())


@pytest.mark.parametrize("family,M", [("wgemm", 40), ("tgemm", 610)])
def test_splitk_rope_kv(dry, family, M):  # noqa: F811
    hip, fake = dry
    Hq, Hkv, D = GEOMS[0]
    N = (Hq + 2 * Hkv) * D
    op = getattr(hip, f"{family}_rope_kv")
    ws = torch.empty(16 * M * N, dtype=torch.float32)
    pos, slot, cs, kc, vc = _rope_inputs(M, Hkv, D, torch.uint8)
    ks, vs = _tables(kc)
    op(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, kv_scale=None)
    assert [n for n, _ in fake.calls] == [f"dmcp_{family}", "dmcp_reduce_rope_kv"] and len(fake.calls[1][1]) == 18
    del fake.calls[:]
    bias = _bf(N)
    op(_bf(M, K), _bf(N, K), pos, slot, cs, kc, vc, Hq, ws, bias=bias, kv_scale=(ks, vs))
    assert [n for n, _ in fake.calls] == [f"dmcp_{family}", "dmcp_reduce_rope_kv_scaled"]
    red = fake.calls[1][1]
    assert len(red) == 22 and red[8:15] == (M, Hq, Hkv, D, 128, 128, 3) and red[16].value == bias.data_ptr()
    assert (red[20].value, red[21].value) == (ks.data_ptr(), vs.data_ptr())


def test_attention_and_fork(dry):  # noqa: F811
    hip, fake = dry
    Hq, Hkv, D = GEOMS[0]
    _, _, _, kc, vc = _rope_inputs(4, Hkv, D, torch.uint8)
    ks, vs = _tables(kc)
    q = _bf(4, Hq, D)
    slot = torch.zeros(4, dtype=torch.int32)
    lens = torch.full((4,), 9, dtype=torch.int32)
    for scale, name, n in ((None, "dmcp_decode_attention", 25), ((ks, vs), "dmcp_decode_attention_scaled", 28)):
        del fake.calls[:]
        hip.decode_attention(q, kc, vc, slot, lens, 0.125, splits=1, kv_scale=scale)
        assert [(c, len(a)) for c, a in fake.calls] == [(name, n)]
    for scale, name, n in ((None, "dmcp_prefill_attention", 20), ((ks, vs), "dmcp_prefill_attention_scaled", 23)):
        del fake.calls[:]
        hip.prefill_attention(q, kc, vc, 1, 5, scale=0.125, nsplit=1, kv_scale=scale)
        assert [(c, len(a)) for c, a in fake.calls] == [(name, n)]
        if scale:
            assert fake.calls[0][1][19].value == ks[1].data_ptr()  # the slot's rows of the table
    k5, v5 = kc[None].contiguous(), vc[None].contiguous()
    for scale, name, n in ((None, "dmcp_kv_fork", 13), ((ks[None].contiguous(), vs[None].contiguous()),
                                                       "dmcp_kv_fork_scaled", 15)):
        del fake.calls[:]
        hip.kv_fork(k5, v5, 0, [1, 2], 0, 8, kv_scale=scale)
        assert [(c, len(a)) for c, a in fake.calls] == [(name, n)]


def test_prefix_and_varlen_forms(dry):  # noqa: F811
    """The prefix slot's rows of the tables travel with the prefix: the last
    two of the 28 decode arguments, and pks / pvs = ks / vs[prefix_slot] of the
    20 varlen and 23 dense-prefill arguments."""
    hip, fake = dry
    from dmcp.ops import SharedPrefix
    Hq, Hkv, D = GEOMS[0]
    _, _, _, kc, vc = _rope_inputs(4, Hkv, D, torch.uint8)
    ks, vs = _tables(kc)
    q = _bf(4, Hq, D)
    slot = torch.zeros(4, dtype=torch.int32)
    lens = torch.full((4,), 40, dtype=torch.int32)
    plen = torch.tensor([16], dtype=torch.int32)
    pre = SharedPrefix(kc[2], vc[2], plen, None, ks[2], vs[2])
    ws = hip.decode_workspace
    part = (torch.empty(4 * Hq * 64 * D), torch.empty(4 * Hq * 64 * 2))
    hip.decode_attention(q, kc, vc, slot, lens, 0.125, workspace=part, splits=1, prefix=pre, kv_scale=(ks, vs))
    (name, a), = fake.calls
    assert name == "dmcp_decode_attention_scaled" and len(a) == 28 and ws is not None
    assert (a[17].value, a[18].value) == (kc[2].data_ptr(), vc[2].data_ptr())
    assert [x.value for x in a[24:28]] == [ks.data_ptr(), vs.data_ptr(), ks[2].data_ptr(), vs[2].data_ptr()]
    with pytest.raises(hip.HipOpsError):  # a scaled cache's prefix without its table rows
        hip.decode_attention(q, kc, vc, slot, lens, 0.125, workspace=part, splits=1,
                             prefix=SharedPrefix(kc[2], vc[2], plen), kv_scale=(ks, vs))
    del fake.calls[:]
    hip.prefill_attention(q, kc, vc, 1, 20, 2, 16, 0.125, nsplit=1, kv_scale=(ks, vs))
    (name, a), = fake.calls
    assert name == "dmcp_prefill_attention_scaled" and len(a) == 23
    assert [x.value for x in a[19:23]] == [ks[1].data_ptr(), vs[1].data_ptr(), ks[2].data_ptr(), vs[2].data_ptr()]
    for scale, name, n in ((None, "dmcp_prefill_varlen", 17), ((ks, vs), "dmcp_prefill_varlen_scaled", 20)):
        del fake.calls[:]
        hip._VARLEN_META.clear()
        hip.prefill_attention_varlen(_bf(6, Hq, D), kc, vc, [0, 2, 6], [0, 1], [20, 0], 2, [16, 0], 0.125,
                                     kv_scale=scale)
        (got, a), = fake.calls
        assert got == name and len(a) == n
        if scale:
            assert [x.value for x in a[16:20]] == [ks.data_ptr(), vs.data_ptr(), ks[2].data_ptr(), vs[2].data_ptr()]
    hip._VARLEN_META.clear()


def test_bad_tables_are_refused_before_a_launch(dry):  # noqa: F811
    hip, fake = dry
    Hq, Hkv, D = GEOMS[0]
    pos, slot, cs, kc, vc = _rope_inputs(8, Hkv, D, torch.uint8)
    ks, vs = _tables(kc)
    qkv = _bf(8, (Hq + 2 * Hkv) * D)
    for bad in ((ks,), (ks, vs[:, :, :-1].contiguous()), (ks.int(), vs), (ks, vs.transpose(0, 1)), "ks"):
        with pytest.raises(hip.HipOpsError):
            hip.rope_kv(qkv, pos, slot, cs, kc, vc, Hq, kv_scale=bad)
        with pytest.raises(hip.HipOpsError):
            hip.decode_attention(_bf(8, Hq, D), kc, vc, slot, slot, 0.125, kv_scale=bad)
    with pytest.raises(hip.HipOpsError):  # bf16 caches have no scaled form
        hip.rope_kv(qkv, pos, slot, cs, kc.bfloat16(), vc.bfloat16(), Hq, kv_scale=(ks, vs))
    with pytest.raises(hip.HipOpsError):  # the fused QKV tile has no scaled writer
        hip.fused_rope_kv(_bf(8, K), _bf(qkv.shape[1], K), 1e-5, pos, slot, cs, kc, vc, Hq, kv_scale=(ks, vs))
    assert not fake.calls


@pytest.mark.parametrize("kv", ["fp8", "bf16"])
def test_unscaled_models_take_the_earlier_entry_points(kv, monkeypatch):
    """No table is allocated and every KV op is called with kv_scale=None
    (which the tests above tie to the earlier entry points)."""
    from dmcp import ops
    from dmcp.models.llm import LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype=kv), device="cpu")
    assert m.k_scale is None and m.v_scale is None and m._kvs(0) is None
    seen = []
    for name in ("rope_kv", "decode_attention"):
        real = getattr(ops, name)

        def spy(*a, _real=real, _name=name, **k):
            seen.append((_name, k.get("kv_scale")))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    m.forward_tokens(torch.tensor([256, 65, 66], dtype=torch.int32), 0, 0)
    one = torch.zeros(1, dtype=torch.int32)
    m.decode(torch.tensor([67], dtype=torch.int32), one, torch.tensor([3], dtype=torch.int32))
    assert {n for n, _ in seen} == {"rope_kv", "decode_attention"} and all(s is None for _, s in seen)
