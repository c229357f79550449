"""The wrapper of the routed expert MLP over block-scaled FP8 weights
(dmcp/ops/hip.py moe_mlp_w8) on the CPU against the recording stand-in of
tests/test_hip_dry_launch_qk_norm.py: the entry point's name and its 27
arguments in order, workspace parts identical to moe_mlp's, every refusal
before any call, the ABI number, and models that never reach the entry point
(bf16 experts, dense)."""
import pytest
import torch

from tests.test_hip_dry_launch_qk_norm import _bf, dry  # noqa: F401 -- the fake-library fixture

H, I, E, K = 320, 192, 8, 2     # 2.5 and 1.5 scale blocks: the scale shapes are ceil-divided
NBH, NBI = 3, 2


def _f8(*shape):
    return torch.zeros(shape, dtype=torch.float8_e4m3fn)


def _f32(*shape):
    return torch.ones(shape, dtype=torch.float32)


def _weights():
    return _bf(E, H), _f8(E, 2 * I, H), _f32(E, 2 * NBI, NBH), _f8(E, H, I), _f32(E, NBH, NBI)


def test_abi_version_stays_20():
    from dmcp.ops import hip
    assert hip.ABI_VERSION == 20
    assert hip.MOE_W8_BLOCK == 128


@pytest.mark.parametrize("T,tile", [(1, 32), (40, 32), (255, 32), (256, 128), (600, 128)])
def test_entry_point_and_its_27_arguments(dry, T, tile):
    hip, fake = dry
    wr, gu8, gs, d8, ds = _weights()
    h, resid, nw = _bf(T, H), _bf(T, H), _bf(H)
    ws = torch.empty(hip._moe_layout(T, H, I, E, K)[1], dtype=torch.uint8)
    out = hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, K, True, residual=resid, norm_w=nw, eps=1e-6, workspace=ws)
    (name, a), = fake.calls
    assert name == "dmcp_moe_mlp_w8" and len(a) == 27
    assert [x.value for x in a[:6]] == [t.data_ptr() for t in (h, wr, gu8, gs, d8, ds)]
    parts = [x.value - ws.data_ptr() for x in a[6:15]]
    assert [x.value for x in a[15:18]] == [resid.data_ptr(), nw.data_ptr(), out.data_ptr()]
    assert a[18:25] == (T, H, I, E, K, 1, tile) and abs(a[25] - 1e-6) < 1e-12 and a[26] is None
    # the workspace parts are moe_mlp's, offset for offset
    del fake.calls[:]
    hip.moe_mlp(h, wr, _bf(E, 2 * I, H), _bf(E, H, I), K, True, residual=resid, norm_w=nw, eps=1e-6, workspace=ws)
    (name16, b), = fake.calls
    assert name16 == "dmcp_moe_mlp" and len(b) == 25
    assert parts == [x.value - ws.data_ptr() for x in b[4:13]] == list(hip._moe_layout(T, H, I, E, K)[0])
    assert a[18:26] == b[16:24]
    # residual alone: no out; neither: out only
    del fake.calls[:]
    assert hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, K, False, residual=resid, workspace=ws) is resid
    a = fake.calls[0][1]
    assert a[15].value == resid.data_ptr() and a[16].value is None and a[17].value is None and a[23] == 0
    del fake.calls[:]
    m = hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, K, True)
    a = fake.calls[0][1]
    assert a[15].value is None and a[16].value is None and a[17].value == m.data_ptr() and m.shape == h.shape


def test_the_library_signature_has_27_arguments():
    """hip.lib() declares the entry point (a library without it is refused by name there)."""
    import inspect
    from dmcp.ops import hip
    src = inspect.getsource(hip.lib)
    assert '"dmcp_moe_mlp_w8": ([_vp] * 18 + [_i, _i, _i, _i, _i, _i, _i, _f, _vp], _i)' in src
    assert '"dmcp_moe_mlp": ([_vp] * 16 + [_i, _i, _i, _i, _i, _i, _i, _f, _vp], _i)' in src


def test_bad_arguments_are_refused_before_any_call(dry):
    hip, fake = dry
    wr, gu8, gs, d8, ds = _weights()
    h = _bf(8, H)
    small = torch.empty(hip._moe_layout(7, H, I, E, K)[1], dtype=torch.uint8)
    bad = [dict(h=_bf(8, H + 64)), dict(h=torch.zeros(8, H)), dict(h=_bf(8, 2 * H)[:, ::2]),
           # the weights: e4m3 only -- not its uint8 view, not bf16 -- and of the op's shapes
           dict(gu8=gu8.view(torch.uint8)), dict(d8=d8.view(torch.uint8)), dict(gu8=_bf(E, 2 * I, H)),
           dict(gu8=torch.zeros(E, 2 * I, H).to(torch.float8_e5m2)),
           dict(gu8=_f8(E, 2 * I, H + 64)), dict(gu8=_f8(E + 1, 2 * I, H)), dict(d8=_f8(E, H, I + 64)),
           dict(gu8=_f8(E, 2 * I, 2 * H)[:, :, ::2]),
           # the scales: fp32, contiguous, exactly [E, 2 ceil(I/128), ceil(H/128)] and [E, ceil(H/128), ceil(I/128)]
           dict(gs=_f32(E, 2 * NBI, NBH).to(torch.bfloat16)), dict(gs=_f32(E, 2 * NBI, NBH).double()),
           dict(gs=_f32(E, NBI, NBH)), dict(gs=_f32(E, 2 * NBI, NBH - 1)), dict(gs=_f32(E, 2, 2)),
           dict(gs=_f32(E, 2 * NBI + 1, NBH)), dict(gs=_f32(E + 1, 2 * NBI, NBH)), dict(gs=_f32(E, 2 * NBI, 2 * NBH)[:, :, ::2]),
           dict(gs=None), dict(ds=None),
           dict(ds=_f32(E, NBI, NBH)), dict(ds=_f32(E, NBH, NBI + 1)), dict(ds=_f32(E, NBH * NBI)),
           dict(ds=_f32(E, NBH, NBI).half()),
           dict(k=0), dict(k=E + 1), dict(k=2.0),
           dict(kw=dict(workspace=small)), dict(kw=dict(workspace=small.float())),
           dict(kw=dict(residual=_bf(7, H))), dict(kw=dict(residual=torch.zeros(8, H))),
           dict(kw=dict(norm_w=_bf(H + 8))), dict(kw=dict(norm_w=torch.zeros(H))),
           dict(kw=dict(out=_bf(4, H)))]
    for b in bad:
        with pytest.raises(hip.HipOpsError):
            hip.moe_mlp_w8(b.get("h", h), wr, b.get("gu8", gu8), b.get("gs", gs), b.get("d8", d8), b.get("ds", ds),
                           b.get("k", K), True, **b.get("kw", {}))
        assert not fake.calls, b
    # geometry outside moe_supported: intermediate 96, hidden 96
    with pytest.raises(hip.HipOpsError, match="moe_supported"):
        hip.moe_mlp_w8(h, wr, _f8(E, 192, H), _f32(E, 2, NBH), _f8(E, H, 96), _f32(E, NBH, 1), K, True)
    with pytest.raises(hip.HipOpsError, match="moe_supported"):
        hip.moe_mlp_w8(_bf(8, 96), _bf(E, 96), _f8(E, 2 * I, 96), _f32(E, 2 * NBI, 1), _f8(E, 96, I),
                       _f32(E, 1, NBI), K, True)
    assert not fake.calls
    # and the well-formed call goes through
    hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, K, True)
    assert [c[0] for c in fake.calls] == ["dmcp_moe_mlp_w8"]


def test_an_empty_batch_launches_nothing(dry):
    hip, fake = dry
    wr, gu8, gs, d8, ds = _weights()
    out = hip.moe_mlp_w8(_bf(0, H), wr, gu8, gs, d8, ds, K, True)
    assert out.shape == (0, H) and not fake.calls


def test_bf16_and_dense_models_never_reach_the_w8_entry_point(monkeypatch):
    from dmcp import ops
    from dmcp.models.llm import LocalLM, preset
    called = []
    monkeypatch.setattr(ops, "moe_mlp_w8", lambda *a, **k: called.append("ops"))
    monkeypatch.setattr(ops.reference, "moe_mlp_w8", lambda *a, **k: called.append("reference"))
    monkeypatch.setattr(ops.hip, "moe_mlp_w8", lambda *a, **k: called.append("hip"))
    kw = dict(max_batch=2, max_seq=64, max_rows=4)
    for cfg in (preset("tiny", **kw), preset("tiny", n_experts=4, experts_per_tok=2, moe_intermediate=64, **kw)):
        m = LocalLM(cfg, device="cpu")
        assert not m.moe_w8 and not any(k.endswith(("we_gu8", "we_down8", "we_gu_s", "we_down_s")) for k in m.w)
        m.forward_tokens(torch.tensor([256, 72, 105], dtype=torch.int32), 0, 0)
        m.prefill_batch([([256, 1, 2], 0, 0), ([256, 3], 1, 0)])
        m.decode(torch.tensor([5, 6], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
                 torch.tensor([3, 2], dtype=torch.int32))
        m.reference_logits([256, 72, 105])
    assert not called


def test_an_fp8b_model_calls_the_w8_op_on_every_path(monkeypatch):
    from dmcp import ops
    from dmcp.models.llm import LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, max_rows=4, n_experts=4, experts_per_tok=2,
                       moe_intermediate=64, moe_weight_dtype="fp8b"), device="cpu")
    calls = {"w8": 0}
    real = ops.moe_mlp_w8

    def spy(*a, **k):
        calls["w8"] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, "moe_mlp_w8", spy)
    monkeypatch.setattr(ops, "moe_mlp", lambda *a, **k: pytest.fail("the bf16 op on an fp8b model"))
    layers = m.cfg.layers
    m.forward_tokens(torch.tensor([256, 72, 105], dtype=torch.int32), 0, 0)
    assert calls["w8"] == layers
    m.prefill_batch([([256, 1, 2], 0, 0), ([256, 3], 1, 0)])
    assert calls["w8"] == 2 * layers
    m.decode(torch.tensor([5, 6], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
             torch.tensor([3, 2], dtype=torch.int32))
    assert calls["w8"] == 3 * layers
    m.moe_rows = 2  # three rows in chunks of two
    m.forward_tokens(torch.tensor([256, 72, 105], dtype=torch.int32), 1, 0)
    assert calls["w8"] == 5 * layers
