"""The sigmoid-routed MLP's wrappers (dmcp/ops/hip.py moe_route_sig /
moe_mlp_sh) on the CPU against the recording stand-in of
tests/test_hip_dry_launch_qk_norm.py: entry-point names and argument lists,
workspace parts sized for k + S pairs and E + S groups, refusals before any
call, and the models that must not reach them."""
import pytest
import torch

from tests.test_hip_dry_launch_qk_norm import _bf, dry  # noqa: F401 -- the fake-library fixture

H, I, E, K = 256, 128, 8, 2


def _weights(S):
    return _bf(E, H), torch.zeros(E), _bf(E + S, 2 * I, H), _bf(E + S, H, I)


def test_abi_version_stays_20():
    from dmcp.ops import hip
    assert hip.ABI_VERSION == 20


def test_shape_contract():
    from dmcp.ops import hip
    assert hip.moe_sh_supported(4096, 1408, 128, 8, 1)       # GLM-4.5-Air
    assert hip.moe_sh_supported(5120, 1536, 160, 8, 1)       # GLM-4.5
    assert hip.moe_sh_supported(64, 64, 1, 1, 0) and hip.moe_sh_supported(8192, 64, 255, 255, 1)
    for bad in ((4096, 1408, 256, 8, 1),                     # E + S > 256
                (4096, 1408, 128, 8, 65), (4096, 1408, 128, 8, -1), (4096, 1408, 8, 9, 1), (4096, 1408, 128, 0, 1),
                (4096, 1400, 128, 8, 1), (4100, 1408, 128, 8, 1), (8256, 1408, 128, 8, 1)):
        assert not hip.moe_sh_supported(*bad), bad
    # S = 0 is moe_supported's contract
    for g in ((2048, 768, 128, 8), (2048, 800, 128, 8), (2048, 768, 257, 8)):
        assert hip.moe_sh_supported(*g, 0) == hip.moe_supported(*g)


@pytest.mark.parametrize("S", [0, 1, 2])
def test_route_entry_point(dry, S):
    hip, fake = dry
    wr, bias, _, _ = _weights(S)
    h = _bf(40, H)
    ids, p = hip.moe_route_sig(h, wr, bias, K, True, 2.5, S)
    (name, a), = fake.calls
    assert name == "dmcp_moe_route_sig" and len(a) == 13
    assert [x.value for x in a[:5]] == [h.data_ptr(), wr.data_ptr(), bias.data_ptr(), ids.data_ptr(), p.data_ptr()]
    assert a[5:11] == (40, H, E, K, S, 1) and a[11] == 2.5
    assert ids.dtype == torch.int32 and p.dtype == torch.float32 and tuple(ids.shape) == tuple(p.shape) == (40, K + S)


@pytest.mark.parametrize("S", [0, 1, 2])
@pytest.mark.parametrize("T", [1, 40, 600])
def test_mlp_entry_point(dry, T, S):
    hip, fake = dry
    wr, bias, wgu, wd = _weights(S)
    h, resid, nw = _bf(T, H), _bf(T, H), _bf(H)
    ws = hip.moe_sh_workspace(T, H, I, E, K, S, "cpu")
    out = hip.moe_mlp_sh(h, wr, bias, wgu, wd, K, True, 2.0, S, residual=resid, norm_w=nw, eps=1e-6, workspace=ws)
    (name, a), = fake.calls
    assert name == "dmcp_moe_mlp_sh" and len(a) == 28
    assert [x.value for x in a[:5]] == [h.data_ptr(), wr.data_ptr(), bias.data_ptr(), wgu.data_ptr(), wd.data_ptr()]
    parts = [x.value - ws.data_ptr() for x in a[5:14]]
    G, KK = E + S, K + S
    offs, need = hip._moe_layout(T, H, I, G, KK)
    assert parts == list(offs) and all(o % 256 == 0 for o in offs) and need == ws.numel()
    P = T * KK
    sizes = (4 * P, 4 * P, 4 * G, 4 * (G + 1), 4 * P, 12 * (-(-P // 32) + G), 4, 2 * P * I, 4 * P * H)
    assert all(o + s <= n for o, s, n in zip(offs, sizes, list(offs[1:]) + [need]))  # parts do not overlap
    assert [x.value for x in a[14:17]] == [resid.data_ptr(), nw.data_ptr(), out.data_ptr()]
    tile = hip.moe_row_tile(T, G, KK)
    assert a[17:24] == (T, H, I, E, K, S, 1) and a[24] == 2.0 and a[25] == tile and abs(a[26] - 1e-6) < 1e-12
    assert tile == (128 if T * KK >= 64 * G else 32)
    # a workspace sized without the shared pairs is too small once S > 0
    if S:
        with pytest.raises(hip.HipOpsError, match="workspace"):
            hip.moe_mlp_sh(h, wr, bias, wgu, wd, K, True, 2.0, S, workspace=hip.moe_workspace(T, H, I, E, K, "cpu"))
    del fake.calls[:]
    assert hip.moe_mlp_sh(h, wr, bias, wgu, wd, K, False, 1.0, S, residual=resid, workspace=ws) is resid
    a = fake.calls[0][1]
    assert a[14].value == resid.data_ptr() and a[15].value is None and a[16].value is None and a[23] == 0


def test_bad_arguments_are_refused_before_any_call(dry):
    hip, fake = dry
    S = 1
    wr, bias, wgu, wd = _weights(S)
    h = _bf(8, H)
    small = hip.moe_sh_workspace(7, H, I, E, K, S, "cpu")
    bad = [dict(h=_bf(8, H + 64)), dict(h=torch.zeros(8, H)), dict(h=_bf(8, 2 * H)[:, ::2]),
           dict(bias=torch.zeros(E + 1)), dict(bias=torch.zeros(E, dtype=torch.bfloat16)), dict(bias=None),
           dict(wgu=_bf(E, 2 * I, H)),                               # the shared slice is missing from the stack
           dict(wgu=_bf(E + 2, 2 * I, H)), dict(wd=_bf(E + S, H, I + 64)), dict(wgu=torch.zeros(E + S, 2 * I, H)),
           dict(k=0), dict(k=E + 1), dict(k=2.0), dict(S=-1), dict(S=1.0), dict(S=True),
           dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(scale="2"),
           dict(kw=dict(workspace=small)), dict(kw=dict(workspace=small.float())),
           dict(kw=dict(residual=_bf(7, H))), dict(kw=dict(norm_w=_bf(H + 8))), dict(kw=dict(out=_bf(4, H)))]
    for b in bad:
        with pytest.raises(hip.HipOpsError):
            hip.moe_mlp_sh(b.get("h", h), wr, b.get("bias", bias), b.get("wgu", wgu), b.get("wd", wd), b.get("k", K),
                           True, b.get("scale", 1.0), b.get("S", S), **b.get("kw", {}))
        assert not fake.calls, b
    with pytest.raises(hip.HipOpsError, match="moe_sh_supported"):   # 256 routed + 1 shared
        hip.moe_route_sig(_bf(8, 64), _bf(256, 64), torch.zeros(256), 2, True, 1.0, 1)
    with pytest.raises(hip.HipOpsError, match="moe_sh_supported"):
        hip.moe_mlp_sh(h, wr, bias, _bf(E + S, 192, H), _bf(E + S, H, 96), K, True, 1.0, S)
    with pytest.raises(hip.HipOpsError):
        hip.moe_sh_workspace(8, H, I, 256, K, 1, "cpu")
    assert not fake.calls


GLM = dict(n_experts=4, experts_per_tok=2, moe_intermediate=64, moe_score="sigmoid", moe_route_scale=2.0, moe_shared=1,
           dense_lead=1, rotary_dim=32)


def _spy(monkeypatch):
    from dmcp import ops
    called = []
    for name in ("moe_mlp", "moe_route", "moe_mlp_w8", "moe_mlp_sh", "moe_route_sig"):
        for mod in (ops, ops.reference):
            real = getattr(mod, name)
            monkeypatch.setattr(mod, name, lambda *a, _n=name, _r=real, **k: (called.append(_n), _r(*a, **k))[1])
    return called


def _run_every_path(m):
    toks = torch.tensor([256, 72, 105], dtype=torch.int32)
    m.forward_tokens(toks, 0, 0)
    m.prefill_batch([([256, 1, 2], 0, 0), ([256, 3], 1, 0)])
    m.decode(torch.tensor([5, 6], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
             torch.tensor([3, 2], dtype=torch.int32))
    m.reference_logits([256, 72, 105])


def test_a_dense_and_a_qwen3_moe_model_reach_no_sigmoid_op(monkeypatch):
    from dmcp.models.llm import LocalLM, preset
    called = _spy(monkeypatch)
    dense = LocalLM(preset("tiny", max_batch=2, max_seq=64, max_rows=4), device="cpu")
    assert not dense.moe and not dense.moe_sig and dense.moe_ws is None
    _run_every_path(dense)
    assert not called
    q = LocalLM(preset("tiny", max_batch=2, max_seq=64, max_rows=4, n_experts=4, experts_per_tok=2,
                       moe_intermediate=64), device="cpu")
    assert q.moe and not q.moe_sig and not any(k.endswith(".router_bias") for k in q.w)
    _run_every_path(q)
    assert called and set(called) == {"moe_mlp"}


def test_a_qwen3_moe_model_still_reaches_dmcp_moe_mlp_with_25_arguments(dry):
    """``LocalLM._moe`` of a softmax-routed model makes the call it made: the
    existing entry point, its 25 arguments, no new one."""
    hip, fake = dry
    from dmcp.models.llm import LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, max_rows=4, n_experts=4, experts_per_tok=2,
                       moe_intermediate=64), device="cpu")
    c = m.cfg
    h, resid = _bf(3, c.hidden), _bf(3, c.hidden)
    hip.moe_mlp(h, m.w["l0.router"], m.w["l0.we_gu"], m.w["l0.we_down"], c.experts_per_tok, c.norm_topk,
                residual=resid, norm_w=m.w["l1.ln1"], eps=c.eps)
    (name, a), = fake.calls
    assert name == "dmcp_moe_mlp" and len(a) == 25 and a[16:23] == (3, 256, 64, 4, 2, 1, 32)


def test_a_glm_preset_runs_the_op_on_every_path(monkeypatch):
    from dmcp.models.llm import LocalLM, preset
    cfg = preset("tiny", max_batch=2, max_seq=64, max_rows=4, **GLM)
    m = LocalLM(cfg, device="cpu")
    assert m.moe and m.moe_sig and "l0.wgu" in m.w and "l0.router" not in m.w
    assert m.w["l1.we_gu"].shape == (5, 128, 256) and m.w["l1.router_bias"].dtype == torch.float32
    assert bool((m.cos_sin[:, 16:, 0] == 1).all()) and bool((m.cos_sin[:, 16:, 1] == 0).all())
    assert cfg.param_count() == sum(v.numel() for k, v in m.w.items() if not k.endswith("router_bias"))
    toks = [256, 72, 105, 33]
    ref = m.reference_logits(toks)[-1]
    got = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float()
    assert (got - ref).abs().max() < 0.05 * max(1.0, ref.abs().max().item())
    both = m.prefill_batch([(toks, 0, 0), (toks[:3], 1, 0)]).float()
    assert (both[0] - ref).abs().max() < 0.05 * max(1.0, ref.abs().max().item())
    m.moe_rows = 3  # a prefill longer than the workspace walks its rows in chunks
    again = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float()
    assert torch.equal(again, got)
    called = _spy(monkeypatch)
    _run_every_path(m)
    # one routed layer x three bf16 forward paths (the 5-row batched prefill in two chunks of <= 3 rows)
    assert set(called) == {"moe_mlp_sh"} and len(called) == 4
    for knob in ("prefill_dtype", "decode_dtype"):
        with pytest.raises(ValueError, match=knob):
            LocalLM(preset("tiny", **GLM, **{knob: "fp8"}), device="cpu")
    for bad in (dict(moe_score="tanh"), dict(moe_shared=-1), dict(moe_route_scale=0.0), dict(dense_lead=3),
                dict(rotary_dim=30 + 1), dict(rotary_dim=128), dict(moe_weight_dtype="fp8b")):
        with pytest.raises(ValueError):
            LocalLM(preset("tiny", **{**GLM, **bad}), device="cpu")
    for bad in (dict(moe_shared=1), dict(moe_route_scale=2.0)):  # the softmax router has neither
        with pytest.raises(ValueError):
            LocalLM(preset("tiny", n_experts=4, experts_per_tok=2, moe_intermediate=64, **bad), device="cpu")
    for bad in (dict(moe_shared=1), dict(moe_route_scale=2.0), dict(dense_lead=1)):  # nor a dense model
        with pytest.raises(ValueError):
            LocalLM(preset("tiny", **bad), device="cpu")


def test_new_config_fields_default_to_the_behaviour_there_was():
    from dmcp.models.llm import LMConfig
    c = LMConfig()
    assert (c.moe_score, c.moe_route_scale, c.moe_shared, c.dense_lead, c.rotary_dim) == ("softmax", 1.0, 0, 0, 0)
    q = LMConfig(n_experts=8, experts_per_tok=2, moe_intermediate=128, layers=3)
    assert all(q.sparse_layer(i) for i in range(3)) and not any(c.sparse_layer(i) for i in range(c.layers))
    assert q.param_count() == 3 * (q.qkv_dim * q.hidden + q.n_heads * q.head_dim * q.hidden
                                   + 8 * (3 * 128 + 1) * q.hidden + 2 * q.hidden) \
        + 2 * q.vocab_size * q.hidden + q.hidden
