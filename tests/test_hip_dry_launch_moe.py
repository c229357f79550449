"""The routed expert MLP's wrappers (dmcp/ops/hip.py moe_route / moe_mlp) on
the CPU against the recording stand-in of tests/test_hip_dry_launch_qk_norm.py:
entry-point names and argument lists, refusals before any call, and a dense
model that never reaches them."""
import pytest
import torch

from tests.test_hip_dry_launch_qk_norm import _bf, dry  # noqa: F401 -- the fake-library fixture

H, I, E, K = 256, 128, 8, 2


def _weights():
    return _bf(E, H), _bf(E, 2 * I, H), _bf(E, H, I)


def test_shape_contract():
    from dmcp.ops import hip
    assert hip.moe_supported(2048, 768, 128, 8)          # Qwen3-30B-A3B
    assert hip.moe_supported(64, 64, 1, 1) and hip.moe_supported(8192, 64, 256, 256)
    for bad in ((2048, 768, 128, 0), (2048, 768, 8, 9), (2048, 768, 257, 8), (2080, 768, 128, 8),
                (2048, 800, 128, 8), (8256, 768, 128, 8), (0, 768, 128, 8)):
        assert not hip.moe_supported(*bad), bad
    assert hip.moe_row_tile(768, 128, 8) == 32 and hip.moe_row_tile(1024, 128, 8) == 128


def test_route_entry_point(dry):
    hip, fake = dry
    wr, _, _ = _weights()
    ids, p = hip.moe_route(_bf(40, H), wr, K, True)
    (name, args), = fake.calls
    assert name == "dmcp_moe_route" and len(args) == 10 and args[4:9] == (40, H, E, K, 1)
    assert ids.dtype == torch.int32 and p.dtype == torch.float32 and tuple(ids.shape) == tuple(p.shape) == (40, K)
    assert (args[2].value, args[3].value) == (ids.data_ptr(), p.data_ptr())


@pytest.mark.parametrize("T,tile", [(1, 32), (40, 32), (255, 32), (256, 128), (600, 128)])
def test_mlp_entry_point(dry, T, tile):
    hip, fake = dry
    wr, wgu, wd = _weights()
    h, resid, nw = _bf(T, H), _bf(T, H), _bf(H)
    ws = torch.empty(hip._moe_layout(T, H, I, E, K)[1], dtype=torch.uint8)
    out = hip.moe_mlp(h, wr, wgu, wd, K, True, residual=resid, norm_w=nw, eps=1e-6, workspace=ws)
    (name, a), = fake.calls
    assert name == "dmcp_moe_mlp" and len(a) == 25
    assert [x.value for x in a[:4]] == [h.data_ptr(), wr.data_ptr(), wgu.data_ptr(), wd.data_ptr()]
    parts = [x.value - ws.data_ptr() for x in a[4:13]]
    offs, need = hip._moe_layout(T, H, I, E, K)
    assert parts == list(offs) and all(o % 256 == 0 for o in offs) and need == ws.numel()
    sizes = (4 * T * K, 4 * T * K, 4 * E, 4 * (E + 1), 4 * T * K, 12 * (-(-T * K // 32) + E), 4, 2 * T * K * I,
             4 * T * K * H)
    assert all(o + s <= n for o, s, n in zip(offs, sizes, list(offs[1:]) + [need]))  # parts do not overlap
    assert [x.value for x in a[13:16]] == [resid.data_ptr(), nw.data_ptr(), out.data_ptr()]
    assert a[16:23] == (T, H, I, E, K, 1, tile) and abs(a[23] - 1e-6) < 1e-12
    # residual alone: no out; neither: out only
    del fake.calls[:]
    assert hip.moe_mlp(h, wr, wgu, wd, K, False, residual=resid, workspace=ws) is resid
    a = fake.calls[0][1]
    assert a[13].value == resid.data_ptr() and a[14].value is None and a[15].value is None and a[21] == 0
    del fake.calls[:]
    m = hip.moe_mlp(h, wr, wgu, wd, K, True)
    a = fake.calls[0][1]
    assert a[13].value is None and a[14].value is None and a[15].value == m.data_ptr() and m.shape == h.shape


def test_bad_arguments_are_refused_before_any_call(dry):
    hip, fake = dry
    wr, wgu, wd = _weights()
    h = _bf(8, H)
    small = torch.empty(hip._moe_layout(7, H, I, E, K)[1], dtype=torch.uint8)
    bad = [dict(h=_bf(8, H + 64)),                                   # hidden does not match the router
           dict(h=torch.zeros(8, H)),                                # dtype
           dict(h=_bf(8, 2 * H)[:, ::2]),                            # not contiguous
           dict(wgu=_bf(E, 2 * I, H + 64)), dict(wgu=_bf(E + 1, 2 * I, H)), dict(wd=_bf(E, H, I + 64)),
           dict(wgu=torch.zeros(E, 2 * I, H)),
           dict(k=0), dict(k=E + 1), dict(k=2.0),
           dict(kw=dict(workspace=small)), dict(kw=dict(workspace=small.float())),
           dict(kw=dict(residual=_bf(7, H))), dict(kw=dict(residual=torch.zeros(8, H))),
           dict(kw=dict(norm_w=_bf(H + 8))), dict(kw=dict(norm_w=torch.zeros(H))),
           dict(kw=dict(out=_bf(4, H)))]
    for b in bad:
        with pytest.raises(hip.HipOpsError):
            hip.moe_mlp(b.get("h", h), wr, b.get("wgu", wgu), b.get("wd", wd), b.get("k", K), True, **b.get("kw", {}))
        assert not fake.calls, b
    # shapes outside the contract: intermediate 96, hidden 96, 257 experts
    with pytest.raises(hip.HipOpsError, match="moe_supported"):
        hip.moe_mlp(h, wr, _bf(E, 192, H), _bf(E, H, 96), K, True)
    with pytest.raises(hip.HipOpsError, match="moe_supported"):
        hip.moe_mlp(_bf(8, 96), _bf(E, 96), _bf(E, 2 * I, 96), _bf(E, 96, I), K, True)
    with pytest.raises(hip.HipOpsError, match="moe_supported"):
        hip.moe_route(_bf(8, 64), _bf(257, 64), 2, True)
    with pytest.raises(hip.HipOpsError):
        hip.moe_route(h, wr, E + 1, True)
    with pytest.raises(hip.HipOpsError):
        hip.moe_workspace(8, H, 96, E, K, "cpu")
    assert not fake.calls


def test_a_dense_model_calls_no_moe_op(monkeypatch):
    from dmcp import ops
    from dmcp.models.llm import LocalLM, preset
    called = []
    for name in ("moe_mlp", "moe_route"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: called.append(_n))
        monkeypatch.setattr(ops.reference, name, lambda *a, _n=name, **k: called.append(_n))
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, max_rows=4), device="cpu")
    assert not m.moe and m.moe_ws is None and m.moe_rows is None
    assert not any(k.endswith((".router", ".we_gu", ".we_down")) for k in m.w)
    toks = torch.tensor([256, 72, 105], dtype=torch.int32)
    m.forward_tokens(toks, 0, 0)
    m.prefill_batch([([256, 1, 2], 0, 0), ([256, 3], 1, 0)])
    m.decode(torch.tensor([5, 6], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
             torch.tensor([3, 2], dtype=torch.int32))
    m.reference_logits([256, 72, 105])
    assert not called


def test_a_moe_preset_runs_the_op_on_every_path():
    from dmcp.models.llm import LocalLM, preset
    cfg = preset("tiny", max_batch=2, max_seq=64, max_rows=4, n_experts=4, experts_per_tok=2, moe_intermediate=64)
    m = LocalLM(cfg, device="cpu")
    assert m.moe and m.w["l0.we_gu"].shape == (4, 128, 256) and "l0.wgu" not in m.w
    toks = [256, 72, 105, 33]
    ref = m.reference_logits(toks)[-1]
    got = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float()
    assert (got - ref).abs().max() < 0.05 * max(1.0, ref.abs().max().item())
    both = m.prefill_batch([(toks, 0, 0), (toks[:3], 1, 0)]).float()
    assert (both[0] - ref).abs().max() < 0.05 * max(1.0, ref.abs().max().item())
    m.moe_rows = 3  # a prefill longer than the workspace walks its rows in chunks
    again = m.forward_tokens(torch.tensor(toks, dtype=torch.int32), 0, 0).float()
    assert torch.equal(again, got)
    for knob in ("prefill_dtype", "decode_dtype"):
        with pytest.raises(ValueError, match=knob):
            LocalLM(preset("tiny", n_experts=4, experts_per_tok=2, moe_intermediate=64, **{knob: "fp8"}), device="cpu")
