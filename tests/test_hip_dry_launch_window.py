"""The ``window`` keyword of the attention wrappers (dmcp/ops/hip.py) on the CPU
against the recording stand-in of tests/test_hip_dry_launch_qk_norm.py: 0 or
None calls the earlier entry points with the earlier argument lists, a window
the ``_window`` ones with W last, a bad window is refused before anything is
launched, and only a model's windowed layers pass one."""
import pytest
import torch

from tests.test_hip_dry_launch_qk_norm import _bf, _FakeLib, _rope_inputs, dry  # noqa: F401

Hq, Hkv, D = 4, 2, 64


def _inputs(kv_dtype):
    _, _, _, kc, vc = _rope_inputs(4, Hkv, D, kv_dtype)
    tabs = (torch.zeros(kc.shape[:-1], dtype=torch.uint8), torch.zeros(kc.shape[:-1], dtype=torch.uint8))
    return kc, vc, tabs, torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32)


def test_abi_version_stays_20():
    from dmcp.ops import hip
    assert hip.ABI_VERSION == 20


@pytest.mark.parametrize("window", [0, None])
def test_no_window_is_the_earlier_call(dry, window):  # noqa: F811
    hip, fake = dry
    kc, vc, tabs, slot, lens = _inputs(torch.uint8)
    q = _bf(4, Hq, D)
    for scale, names in ((None, ("dmcp_decode_attention", "dmcp_prefill_attention", "dmcp_prefill_varlen")),
                         (tabs, ("dmcp_decode_attention_scaled", "dmcp_prefill_attention_scaled",
                                 "dmcp_prefill_varlen_scaled"))):
        del fake.calls[:]
        hip.decode_attention(q, kc, vc, slot, lens, 0.125, splits=1, kv_scale=scale, window=window)
        hip.prefill_attention(q, kc, vc, 1, 0, scale=0.125, nsplit=1, kv_scale=scale, window=window)
        hip.prefill_attention_varlen(q, kc, vc, [0, 4], [1], [0], scale=0.125, kv_scale=scale, window=window)
        assert tuple(n for n, _ in fake.calls) == names
        assert [len(a) for _, a in fake.calls] == ([25, 20, 17] if scale is None else [28, 23, 20])


@pytest.mark.parametrize("kv", ["bf16", "fp8", "fp8s"])
def test_window_calls_the_window_entry_points(dry, kv):  # noqa: F811
    hip, fake = dry
    kc, vc, tabs, slot, lens = _inputs(torch.bfloat16 if kv == "bf16" else torch.uint8)
    scale = tabs if kv == "fp8s" else None
    kv8 = int(kv != "bf16")
    q = _bf(4, Hq, D)
    W = 37
    from dmcp.ops.reference import SharedPrefix
    pre = SharedPrefix(kc[2], vc[2], torch.zeros(1, dtype=torch.int32), None,
                       tabs[0][2] if scale else None, tabs[1][2] if scale else None)
    hip.decode_attention(q, kc, vc, slot, lens, 0.125, splits=1, prefix=pre, kv_scale=scale, window=W)
    hip.prefill_attention(q, kc, vc, 1, 8, 2, 8, 0.125, nsplit=1, kv_scale=scale, window=W)
    hip.prefill_attention_varlen(q, kc, vc, [0, 4], [1], [8], 2, [8], 0.125, kv_scale=scale, window=W)
    (n0, a0), (n1, a1), (n2, a2) = fake.calls
    assert (n0, n1, n2) == ("dmcp_decode_attention_window", "dmcp_prefill_attention_window",
                            "dmcp_prefill_varlen_window")
    assert (len(a0), len(a1), len(a2)) == (30, 25, 22)
    assert a0[-1] == a1[-1] == a2[-1] == W  # the window is the last argument of each
    assert a0[21] == a1[18] == a2[15] == kv8  # kv8 where the unscaled sibling has it
    # the exponent tables (k, v, prefix k, v) behind the stream: null for the unscaled formats
    for a, first in ((a0, 25), (a1, 20), (a2, 17)):
        ptrs = [a[first + i].value for i in range(4)]
        assert all(p is not None for p in ptrs) if scale else all(p is None for p in ptrs), (kv, ptrs)
    assert a0[25].value == (tabs[0].data_ptr() if scale else None)
    assert a1[20].value == (tabs[0][1].data_ptr() if scale else None)
    assert a1[22].value == (tabs[0][2].data_ptr() if scale else None)


@pytest.mark.parametrize("bad", [-1, 2.0, "8", True])
def test_bad_windows_are_refused_before_any_call(dry, bad):  # noqa: F811
    hip, fake = dry
    kc, vc, _, slot, lens = _inputs(torch.bfloat16)
    q = _bf(4, Hq, D)
    with pytest.raises(hip.HipOpsError, match="window"):
        hip.decode_attention(q, kc, vc, slot, lens, 0.125, splits=1, window=bad)
    with pytest.raises(hip.HipOpsError, match="window"):
        hip.prefill_attention(q, kc, vc, 1, 0, scale=0.125, nsplit=1, window=bad)
    with pytest.raises(hip.HipOpsError, match="window"):
        hip.prefill_attention_varlen(q, kc, vc, [0, 4], [1], [0], scale=0.125, window=bad)
    assert not fake.calls
    from dmcp.ops import reference
    with pytest.raises(ValueError, match="window"):
        reference.decode_attention(q, kc, vc, slot, lens, 0.125, window=bad)


def _spy(monkeypatch):
    from dmcp import ops
    seen = []
    for name in ("decode_attention", "prefill_attention", "prefill_attention_varlen"):
        real = getattr(ops, name)

        def spy(*a, _real=real, _name=name, **k):
            seen.append((_name, k.get("window", "absent")))
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    real_ref = ops.reference.prefill_attention

    def ref_spy(*a, **k):
        seen.append(("reference.prefill_attention", k.get("window", "absent")))
        return real_ref(*a, **k)
    monkeypatch.setattr(ops.reference, "prefill_attention", ref_spy)
    return seen


def _step(m):
    m.prefill_batch([([256, 65, 66], 0, 0), ([256, 67], 1, 0)])
    m.forward_tokens(torch.tensor([68, 69], dtype=torch.int32), 0, 3)
    one = torch.zeros(1, dtype=torch.int32)
    m.decode(torch.tensor([67], dtype=torch.int32), one, torch.tensor([5], dtype=torch.int32))


def test_full_attention_model_makes_no_windowed_call(monkeypatch):
    from dmcp.models.llm import LocalLM, preset
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64), device="cpu")
    assert m.windows is None and all(m._wkw(i) == {} for i in range(2))
    seen = _spy(monkeypatch)
    _step(m)
    top = [(n, w) for n, w in seen if not n.startswith("reference.")]
    assert {n for n, _ in top} == {"decode_attention", "prefill_attention_varlen"}
    assert all(w == "absent" for _, w in top)  # the calls as they always were: no window keyword at all
    assert all(w in (0, "absent") for _, w in seen)  # (the varlen reference walks its sequences with window 0)
    # windows that no sequence can outgrow are none
    m = LocalLM(preset("tiny", max_batch=2, max_seq=64, layer_windows=(0, 0)), device="cpu")
    assert m.windows is None


def test_qwen2_max_window_layers_one_call_of_each_kind_per_step(tmp_path, monkeypatch):
    from dmcp.models.llm import LocalLM
    from dmcp.utils import synth
    d = synth.llama_checkpoint(str(tmp_path / "q2"), layers=2, hidden=256, heads=4, kv_heads=2, intermediate=512,
                               vocab=512, tokenizer="", outliers=(), device="cpu", qkv_bias=True, model_type="qwen2",
                               sliding_window=4, max_window_layers=1)
    m = LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=2, max_rows=2)
    assert m.cfg.layer_windows == (0, 4) and m.windows == (0, 4)
    seen = _spy(monkeypatch)
    _step(m)
    for name in ("decode_attention", "prefill_attention_varlen"):
        assert [w for n, w in seen if n == name] == ["absent", 4], (name, seen)
    # the single-sequence extend on the CPU: SDPA for the full layer, the windowed reference for the other
    assert [w for n, w in seen if n == "reference.prefill_attention"][-1:] == [4]
    with pytest.raises(ValueError, match="layer_windows"):
        LocalLM.load_safetensors(d, device="cpu", max_seq=64, max_batch=2, max_rows=2, layer_windows=(4,))
