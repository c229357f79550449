"""The sampling wrappers of dmcp/ops/hip.py on the CPU against the recording
stand-in of tests/test_hip_dry_launch.py: above temperature 0 they call the
sampling entry points with their argument lists, at temperature 0 the greedy
entry points with the greedy lists, and a bad temperature or bad keys are
refused before anything is launched.  A library without the new symbols is a
"rebuild" HipOpsError."""
import ctypes

import numpy as np
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

    def req(t, dtype, name):  # the dtype / layout checks, without the device check
        if t.dtype != dtype:
            raise hip.HipOpsError(f"{name}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise hip.HipOpsError(f"{name}: tensor must be contiguous")
    monkeypatch.setattr(hip, "_req", req)
    monkeypatch.setattr(hip, "_stream", lambda: None)
    monkeypatch.setattr(hip, "lib", lambda: fake)
    return hip, fake


def _bf(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


def _keys(n):
    return torch.arange(n, dtype=torch.int32), torch.arange(n, dtype=torch.int32) + 7


T, SEED = 0.7, 2 ** 32 + 5          # the seed is taken modulo 2^32
INV_T = float(np.float32(1.0 / T))  # 1 / T as fp32, the number the reference multiplies by


def test_masked_sample_entry_points(dry):
    hip, fake = dry
    B, V, ld = 5, 250, 256
    logits, masks = _bf(B, ld), torch.zeros(3, 8, dtype=torch.int32)
    midx = torch.zeros(B, dtype=torch.int32)
    slots, pos = _keys(B)
    out = hip.masked_sample(logits, masks, V, None, midx, slots, pos, T, SEED)
    (name, a), = fake.calls
    assert name == "dmcp_masked_sample" and len(a) == 13 and tuple(out.shape) == (B,)
    assert [a[i].value for i in (0, 1, 2)] == [logits.data_ptr(), masks.data_ptr(), midx.data_ptr()]
    assert (a[3], a[5], a[6], a[7]) == (3, B, V, ld) and a[4].value == out.data_ptr()
    assert (a[8].value, a[9].value, a[10], a[11], a[12]) == (slots.data_ptr(), pos.data_ptr(), 5, INV_T, None)
    for kw in ({"temperature": 0.0, "seed": SEED}, {"temperature": 0}, {}):
        del fake.calls[:]
        hip.masked_sample(logits, masks, V, None, midx, slots, pos, **kw)
        (name, old), = fake.calls
        assert name == "dmcp_masked_argmax" and len(old) == 9
        assert [old[i].value for i in (0, 1, 2)] == [a[i].value for i in (0, 1, 2)] and old[3:4] + old[5:9] == \
            a[3:4] + a[5:8] + (None,)


@pytest.mark.parametrize("M,V", [(40, 448), (300, 512), (700, 512)])
def test_lm_head_sample_entry_points(dry, M, V):
    hip, fake = dry
    K = 128
    x, w = _bf(M, K), _bf(V, K)
    masks, midx = torch.zeros(4, V // 32, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    out = hip.lm_head_sample(x, w, masks, midx, slots=slots, positions=pos, temperature=T, seed=SEED)
    chunks = [(m0, min(hip.WGEMM_MAX_ROWS, M - m0)) for m0 in range(0, M, hip.WGEMM_MAX_ROWS)]
    assert [n for n, _ in fake.calls] == ["dmcp_lm_head_sample"] * len(chunks) and tuple(out.shape) == (M,)
    new = [a for _, a in fake.calls]
    for (m0, mc), a in zip(chunks, new):
        assert len(a) == 17
        assert a[0].value == x[m0:].data_ptr() and a[1].value == w.data_ptr() and a[3].value == midx[m0:].data_ptr()
        assert (a[4], a[5], a[8], a[9], a[10], a[11]) == (4, V // 32, mc, V, K, -(-mc // 256))
        assert a[7].value == out[m0:].data_ptr()
        assert (a[12].value, a[13].value) == (slots[m0:].data_ptr(), pos[m0:].data_ptr())
        assert (a[14], a[15], a[16]) == (5, INV_T, None)
    del fake.calls[:]
    ws = hip.lm_head_workspace(V, "cpu", min(M, hip.WGEMM_MAX_ROWS))
    hip.lm_head_sample(x, w, masks, midx, out, ws, slots, pos, 0.0, SEED)
    assert [n for n, _ in fake.calls] == ["dmcp_lm_head_argmax"] * len(chunks)
    for (_, old), a in zip(fake.calls, new):
        assert len(old) == 13 and old[4:6] + old[8:12] == a[4:6] + a[8:12] and old[12] is None
        assert [old[i].value for i in (0, 1, 2, 3, 7)] == [a[i].value for i in (0, 1, 2, 3, 7)]


@pytest.mark.parametrize("M", [257, 300])
def test_tgemm_lm_head_sample_entry_points(dry, M):
    hip, fake = dry
    V, K = 512, 256
    x, w = _bf(M, K), _bf(V, K)
    masks, midx = torch.zeros(2, V // 32, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    ws = torch.empty(2 * (V // 64) * M, dtype=torch.float32)
    out = hip.tgemm_lm_head_sample(x, w, masks, midx, workspace=ws, slots=slots, positions=pos, temperature=T,
                                   seed=SEED)
    (name, a), = fake.calls
    assert name == "dmcp_tgemm_sample" and len(a) == 17
    assert [a[i].value for i in (0, 1, 2, 7, 8, 11, 12, 13)] == [t.data_ptr() for t in (x, w, ws, masks, midx, out,
                                                                                      slots, pos)]
    assert a[3:7] == (M, V, K, 2) and a[9:11] == (2, V // 32) and a[14:] == (5, INV_T, None)
    del fake.calls[:]
    hip.tgemm_lm_head_sample(x, w, masks, midx, out, ws, 0, slots, pos, 0.0, SEED)
    (name, old), = fake.calls
    assert name == "dmcp_tgemm" and len(old) == 17
    assert old[4:11] == (M, V, K, 1, 2, 3, 0) and old[13:15] == (2, V // 32) and old[16] is None
    assert [old[i].value for i in (0, 1, 2, 3, 11, 12, 15)] == [x.data_ptr(), w.data_ptr(), None, ws.data_ptr(),
                                                               masks.data_ptr(), midx.data_ptr(), out.data_ptr()]


def test_bad_temperature_and_keys_are_refused_before_any_launch(dry):
    hip, fake = dry
    M, V, K = 300, 512, 256
    x, w, logits = _bf(M, K), _bf(V, K), _bf(M, V)
    masks, midx = torch.zeros(2, V // 32, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    calls = {
        "masked": lambda s, p, t: hip.masked_sample(logits, masks, V, None, midx, s, p, t, 1),
        "wgemm": lambda s, p, t: hip.lm_head_sample(x, w, masks, midx, None, None, s, p, t, 1),
        "tgemm": lambda s, p, t: hip.tgemm_lm_head_sample(x, w, masks, midx, None, None, 0, s, p, t, 1),
    }
    bad_keys = [(None, pos), (slots, None),                       # missing
                (slots.long(), pos), (slots, pos.float()),        # wrong dtype
                (slots[:-1], pos), (slots, torch.cat([pos, pos])),  # wrong length
                (torch.stack([slots, slots], 1)[:, 0], pos)]      # not contiguous
    for op in calls.values():
        for t in (-0.1, float("nan"), float("inf"), -float("inf"), "warm", 1e-45):
            with pytest.raises(hip.HipOpsError, match="temperature"):
                op(slots, pos, t)
        for s, p in bad_keys:
            for t in (0.7, 0.0):  # the keys are checked at temperature 0 too: a caller's mistake shows at once
                with pytest.raises(hip.HipOpsError):
                    op(s, p, t)
        assert not fake.calls
    # the greedy siblings' own checks still hold on the sampling path
    with pytest.raises(hip.HipOpsError, match="mask_idx"):
        hip.masked_sample(logits, masks, V, None, midx[:5], slots, pos, 0.7, 1)
    with pytest.raises(hip.HipOpsError, match="out"):
        hip.lm_head_sample(x, w, masks, midx, torch.zeros(M - 1, dtype=torch.int32), None, slots, pos, 0.7, 1)
    with pytest.raises(hip.HipOpsError, match="workspace"):
        hip.tgemm_lm_head_sample(x, w, masks, midx, None, torch.empty(8), 0, slots, pos, 0.7, 1)
    assert not fake.calls


def test_a_library_without_the_sampling_symbols_asks_for_a_rebuild(monkeypatch, tmp_path):
    from dmcp.ops import hip

    class _Stale:
        def __getattr__(self, name):
            if name.endswith("_sample"):
                raise AttributeError(name)

            class _Fn:
                argtypes = restype = None

                def __call__(self):
                    return hip.ABI_VERSION
            return _Fn()
    so = tmp_path / "stale.so"
    so.write_bytes(b"")
    monkeypatch.setenv("DMCP_HIPOPS_SO", str(so))
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: _Stale())
    with pytest.raises(hip.HipOpsError, match="rebuild"):
        hip.lib()
    assert hip._lib is None
    assert hip.ABI_VERSION == 20
