"""The penalty arguments of dmcp/ops/hip.py's selection wrappers on the CPU
against a recording stand-in (the idiom of tests/test_hip_dry_launch_sampling.py):
with a Penalty they call the *_penal entry points with the documented lists,
with None or (theta 1, alpha 0) the existing entry points with the existing
lists, bad penalties are refused before anything is launched, and a library
without the new symbols is a "rebuild" HipOpsError."""
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


T, SEED = 0.7, 2 ** 32 + 5
INV_T = float(np.float32(1.0 / T))
THETA, ALPHA, N_SLOTS = 1.3, 0.5, 900
F_THETA, F_INV, F_ALPHA = (float(np.float32(v)) for v in (THETA, np.float32(1.0) / np.float32(THETA), ALPHA))


def _pen(hip, rows, W, n_flags=None, theta=THETA, alpha=ALPHA):
    hist = torch.zeros(N_SLOTS, W, dtype=torch.int32)
    flags = None if n_flags is None else torch.ones(n_flags, dtype=torch.int32)
    return hip.Penalty(hist, torch.arange(rows, dtype=torch.int32), theta, alpha, flags)


def _pen_tail(a, pen, W, n_rows, m0=0):
    """The nine penalty arguments + the stream at the end of an argument list."""
    t = a[-10:]
    assert [t[0].value, t[3].value] == [pen.history.data_ptr(), pen.slots[m0:].data_ptr()]
    assert t[4].value == (None if pen.rows is None else pen.rows.data_ptr())
    assert t[1:3] == (W, N_SLOTS) and t[5] == (0 if pen.rows is None else n_rows)
    assert t[6:] == (F_THETA, F_INV, F_ALPHA, None)


def _off(hip, rows, W):
    return (None, _pen(hip, rows, W, theta=1.0, alpha=0.0), _pen(hip, rows, W, theta=1, alpha=0))


def test_masked_entry_points(dry):
    hip, fake = dry
    B, V, ld = 5, 250, 256
    logits, masks = _bf(B, ld), torch.zeros(3, 8, dtype=torch.int32)
    midx = torch.zeros(B, dtype=torch.int32)
    slots, pos = _keys(B)
    pen = _pen(hip, B, 8, 3)
    out = hip.masked_sample(logits, masks, V, None, midx, slots, pos, T, SEED, penalty=pen)
    (name, a), = fake.calls
    assert name == "dmcp_masked_penal" and len(a) == 22 and tuple(out.shape) == (B,)
    assert [a[i].value for i in (0, 1, 2, 4)] == [logits.data_ptr(), masks.data_ptr(), midx.data_ptr(),
                                                  out.data_ptr()]
    assert (a[3], a[5], a[6], a[7]) == (3, B, V, ld)
    assert (a[8].value, a[9].value, a[10], a[11]) == (slots.data_ptr(), pos.data_ptr(), 5, INV_T)
    _pen_tail(a, pen, 8, 3)
    del fake.calls[:]
    # greedy: 1 / T = 0 and no sampling keys; per-row masks: one flag per row
    pen = _pen(hip, B, 8, B)
    hip.masked_argmax(logits, torch.zeros(B, 8, dtype=torch.int32), V, penalty=pen)
    (name, a), = fake.calls
    assert name == "dmcp_masked_penal" and a[2].value is None and a[3] == 0
    assert (a[8].value, a[9].value, a[10], a[11]) == (None, None, 0, 0.0)
    _pen_tail(a, pen, 8, B)
    del fake.calls[:]
    hip.masked_sample(logits, masks, V, None, midx, slots, pos, 0.0, SEED, penalty=_pen(hip, B, 8))
    assert fake.calls[0][0] == "dmcp_masked_penal" and fake.calls[0][1][11] == 0.0
    for off in _off(hip, B, 8):
        del fake.calls[:]
        hip.masked_sample(logits, masks, V, None, midx, slots, pos, T, SEED, penalty=off)
        hip.masked_argmax(logits, masks, V, None, midx, penalty=off)
        assert [(n, len(a)) for n, a in fake.calls] == [("dmcp_masked_sample", 13), ("dmcp_masked_argmax", 9)]


def test_truncated_entry_point(dry):
    hip, fake = dry
    B, V, ld = 5, 250, 256
    logits, masks = _bf(B, ld), torch.zeros(3, 8, dtype=torch.int32)
    midx = torch.zeros(B, dtype=torch.int32)
    slots, pos = _keys(B)
    stats = torch.zeros(B, 2, dtype=torch.int32)
    pen = _pen(hip, B, 8, 3)
    hip.truncated_sample(logits, masks, V, None, midx, slots, pos, T, SEED, 20, 0.95, 0.0, stats, penalty=pen)
    (name, a), = fake.calls
    assert name == "dmcp_truncated_penal" and len(a) == 26
    assert a[10:15] == (5, INV_T, 20, float(np.float32(0.95)), float("-inf")) and a[15].value == stats.data_ptr()
    _pen_tail(a, pen, 8, 3)
    for off in _off(hip, B, 8):
        del fake.calls[:]
        hip.truncated_sample(logits, masks, V, None, midx, slots, pos, T, SEED, 20, 0.95, 0.0, stats, penalty=off)
        assert [(n, len(a)) for n, a in fake.calls] == [("dmcp_truncated_sample", 17)]
    del fake.calls[:]
    hip.truncated_sample(logits, masks, V, None, midx, slots, pos, 0.0, SEED, 20, 0.95, 0.0, stats, penalty=pen)
    assert [n for n, _ in fake.calls] == ["dmcp_masked_penal"]  # temperature 0: the greedy id, penalised


@pytest.mark.parametrize("M,V", [(40, 448), (700, 512)])
def test_lm_head_entry_points(dry, M, V):
    hip, fake = dry
    K, W = 128, V // 32
    x, w = _bf(M, K), _bf(V, K)
    masks, midx = torch.zeros(4, W, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    pen = _pen(hip, M, W, 4)
    chunks = [(m0, min(hip.WGEMM_MAX_ROWS, M - m0)) for m0 in range(0, M, hip.WGEMM_MAX_ROWS)]
    for sample in (True, False):
        del fake.calls[:]
        if sample:
            out = hip.lm_head_sample(x, w, masks, midx, slots=slots, positions=pos, temperature=T, seed=SEED,
                                     penalty=pen)
        else:
            out = hip.lm_head_argmax(x, w, masks, midx, penalty=pen)
        assert [n for n, _ in fake.calls] == ["dmcp_lm_head_penal"] * len(chunks)
        for (m0, mc), (_, a) in zip(chunks, fake.calls):
            assert len(a) == 26
            assert a[0].value == x[m0:].data_ptr() and a[3].value == midx[m0:].data_ptr()
            assert a[7].value == out[m0:].data_ptr()
            assert (a[4], a[5], a[8], a[9], a[10], a[11]) == (4, W, mc, V, K, -(-mc // 256))
            if sample:
                assert (a[12].value, a[13].value, a[14], a[15]) == (slots[m0:].data_ptr(), pos[m0:].data_ptr(), 5,
                                                                    INV_T)
            else:
                assert (a[12].value, a[13].value, a[14], a[15]) == (None, None, 0, 0.0)
            _pen_tail(a, pen, W, 4, m0)
    for off in _off(hip, M, W):
        del fake.calls[:]
        hip.lm_head_sample(x, w, masks, midx, None, None, slots, pos, T, SEED, penalty=off)
        hip.lm_head_argmax(x, w, masks, midx, penalty=off)
        assert [(n, len(a)) for n, a in fake.calls] == ([("dmcp_lm_head_sample", 17)] * len(chunks)
                                                       + [("dmcp_lm_head_argmax", 13)] * len(chunks))


@pytest.mark.parametrize("M", [257, 300])
def test_tgemm_lm_head_entry_points(dry, M):
    hip, fake = dry
    V, K, W = 512, 256, 16
    x, w = _bf(M, K), _bf(V, K)
    masks, midx = torch.zeros(2, W, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    ws = torch.empty(2 * (V // 64) * M, dtype=torch.float32)
    pen = _pen(hip, M, W, 2)
    out = hip.tgemm_lm_head_sample(x, w, masks, midx, workspace=ws, slots=slots, positions=pos, temperature=T,
                                   seed=SEED, penalty=pen)
    (name, a), = fake.calls
    assert name == "dmcp_tgemm_penal" and len(a) == 26
    assert [a[i].value for i in (0, 1, 2, 7, 8, 11, 12, 13)] == [t.data_ptr() for t in (x, w, ws, masks, midx, out,
                                                                                      slots, pos)]
    assert a[3:7] == (M, V, K, 2) and a[9:11] == (2, W) and a[14:16] == (5, INV_T)
    _pen_tail(a, pen, W, 2)
    del fake.calls[:]
    hip.tgemm_lm_head_argmax(x, w, masks, midx, out, ws, penalty=pen)
    (name, a), = fake.calls
    assert name == "dmcp_tgemm_penal" and (a[12].value, a[13].value, a[14], a[15]) == (None, None, 0, 0.0)
    _pen_tail(a, pen, W, 2)
    for off in _off(hip, M, W):
        del fake.calls[:]
        hip.tgemm_lm_head_sample(x, w, masks, midx, out, ws, 0, slots, pos, T, SEED, penalty=off)
        hip.tgemm_lm_head_argmax(x, w, masks, midx, out, ws, penalty=off)
        assert [(n, len(a)) for n, a in fake.calls] == [("dmcp_tgemm_sample", 17), ("dmcp_tgemm", 17)]


def test_history_entry_points(dry):
    hip, fake = dry
    hist = torch.zeros(6, 8, dtype=torch.int32)
    tokens, slots = _keys(5)
    src, last, exempt = torch.zeros(5, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), \
        torch.zeros(8, dtype=torch.int32)
    assert hip.history_mark(hist, tokens, slots, src, last, exempt, 250) is hist
    (name, a), = fake.calls
    assert name == "dmcp_history_mark" and len(a) == 12
    assert [a[i].value for i in (0, 3, 4, 5, 6, 8)] == [t.data_ptr() for t in (hist, tokens, slots, src, last, exempt)]
    assert (a[1], a[2], a[7], a[9], a[10], a[11]) == (8, 6, 9, 5, 250, None)
    del fake.calls[:]
    hip.history_mark(hist, tokens, slots)
    a = fake.calls[0][1]
    assert [a[i].value for i in (5, 6, 8)] == [None] * 3 and (a[7], a[10]) == (0, 256)
    del fake.calls[:]
    hip.history_reset(hist, [4, 1])
    (name, a), = fake.calls
    assert name == "dmcp_history_reset" and len(a) == 6 and list(a[3]) == [4, 1]
    assert a[0].value == hist.data_ptr() and (a[1], a[2], a[4], a[5]) == (8, 6, 2, None)
    del fake.calls[:]
    hip.history_reset(hist, [])
    for bad in (lambda: hip.history_mark(hist, tokens, slots[:4]), lambda: hip.history_mark(hist, tokens, slots, src),
                lambda: hip.history_mark(hist, tokens, slots, vocab=257),
                lambda: hip.history_mark(hist, tokens, slots, exempt=exempt[:7]),
                lambda: hip.history_mark(hist.long(), tokens, slots), lambda: hip.history_reset(hist, 3)):
        with pytest.raises(hip.HipOpsError):
            bad()
    assert not fake.calls


def test_bad_penalties_are_refused_before_any_launch(dry):
    hip, fake = dry
    M, V, K, W = 300, 512, 256, 16
    x, w, logits = _bf(M, K), _bf(V, K), _bf(M, V)
    masks, midx = torch.zeros(2, W, dtype=torch.int32), torch.zeros(M, dtype=torch.int32)
    slots, pos = _keys(M)
    calls = [
        lambda p, t: hip.masked_sample(logits, masks, V, None, midx, slots, pos, t, 1, penalty=p),
        lambda p, t: hip.masked_argmax(logits, masks, V, None, midx, penalty=p),
        lambda p, t: hip.truncated_sample(logits, masks, V, None, midx, slots, pos, t, 1, 20, penalty=p),
        lambda p, t: hip.lm_head_sample(x, w, masks, midx, None, None, slots, pos, t, 1, penalty=p),
        lambda p, t: hip.lm_head_argmax(x, w, masks, midx, penalty=p),
        lambda p, t: hip.tgemm_lm_head_sample(x, w, masks, midx, None, None, 0, slots, pos, t, 1, penalty=p),
        lambda p, t: hip.tgemm_lm_head_argmax(x, w, masks, midx, penalty=p),
    ]
    hist = torch.zeros(N_SLOTS, W, dtype=torch.int32)
    sl = torch.arange(M, dtype=torch.int32)
    P = hip.Penalty
    bad = [("theta", P(hist, sl, 0.0)), ("theta", P(hist, sl, -1.3)), ("theta", P(hist, sl, float("nan"))),
           ("theta", P(hist, sl, float("inf"))), ("theta", P(hist, sl, "warm")), ("theta", P(hist, sl, 1e-45)),
           ("alpha", P(hist, sl, 1.1, float("nan"))), ("alpha", P(hist, sl, 1.1, float("inf"))),
           ("history", P(hist.long(), sl, 1.1)), ("history", P(hist[:, :W - 1], sl, 1.1)),
           ("history", P(hist[0], sl, 1.1)), ("history", P(torch.zeros(4, 2 * W, dtype=torch.int32)[:, ::2], sl, 1.1)),
           ("slots", P(hist, sl.long(), 1.1)), ("slots", P(hist, sl[:-1], 1.1)),
           ("slots", P(hist, sl + (N_SLOTS - M + 1), 1.1)),  # a live slot past the table
           ("slots", P(hist, None, 1.1)),
           ("rows", P(hist, sl, 1.1, 0.0, torch.ones(3, dtype=torch.int32))),
           ("rows", P(hist, sl, 1.1, 0.0, torch.ones(2, dtype=torch.int64))),
           ("Penalty", (1.1, 0.5))]
    for op in calls:
        for what, p in bad:
            for t in (0.7, 0.0):
                with pytest.raises(hip.HipOpsError, match=what):
                    op(p, t)
        # theta / alpha are checked even when they would switch the penalty off
        with pytest.raises(hip.HipOpsError, match="history"):
            op(P(hist[:, :W - 1], sl, 1.0, 0.0), 0.7)
    assert not fake.calls


def test_a_library_without_the_penalty_symbols_asks_for_a_rebuild(monkeypatch, tmp_path):
    from dmcp.ops import hip
    for missing in ("_penal", "dmcp_history_mark", "dmcp_history_reset"):
        class _Stale:
            def __getattr__(self, name, missing=missing):
                if name.endswith(missing):
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
        monkeypatch.setattr(ctypes, "CDLL", lambda path, _Stale=_Stale: _Stale())
        with pytest.raises(hip.HipOpsError, match="rebuild"):
            hip.lib()
        assert hip._lib is None
    assert hip.ABI_VERSION == 20
