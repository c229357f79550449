"""Plain-PyTorch fp32 reference implementations of every HIP op.

Used (a) by the numerics tests, which compare each gfx950 kernel against
these, and (b) for CPU tensors (unit tests on the GPU-less build host).
Signatures mirror :mod:`dmcp.ops.hip`.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch


def add_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    h = x
    if residual is not None:
        h = (x.float() + residual.float()).to(x.dtype)
        residual.copy_(h)
    hf = h.float()
    y = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()
    y = y.to(x.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


# FP8 KV cache: uint8 tensors holding OCP e4m3fn bytes (unit scale, saturated)
FP8_MAX = 448.0


def kv_float(t: torch.Tensor) -> torch.Tensor:
    """Cache values as fp32 (bf16 caches, or fp8 e4m3 caches stored as uint8).
    An fp64 tensor stays fp64: the attention references then run in fp64
    (tests/needles.py decodes the caches and passes them that way)."""
    if t.dtype == torch.uint8:
        return t.view(torch.float8_e4m3fn).float()
    return t if t.dtype == torch.float64 else t.float()


def kv_encode(x: torch.Tensor, cache_dtype: torch.dtype) -> torch.Tensor:
    """Values in a cache's storage format (bf16, or saturated e4m3 bytes)."""
    if cache_dtype == torch.uint8:
        return x.float().clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return x.to(cache_dtype)


# ---- per-row scaled FP8 KV cache (kv_dtype "fp8s"): the e4m3 bytes of a
# cached row (one kv head's D values at one position) plus one exponent byte,
# kept in tables beside the caches: k_scale / v_scale uint8 [S, Hkv, MAXS] for
# caches [S, Hkv, MAXS, D].  With amax the largest |x| of the row's bf16 values:
#   e     = the smallest exponent with amax / 2^e <= 448, 0 for an all-zero row
#           (the MX rule of :func:`mx_quant`; csrc/dmcp_common.hpp mx_exp)
#   byte  = e + 127
#   bytes = e4m3(x * 2^-e)        (the scaling is exact; saturating convert)
# and a reader decodes e4m3 * 2^(byte - 127) for ANY byte 0 .. 254, not only the
# minimal one (255 is E8M0's NaN: 2^128 is no fp32 value, no writer produces it).
# The ops below take the tables as ``kv_scale=(k_scale, v_scale)``; None is the
# unit-scale format.
KV_FORMATS = ("bf16", "fp8", "fp8s")


def kv_row_exp(amax: torch.Tensor) -> torch.Tensor:
    """The row exponent e (int32) of rows whose largest magnitude is ``amax``."""
    af = amax.float()
    _, e = torch.frexp(af * torch.tensor(1.0 / FP8_MAX, dtype=torch.float32, device=af.device))
    return torch.where(af > 0, e, torch.zeros_like(e)).clamp(-127, 127).to(torch.int32)


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e (fp64, exact) of integer exponents in [-1022, 1023], built from the
    bits: ``torch.ldexp`` multiplies by a computed ``pow`` that is one ulp short
    on some devices, which moves values that sit on an e4m3 rounding tie."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def kv_encode_scaled(x: torch.Tensor) -> tuple:
    """x [..., D] -> (e4m3 bytes uint8 [..., D], exponent bytes uint8 [...])."""
    xf = x.float()
    e = kv_row_exp(xf.abs().amax(-1))
    q = (xf.double() * _pow2(-e)[..., None]).float()
    return (q.clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8),
            (e + 127).to(torch.uint8))


def kv_decode_scaled(q: torch.Tensor, s: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """The values [..., D] (``dtype``: fp32 or fp64) of e4m3 bytes ``q`` under
    the exponent bytes ``s`` [...] -- any byte, minimal or not."""
    v = q.view(torch.float8_e4m3fn).to(torch.float64)
    return (v * _pow2(s.to(torch.int32) - 127)[..., None]).to(dtype)


def _kv_rows(cache: torch.Tensor, scale: Optional[torch.Tensor], idx) -> torch.Tensor:
    """``cache[idx]`` as floats (:func:`kv_float`), decoded with ``scale[idx]``
    where the cache is a scaled one."""
    if scale is None:
        return kv_float(cache[idx])
    return kv_decode_scaled(cache[idx], scale[idx])


def _kv_scale_pair(kv_scale, k_cache: torch.Tensor, name: str) -> tuple:
    """(k_scale, v_scale) validated against the caches, (None, None) for None."""
    if kv_scale is None:
        return None, None
    if not isinstance(kv_scale, (tuple, list)) or len(kv_scale) != 2:
        raise ValueError(f"{name}: kv_scale must be (k_scale, v_scale)")
    if k_cache.dtype != torch.uint8:
        raise ValueError(f"{name}: kv_scale needs fp8 (uint8) caches, got {k_cache.dtype}")
    for t, which in zip(kv_scale, ("k_scale", "v_scale")):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != tuple(k_cache.shape[:-1])
                or t.device != k_cache.device):
            raise ValueError(f"{name}.{which}: expected uint8 {tuple(k_cache.shape[:-1])} on the caches' device")
    return kv_scale[0], kv_scale[1]


ROPE_TYPES = ("default", "linear", "llama3")


def rope_scaling_key(scaling) -> Optional[tuple]:
    """A checkpoint's ``rope_scaling`` / ``rope_parameters`` dict as the
    hashable form :class:`dmcp.models.llm.LMConfig` keeps: sorted (key, value)
    pairs with the type under ``rope_type`` (the legacy key ``type`` is
    renamed); None for no scaling.  Raises ValueError for a type outside
    :data:`ROPE_TYPES` or a missing parameter."""
    if not scaling:
        return None
    d = dict(scaling)
    kind = d.pop("rope_type", None) or d.pop("type", None) or "default"
    d.pop("type", None)
    d.pop("rope_theta", None)  # rope_parameters carries theta too; LMConfig.rope_theta holds it
    if kind not in ROPE_TYPES:
        raise ValueError(f"rope_type {kind!r} is not supported (supported: {', '.join(ROPE_TYPES)})")
    if kind == "default":
        return None
    need = {"linear": ("factor",),
            "llama3": ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings")}[kind]
    missing = [k for k in need if k not in d]
    if missing:
        raise ValueError(f"rope_type {kind!r} needs {', '.join(missing)}")
    return tuple(sorted([("rope_type", kind)] + [(k, float(d[k])) for k in need]))


def rotary_dim_arg(head_dim: int, rotary_dim: int) -> int:
    """The rotated width R of a head of ``head_dim``: ``rotary_dim`` 0 means
    the whole head; else even and in (0, head_dim]."""
    if isinstance(rotary_dim, bool) or not isinstance(rotary_dim, int) or rotary_dim < 0 or rotary_dim > head_dim \
            or rotary_dim % 2:
        raise ValueError(f"rotary_dim {rotary_dim!r} must be 0 (the whole head) or even and in (0, head_dim {head_dim}]")
    return rotary_dim or head_dim


def partial_rotary_perm(head_dim: int, rotary_dim: int) -> torch.Tensor:
    """Partial rotary embedding on kernels that rotate the whole head.  The
    checkpoint's code rotates the first R = ``rotary_dim`` dims of a head in
    half-split pairs (i, i + R/2) and passes dims R .. D-1 through.  The
    kernels rotate pairs (i, i + D/2) of the whole head.  This index tensor
    ``perm`` [D] (new[j] = old[perm[j]]) moves pair (i, i + R/2) to
    (i, i + D/2) and the pass-through dims to the remaining pairs, which
    :func:`rope_tables` gives frequency 0 (cos 1, sin 0 exactly: unrotated).
    The loader applies it to each head's rows of q_proj / k_proj (their biases
    and q_norm / k_norm weights too); the same permutation on q and k leaves
    every q . k unchanged, so V, o_proj and the attention are untouched."""
    R = rotary_dim_arg(head_dim, rotary_dim)
    half, rh = head_dim // 2, R // 2
    rest = torch.arange(R, head_dim)
    n1 = half - rh  # pass-through dims in the first half
    return torch.cat([torch.arange(0, rh), rest[:n1], torch.arange(rh, R), rest[n1:]])


def rope_inv_freq(head_dim: int, theta: float = 10000.0, scaling=None, rotary_dim: int = 0) -> torch.Tensor:
    """The rotary pairs' frequencies [D/2] (float64) under ``scaling``: None /
    "default", "linear" (inv_freq / factor) or "llama3" (pairs of wavelength >
    orig / low_freq_factor divided by factor, < orig / high_freq_factor
    unchanged, interpolated between).  The scaling is evaluated in fp32, as
    the checkpoints' own code does, so the frequencies are the ones the model
    was trained with to the last bit.

    ``rotary_dim`` R (0 = the whole head): only R/2 pairs rotate, with the
    exponent's denominator R, not D; pairs R/2 .. D/2 - 1 get frequency 0
    (the layout of :func:`partial_rotary_perm`)."""
    R = rotary_dim_arg(head_dim, rotary_dim)
    if R != head_dim:
        inv = rope_inv_freq(R, theta, scaling)
        return torch.cat([inv, torch.zeros(head_dim // 2 - R // 2, dtype=inv.dtype)])
    half = head_dim // 2
    inv = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64) / half))
    sc = dict(rope_scaling_key(scaling) or ())
    if not sc:
        return inv
    # fp32 from the start, the way the checkpoints' own code builds them
    f = 1.0 / (theta ** (torch.arange(0, 2 * half, 2, dtype=torch.int64).to(torch.float32) / (2 * half)))
    if sc["rope_type"] == "linear":
        return (f / sc["factor"]).to(torch.float64)
    factor, low, high = sc["factor"], sc["low_freq_factor"], sc["high_freq_factor"]
    orig = sc["original_max_position_embeddings"]
    wavelen = 2 * math.pi / f
    out = torch.where(wavelen > orig / low, f / factor, f)
    smooth = (orig / wavelen - low) / (high - low)
    mid = (1 - smooth) * out / factor + smooth * out
    is_mid = ~(wavelen < orig / high) & ~(wavelen > orig / low)
    return torch.where(is_mid, mid, out).to(torch.float64)


def rope_tables(max_pos: int, head_dim: int, theta: float = 10000.0, device=None, scaling=None,
                fp32_angles: bool = False, rotary_dim: int = 0) -> torch.Tensor:
    """[max_pos, D/2, 2] float32 (cos, sin) -- viewed as float2 by the kernel.
    ``rotary_dim`` (0 = the whole head): see :func:`rope_inv_freq`; the
    pass-through pairs' rows are cos 1, sin 0 exactly.
    ``scaling``: a ``rope_scaling`` dict (or its :func:`rope_scaling_key`
    form) of type "linear" or "llama3"; None = the plain ``theta`` table.
    ``fp32_angles``: frequencies, angles and cos / sin in fp32, the way the
    checkpoints' own code computes them (position x inv_freq rounded to fp32:
    up to 3e-5 rad at position 1,000).  QK-norm models use it: their unit-RMS
    q / k turn that angle rounding into attention-logit differences ~40x the
    fp32 noise of an un-normed model (tests/test_checkpoint_qwen3.py)."""
    R = rotary_dim_arg(head_dim, rotary_dim)
    if R != head_dim:
        t = rope_tables(max_pos, R, theta, None, scaling, fp32_angles)
        rest = torch.zeros((max_pos, head_dim // 2 - R // 2, 2), dtype=t.dtype)
        rest[..., 0] = 1.0
        return torch.cat([t, rest], dim=1).to(device)
    if fp32_angles:
        half = head_dim // 2
        if rope_scaling_key(scaling) is None:
            f = 1.0 / (theta ** (torch.arange(0, 2 * half, 2, dtype=torch.int64).to(torch.float32) / (2 * half)))
        else:
            f = rope_inv_freq(head_dim, theta, scaling).to(torch.float32)  # evaluated in fp32: exact
        ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * f[None, :]
        return torch.stack([ang.cos(), ang.sin()], dim=-1).to(device)
    inv = rope_inv_freq(head_dim, theta, scaling)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).to(torch.float32).to(device)


def apply_rope(x: torch.Tensor, pos: torch.Tensor, cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, H, D] -> rotate-half RoPE at positions pos [T] (fp32 math)."""
    D = x.shape[-1]
    half = D // 2
    cs = cos_sin[pos.long().clamp(0, cos_sin.shape[0] - 1)].to(x.device)  # [T, half, 2]
    c = cs[..., 0][:, None, :]
    s = cs[..., 1][:, None, :]
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def head_rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """RMSNorm over the last axis of x [T, H, D] with one weight [D] for all
    heads (QK-norm): fp32 in and out, no rounding."""
    xf = x.float()
    return xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()


def rope_kv(qkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cos_sin: torch.Tensor,
            k_cache: torch.Tensor, v_cache: torch.Tensor, n_q_heads: int, q_out: Optional[torch.Tensor] = None,
            qk_norm: Optional[tuple] = None, kv_scale: Optional[tuple] = None) -> torch.Tensor:
    """``qk_norm`` (q_weight [D], k_weight [D], eps): per-head RMSNorm of the q
    and k heads in fp32 between the projection and the rotation.
    ``kv_scale`` (k_scale, v_scale): append in the per-row scaled fp8 format."""
    S, Hkv, MAXS, D = k_cache.shape
    ks, vs = _kv_scale_pair(kv_scale, k_cache, "rope_kv")
    T = qkv.shape[0]
    x = qkv.view(T, n_q_heads + 2 * Hkv, D)
    xq, xk = x[:, :n_q_heads], x[:, n_q_heads:n_q_heads + Hkv]
    if qk_norm is not None:
        qw, kw, neps = qk_norm
        xq, xk = head_rmsnorm(xq, qw, neps), head_rmsnorm(xk, kw, neps)
    q = apply_rope(xq, pos, cos_sin).to(qkv.dtype)
    k = apply_rope(xk, pos, cos_sin).to(qkv.dtype)
    v = x[:, n_q_heads + Hkv:]
    for t in range(T):
        p, s = int(pos[t]), int(slot[t])
        if 0 <= p < MAXS and 0 <= s < S and ks is not None:
            k_cache[s, :, p], ks[s, :, p] = kv_encode_scaled(k[t])
            v_cache[s, :, p], vs[s, :, p] = kv_encode_scaled(v[t])
        elif 0 <= p < MAXS and 0 <= s < S:
            k_cache[s, :, p] = kv_encode(k[t], k_cache.dtype)
            v_cache[s, :, p] = kv_encode(v[t], v_cache.dtype)
    if q_out is not None:
        q_out.copy_(q)
        return q_out
    return q


def _linear_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    y = x.float() @ w.float().t()
    return y if bias is None else y + bias.float()


def fused_rope_kv(x: torch.Tensor, w: torch.Tensor, eps: float, pos: torch.Tensor, slot: torch.Tensor,
                  cos_sin: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, n_q_heads: int,
                  q_out: Optional[torch.Tensor] = None, wk: int = 8,
                  bias: Optional[torch.Tensor] = None, qk_norm: Optional[tuple] = None,
                  kv_scale: Optional[tuple] = None) -> torch.Tensor:
    """rope_kv(rms(x) . w^T + bias) with the product kept in fp32 up to RoPE
    (the fused kernel rotates its accumulator); ``wk`` is the kernel's.
    ``qk_norm`` is part of this CPU model only: the HIP kernel takes none.
    ``kv_scale``: the fused kernel has no scaled writer -- a ValueError, as on the GPU."""
    if kv_scale is not None:
        raise ValueError("fused_rope_kv: no per-row scaled (fp8s) cache writer; use wgemm_rope_kv, or "
                         "fused_linear_norm + rope_kv")
    xf = x.float()
    xn = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return rope_kv(_linear_f32(xn, w, bias), pos, slot, cos_sin, k_cache, v_cache, n_q_heads, q_out,
                   qk_norm=qk_norm).to(torch.bfloat16)


def wgemm_rope_kv(x: torch.Tensor, w: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cos_sin: torch.Tensor,
                  k_cache: torch.Tensor, v_cache: torch.Tensor, n_q_heads: int, workspace=None,
                  q_out: Optional[torch.Tensor] = None, splits: int = 0,
                  bias: Optional[torch.Tensor] = None, qk_norm: Optional[tuple] = None,
                  kv_scale: Optional[tuple] = None) -> torch.Tensor:
    """rope_kv(bf16(x . w^T + bias)): the split-K reduction rounds the biased
    fp32 sum to bf16 before the QK-norm and RoPE (what F.linear + rope_kv
    compute)."""
    return rope_kv(_linear_f32(x, w, bias).to(torch.bfloat16), pos, slot, cos_sin, k_cache, v_cache, n_q_heads, q_out,
                   qk_norm=qk_norm, kv_scale=kv_scale)


def tgemm_rope_kv(x: torch.Tensor, w: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cos_sin: torch.Tensor,
                  k_cache: torch.Tensor, v_cache: torch.Tensor, n_q_heads: int, workspace=None,
                  q_out: Optional[torch.Tensor] = None, splits: int = 0,
                  bias: Optional[torch.Tensor] = None, qk_norm: Optional[tuple] = None,
                  kv_scale: Optional[tuple] = None) -> torch.Tensor:
    """The same composition as :func:`wgemm_rope_kv` (one reduction serves both)."""
    return wgemm_rope_kv(x, w, pos, slot, cos_sin, k_cache, v_cache, n_q_heads, workspace, q_out, splits, bias,
                         qk_norm, kv_scale)


class SharedPrefix(NamedTuple):
    """Keys/values shared by the rows of a decode step (cascade decoding):
    ``k`` / ``v`` [Hkv, MAXS, D] (the prefix slot of the caches),
    ``length`` int32 [1] on the device (0 = no prefix) and ``rows`` (int32
    [B], optional: 0 = this row does not use the prefix).  ``k_scale`` /
    ``v_scale`` [Hkv, MAXS]: the prefix slot's exponent bytes (per-row scaled
    caches only)."""
    k: torch.Tensor
    v: torch.Tensor
    length: torch.Tensor
    rows: Optional[torch.Tensor] = None
    k_scale: Optional[torch.Tensor] = None
    v_scale: Optional[torch.Tensor] = None


# ---- sliding-window attention.  A query at logical position i attends key j
# iff j <= i and j > i - W: W keys including its own (the mask transformers
# builds for Mistral / Qwen2).  Positions are the logical ones of the ops
# below -- keys [0, P) from the shared prefix, keys up to the fork end from the
# parent slot, the rest from the own slot -- and the window cuts that logical
# sequence: where a key is stored does not matter.  ``window`` 0 (or None) is
# full attention.  The cache stays linear; nothing is evicted.
def window_arg(window, name: str = "window") -> int:
    """``window`` validated: an int >= 0 (None = 0 = full attention); a
    ValueError names the argument."""
    if window is None:
        return 0
    if isinstance(window, bool) or not isinstance(window, int) or window < 0:
        raise ValueError(f"{name} must be an integer >= 0 (0 = full attention), got {window!r}")
    return int(window)


def decode_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slot: torch.Tensor,
                     seq_len: torch.Tensor, scale: float, workspace=None, chunk: int = 256,
                     out: Optional[torch.Tensor] = None, prefix: Optional[SharedPrefix] = None,
                     fork: Optional[torch.Tensor] = None, kv_scale: Optional[tuple] = None,
                     window: int = 0) -> torch.Tensor:
    """``window`` > 0: a row of live length L attends keys [max(0, L - window), L)
    of its logical sequence only.  ``fork`` [S, 2] (parent slot, end): keys below ``end`` of a row whose
    slot has a parent come from the parent's slot (a method branch reading
    its class head's KV in place).  ``kv_scale`` (k_scale, v_scale): the caches
    are per-row scaled fp8; every key is decoded with the exponent byte of the
    slot it is read from (``prefix.k_scale`` / ``v_scale`` for the prefix)."""
    B, Hq, D = q.shape
    S, Hkv, MAXS, _ = k_cache.shape
    window = window_arg(window, "decode_attention: window")
    ks, vs = _kv_scale_pair(kv_scale, k_cache, "decode_attention")
    if ks is not None and prefix is not None and (prefix.k_scale is None or prefix.v_scale is None):
        raise ValueError("decode_attention: a scaled cache's prefix needs k_scale / v_scale")
    G = Hq // Hkv
    P = int(prefix.length.reshape(-1)[0]) if prefix is not None else 0
    res = torch.zeros((B, Hq, D), dtype=kv_float(q).dtype, device=q.device)
    for b in range(B):
        s, L = int(slot[b]), min(int(seq_len[b]), MAXS)
        if not (0 <= s < S) or L <= 0:
            continue
        own = (s, slice(None), slice(0, L))
        k = _kv_rows(k_cache, ks, own)  # [Hkv, L, D]
        v = _kv_rows(v_cache, vs, own)
        if fork is not None:
            ps, fe = int(fork[s, 0]), min(int(fork[s, 1]), L)
            if fe > 0 and 0 <= ps < S and ps != s:
                par = (ps, slice(None), slice(0, fe))
                k = torch.cat([_kv_rows(k_cache, ks, par), k[:, fe:]], dim=1)
                v = torch.cat([_kv_rows(v_cache, vs, par), v[:, fe:]], dim=1)
        if P > 0 and (prefix.rows is None or int(prefix.rows[b]) != 0):  # the first P keys: the shared prefix
            pre = (slice(None), slice(0, P))
            k = torch.cat([_kv_rows(prefix.k, prefix.k_scale if ks is not None else None, pre), k[:, P:]], dim=1)
            v = torch.cat([_kv_rows(prefix.v, prefix.v_scale if ks is not None else None, pre), v[:, P:]], dim=1)
        if 0 < window < L:  # the last `window` keys of the logical sequence
            k, v = k[:, L - window:], v[:, L - window:]
        qb = kv_float(q[b]).view(Hkv, G, D)
        att = torch.einsum("hgd,hld->hgl", qb, k) * scale
        p = torch.softmax(att, dim=-1)
        res[b] = torch.einsum("hgl,hld->hgd", p, v).reshape(Hq, D)
    y = res.to(q.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def prefill_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slot: int, start: int,
                      prefix_slot: Optional[int] = None, prefix_len: int = 0, scale: float = 1.0,
                      out: Optional[torch.Tensor] = None, variant: int = 0, nsplit: int = 0,
                      kv_scale: Optional[tuple] = None, window: int = 0) -> torch.Tensor:
    """q [T, Hq, D] at positions [start, start+T) of ``slot``; every query
    sees the keys at or before its position.  Keys [0, prefix_len) come from
    ``prefix_slot``, the rest from ``slot``.  fp32 math, returns [T, Hq, D].
    ``kv_scale`` (k_scale, v_scale): per-row scaled fp8 caches.
    ``window`` > 0: the query at position i sees keys (i - window, i] only."""
    T, Hq, D = q.shape
    window = window_arg(window, "prefill_attention: window")
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    L = start + T
    ks, vs = _kv_scale_pair(kv_scale, k_cache, "prefill_attention")
    own = (slot, slice(None), slice(0, L))
    k = _kv_rows(k_cache, ks, own)
    v = _kv_rows(v_cache, vs, own)
    if prefix_len > 0:
        pre = (prefix_slot, slice(None), slice(0, prefix_len))
        k = torch.cat([_kv_rows(k_cache, ks, pre), k[:, prefix_len:]], dim=1)
        v = torch.cat([_kv_rows(v_cache, vs, pre), v[:, prefix_len:]], dim=1)
    qf = kv_float(q).view(T, Hkv, G, D)
    att = torch.einsum("thgd,hld->hgtl", qf, k) * scale  # [Hkv, G, T, L]
    pos = torch.arange(start, L, device=q.device)[:, None]
    keys = torch.arange(L, device=q.device)[None, :]
    att = att.masked_fill(keys > pos, float("-inf"))
    if window > 0:
        att = att.masked_fill(keys <= pos - window, float("-inf"))
    y = torch.einsum("hgtl,hld->thgd", torch.softmax(att, dim=-1), v).reshape(T, Hq, D).to(q.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


def prefill_attention_varlen(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, offsets, slots, starts,
                             prefix_slot: Optional[int] = None, prefix_lens=None, scale: float = 1.0,
                             out: Optional[torch.Tensor] = None, kv_scale: Optional[tuple] = None,
                             window: int = 0) -> torch.Tensor:
    """Several sequences' prefill in one packed q [Ttot, Hq, D]: sequence i
    is rows [offsets[i], offsets[i+1]) at positions [starts[i], ...) of
    ``slots[i]``, keys [0, prefix_lens[i]) read from ``prefix_slot``.
    fp32 math per sequence (:func:`prefill_attention`, ``window`` included)."""
    window = window_arg(window, "prefill_attention_varlen: window")
    out = torch.empty_like(q) if out is None else out
    for i in range(len(slots)):
        a, b = int(offsets[i]), int(offsets[i + 1])
        P = int(prefix_lens[i]) if prefix_lens is not None else 0
        out[a:b] = prefill_attention(q[a:b], k_cache, v_cache, int(slots[i]), int(starts[i]),
                                     prefix_slot if P else None, P, scale, kv_scale=kv_scale, window=window)
    return out


def silu_mul(gate_up: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    I = gate_up.shape[-1] // 2
    g, u = gate_up[..., :I].float(), gate_up[..., I:].float()
    y = (torch.nn.functional.silu(g) * u).to(gate_up.dtype)
    if out is not None:
        out.copy_(y)
        return out
    return y


_M32 = 0xFFFFFFFF


# ---- repetition / presence penalty.  ``history`` is an int32 [n_slots, W]
# bitset table (W = ceil(V / 32)), one row per KV slot: bit v of row s is set
# once token v has been fed to slot s by a decode row (:func:`history_mark`).
# An allowed id v of a row whose history bit v is set competes with
#   x  = fp32(bf16 logit)
#   y  = (x > 0 ? x * inv_theta : x * theta) - alpha      (two fp32 roundings)
#   x' = fp32(bf16_rne(y))
# theta the repetition penalty, inv_theta = fp32(1 / theta) computed once on
# the host (one fp32 ulp from a division by theta), alpha the presence
# penalty; ids whose bit is clear keep x.  x' is a bf16 value again, so every
# selection rule works on it unchanged: greedy is the argmax of x',
# sampling scores x' * inv_t + noise, truncation thresholds the x' values.
# A selection under mask row r is penalised only where ``rows[r] != 0`` (None =
# every row): the engine flags its free-text masks, not its choice masks.
# csrc/dmcp_common.hpp penalize and the PENAL kernel variants follow these.
def penalty_args(theta, alpha=0.0) -> tuple:
    """(theta, fp32(1 / theta), alpha) validated: ``theta`` finite and > 0
    with a positive finite fp32 reciprocal, ``alpha`` finite; a ValueError
    names the offending argument."""
    try:
        t, a = float(theta), float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"theta / alpha must be numbers, got {theta!r} / {alpha!r}") from None
    if not math.isfinite(t) or t <= 0:
        raise ValueError(f"theta (repetition penalty) must be finite and > 0, got {theta!r}")
    if not math.isfinite(a):
        raise ValueError(f"alpha (presence penalty) must be finite, got {alpha!r}")
    t = float(torch.tensor(t, dtype=torch.float32))
    inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(t, dtype=torch.float32))
    a = float(torch.tensor(a, dtype=torch.float32))
    if not (t > 0 and math.isfinite(inv) and inv > 0 and math.isfinite(a)):
        raise ValueError(f"theta (repetition penalty) {theta!r} / alpha {alpha!r} are not usable fp32 numbers")
    return t, inv, a


def penalty_settings(repetition_penalty=1.0, presence_penalty=0.0) -> tuple:
    """The engine's two penalty settings, validated: ``repetition_penalty``
    finite and > 0 (1 = off), ``presence_penalty`` finite (0 = off); a
    ValueError names the offending setting.  Returns them as floats."""
    try:
        theta = float(repetition_penalty)
    except (TypeError, ValueError):
        theta = float("nan")
    if not math.isfinite(theta) or theta <= 0:
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty!r}")
    try:
        alpha = float(presence_penalty)
    except (TypeError, ValueError):
        alpha = float("nan")
    if not math.isfinite(alpha):
        raise ValueError(f"presence_penalty must be finite, got {presence_penalty!r}")
    try:
        penalty_args(theta, alpha)
    except ValueError:
        raise ValueError(f"repetition_penalty {repetition_penalty!r} has no usable fp32 reciprocal") from None
    return theta, alpha


class Penalty:
    """The repetition / presence penalty of one selection call: ``history``
    int32 [n_slots, W], ``slots`` int32 [rows] (each row's history row; < 0 =
    padding, not penalised), ``theta`` / ``alpha`` as above, ``rows``
    (optional) int32 flags per mask row.  ``off`` (theta 1, alpha 0): the
    selection ops take their unpenalised path."""

    __slots__ = ("history", "slots", "theta", "alpha", "rows", "check_slots")

    def __init__(self, history, slots, theta, alpha=0.0, rows=None, check_slots=True):
        self.history, self.slots, self.theta, self.alpha, self.rows = history, slots, theta, alpha, rows
        # False: the caller vouches for the slot values (a device tensor is
        # not read back: no host synchronisation; the kernels skip a slot
        # outside the table either way)
        self.check_slots = check_slots

    @property
    def off(self) -> bool:
        return self.theta == 1 and self.alpha == 0

    def check(self, name: str, B: int, W: int, n_rows: int, values: bool = True, device=None) -> tuple:
        """Validate against a launch of ``B`` rows, ``W`` mask words per row
        and ``n_rows`` mask rows; returns (theta, inv_theta, alpha) as fp32
        values.  ``values``: also read ``slots`` to check every live slot
        against the table (a device tensor is read back)."""
        try:
            keys = penalty_args(self.theta, self.alpha)
        except ValueError as e:
            raise ValueError(f"{name}: penalty {e}") from None
        h, sl, rw = self.history, self.slots, self.rows
        if isinstance(h, torch.Tensor) and device is not None and h.device != device:
            raise ValueError(f"{name}: penalty history is on {h.device}, the selection's input on {device}")
        if (not isinstance(h, torch.Tensor) or h.dtype != torch.int32 or h.dim() != 2 or not h.is_contiguous()
                or h.shape[0] < 1 or h.shape[1] != W):
            raise ValueError(f"{name}: penalty history must be a contiguous int32 [n_slots, {W}] bitset table")
        if (not isinstance(sl, torch.Tensor) or sl.dtype != torch.int32 or sl.numel() != B
                or not sl.is_contiguous() or sl.device != h.device):
            raise ValueError(f"{name}: penalty slots must be int32 [{B}] on the history's device")
        if values and self.check_slots and B > 0 and int(sl.max()) >= h.shape[0]:
            raise ValueError(f"{name}: penalty slots reach {int(sl.max())}, the history has {h.shape[0]} rows")
        if rw is not None and (not isinstance(rw, torch.Tensor) or rw.dtype != torch.int32 or rw.numel() != n_rows
                               or not rw.is_contiguous() or rw.device != h.device):
            raise ValueError(f"{name}: penalty rows must be int32 [{n_rows}] (one flag per mask row)")
        return keys


def unpack_bits(words: torch.Tensor, vocab: int) -> torch.Tensor:
    """bool [..., vocab] of int32 bitset rows [..., >= ceil(vocab / 32)]."""
    idx = torch.arange(vocab, device=words.device)
    return ((words.to(torch.int64)[..., idx // 32] >> (idx % 32)) & 1) != 0


def penalize(logits: torch.Tensor, history_rows: Optional[torch.Tensor], theta: float, alpha: float = 0.0
             ) -> torch.Tensor:
    """fp32 [B, V] of the penalised values x' defined above: ``logits`` [B, V]
    (rounded to bf16 first), ``history_rows`` int32 [B, >= ceil(V / 32)] bitset
    rows (None = nothing seen).  Every selection reference calls this."""
    x = logits.to(torch.bfloat16).float()
    if history_rows is None:
        return x
    t, inv, a = (torch.tensor(v, dtype=torch.float32, device=x.device) for v in penalty_args(theta, alpha))
    y = (torch.where(x > 0, x * inv, x * t) - a).to(torch.bfloat16).float()
    return torch.where(unpack_bits(history_rows, x.shape[-1]), y, x)


def _mask_rows(B: int, mask, mask_idx, device) -> torch.Tensor:
    """The mask row index of each logits row (row b itself without ``mask_idx``)."""
    if mask is not None and mask_idx is not None:
        return mask_idx.long().clamp(0, mask.shape[0] - 1)
    return torch.arange(B, device=device)


def penalized(logits: torch.Tensor, vocab: int, mask, mask_idx, penalty: Optional[Penalty], name: str) -> torch.Tensor:
    """fp32 [B, V] values a selection compares: the bf16 logits, penalised
    where ``penalty`` (None or off: nowhere) covers the row -- its slot is
    inside the table and its mask row's flag is set."""
    B = logits.shape[0]
    x = logits[:, :vocab].to(torch.bfloat16).float()
    if penalty is None or penalty.off:
        return x
    n_rows = mask.shape[0] if (mask is not None and mask_idx is not None) else B
    theta, _, alpha = penalty.check(name, B, (vocab + 31) // 32, n_rows, device=logits.device)
    sl = penalty.slots.long()
    on = sl >= 0
    if penalty.rows is not None:
        on = on & (penalty.rows[_mask_rows(B, mask, mask_idx, logits.device)] != 0)
    rows = penalty.history[sl.clamp(0, penalty.history.shape[0] - 1)]
    rows = torch.where(on[:, None], rows, torch.zeros_like(rows))
    return penalize(x, rows, theta, alpha)


def history_mark(history: torch.Tensor, tokens: torch.Tensor, slots: torch.Tensor,
                 src: Optional[torch.Tensor] = None, last_ids: Optional[torch.Tensor] = None,
                 exempt: Optional[torch.Tensor] = None, vocab: Optional[int] = None) -> torch.Tensor:
    """Record the tokens a decode step feeds: for every row r with
    ``slots[r]`` inside the table, set bit t of ``history[slots[r]]``, t =
    ``last_ids[src[r]]`` where ``src[r] >= 0`` else ``tokens[r]`` (the gather
    of :func:`decode_embed_norm`); tokens outside [0, vocab) and ids whose bit
    is set in ``exempt`` (int32 [W]) are not recorded.  In place."""
    W = history.shape[1]
    V = vocab or 32 * W
    toks = tokens.long()
    if src is not None:
        s = src.long()
        toks = torch.where(s >= 0, last_ids.long()[s.clamp(0, last_ids.numel() - 1)], toks)
    sl = slots.long()
    ok = (sl >= 0) & (sl < history.shape[0]) & (toks >= 0) & (toks < V)
    if exempt is not None:
        ex = (exempt.to(torch.int64)[(toks.clamp(0, V - 1)) // 32] >> (toks.clamp(0, V - 1) % 32)) & 1
        ok = ok & (ex == 0)
    h64 = history.to(torch.int64) & _M32
    for r in torch.nonzero(ok).flatten().tolist():
        t = int(toks[r])
        h64[int(sl[r]), t // 32] |= 1 << (t % 32)
    history.copy_(torch.where(h64 >= 2 ** 31, h64 - 2 ** 32, h64).to(torch.int32))
    return history


def history_reset(history: torch.Tensor, slots) -> torch.Tensor:
    """Zero the history rows of ``slots`` (a sequence of ints; entries outside
    the table are ignored).  In place."""
    for s in slots:
        if 0 <= int(s) < history.shape[0]:
            history[int(s)].zero_()
    return history


def masked_argmax(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, vocab: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, mask_idx: Optional[torch.Tensor] = None,
                  penalty: Optional[Penalty] = None) -> torch.Tensor:
    B, ld = logits.shape
    V = vocab or ld
    if penalty is None or penalty.off:
        x = logits[:, :V].float().clone()
    else:
        x = penalized(logits, V, mask, mask_idx, penalty, "masked_argmax")
    if mask is not None and mask_idx is not None:
        mask = mask[mask_idx.long().clamp(0, mask.shape[0] - 1)]
    if mask is not None:
        idx = torch.arange(V, device=logits.device)
        words = mask.to(torch.int64)[:, idx // 32]
        bits = (words >> (idx % 32)) & 1
        x[bits == 0] = float("-inf")
    ids = torch.argmax(x, dim=-1).to(torch.int32)  # first index among ties
    if out is not None:
        out.copy_(ids)
        return out
    return ids


def lm_head_argmax(x: torch.Tensor, w: torch.Tensor, masks: torch.Tensor, mask_idx: torch.Tensor,
                   out: Optional[torch.Tensor] = None, workspace=None,
                   penalty: Optional[Penalty] = None) -> torch.Tensor:
    """The fused LM head + masked argmax's definition: F.linear then masked_argmax."""
    logits = (x.float() @ w.float().t()).to(torch.bfloat16)
    return masked_argmax(logits, masks, w.shape[0], out, mask_idx, penalty)


# ---- temperature sampling as a perturbed argmax (Gumbel-max).  The noise is
# defined in uint32 arithmetic (here: int64 masked to 32 bits), so these
# functions and the three selection kernels (csrc/dmcp_common.hpp
# gumbel_score) draw from the same bits:
#   fmix32(h):  h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
#   key(row)     = fmix32(seed ^ fmix32(slot * 0x9E3779B1 + position))
#   bits(row, v) = fmix32(key(row) + v * 0x9E3779B1)
#   u = ((bits >> 9) + 0.5) * 2^-23       (exact in fp32, never 0 or 1)
#   g = -log(-log(u))
#   score(row, v) = bf16(logit) * fp32(1 / T) + g
_GOLD = 0x9E3779B1


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    """MurmurHash3's 32-bit finaliser on int64 tensors holding uint32 values."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def gumbel_bits(seed: int, slots: torch.Tensor, positions: torch.Tensor, vocab: int) -> torch.Tensor:
    """The noise bits [rows, vocab] (uint32 values in int64) of rows keyed by
    ``slots`` / ``positions`` under ``seed``."""
    s = slots.to(torch.int64) & _M32          # two's complement, as the kernels' uint32 cast
    p = positions.to(torch.int64) & _M32
    key = _fmix32((int(seed) & _M32) ^ _fmix32((s * _GOLD + p) & _M32))
    v = torch.arange(vocab, dtype=torch.int64, device=slots.device)
    return _fmix32((key[:, None] + ((v * _GOLD) & _M32)[None, :]) & _M32)


def gumbel_noise(seed: int, slots: torch.Tensor, positions: torch.Tensor, vocab: int,
                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Standard Gumbel variates [rows, vocab] in ``dtype`` (fp32 or fp64) from :func:`gumbel_bits`."""
    bits = gumbel_bits(seed, slots, positions, vocab)
    u = ((bits >> 9) * 2 + 1).to(dtype) * 2.0 ** -24  # ((bits >> 9) + 0.5) * 2^-23, exact in fp32
    return -torch.log(-torch.log(u))


def _sample_args(B: int, slots, positions, temperature) -> float:
    t = float(temperature)
    if not math.isfinite(t) or t < 0:
        raise ValueError(f"masked_sample: temperature must be finite and >= 0, got {temperature!r}")
    for key, which in ((slots, "slots"), (positions, "positions")):
        if not isinstance(key, torch.Tensor) or key.dtype != torch.int32 or key.numel() != B:
            raise ValueError(f"masked_sample: {which} must be int32 [{B}] (they key each row's noise)")
    return t


def sample_scores(logits: torch.Tensor, mask: Optional[torch.Tensor], vocab: Optional[int],
                  mask_idx: Optional[torch.Tensor], slots: torch.Tensor, positions: torch.Tensor,
                  temperature: float, seed: int, dtype: torch.dtype = torch.float32,
                  penalty: Optional[Penalty] = None) -> torch.Tensor:
    """The scores [B, V] whose row-wise argmax :func:`masked_sample` returns
    (temperature > 0): bf16(logit) * fp32(1 / T) + Gumbel noise in ``dtype``
    (fp32 as the kernels compute, fp64 for tests), -inf for the ids the row's
    mask excludes and for every id of a row whose slot is < 0.  Under a
    ``penalty`` the bf16 logit is the penalised value (:func:`penalize`)."""
    B, ld = logits.shape
    t = _sample_args(B, slots, positions, temperature)
    if t == 0:
        raise ValueError("sample_scores: temperature must be > 0")
    V = vocab or ld
    inv_t = float(torch.tensor(1.0 / t, dtype=torch.float32))
    x = (penalized(logits, V, mask, mask_idx, penalty, "masked_sample").to(dtype) * inv_t
         + gumbel_noise(seed, slots, positions, V, dtype))
    if mask is not None and mask_idx is not None:
        mask = mask[mask_idx.long().clamp(0, mask.shape[0] - 1)]
    if mask is not None:
        idx = torch.arange(V, device=logits.device)
        words = mask.to(torch.int64)[:, idx // 32]
        bits = (words >> (idx % 32)) & 1
        x[bits == 0] = float("-inf")
    x[slots.long() < 0] = float("-inf")
    return x


def masked_sample(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, vocab: Optional[int] = None,
                  out: Optional[torch.Tensor] = None, mask_idx: Optional[torch.Tensor] = None,
                  slots: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None,
                  temperature: float = 0.0, seed: int = 0, penalty: Optional[Penalty] = None) -> torch.Tensor:
    """:func:`masked_argmax` at a temperature: the allowed id with the highest
    bf16(logit) / T + Gumbel noise, an exact sample of softmax(logits / T) over
    the allowed ids; the lowest id among ties, 0 when nothing is allowed or the
    row's slot is < 0 (padding).  Temperature 0 is :func:`masked_argmax`."""
    if _sample_args(logits.shape[0], slots, positions, temperature) == 0:
        return masked_argmax(logits, mask, vocab, out, mask_idx, penalty)
    x = sample_scores(logits, mask, vocab, mask_idx, slots, positions, temperature, seed, penalty=penalty)
    ids = torch.argmax(x, dim=-1).to(torch.int32)  # first index among ties; 0 for an all -inf row
    if out is not None:
        out.copy_(ids)
        return out
    return ids


def lm_head_sample(x: torch.Tensor, w: torch.Tensor, masks: torch.Tensor, mask_idx: torch.Tensor,
                   out: Optional[torch.Tensor] = None, workspace=None, slots: Optional[torch.Tensor] = None,
                   positions: Optional[torch.Tensor] = None, temperature: float = 0.0,
                   seed: int = 0, penalty: Optional[Penalty] = None) -> torch.Tensor:
    """The fused LM head + sampling's definition: F.linear then masked_sample."""
    logits = (x.float() @ w.float().t()).to(torch.bfloat16)
    return masked_sample(logits, masks, w.shape[0], out, mask_idx, slots, positions, temperature, seed, penalty)


# ---- top-k / top-p / min-p truncation of the sampled selection.  Per row: A =
# the ids the mask allows (below vocab), x_v the bf16 logit widened to fp32,
# x_max = max over A.  Every filter is a threshold on the VALUE (ties are kept
# together, nothing depends on id order): kept = {v in A : x_v >= tau}, tau =
# max(tau_k, tau_p, tau_m) with
#   tau_k  the k-th largest x over A counting multiplicity; -inf when k = 0 or
#          k >= |A|
#   tau_p  over the top-k survivors (top-k, then top-p, as transformers
#          orders them): walking the distinct values downwards and
#          accumulating count(value) * exp((value - x_max) * fp32(1 / T)), the
#          first value at which the running sum reaches p * Z, Z the
#          survivors' total; -inf when p = 1
#   tau_m  v is kept iff (x_v - x_max) * inv_t >= ln_min_p in fp32 (a
#          subtract, then a multiply; ln_min_p = fp32(log(min_p)), the same
#          bits on the host and in the kernel): tau_m is the lowest value of A
#          that passes; -inf when min_p = 0
# The chosen id is the argmax over the kept set of the scores of
# :func:`sample_scores` (same hash, key and tie rule): with every filter off
# it is :func:`masked_sample`'s.  csrc/truncate.hip follows these definitions.
TOP_P_AMBIGUITY = 1e-4  # of Z: see truncation_threshold


def truncation_args(top_k=0, top_p=1.0, min_p=0.0) -> tuple:
    """The three truncation settings, validated: ``top_k`` an int >= 0 (0 =
    off), 0 < ``top_p`` <= 1 (1 = off), 0 <= ``min_p`` < 1 (0 = off); a
    ValueError names the offending knob.  Returns (top_k, top_p, min_p)."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    try:
        p, m = float(top_p), float(min_p)
    except (TypeError, ValueError):
        raise ValueError(f"top_p / min_p must be numbers, got {top_p!r} / {min_p!r}") from None
    if not (0.0 < p <= 1.0):
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    if not (0.0 <= m < 1.0):
        raise ValueError(f"min_p must be in [0, 1), got {min_p!r}")
    return int(top_k), p, m


def ln_min_p(min_p: float) -> float:
    """fp32(log(min_p)) as the kernel and the reference compare against
    (-inf for min_p = 0: nothing is cut)."""
    return float(torch.tensor(math.log(min_p), dtype=torch.float32)) if min_p > 0 else float("-inf")


def _allowed(logits: torch.Tensor, mask, vocab, mask_idx, slots) -> torch.Tensor:
    B, ld = logits.shape
    V = vocab or ld
    ok = torch.ones((B, V), dtype=torch.bool, device=logits.device)
    if mask is not None and mask_idx is not None:
        mask = mask[mask_idx.long().clamp(0, mask.shape[0] - 1)]
    if mask is not None:
        idx = torch.arange(V, device=logits.device)
        ok = ((mask.to(torch.int64)[:, idx // 32] >> (idx % 32)) & 1) != 0
    return ok & (slots.long() >= 0)[:, None]


def truncation_threshold(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, vocab: Optional[int] = None,
                         mask_idx: Optional[torch.Tensor] = None, slots: Optional[torch.Tensor] = None,
                         temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                         min_p: float = 0.0, penalty: Optional[Penalty] = None) -> tuple:
    """(tau fp32 [B], kept count int64 [B], ambiguous bool [B]) of the
    definitions above, thresholds in fp64 (the min-p comparison in fp32, as
    defined).  tau is -inf where no filter is on, the mask allows nothing or
    the row's slot is < 0.  A row is *ambiguous* when either running sum
    adjacent to tau_p is within ``TOP_P_AMBIGUITY`` * Z of p * Z: an fp32 sum
    of the same terms may then stop one value level earlier or later."""
    B, ld = logits.shape
    V = vocab or ld
    top_k, top_p, min_p = truncation_args(top_k, top_p, min_p)
    t = float(temperature)
    if not math.isfinite(t) or t <= 0:
        raise ValueError(f"truncation_threshold: temperature must be finite and > 0, got {temperature!r}")
    if slots is None:
        slots = torch.zeros(B, dtype=torch.int32, device=logits.device)
    inv_t = float(torch.tensor(1.0 / t, dtype=torch.float32))
    # -0 -> +0: a threshold on the value (the penalised value under a penalty)
    x = penalized(logits, V, mask, mask_idx, penalty, "truncation_threshold") + 0.0
    ok = _allowed(logits, mask, V, mask_idx, slots)
    tau = torch.full((B,), float("-inf"), dtype=torch.float32)
    kept = torch.zeros(B, dtype=torch.int64)
    amb = torch.zeros(B, dtype=torch.bool)
    lnm = ln_min_p(min_p)
    for b in range(B):
        xa = x[b][ok[b]]
        n = xa.numel()
        if n == 0:
            continue
        x_max = xa.max()
        tk = tp = tm = float("-inf")
        if 0 < top_k < n:
            tk = float(torch.topk(xa, top_k).values[-1])
        if top_p < 1.0:
            vals, counts = torch.unique(xa[xa >= tk], return_counts=True)  # ascending
            vals, counts = vals.flip(0), counts.flip(0)
            cum = torch.cumsum(counts.double() * torch.exp((vals.double() - float(x_max)) * inv_t), 0)
            z = float(cum[-1])
            i = min(int(torch.searchsorted(cum, torch.tensor(top_p * z, dtype=torch.float64))), vals.numel() - 1)
            tp = float(vals[i])
            near = [float(cum[i])] + ([float(cum[i - 1])] if i > 0 else [])
            amb[b] = any(abs(s - top_p * z) <= TOP_P_AMBIGUITY * z for s in near)
        if min_p > 0.0:
            tm = float(xa[(xa - x_max) * inv_t >= lnm].min())
        tau[b] = max(tk, tp, tm)
        kept[b] = int((xa >= tau[b]).sum())
    return tau, kept, amb


def tau_bits(tau: torch.Tensor) -> torch.Tensor:
    """The bf16 bit patterns (int32, 0 .. 0xFFFF) of thresholds, as the kernel reports them."""
    return tau.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF


def truncated_sample_at(tau: torch.Tensor, logits: torch.Tensor, mask: Optional[torch.Tensor] = None,
                        vocab: Optional[int] = None, mask_idx: Optional[torch.Tensor] = None,
                        slots: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None,
                        temperature: float = 1.0, seed: int = 0, penalty: Optional[Penalty] = None) -> tuple:
    """(ids int32 [B], kept count [B]) of the sampled selection over the
    allowed ids whose value is >= ``tau`` (fp32 [B]): what
    :func:`truncated_sample` returns for its own thresholds, and the expected
    result at a neighbouring value level for a row whose top-p sum is
    ambiguous."""
    V = vocab or logits.shape[1]
    scores = sample_scores(logits, mask, vocab, mask_idx, slots, positions, temperature, seed, penalty=penalty)
    cut = (penalized(logits, V, mask, mask_idx, penalty, "truncated_sample")
           < tau.to(torch.float32).to(logits.device)[:, None])
    kept = (_allowed(logits, mask, V, mask_idx, slots) & ~cut).sum(dim=1)
    scores[cut] = float("-inf")
    return torch.argmax(scores, dim=-1).to(torch.int32), kept  # first index among ties; 0 for an all -inf row


def truncated_sample(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, vocab: Optional[int] = None,
                     out: Optional[torch.Tensor] = None, mask_idx: Optional[torch.Tensor] = None,
                     slots: Optional[torch.Tensor] = None, positions: Optional[torch.Tensor] = None,
                     temperature: float = 0.0, seed: int = 0, top_k: int = 0, top_p: float = 1.0,
                     min_p: float = 0.0, stats: Optional[torch.Tensor] = None,
                     penalty: Optional[Penalty] = None) -> torch.Tensor:
    """:func:`masked_sample` over the ids :func:`truncation_threshold` keeps:
    the kept id with the highest score of :func:`sample_scores`, the lowest id
    among ties, 0 when nothing is allowed or the row's slot is < 0.
    Temperature 0 is :func:`masked_argmax` (the greedy id survives every
    truncation; ``stats`` is not written).  ``stats`` int32 [B, 2] receives
    the bf16 bits of tau and the kept count."""
    top_k, top_p, min_p = truncation_args(top_k, top_p, min_p)
    if _sample_args(logits.shape[0], slots, positions, temperature) == 0:
        return masked_argmax(logits, mask, vocab, out, mask_idx, penalty)
    tau, kept, _ = truncation_threshold(logits, mask, vocab, mask_idx, slots, temperature, top_k, top_p, min_p,
                                        penalty)
    ids, _ = truncated_sample_at(tau, logits, mask, vocab, mask_idx, slots, positions, temperature, seed, penalty)
    if stats is not None:
        stats.copy_(torch.stack([tau_bits(tau), kept.to(torch.int32)], dim=1).to(stats.device))
    if out is not None:
        out.copy_(ids)
        return out
    return ids


def embedding(table: torch.Tensor, ids: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = table[ids.long().clamp(0, table.shape[0] - 1)]
    if out is not None:
        out.copy_(y)
        return out
    return y


def decode_embed_norm(table: torch.Tensor, tokens: torch.Tensor, positions: torch.Tensor,
                      weight: Optional[torch.Tensor], eps: float, src: Optional[torch.Tensor] = None,
                      last_ids: Optional[torch.Tensor] = None, mask_idx: Optional[torch.Tensor] = None,
                      mask_alt: Optional[torch.Tensor] = None, alt_token: int = -1) -> tuple:
    """(resid, h, seq_len) of the decode step's first op (see the HIP kernel);
    ``mask_alt``: gathered rows whose token is ``alt_token`` switch
    ``mask_idx`` (in place) to ``mask_alt`` where that is >= 0."""
    toks = tokens
    if src is not None:
        s = src.long()
        gathered = last_ids.long()[s.clamp(0, last_ids.numel() - 1)].to(tokens.dtype)
        toks = torch.where(s >= 0, gathered, tokens)
        if mask_alt is not None:
            sw = (s >= 0) & (gathered == alt_token) & (mask_alt >= 0)
            mask_idx.copy_(torch.where(sw, mask_alt, mask_idx))
    resid = embedding(table, toks)
    h = add_rmsnorm(resid, weight, eps) if weight is not None else None
    return resid, h, positions + 1


# ---- MXFP8 prefill GEMMs (csrc/pgemm.hip): activations as e4m3 bytes with one
# power-of-two (E8M0) scale per 32 consecutive elements of a row, weights as
# e4m3 bytes with one fp32 scale per output row.
_INV_FP8_MAX = torch.tensor(1.0 / FP8_MAX, dtype=torch.float32)


def mx_quant(x: torch.Tensor, q: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None) -> tuple:
    """[M, K] (K % 32 == 0) -> (q uint8 [M, K] e4m3, s uint8 [M, K / 32] E8M0):
    block exponent e = the smallest with max|x| / 2^e <= 448, q = x / 2^e."""
    M, K = x.shape
    xf = x.float().reshape(M, K // 32, 32)
    amax = xf.abs().amax(-1)
    _, e = torch.frexp(amax * _INV_FP8_MAX.to(x.device))
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127)
    qv = torch.ldexp(xf, (-e)[..., None].to(torch.float32))
    qb = qv.clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8).reshape(M, K)
    sb = (e + 127).to(torch.uint8)
    if q is not None:
        q.copy_(qb)
        s.copy_(sb)
        return q, s
    return qb, sb


def mx_dequant(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 values of an MXFP8 tensor."""
    M, K = q.shape
    v = q.view(torch.float8_e4m3fn).float().reshape(M, K // 32, 32)
    return torch.ldexp(v, (s.to(torch.int32) - 127)[..., None].to(torch.float32)).reshape(M, K)


def quantize_weight(w: torch.Tensor) -> tuple:
    """[N, K] -> (e4m3 bytes [N, K], fp32 scale [N]): per-output-row scale max|w| / 448."""
    wf = w.float()
    sc = wf.abs().amax(-1) / FP8_MAX
    sc = torch.where(sc > 0, sc, torch.ones_like(sc))
    wq = (wf / sc[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return wq.contiguous(), sc.to(torch.float32).contiguous()


def weight_dequant(wq: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    return wq.view(torch.float8_e4m3fn).float() * ws[:, None].float()


def _pgemm_f32(aq, as_, wq, ws) -> torch.Tensor:
    return mx_dequant(aq, as_) @ weight_dequant(wq, ws).t()


def rmsnorm_mx(resid: torch.Tensor, weight: torch.Tensor, eps: float, add: Optional[torch.Tensor] = None,
               q: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None) -> tuple:
    """resid += add (bf16, in place); RMSNorm(resid) * weight as MXFP8."""
    if add is not None:
        resid.copy_((resid.float() + add.float()).to(resid.dtype))
    hf = resid.float()
    y = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()
    return mx_quant(y, q, s)


def pgemm(aq, as_, wq, ws, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    y = _pgemm_f32(aq, as_, wq, ws).to(torch.bfloat16)
    if out is not None:
        out.copy_(y)
        return out
    return y


def pgemm_resid(aq, as_, wq, ws, resid: torch.Tensor) -> torch.Tensor:
    y = _pgemm_f32(aq, as_, wq, ws).to(torch.bfloat16)
    resid.copy_((resid.float() + y.float()).to(resid.dtype))
    return resid


def pgemm_swiglu(aq, as_, wq, ws, q: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None) -> tuple:
    """silu(gate) * up of the stacked [gate; up] weight, as MXFP8 [M, I]."""
    gu = _pgemm_f32(aq, as_, wq, ws).to(torch.bfloat16).float()
    inter = gu.shape[1] // 2
    g, u = gu[:, :inter], gu[:, inter:]
    return mx_quant(g / (1.0 + torch.exp(-g)) * u, q, s)


def pgemm_qkv(aq, as_, wq, ws, pos, slot, cos_sin, k_cache, v_cache, n_q_heads: int,
              q_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    qkv = _pgemm_f32(aq, as_, wq, ws).to(torch.bfloat16)
    return rope_kv(qkv, pos, slot, cos_sin, k_cache, v_cache, n_q_heads, q_out)


# ---- routed expert MLP (Qwen3-MoE sparse block; csrc/moe.hip).  For each row
# of h [T, H]: router logits h . Wr^T over E experts, softmax over all E, the k
# largest probabilities (a tie goes to the lower expert id), optionally
# renormalised to sum 1, then y = sum_j p_j * down_e(silu(gate_e(h)) * up_e(h))
# over the chosen experts in rank order.  w_gu [E, 2 I, H] holds an expert's
# gate rows first, then its up rows (the dense wgu convention); w_down [E, H, I].
def moe_route_math(h: torch.Tensor, w_router: torch.Tensor, top_k: int, norm_topk: bool) -> tuple:
    """(ids int64 [T, k], p [T, k]) in the dtype of ``h`` (fp32 or fp64):
    the definition, shared by the bf16 op, the model's fp32 reference forward
    and the tests' fp64 oracle."""
    E = w_router.shape[0]
    if not 1 <= top_k <= E:
        raise ValueError(f"moe_route: top_k {top_k} outside [1, {E}] (num_experts)")
    prob = torch.softmax(h @ w_router.t(), dim=-1)
    # a stable descending sort keeps the lower id first among equal probabilities
    order = torch.sort(prob, dim=-1, descending=True, stable=True).indices[:, :top_k]
    p = prob.gather(1, order)
    if norm_topk:
        p = p / p.sum(-1, keepdim=True)
    return order, p


def moe_mlp_math(h: torch.Tensor, w_router: torch.Tensor, w_gu: torch.Tensor, w_down: torch.Tensor, top_k: int,
                 norm_topk: bool, round_act=None) -> torch.Tensor:
    """y [T, H] in the dtype of ``h`` (fp32 or fp64; weights of that dtype).
    ``round_act``: applied to silu(gate) * up (the kernel keeps it in bf16)."""
    ids, p = moe_route_math(h, w_router, top_k, norm_topk)
    inter = w_down.shape[2]
    y = torch.zeros_like(h)
    for j in range(top_k):  # rank order
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            x = h[rows]
            gu = x @ w_gu[e].t()
            g, u = gu[:, :inter], gu[:, inter:]
            act = g / (1.0 + torch.exp(-g)) * u
            if round_act is not None:
                act = round_act(act)
            y[rows] += p[rows, j:j + 1] * (act @ w_down[e].t())
    return y


def _moe_check(h, w_router, w_gu, w_down, top_k, name):
    E, H = w_router.shape
    if h.dim() != 2 or h.shape[1] != H:
        raise ValueError(f"{name}: h {tuple(h.shape)} does not match the router {tuple(w_router.shape)}")
    if not 1 <= top_k <= E:
        raise ValueError(f"{name}: top_k {top_k} outside [1, {E}] (num_experts)")
    if w_gu is not None:
        inter = w_down.shape[2] if w_down.dim() == 3 else -1
        if tuple(w_gu.shape) != (E, 2 * inter, H) or tuple(w_down.shape) != (E, H, inter):
            raise ValueError(f"{name}: w_gu {tuple(w_gu.shape)} / w_down {tuple(w_down.shape)} are not "
                             f"[E, 2I, H] / [E, H, I] for E {E}, H {H}")


def moe_route(h: torch.Tensor, w_router: torch.Tensor, top_k: int, norm_topk: bool) -> tuple:
    """(ids int32 [T, k], p fp32 [T, k]) of bf16 rows ``h`` [T, H] under the
    bf16 router ``w_router`` [E, H]; logits, softmax and selection in fp32."""
    _moe_check(h, w_router, None, None, top_k, "moe_route")
    ids, p = moe_route_math(h.float(), w_router.float(), int(top_k), bool(norm_topk))
    return ids.to(torch.int32), p


def moe_mlp(h: torch.Tensor, w_router: torch.Tensor, w_gu: torch.Tensor, w_down: torch.Tensor, top_k: int,
            norm_topk: bool, residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
            eps: float = 0.0, workspace: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The routed expert MLP of bf16 rows ``h`` [T, H] (already normalised),
    with what follows it in the model: m = bf16(y), then
    ``add_rmsnorm(m, norm_w, eps, residual=residual)`` when ``norm_w`` is
    given (``residual`` updated in place, the normalised rows returned);
    ``residual`` alone: residual += m, returned; neither: m.  ``workspace``
    is the GPU kernels' scratch (:func:`dmcp.ops.hip.moe_workspace`), unused here."""
    _moe_check(h, w_router, w_gu, w_down, top_k, "moe_mlp")
    m = moe_mlp_math(h.float(), w_router.float(), w_gu.float(), w_down.float(), int(top_k), bool(norm_topk),
                     round_act=lambda a: a.to(torch.bfloat16).float()).to(h.dtype)
    if norm_w is not None:
        return add_rmsnorm(m, norm_w, eps, residual=residual, out=out)
    if residual is not None:
        residual.copy_((m.float() + residual.float()).to(residual.dtype))
        return residual
    if out is not None:
        out.copy_(m)
        return out
    return m


# ---- sigmoid routing with shared experts (GLM-4.5, ``glm4_moe``; the router
# of DeepSeek-V3-style blocks with one expert group).  For each row of h:
#
#   s      = sigmoid(h . Wr^T)                          over E experts
#   chosen = the k largest of s + bias (bias fp32 [E], ``e_score_correction_bias``:
#            it enters the selection only); a tie goes to the lower expert id
#   weight = the unbiased s of the chosen experts, divided by (sum + 1e-20)
#            when norm_topk, then multiplied by route_scale
#   y      = sum_j weight_j * expert_{chosen_j}(h) + shared(h)
#
# where shared is an always-on SwiGLU MLP of width S * I (S = n_shared).  A NaN
# logit never wins and never blocks the selection (its selection score is
# -inf, its weight 0).
#
# A SwiGLU MLP is a sum over slices of its intermediate dimension:
#   down(silu(gate(h)) * up(h)) = sum_s down[:, sI:(s+1)I] (silu(gate[sI:(s+1)I] h) * up[sI:(s+1)I] h)
# so a shared MLP of width S * I is exactly S always-chosen experts of width I
# with weight 1.  The ops take it that way: w_gu [E + S, 2 I, H] and w_down
# [E + S, H, I] stack the E routed experts, then the S slices
# (:func:`moe_stack_shared`), and a row has k + S (expert, weight) pairs -- its
# k routed ones in rank order, then (E + s, 1.0) for s = 0 .. S - 1.
def moe_route_sig_math(h: torch.Tensor, w_router: torch.Tensor, bias: torch.Tensor, top_k: int, norm_topk: bool,
                       route_scale: float = 1.0, n_shared: int = 0) -> tuple:
    """(ids int64 [T, k + S], p [T, k + S]) in the dtype of ``h`` (fp32 or
    fp64): the definition above, shared by the bf16 op, the model's fp32
    reference forward and the tests' fp64 oracle."""
    E = w_router.shape[0]
    if not 1 <= top_k <= E:
        raise ValueError(f"moe_route_sig: top_k {top_k} outside [1, {E}] (num_experts)")
    if n_shared < 0:
        raise ValueError(f"moe_route_sig: n_shared {n_shared} is negative")
    logits = h @ w_router.t()
    bad = logits.isnan()
    s = torch.where(bad, torch.zeros_like(logits), torch.sigmoid(logits))
    choice = s + bias.to(s.dtype)
    choice = torch.where(bad | choice.isnan(), torch.full_like(choice, float("-inf")), choice)
    # a stable descending sort keeps the lower id first among equal scores
    order = torch.sort(choice, dim=-1, descending=True, stable=True).indices[:, :top_k]
    p = s.gather(1, order)
    if norm_topk:
        p = p / (p.sum(-1, keepdim=True) + 1e-20)
    p = p * route_scale
    if n_shared:
        T = h.shape[0]
        order = torch.cat([order, (E + torch.arange(n_shared, device=order.device)).expand(T, n_shared)], 1)
        p = torch.cat([p, torch.ones((T, n_shared), dtype=p.dtype, device=p.device)], 1)
    return order, p


def moe_stack_shared(w_gu: torch.Tensor, w_down: torch.Tensor, sh_gate: Optional[torch.Tensor],
                     sh_up: Optional[torch.Tensor], sh_down: Optional[torch.Tensor], n_shared: int) -> tuple:
    """(w_gu [E + S, 2I, H], w_down [E + S, H, I]): the routed stacks with the
    shared MLP (gate / up [S I, H], down [H, S I]) appended as S slices of
    width I: slice s takes gate rows [sI, (s+1)I), the same up rows and down
    columns [sI, (s+1)I)."""
    if not n_shared:
        return w_gu, w_down
    E, H, inter = w_down.shape
    if tuple(sh_gate.shape) != (n_shared * inter, H) or tuple(sh_up.shape) != (n_shared * inter, H) \
            or tuple(sh_down.shape) != (H, n_shared * inter):
        raise ValueError(f"moe_stack_shared: shared gate {tuple(sh_gate.shape)} / up {tuple(sh_up.shape)} / down "
                         f"{tuple(sh_down.shape)} are not [S I, H] / [S I, H] / [H, S I] for S {n_shared}, I {inter}, "
                         f"H {H}")
    gu = torch.cat([sh_gate.view(n_shared, inter, H), sh_up.view(n_shared, inter, H)], 1)
    down = sh_down.view(H, n_shared, inter).permute(1, 0, 2)
    return torch.cat([w_gu, gu.to(w_gu.dtype)], 0).contiguous(), torch.cat([w_down, down.to(w_down.dtype)], 0).contiguous()


def moe_mlp_sh_math(h: torch.Tensor, w_router: torch.Tensor, bias: torch.Tensor, w_gu: torch.Tensor,
                    w_down: torch.Tensor, top_k: int, norm_topk: bool, route_scale: float = 1.0, n_shared: int = 0,
                    round_act=None) -> torch.Tensor:
    """y [T, H] in the dtype of ``h`` (fp32 or fp64; weights of that dtype):
    the routed ranks in rank order, then the shared slices in order.
    ``round_act``: applied to silu(gate) * up (the kernel keeps it in bf16)."""
    ids, p = moe_route_sig_math(h, w_router, bias, top_k, norm_topk, route_scale, n_shared)
    inter = w_down.shape[2]
    y = torch.zeros_like(h)
    for j in range(top_k + n_shared):
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            x = h[rows]
            gu = x @ w_gu[e].t()
            g, u = gu[:, :inter], gu[:, inter:]
            act = g / (1.0 + torch.exp(-g)) * u
            if round_act is not None:
                act = round_act(act)
            y[rows] += p[rows, j:j + 1] * (act @ w_down[e].t())
    return y


def _moe_sh_check(h, w_router, bias, w_gu, w_down, top_k, route_scale, n_shared, name):
    E, H = w_router.shape
    if h.dim() != 2 or h.shape[1] != H:
        raise ValueError(f"{name}: h {tuple(h.shape)} does not match the router {tuple(w_router.shape)}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= E:
        raise ValueError(f"{name}: top_k {top_k} outside [1, {E}] (num_experts)")
    if isinstance(n_shared, bool) or not isinstance(n_shared, int) or n_shared < 0:
        raise ValueError(f"{name}: n_shared {n_shared!r} must be an integer >= 0")
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (E,):
        raise ValueError(f"{name}: bias must be fp32 [{E}], got "
                         f"{getattr(bias, 'dtype', type(bias).__name__)} {tuple(getattr(bias, 'shape', ()))}")
    if not (math.isfinite(route_scale) and route_scale > 0):
        raise ValueError(f"{name}: route_scale {route_scale!r} must be finite and > 0")
    if w_gu is not None:
        G = E + n_shared
        inter = w_down.shape[2] if w_down.dim() == 3 else -1
        if tuple(w_gu.shape) != (G, 2 * inter, H) or tuple(w_down.shape) != (G, H, inter):
            raise ValueError(f"{name}: w_gu {tuple(w_gu.shape)} / w_down {tuple(w_down.shape)} are not "
                             f"[E + S, 2I, H] / [E + S, H, I] for E {E}, S {n_shared}, H {H}")


def moe_route_sig(h: torch.Tensor, w_router: torch.Tensor, bias: torch.Tensor, top_k: int, norm_topk: bool,
                  route_scale: float = 1.0, n_shared: int = 0) -> tuple:
    """(ids int32 [T, k + S], p fp32 [T, k + S]) of bf16 rows ``h`` [T, H]
    under the bf16 router ``w_router`` [E, H] and the fp32 selection bias [E]:
    logits, sigmoid and selection in fp32."""
    _moe_sh_check(h, w_router, bias, None, None, top_k, route_scale, n_shared, "moe_route_sig")
    ids, p = moe_route_sig_math(h.float(), w_router.float(), bias, int(top_k), bool(norm_topk), float(route_scale),
                                int(n_shared))
    return ids.to(torch.int32), p


def moe_mlp_sh(h: torch.Tensor, w_router: torch.Tensor, bias: torch.Tensor, w_gu: torch.Tensor, w_down: torch.Tensor,
               top_k: int, norm_topk: bool, route_scale: float = 1.0, n_shared: int = 0,
               residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0,
               workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`moe_mlp` under the sigmoid router with ``n_shared`` shared
    pseudo-experts stacked after the routed ones (the definition above);
    residual / norm_w / out as there."""
    _moe_sh_check(h, w_router, bias, w_gu, w_down, top_k, route_scale, n_shared, "moe_mlp_sh")
    m = moe_mlp_sh_math(h.float(), w_router.float(), bias, w_gu.float(), w_down.float(), int(top_k), bool(norm_topk),
                        float(route_scale), int(n_shared),
                        round_act=lambda a: a.to(torch.bfloat16).float()).to(h.dtype)
    if norm_w is not None:
        return add_rmsnorm(m, norm_w, eps, residual=residual, out=out)
    if residual is not None:
        residual.copy_((m.float() + residual.float()).to(residual.dtype))
        return residual
    if out is not None:
        out.copy_(m)
        return out
    return m


# ---- block-scaled FP8 weights (the hub's ``quant_method: "fp8"`` layout with
# ``weight_block_size: [128, 128]``).  A linear weight W [N, K] is stored as
# ``X.weight`` in e4m3fn (torch.float8_e4m3fn) plus ``X.weight_scale_inv``, fp32
# [ceil(N / 128), ceil(K / 128)]; despite the name the stored number is the
# multiplier: W[n, k] = float(w8[n, k]) * scale_inv[n // 128, k // 128].  Edge
# blocks are partial.  Leading axes (a stack of experts) pass through.
#
# The routed expert MLP's stacked tensors: w_gu8 [E, 2I, H] (gate rows, then up
# rows) with s_gu [E, 2 ceil(I / 128), ceil(H / 128)] -- the gate's block rows
# first, then the up's, each projection's blocks counted from its own row 0 --
# and w_down8 [E, H, I] with s_down [E, ceil(H / 128), ceil(I / 128)].
FP8_BLOCK = 128
FP8_E4M3_MAX = 448.0


def _block_expand(scale: torch.Tensor, rows: int, cols: int, block: int) -> torch.Tensor:
    """One scale per element: [..., ceil(rows / b), ceil(cols / b)] -> [..., rows, cols]."""
    return scale.repeat_interleave(block, dim=-2)[..., :rows, :].repeat_interleave(block, dim=-1)[..., :cols]


def block_fp8_dequant(w8: torch.Tensor, scale_inv: torch.Tensor, dtype: torch.dtype = torch.float32,
                      block: int = FP8_BLOCK) -> torch.Tensor:
    """W = float(w8) * scale_inv[n // block, k // block], computed in fp32
    (exact: an e4m3 value times an fp32 scale rounds once) and cast to ``dtype``."""
    if w8.dtype != torch.float8_e4m3fn:
        raise ValueError(f"block_fp8_dequant: expected float8_e4m3fn, got {w8.dtype}")
    rows, cols = w8.shape[-2:]
    want = tuple(w8.shape[:-2]) + (-(-rows // block), -(-cols // block))
    if tuple(scale_inv.shape) != want:
        raise ValueError(f"block_fp8_dequant: scale_inv {tuple(scale_inv.shape)} does not match weight "
                         f"{tuple(w8.shape)} (expected {want})")
    return (w8.float() * _block_expand(scale_inv.float(), rows, cols, block)).to(dtype)


def block_fp8_quant(w: torch.Tensor, block: int = FP8_BLOCK) -> tuple:
    """(w8 e4m3fn, scale_inv fp32) of ``w`` [..., N, K]: per block scale =
    amax / 448 (1 for an all-zero block), values divided by it, clamped to
    +-448 and cast (round to nearest even)."""
    rows, cols = w.shape[-2:]
    nb, kb = -(-rows // block), -(-cols // block)
    wf = w.float()
    pad = torch.zeros(tuple(w.shape[:-2]) + (nb * block, kb * block), dtype=torch.float32, device=w.device)
    pad[..., :rows, :cols] = wf.abs()
    amax = pad.view(*w.shape[:-2], nb, block, kb, block).amax(dim=(-3, -1))
    scale = torch.where(amax > 0, amax / FP8_E4M3_MAX, torch.ones_like(amax))
    q = (wf / _block_expand(scale, rows, cols, block)).clamp(-FP8_E4M3_MAX, FP8_E4M3_MAX)
    return q.to(torch.float8_e4m3fn), scale


def _moe_w8_check(h, w_router, w_gu8, s_gu, w_down8, s_down, top_k, name):
    _moe_check(h, w_router, w_gu8, w_down8, top_k, name)
    E, H = w_router.shape
    inter = w_down8.shape[2]
    for t, which in ((w_gu8, "w_gu8"), (w_down8, "w_down8")):
        if t.dtype != torch.float8_e4m3fn:
            raise ValueError(f"{name}: {which} must be float8_e4m3fn, got {t.dtype}")
    nbi, nbh = -(-inter // FP8_BLOCK), -(-H // FP8_BLOCK)
    for t, which, want in ((s_gu, "s_gu", (E, 2 * nbi, nbh)), (s_down, "s_down", (E, nbh, nbi))):
        if t.dtype != torch.float32 or tuple(t.shape) != want:
            raise ValueError(f"{name}: {which} is {t.dtype} {tuple(t.shape)}, expected float32 {want}")


def moe_w8_dequant(w_gu8: torch.Tensor, s_gu: torch.Tensor, w_down8: torch.Tensor, s_down: torch.Tensor,
                   dtype: torch.dtype = torch.float32) -> tuple:
    """(w_gu [E, 2I, H], w_down [E, H, I]) of the stacked expert tensors: the
    gate and up halves are dequantised each with its own block rows."""
    inter = w_down8.shape[2]
    nbi = s_gu.shape[1] // 2
    gate = block_fp8_dequant(w_gu8[:, :inter], s_gu[:, :nbi], dtype)
    up = block_fp8_dequant(w_gu8[:, inter:], s_gu[:, nbi:], dtype)
    return torch.cat([gate, up], 1), block_fp8_dequant(w_down8, s_down, dtype)


def moe_mlp_w8(h: torch.Tensor, w_router: torch.Tensor, w_gu8: torch.Tensor, s_gu: torch.Tensor,
               w_down8: torch.Tensor, s_down: torch.Tensor, top_k: int, norm_topk: bool,
               residual: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None, eps: float = 0.0,
               workspace: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`moe_mlp` over block-scaled FP8 expert weights, dequantised
    exactly in fp32 (never rounded to bf16); activations stay bf16, with the
    same bf16 rounding of act and of m and the same ``add_rmsnorm`` contract."""
    _moe_w8_check(h, w_router, w_gu8, s_gu, w_down8, s_down, top_k, "moe_mlp_w8")
    w_gu, w_down = moe_w8_dequant(w_gu8, s_gu, w_down8, s_down)
    m = moe_mlp_math(h.float(), w_router.float(), w_gu, w_down, int(top_k), bool(norm_topk),
                     round_act=lambda a: a.to(torch.bfloat16).float()).to(h.dtype)
    if norm_w is not None:
        return add_rmsnorm(m, norm_w, eps, residual=residual, out=out)
    if residual is not None:
        residual.copy_((m.float() + residual.float()).to(residual.dtype))
        return residual
    if out is not None:
        out.copy_(m)
        return out
    return m
