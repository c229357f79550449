"""Device ops for the local enrichment model.

GPU (HIP) tensors run the hand-written gfx950 kernels of ``dmcp/ops/csrc``
(:mod:`dmcp.ops.hip`, loaded from the in-tree ``_hipops.so``; a missing
library is an error, never a silent fallback).  CPU tensors run the fp32
PyTorch references of :mod:`dmcp.ops.reference` -- that path exists for
GPU-less unit tests, and only for the ops below that have one; the other
fused / weight-streaming GEMMs are GPU-only and are re-exported from :mod:`.hip`.

Launch limits and plans (row limits, split counts, workspaces) are defined
once, in :mod:`.hip`, next to the kernels they describe.
"""
from __future__ import annotations

from . import hip, reference
from .hip import (FUSED_MAX_ROWS, PREFIX_MFMA_MAX_SPLITS, WGEMM_MAX_ROWS, decode_workspace,  # noqa: F401
                  fused_linear_norm, fused_rope_kv, fused_swiglu, lm_head_supported, lm_head_workspace,
                  prefill_supported, wgemm_resid_norm, wgemm_rope_kv, wgemm_swiglu, wgemm_workspace)
from .hip import (PGEMM_TILE_N, WMX_MAX_ROWS, pgemm_supported, wgemm_mx_resid_norm, wgemm_mx_rope_kv,  # noqa: F401
                  wgemm_mx_swiglu, wmx_plan)
from .hip import (TGEMM_MAX_ROWS, tgemm, tgemm_lm_head_argmax, tgemm_lm_head_sample,  # noqa: F401
                  tgemm_resid_norm, tgemm_rope_kv, tgemm_swiglu, wgemm)
from .hip import MOE_MAX_PAIRS, moe_sh_supported, moe_sh_workspace, moe_supported, moe_workspace  # noqa: F401
from .reference import Penalty, penalize  # noqa: F401
from .reference import SharedPrefix, mx_dequant, quantize_weight, rope_tables, weight_dequant  # noqa: F401
from .reference import block_fp8_dequant, block_fp8_quant  # noqa: F401


def _on(t):
    """The implementation for tensor ``t``'s device."""
    return hip if t.is_cuda else reference


def _by_device(name: str):
    """``name`` dispatched on its first tensor argument's device: the gfx950
    kernel (:mod:`.hip`) for GPU tensors, the fp32 reference for CPU ones.
    Both modules implement these ops with the same signature
    (tests/test_launch_plans.py::test_device_ops_share_one_signature); the
    GPU kernel's docstring is the op's."""
    k, r = getattr(hip, name), getattr(reference, name)

    def op(first, *args, **kw):
        return (k if first.is_cuda else r)(first, *args, **kw)
    op.__name__ = op.__qualname__ = name
    op.__doc__ = k.__doc__ or r.__doc__
    op.__wrapped__ = k  # inspect.signature reports the kernel's parameters
    return op


# ops with an fp32 CPU reference: norms, RoPE + KV append, prefill attention,
# SwiGLU, selection (greedy, sampled at a temperature, and sampled under
# top-k / top-p / min-p truncation; each optionally under a repetition /
# presence penalty, whose history table history_mark / history_reset keep),
# embedding, the
# decode step's input gather + first norm, the MXFP8 prefill path
# (csrc/pgemm.hip), and the three fused QKV projections (their references
# define where the optional bias and QK-norm enter)
DEVICE_OPS = ("history_mark", "history_reset",
              "add_rmsnorm", "rope_kv", "prefill_attention", "prefill_attention_varlen", "silu_mul",
              "masked_argmax", "lm_head_argmax", "masked_sample", "lm_head_sample", "truncated_sample", "embedding",
              "decode_embed_norm",
              "mx_quant", "rmsnorm_mx", "pgemm", "pgemm_resid", "pgemm_swiglu", "pgemm_qkv", "fused_rope_kv",
              "wgemm_rope_kv", "tgemm_rope_kv",
              # the routed expert MLP of a mixture-of-experts layer (csrc/moe.hip), over bf16 and over
              # block-scaled FP8 expert weights; and under the sigmoid router with shared experts (GLM-4.5)
              "moe_route", "moe_mlp", "moe_mlp_w8", "moe_route_sig", "moe_mlp_sh")
for _name in DEVICE_OPS:
    globals()[_name] = _by_device(_name)
del _name


def decode_attention(q, k_cache, v_cache, slot, seq_len, scale, workspace=None, chunk: int = 256, out=None,
                     prefix=None, splits=None, fork=None, kv_scale=None, window: int = 0):
    """Per-row decode attention; the CPU reference takes no split count.
    ``window`` > 0: sliding-window attention (0 = every key, the call as it was)."""
    if q.is_cuda:
        if not window:
            return hip.decode_attention(q, k_cache, v_cache, slot, seq_len, scale, workspace, chunk, out, prefix,
                                        splits, fork, kv_scale)
        return hip.decode_attention(q, k_cache, v_cache, slot, seq_len, scale, workspace, chunk, out, prefix, splits,
                                    fork, kv_scale, window)
    return reference.decode_attention(q, k_cache, v_cache, slot, seq_len, scale, workspace, chunk, out, prefix, fork,
                                      kv_scale, window)


# GPU-only fused GEMM with a shape-dependent default
def fused_resid(x, w, residual, wk: int = 0):
    """residual += x . w^T in one gfx950 kernel; K-split waves by K."""
    return hip.fused_resid(x, w, residual, wk or (16 if x.shape[1] >= 4096 else 8))


def decode_plan(rows, n_kv_heads, max_seq, kv_dtype: str = "bf16"):
    """(chunk, splits) of the per-row decode attention (:func:`dmcp.ops.hip.decode_plan`).
    An fp8 cache halves the bytes per key, so fewer, longer splits keep the
    same bytes in flight: 2,048 target waves instead of 4,096 (fp8 step 2.35
    -> 2.30 ms at 78 rows, 5.54 -> 5.36 at 320; bf16 2.84 vs 2.94 the other
    way -- profiles/decode_target_waves_r2.txt).  The per-row scaled format
    ("fp8s") has fp8's bytes per key and takes fp8's plan."""
    return hip.decode_plan(rows, n_kv_heads, max_seq, target_waves=2048 if kv_dtype in ("fp8", "fp8s") else 4096)
