"""Llama-style decoder for local (on-GPU) enrichment -- MI355X extension.

Not part of the reference (it calls the Anthropic API, ``ClaudeApiClient``);
SURVEY §5.8 identifies a local enrichment model as the only legitimate GPU
workload of this service.  Architecture: RMSNorm, rotate-half RoPE, GQA
attention, SwiGLU MLP, untied LM head, bf16 weights and KV cache.

MI355X mapping:

* small decode steps (<= ``fused_max_rows`` = 16 rows: the tail of a batch,
  single requests) run every weight product on the fused gfx950 MFMA GEMMs
  of :mod:`dmcp.ops` (``csrc/fused_gemm.hip``): RMSNorm folded into the
  QKV / gate-up / LM-head prologue (norm weights are folded into those
  matrices at load time, :meth:`LocalLM._fold_norms`), RoPE + KV-cache
  append in the QKV epilogue, SwiGLU in the gate/up epilogue, the residual
  add in the O / down epilogues -- a layer is 4 GEMM launches + attention
  (measured: 60 vs 77 us per layer at 16 rows);
* decode steps of 17-512 rows (the enrichment operating point is 300-500)
  run every projection on the weight-streaming GEMM (``csrc/wgemm.hip``:
  each weight tile read from HBM once per step, all rows of an M part per
  block, the M parts of a tile on one XCD) with the neighbour op fused:
  QKV + RoPE + KV append, O + residual + RMSNorm, gate/up + SwiGLU, down +
  residual + next RMSNorm -- 4 GEMMs + 3 row reductions per layer;
* prefill / extend use hipBLASLt through ``torch.nn.functional.linear``
  (thousands of rows: large MFMA tiles win) with the hand-written
  element-wise kernels between (fused residual-add + RMSNorm, RoPE +
  KV-cache append, SwiGLU);
* decode attention (per-row split-K kernel + the shared-prefix kernel,
  merged by log-sum-exp), masked greedy sampling and the embedding gather
  are hand-written gfx950 kernels on every path;
* prefill / extend attention runs on the MFMA flash kernel
  (``csrc/prefill_attn.hip``): the shared prompt prefix is read in place
  from its cache slot (a fork costs no copy), causal masking of the own
  keys; PyTorch SDPA only where the kernel's head shapes do not apply;
* the KV cache is one preallocated slab ``[layers, slots, Hkv, max_seq, D]``
  in bf16 or FP8 e4m3 (``LMConfig.kv_dtype``; 288 GB of HBM per GPU: no
  paging needed at these sizes) so decode reads every key row of a
  (slot, kv-head) contiguously;
* the batched decode step is captured into hipGraphs per batch-size bucket
  (:class:`DecodeGraphs`), removing ~10 launches/layer of host overhead.

Weights are random-initialised by default (no checkpoint on this host) or
loaded from a Llama-, Qwen2-, Qwen3-, Qwen3-MoE- or GLM-4.5-format safetensors
directory (``load_safetensors``: RoPE scaling, q/k/v biases, Qwen3's per-head q/k
RMSNorm, Qwen3-MoE's routed expert MLP -- ``ops.moe_mlp``, csrc/moe.hip -- and
GLM-4.5's sigmoid router with shared experts, leading dense layers and partial
rotary embedding -- ``ops.moe_mlp_sh`` -- on every forward path; a directory
it cannot reproduce is refused, ``check_checkpoint``).
"""
from __future__ import annotations

import json
import math
import os
import time
from dataclasses import asdict, dataclass, field, replace
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .. import ops
from ..ops.reference import truncation_args

BYTE_VOCAB = 256
BOS, EOS, PAD = 256, 257, 258


@dataclass(frozen=True)
class LMConfig:
    name: str = "dmcp-coder-1b"
    vocab_size: int = 320           # 259 byte-level tokens, padded to a multiple of 64
    hidden: int = 2048
    layers: int = 16
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 64
    intermediate: int = 8192
    rope_theta: float = 10000.0
    eps: float = 1e-5
    max_seq: int = 8192             # KV capacity per slot (prompt + generation)
    # KV slots = concurrent sequences: 256 x 8,192 positions is 69 GB of bf16
    # KV (34 GB fp8) -- sized for one MI355X's 288 GB; the decode step's
    # weight GEMMs are HBM-bound and cost about the same at 78 or 300 rows, so
    # wide steps amortise them (measured: batch 64 -> 256, 23 -> 34 classes/s)
    max_batch: int = 256
    max_rows: int = 384             # token rows per batched decode/extend step (jump-forward)
    # KV cache storage: "bf16", "fp8" (e4m3, unit scale, half the bytes) or
    # "fp8s" (e4m3 + one power-of-two exponent byte per cached row: rows that
    # leave e4m3's range at unit scale -- Qwen2's K biases -- or sit in its
    # subnormals keep their 3 mantissa bits; ops.reference.kv_encode_scaled)
    kv_dtype: str = "bf16"
    # batched-prefill projections: "bf16" (hipBLASLt) or "fp8" (MXFP8
    # activations x per-row-scaled e4m3 weights on the MX matrix cores,
    # csrc/pgemm.hip, epilogues fused); decode keeps the bf16 weights.
    # "auto": fp8 where the kernels run (a gfx950 device and supported dims;
    # 1.37x the bf16 batched prefill, profiles/fp8_paths_r4_cvtpk.jsonl),
    # else bf16
    prefill_dtype: str = "bf16"
    # decode steps of fused_max_rows < rows <= WMX_MAX_ROWS: "bf16" (wgemm.hip /
    # hipBLASLt) or "fp8" (the same e4m3 weights, MXFP8 activations written by
    # the producing norm / SwiGLU: csrc/pgemm.hip wmx_kernel)
    decode_dtype: str = "bf16"
    # the preset's tokenizer: "" = byte-level (dmcp.enrich.tokenizer.ByteTokenizer),
    # else an asset directory under dmcp/models/assets (tokenizer.json.gz)
    tokenizer: str = ""
    # RoPE frequency scaling of a loaded checkpoint: None, or the sorted
    # (key, value) pairs of its rope_scaling dict (ops.reference.rope_scaling_key:
    # "linear" or "llama3"; hashable, so a config stays a dict key)
    rope_scaling: Optional[tuple] = None
    # mixture-of-experts MLP (Qwen3-MoE): every layer's MLP is a router over
    # n_experts SwiGLU experts of width moe_intermediate, experts_per_tok of
    # them per token, their probabilities renormalised when norm_topk
    # (ops.moe_mlp, csrc/moe.hip).  n_experts 0: the dense MLP of `intermediate`
    n_experts: int = 0
    experts_per_tok: int = 0
    moe_intermediate: int = 0
    norm_topk: bool = True
    # the experts' weight format: "bf16", or "fp8b" -- e4m3 bytes with one fp32
    # scale per 128 x 128 block (ops.reference.block_fp8_dequant; ops.moe_mlp_w8),
    # as a block-scaled FP8 checkpoint stores them.  Set by the loader from the
    # checkpoint; a random-init preset with "fp8b" quantises its random experts
    moe_weight_dtype: str = "bf16"
    # the router (ops.reference): "softmax" (Qwen3-MoE: top-k of the softmax) or
    # "sigmoid" (GLM-4.5: the k largest of sigmoid + a per-expert selection
    # bias w["l{i}.router_bias"], weighted by the unbiased scores, renormalised
    # when norm_topk, then times moe_route_scale; ops.moe_mlp_sh).  moe_shared:
    # always-on shared experts, a SwiGLU MLP of width moe_shared x
    # moe_intermediate beside the routed ones (sigmoid router only).
    # dense_lead: the first dense_lead layers keep the dense MLP of
    # `intermediate`, the rest are routed.  The defaults are Qwen3-MoE's block
    moe_score: str = "softmax"
    moe_route_scale: float = 1.0
    moe_shared: int = 0
    dense_lead: int = 0
    # partial rotary embedding: the width of a head that RoPE rotates (0 = the
    # whole head).  The loader permutes each head's q / k rows so the kernels'
    # whole-head rotation applies it (ops.reference.partial_rotary_perm); the
    # cos / sin table holds cos 1, sin 0 for the pass-through pairs
    rotary_dim: int = 0
    # sliding-window attention (Mistral; Qwen2 / Qwen3 with use_sliding_window):
    # one int per layer, the keys a query attends including its own (0 = every
    # key); None = full attention in every layer.  The loader resolves it from
    # sliding_window / max_window_layers / layer_types (checkpoint_windows); a
    # window >= max_seq is stored as 0.  The KV cache stays linear.
    layer_windows: Optional[tuple] = None

    @property
    def qkv_dim(self) -> int:
        return (self.n_heads + 2 * self.n_kv_heads) * self.head_dim

    def sparse_layer(self, i: int) -> bool:
        """Layer i's MLP is the routed one (else the dense MLP of ``intermediate``)."""
        return self.n_experts > 0 and i >= self.dense_lead

    def param_count(self) -> int:
        dense = 3 * self.intermediate * self.hidden
        routed = ((self.n_experts + self.moe_shared) * 3 * self.moe_intermediate + self.n_experts) * self.hidden
        n_sparse = max(0, self.layers - self.dense_lead) if self.n_experts else 0
        per_layer = self.qkv_dim * self.hidden + self.n_heads * self.head_dim * self.hidden + 2 * self.hidden
        return (self.layers * per_layer + n_sparse * routed + (self.layers - n_sparse) * dense
                + 2 * self.vocab_size * self.hidden + self.hidden)

    @property
    def kv_elem_bytes(self) -> int:
        return 1 if self.kv_dtype in ("fp8", "fp8s") else 2

    def kv_bytes(self) -> int:
        """The K + V slab of ``max_batch`` slots; "fp8s" counts its exponent
        tables (one byte per cached row: 1 / head_dim of the cache)."""
        rows = 2 * self.layers * self.max_batch * self.n_kv_heads * self.max_seq
        return rows * self.head_dim * self.kv_elem_bytes + (rows if self.kv_dtype == "fp8s" else 0)


PRESETS: Dict[str, LMConfig] = {
    "dmcp-coder-1b": LMConfig(),
    "dmcp-coder-3b": LMConfig(name="dmcp-coder-3b", hidden=3072, layers=28, n_heads=24, n_kv_heads=8,
                              head_dim=128, intermediate=8192),
    # Llama-3.2-1B geometry with a production-size code vocabulary: 128,256
    # ids (128,000 byte-level BPE pieces trained on source code, ~4 bytes per
    # token, + the 256-id special block; scripts/train_code_bpe.py).  No
    # checkpoint exists on this host, so weights are random: this preset pins
    # the OPERATING POINT of a real 1B code model -- LM head of 263 M params
    # (a fifth of the weight bytes per decode step), prompts and replies 3-4x
    # fewer tokens than the byte preset's -- not its reply quality.
    "llama3.2-1b-code": LMConfig(name="llama3.2-1b-code", vocab_size=128256, hidden=2048, layers=16, n_heads=32,
                                 n_kv_heads=8, head_dim=64, intermediate=8192, rope_theta=500000.0,
                                 tokenizer="code-bpe-128k"),
    "tiny": LMConfig(name="tiny", hidden=256, layers=2, n_heads=4, n_kv_heads=2, head_dim=64,
                     intermediate=512, max_seq=1024, max_batch=8, max_rows=64),
    # the tiny model over the code BPE vocabulary (CPU tests of the 128k-id path)
    "tiny-bpe": LMConfig(name="tiny-bpe", vocab_size=128256, hidden=256, layers=2, n_heads=4, n_kv_heads=2,
                         head_dim=64, intermediate=512, max_seq=1024, max_batch=8, max_rows=64,
                         tokenizer="code-bpe-128k"),
}


def fused_shapes_ok(c: LMConfig) -> bool:
    """The fused decode GEMMs' shape contract (``dmcp.ops.hip._fused_xw`` and
    the ``fused_*`` wrappers): every reduction depth a multiple of 32 (hidden
    for QKV / gate-up / LM head, heads x head_dim for O, intermediate for
    down), head_dim a multiple of 32 (RoPE epilogue), and the residual / LM
    head widths multiples of 16.  A checkpoint outside it (vocab 32001,
    50257, ...) keeps every decode step on the hipBLASLt path."""
    return (c.hidden % 32 == 0 and (c.n_heads * c.head_dim) % 32 == 0 and c.intermediate % 32 == 0
            and c.head_dim % 32 == 0 and c.vocab_size % 16 == 0 and c.hidden % 16 == 0)


def tgemm_shapes_ok(c: LMConfig) -> bool:
    """The large-tile GEMM's contract (csrc/tgemm.hip) for every decode
    projection: output widths (QKV, hidden, 2 x intermediate) multiples of
    256, reduction depths multiples of 64, plus the fused reductions' <= 8192."""
    return (c.qkv_dim % 256 == 0 and c.hidden % 256 == 0 and (2 * c.intermediate) % 256 == 0
            and c.hidden % 64 == 0 and (c.n_heads * c.head_dim) % 64 == 0 and c.intermediate % 64 == 0
            and c.qkv_dim <= 8192 and c.hidden <= 8192 and c.head_dim % 16 == 0)


def wgemm_shapes_ok(c: LMConfig) -> bool:
    """The weight-streaming GEMMs' contract (csrc/wgemm.hip): reduction
    depths (hidden, heads x head_dim, intermediate) multiples of 64, output
    widths (QKV, hidden) multiples of 64 and <= 8192 (the fused row
    reductions), the gate/up halves multiples of 64."""
    return (c.hidden % 64 == 0 and (c.n_heads * c.head_dim) % 64 == 0 and c.intermediate % 64 == 0
            and c.qkv_dim % 64 == 0 and c.qkv_dim <= 8192 and c.hidden <= 8192 and c.head_dim % 16 == 0)


# The MXFP8 prefill's numerics gate on a checkpoint: last-position logit
# cosine against the fp32 reference model and top-1 agreement, measured on
# trained-like weights of Llama-3.2-1B geometry (heavy-tailed matrices,
# non-trivial norms, 100x residual outlier channels, an embedding that does
# not dominate the residual stream: dmcp.utils.synth.llama_checkpoint).
# Round 6 measured cosine 0.89-0.93 and top-1 3 / 12 there -- e4m3's ~3.6 %
# rms rounding of every weight and activation compounds over 16 layers once
# the layers, not the embedding, carry the logits (random-init presets pass
# at 0.999 only because their std-1 embedding dominates) -- so a loaded
# checkpoint keeps the bf16 prefill (MXFP8_CHECKPOINT_OK, asserted against a
# fresh measurement by
# tests/test_gpu_checkpoint_full.py::test_full_checkpoint_mxfp8_prefill_gate)
MXFP8_CHECKPOINT_GATE = {"cosine": 0.995, "top1": 0.75}
MXFP8_CHECKPOINT_OK = False


class CheckpointUnsupported(ValueError):
    """A checkpoint directory this loader cannot reproduce faithfully
    (:func:`check_checkpoint` gives the reason)."""


SUPPORTED_MODEL_TYPES = ("llama", "qwen2", "qwen3", "qwen3_moe", "mistral", "glm4_moe")
SUPPORTED_ARCHITECTURES = ("LlamaForCausalLM", "Qwen2ForCausalLM", "Qwen3ForCausalLM", "Qwen3MoeForCausalLM",
                           "MistralForCausalLM", "Glm4MoeForCausalLM")
MOE_ARCHITECTURE = "Qwen3MoeForCausalLM"
GLM_MOE_ARCHITECTURE = "Glm4MoeForCausalLM"
MISTRAL_ARCHITECTURE = "MistralForCausalLM"
_LAYER_TYPES = ("full_attention", "sliding_attention")
_DENSE_MLP = ("mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
_EXPERT_PROJS = ("gate_proj", "up_proj", "down_proj")


def _positive_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and v > 0


def checkpoint_windows(hf: dict) -> Tuple[Optional[tuple], Optional[str]]:
    """(one sliding window per layer -- 0 = full attention -- or None when no
    layer has one, None) of a config.json, or (None, reason) naming the key.

    * ``layer_types``, when present, decides per layer: ``sliding_attention``
      takes ``sliding_window``, ``full_attention`` none;
    * else ``model_type`` "mistral": a positive-integer ``sliding_window``
      applies to every layer (null / absent: none);
    * else (qwen2 / qwen3 / qwen3_moe) ``use_sliding_window`` true: the layers
      ``i >= max_window_layers`` take ``sliding_window``."""
    n = hf["num_hidden_layers"]
    sw = hf.get("sliding_window")
    lt = hf.get("layer_types")
    mt = hf.get("model_type")
    if hf.get("use_sliding_window"):  # whatever decides the layers, the switch needs a window to switch on
        if mt not in ("qwen2", "qwen3", "qwen3_moe"):
            return None, (f"use_sliding_window true is not supported for model_type {mt!r} "
                          f"(qwen2 / qwen3 / qwen3_moe read it)")
        if not _positive_int(sw):
            return None, (f"use_sliding_window is true but sliding_window is {sw!r} (a positive integer is "
                          f"needed)")
    if lt:
        other = sorted({str(t) for t in lt if t not in _LAYER_TYPES})
        if other:
            return None, (f"layer_types contains {', '.join(other)} (supported: {', '.join(_LAYER_TYPES)})")
        if len(lt) != n:
            return None, f"layer_types has {len(lt)} entries, num_hidden_layers is {n}"
        if "sliding_attention" not in lt:
            return None, None
        if not _positive_int(sw):
            return None, (f"layer_types contains sliding_attention but sliding_window is {sw!r} "
                          f"(a positive integer is needed)")
        return tuple(sw if t == "sliding_attention" else 0 for t in lt), None
    if mt == "mistral":
        if sw is None:
            return None, None
        if not _positive_int(sw):
            return None, f"sliding_window is {sw!r} (a positive integer or null is needed)"
        return (sw,) * n, None
    if hf.get("use_sliding_window"):
        mwl = hf.get("max_window_layers", n)
        if not isinstance(mwl, int) or isinstance(mwl, bool) or mwl < 0:
            return None, f"use_sliding_window is true but max_window_layers is {mwl!r} (an integer >= 0 is needed)"
        wins = tuple(sw if i >= mwl else 0 for i in range(n))
        return (wins if any(wins) else None), None
    return None, None


def resolve_windows(windows: Optional[tuple], max_seq: int) -> Optional[tuple]:
    """``windows`` as the model runs them in slots of ``max_seq`` positions: a
    window that no sequence can outgrow is 0 (today's kernels, untouched);
    None when no layer is left with one."""
    if not windows:
        return None
    out = tuple(0 if w >= max_seq else int(w) for w in windows)
    return out if any(out) else None


def windows_label(windows: Optional[tuple]) -> str:
    """The resolved windows for logs and the worker witness: "none",
    "4096@all", "4096@28.." (from layer 28 on) or "4096@0,2,4"."""
    if not windows or not any(windows):
        return "none"
    parts = []
    for w in sorted({w for w in windows if w}):
        idx = [i for i, x in enumerate(windows) if x == w]
        if len(idx) == len(windows):
            where = "all"
        elif idx == list(range(idx[0], len(windows))):
            where = f"{idx[0]}.."
        else:
            where = ",".join(str(i) for i in idx)
        parts.append(f"{w}@{where}")
    return "+".join(parts)


def _moe_config(hf: dict) -> Tuple[Optional[tuple], Optional[str]]:
    """((n_experts, experts_per_tok, moe_intermediate, norm_topk), None) of a
    ``qwen3_moe`` config.json, or (None, reason) naming the key."""
    ne = hf.get("num_experts", hf.get("num_local_experts"))
    if not isinstance(ne, int) or ne <= 0:
        return None, "model_type 'qwen3_moe' needs num_experts (or num_local_experts) in config.json"
    k, inter = hf.get("num_experts_per_tok"), hf.get("moe_intermediate_size")
    if not isinstance(k, int) or k <= 0:
        return None, "config.json: num_experts_per_tok is missing or not a positive integer"
    if not isinstance(inter, int) or inter <= 0:
        return None, "config.json: moe_intermediate_size is missing or not a positive integer"
    if k > ne:
        return None, f"num_experts_per_tok {k} exceeds num_experts {ne}"
    if hf.get("mlp_only_layers"):
        return None, (f"mlp_only_layers {hf['mlp_only_layers']!r} is not supported (every layer's MLP must be "
                      f"the routed one)")
    if hf.get("decoder_sparse_step", 1) != 1:
        return None, f"decoder_sparse_step {hf['decoder_sparse_step']!r} is not supported (only 1: every layer sparse)"
    if not ops.moe_supported(hf["hidden_size"], inter, ne, k):
        return None, (f"hidden_size {hf['hidden_size']} / moe_intermediate_size {inter} / num_experts {ne} / "
                      f"num_experts_per_tok {k} are outside the routed MLP kernels' contract (hidden and "
                      f"intermediate multiples of 64, hidden <= 8192, at most 256 experts)")
    return (ne, k, inter, bool(hf.get("norm_topk_prob", False))), None


def _partial_rotary(hf: dict, head_dim: int) -> Tuple[Optional[int], Optional[str]]:
    """(LMConfig.rotary_dim, None) of a ``glm4_moe`` config.json --
    ``partial_rotary_factor`` at the top level or inside ``rope_parameters`` /
    ``rope_scaling``; 0 for the whole head -- or (None, reason).  A config
    without the key has the factor 0.5, as the checkpoint's own code assumes."""
    f = hf.get("partial_rotary_factor")
    for key in ("rope_parameters", "rope_scaling"):
        d = hf.get(key)
        if f is None and isinstance(d, dict):
            f = d.get("partial_rotary_factor")
    if f is None:
        f = 0.5
    if isinstance(f, bool) or not isinstance(f, (int, float)) or not math.isfinite(f):
        return None, f"partial_rotary_factor {f!r} is not a number"
    R = int(head_dim * f)
    if not 0 < R <= head_dim or R % 2:
        return None, (f"partial_rotary_factor {f!r} gives a rotary width of {R} for head_dim {head_dim} (it must "
                      f"be even and in (0, head_dim])")
    return (0 if R == head_dim else R), None


def _glm_moe_config(hf: dict) -> Tuple[Optional[dict], Optional[str]]:
    """The routed-MLP keys of a ``glm4_moe`` config.json as LMConfig fields
    (n_experts, experts_per_tok, moe_intermediate, norm_topk, moe_score,
    moe_route_scale, moe_shared, dense_lead) plus ``qk_norm`` and ``mtp`` (the
    appended multi-token-prediction layers, which are not loaded), or (None,
    reason) naming the key.  Absent keys take the values the checkpoint's own
    code gives them."""
    ne = hf.get("n_routed_experts", hf.get("num_experts", hf.get("num_local_experts")))
    if isinstance(ne, bool) or not isinstance(ne, int) or ne <= 0:
        return None, "model_type 'glm4_moe' needs n_routed_experts (a positive integer) in config.json"
    k, inter = hf.get("num_experts_per_tok"), hf.get("moe_intermediate_size")
    if isinstance(k, bool) or not isinstance(k, int) or k <= 0:
        return None, "config.json: num_experts_per_tok is missing or not a positive integer"
    if isinstance(inter, bool) or not isinstance(inter, int) or inter <= 0:
        return None, "config.json: moe_intermediate_size is missing or not a positive integer"
    if k > ne:
        return None, f"num_experts_per_tok {k} exceeds n_routed_experts {ne}"
    for key in ("n_group", "topk_group"):
        if hf.get(key, 1) not in (1, None):
            return None, (f"{key} {hf[key]!r} is not supported (only 1: group-limited routing is not implemented)")
    S = hf.get("n_shared_experts", 1)
    S = 0 if S is None else S
    if isinstance(S, bool) or not isinstance(S, int) or S < 0:
        return None, f"n_shared_experts {S!r} is not an integer >= 0"
    layers = hf["num_hidden_layers"]
    lead = hf.get("first_k_dense_replace", 1)
    if isinstance(lead, bool) or not isinstance(lead, int) or not 0 <= lead <= layers:
        return None, f"first_k_dense_replace {lead!r} is outside [0, num_hidden_layers {layers}]"
    scale = hf.get("routed_scaling_factor", 1.0)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not (math.isfinite(scale) and scale > 0):
        return None, f"routed_scaling_factor {scale!r} is not a finite number > 0"
    mtp = hf.get("num_nextn_predict_layers", 0)
    mtp = 0 if mtp is None else mtp
    if isinstance(mtp, bool) or not isinstance(mtp, int) or mtp < 0:
        return None, f"num_nextn_predict_layers {mtp!r} is not an integer >= 0"
    if hf.get("quantization_config") is not None:
        return None, ("quantization_config is not supported for model_type 'glm4_moe' (the e4m3 expert GEMMs do not "
                      "run under the sigmoid router with shared experts yet; load the bf16 checkpoint)")
    if not ops.moe_sh_supported(hf["hidden_size"], inter, ne, k, S):
        return None, (f"hidden_size {hf['hidden_size']} / moe_intermediate_size {inter} / n_routed_experts {ne} / "
                      f"num_experts_per_tok {k} / n_shared_experts {S} are outside the routed MLP kernels' contract "
                      f"(hidden and intermediate multiples of 64, hidden <= 8192, routed + shared experts <= 256, "
                      f"at most 64 shared)")
    return dict(n_experts=ne, experts_per_tok=k, moe_intermediate=inter, norm_topk=bool(hf.get("norm_topk_prob", True)),
                moe_score="sigmoid", moe_route_scale=float(scale), moe_shared=S, dense_lead=lead,
                qk_norm=bool(hf.get("use_qk_norm", False)), mtp=mtp), None


_GLM_SHARED = ("mlp.shared_experts.gate_proj.weight", "mlp.shared_experts.up_proj.weight",
               "mlp.shared_experts.down_proj.weight")
_GLM_ROUTER_BIAS = "mlp.gate.e_score_correction_bias"


# Block-scaled FP8 checkpoints (quantization_config.quant_method "fp8"): the
# projections that may be stored as F8_E4M3 with an F32 ``weight_scale_inv``
# sibling of shape [ceil(N / 128), ceil(K / 128)].  Everything else -- embeddings,
# lm_head, norms, biases, the router mlp.gate.weight -- must stay unquantised.
FP8_BLOCK = 128
_FP8_PROJ_SUFFIXES = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                      "self_attn.o_proj.weight", "gate_proj.weight", "up_proj.weight", "down_proj.weight")
_SCALE_SUFFIX = "_scale_inv"


def _fp8_config(hf: dict) -> Tuple[bool, Optional[str]]:
    """(the checkpoint declares the block-scaled FP8 layout, None), or
    (False, reason) naming the ``quantization_config`` key that is refused."""
    qc = hf.get("quantization_config")
    if qc is None:
        return False, None
    if not isinstance(qc, dict):
        return False, "quantization_config is not an object"
    method = qc.get("quant_method")
    if method != "fp8":
        return False, (f"quantization_config.quant_method {method!r} is not supported (only 'fp8' with "
                       f"weight_block_size [128, 128])")
    fmt = qc.get("fmt", "e4m3")
    if fmt != "e4m3":
        return False, f"quantization_config.fmt {fmt!r} is not supported (only 'e4m3')"
    wbs = qc.get("weight_block_size")
    if wbs is None or list(wbs) != [FP8_BLOCK, FP8_BLOCK]:
        return False, (f"quantization_config.weight_block_size {wbs!r} is not supported (only [128, 128]: "
                       f"per-tensor FP8 with weight_scale / input_scale is not loaded)")
    scheme = qc.get("activation_scheme", "dynamic")
    if scheme != "dynamic":
        return False, (f"quantization_config.activation_scheme {scheme!r} is not supported (only 'dynamic': "
                       f"there are no stored activation scales to apply; activations stay bf16)")
    return True, None


def _checkpoint_headers(path: str) -> Dict[str, tuple]:
    """name -> (safetensors dtype string, shape) of every tensor (headers only)."""
    from safetensors import safe_open
    heads: Dict[str, tuple] = {}
    for fn in sorted(os.listdir(path)):
        if fn.endswith(".safetensors"):
            with safe_open(os.path.join(path, fn), framework="pt") as f:
                for k in f.keys():
                    sl = f.get_slice(k)
                    heads[k] = (str(sl.get_dtype()), tuple(sl.get_shape()))
    return heads


def _fp8_tensor_problem(heads: Dict[str, tuple], fp8: bool) -> Optional[str]:
    """The first tensor that breaks the block-scaled FP8 layout, decided per
    tensor from the headers: an F8_E4M3 projection weight needs its F32
    ``weight_scale_inv`` of the ceil-divided shape, any other weight must
    have none, and nothing but a projection may be F8."""
    for n in sorted(heads):
        dt, shape = heads[n]
        if n.endswith(".weight" + _SCALE_SUFFIX):
            base = n[:-len(_SCALE_SUFFIX)]
            if base not in heads or not heads[base][0].startswith("F8"):
                return f"tensor {n} has no F8_E4M3 tensor {base} to scale"
            continue
        if n.endswith((".weight_scale", ".input_scale")):
            return (f"tensor {n} is not supported (per-tensor FP8 scales; only the block-scaled layout with "
                    f"weight_scale_inv is loaded)")
        if not dt.startswith("F8"):
            continue
        if dt != "F8_E4M3":
            return f"tensor {n} has dtype {dt} (only F8_E4M3 is supported)"
        if not fp8:
            return f"tensor {n} is F8_E4M3 but config.json has no quantization_config"
        if not (n.startswith("model.layers.") and n.endswith(_FP8_PROJ_SUFFIXES)):
            return (f"tensor {n} must not be F8_E4M3 (only the q/k/v/o, dense-MLP and expert projections may be "
                    f"quantised)")
        sn = n + _SCALE_SUFFIX
        if sn not in heads:
            return f"tensor {sn} is missing (the scales of the F8_E4M3 tensor {n})"
        want = tuple(-(-d // FP8_BLOCK) for d in shape)
        if heads[sn][0] != "F32":
            return f"tensor {sn} has dtype {heads[sn][0]}, expected F32"
        if len(shape) != 2 or heads[sn][1] != want:
            return (f"tensor {sn} has shape {list(heads[sn][1])}, expected {list(want)} (one scale per 128 x 128 "
                    f"block of {list(shape)})")
    return None


_LAYER_TENSORS = ("input_layernorm.weight", "post_attention_layernorm.weight", "self_attn.q_proj.weight",
                  "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                  "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
_QKV_BIASES = ("self_attn.q_proj.bias", "self_attn.k_proj.bias", "self_attn.v_proj.bias")
# Qwen3: RMSNorm over each q head and each k head (weight [head_dim]) between
# the projection and RoPE
_QK_NORMS = ("self_attn.q_norm.weight", "self_attn.k_norm.weight")
QK_NORM_HEAD_DIMS = (64, 128)  # what the QK-norm kernels (and the attention kernels) take


def _checkpoint_rope(hf: dict) -> Tuple[float, Optional[tuple]]:
    """(theta, LMConfig.rope_scaling) of a config.json: ``rope_scaling`` keyed
    by ``rope_type`` or the legacy ``type``, or the newer ``rope_parameters``
    dict, which may carry ``rope_theta`` too.  ValueError on an unsupported type."""
    params = hf.get("rope_parameters") or {}
    scaling = hf.get("rope_scaling") or params
    theta = hf.get("rope_theta", params.get("rope_theta", 10000.0))
    return float(theta), ops.reference.rope_scaling_key(scaling)


def _checkpoint_tensor_shapes(path: str, suffixes: tuple) -> Dict[str, tuple]:
    """Shapes of the tensors whose names end in ``suffixes`` (headers only)."""
    from safetensors import safe_open
    shapes: Dict[str, tuple] = {}
    for fn in sorted(os.listdir(path)):
        if fn.endswith(".safetensors"):
            with safe_open(os.path.join(path, fn), framework="pt") as f:
                for k in f.keys():
                    if k.endswith(suffixes):
                        shapes[k] = tuple(f.get_slice(k).get_shape())
    return shapes


class _LazyTensors:
    """name -> tensor over the mapped *.safetensors files of a directory: each
    lookup reads that tensor alone (safe_open), nothing is kept.  A context
    manager: leaving it closes the files and drops their mappings."""

    def __init__(self, files: Sequence[str]) -> None:
        from contextlib import ExitStack
        from safetensors import safe_open
        self._stack = ExitStack()
        try:
            handles = [self._stack.enter_context(safe_open(f, framework="pt")) for f in files]
        except BaseException:
            self._stack.close()
            raise
        self._where = {k: h for h in handles for k in h.keys()}

    def __enter__(self) -> "_LazyTensors":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def close(self) -> None:
        self._where = {}
        self._stack.close()

    def __contains__(self, name: str) -> bool:
        return name in self._where

    def __getitem__(self, name: str) -> torch.Tensor:
        return self._where[name].get_tensor(name)


def check_checkpoint(path: str, chat_template: Optional[str] = "auto") -> Optional[str]:
    """Why the checkpoint directory ``path`` cannot be loaded as the model it
    is -- naming the config key or tensor -- or None when
    :meth:`LocalLM.load_safetensors` reproduces it.  Reads ``config.json`` and
    the safetensors headers only: no tensor data, no device.

    ``chat_template``: the ``LOCAL_LLM_CHAT_TEMPLATE`` knob.  The chat
    template it selects (:mod:`dmcp.enrich.chat`) is compiled and rendered
    once; one that cannot be used is a reason too.  None: the model only."""
    cfg_path = os.path.join(path, "config.json")
    try:
        with open(cfg_path) as f:
            hf = json.load(f)
    except (OSError, ValueError) as e:
        return f"config.json of {path} cannot be read ({e})"
    mt = hf.get("model_type")
    archs = hf.get("architectures") or []
    if mt is not None and mt not in SUPPORTED_MODEL_TYPES:
        return f"model_type {mt!r} is not supported (supported: {', '.join(SUPPORTED_MODEL_TYPES)})"
    # a config naming neither is taken as the Llama layout (the tensor names below still have to match)
    if any(a not in SUPPORTED_ARCHITECTURES for a in archs):
        return f"architectures {archs!r} is not supported (supported: {', '.join(SUPPORTED_ARCHITECTURES)})"
    for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size"):
        if not isinstance(hf.get(k), int) or hf[k] <= 0:
            return f"config.json: {k} is missing or not a positive integer"
    act = hf.get("hidden_act", "silu")
    if act != "silu":
        return f"hidden_act {act!r} is not supported (the MLP kernels compute SwiGLU with silu)"
    if hf.get("mlp_bias"):
        return "mlp_bias true is not supported (the MLP projections take no bias)"
    if archs and (MISTRAL_ARCHITECTURE in archs) != (mt == "mistral") or (mt == "mistral" and len(archs) > 1):
        if mt == "mistral":
            return f"model_type 'mistral' does not match architectures {archs!r} (expected [{MISTRAL_ARCHITECTURE!r}])"
        return f"architectures {archs!r} does not match model_type {mt!r}"
    _, why = checkpoint_windows(hf)
    if why is not None:
        return why
    heads = hf["num_attention_heads"]
    kvh = hf.get("num_key_value_heads", heads)
    if not isinstance(kvh, int) or kvh <= 0 or heads % kvh:
        return f"num_attention_heads {heads} is not a multiple of num_key_value_heads {kvh}"
    moe = glm = None
    if mt == "qwen3_moe":
        moe, why = _moe_config(hf)
        if moe is None:
            return why
    if mt == "glm4_moe":
        glm, why = _glm_moe_config(hf)
        if glm is None:
            return why
        moe = (glm["n_experts"], glm["experts_per_tok"], glm["moe_intermediate"], glm["norm_topk"])
    if archs and ((MOE_ARCHITECTURE in archs) != (mt == "qwen3_moe")
                  or (GLM_MOE_ARCHITECTURE in archs) != (glm is not None)):
        return f"architectures {archs!r} does not match model_type {mt!r}"
    qk_norm = mt in ("qwen3", "qwen3_moe") or bool(glm and glm["qk_norm"])
    head_dim = hf.get("head_dim") or hf["hidden_size"] // heads
    if qk_norm and head_dim not in QK_NORM_HEAD_DIMS:
        return f"head_dim {head_dim} is not supported with q_norm / k_norm (supported: 64, 128)"
    if glm is not None:
        _, why = _partial_rotary(hf, head_dim)
        if why is not None:
            return why
    try:
        _checkpoint_rope(hf)
    except (ValueError, TypeError) as e:
        return f"rope_scaling: {e}"
    fp8, why = _fp8_config(hf)
    if why is not None:
        return why
    try:
        heads = _checkpoint_headers(path)
    except Exception as e:  # noqa: BLE001 -- a truncated or foreign file: refuse with its error
        return f"safetensors of {path} cannot be read ({e})"
    if not heads:
        return f"{path} holds no *.safetensors file"
    why = _fp8_tensor_problem(heads, fp8)
    if why is not None:
        return why
    # the scales are consumed with their tensors (checked above)
    names = [n for n in heads if not n.endswith(".weight" + _SCALE_SUFFIX)]
    layers = hf["num_hidden_layers"]
    lead = glm["dense_lead"] if glm else 0
    if glm and glm["mtp"]:
        # the multi-token-prediction layers the hub files carry after the last
        # decoder layer are not part of the model, and only those are skipped
        mtp = tuple(f"model.layers.{i}." for i in range(layers, layers + glm["mtp"]))
        names = [n for n in names if not n.startswith(mtp)]
    consumed = {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
    required = {"model.embed_tokens.weight", "model.norm.weight"}
    for i in range(layers):
        p = f"model.layers.{i}."
        sparse = moe is not None and i >= lead
        required.update(p + n for n in _LAYER_TENSORS if not sparse or n not in _DENSE_MLP)
        if sparse:
            required.add(p + "mlp.gate.weight")
            required.update(f"{p}mlp.experts.{e}.{n}.weight" for e in range(moe[0]) for n in _EXPERT_PROJS)
            if glm:
                required.add(p + _GLM_ROUTER_BIAS)
                if glm["moe_shared"]:
                    required.update(p + n for n in _GLM_SHARED)
        consumed.update(p + n for n in _QKV_BIASES)
        if qk_norm:
            required.update(p + n for n in _QK_NORMS)
    consumed |= required
    have = set(names)
    for n in names:  # the first tensor the loader would drop
        if n in consumed or n.endswith("rotary_emb.inv_freq"):
            continue
        if n.endswith((".o_proj.bias", ".gate_proj.bias", ".up_proj.bias", ".down_proj.bias")):
            return f"tensor {n} is not supported (only the q/k/v projections take a bias)"
        if "shared_expert" in n and glm is not None:
            return (f"tensor {n} is not supported (n_shared_experts is {glm['moe_shared']}: shared expert tensors "
                    f"belong to the sparse layers of a checkpoint with n_shared_experts > 0)")
        if "shared_expert" in n:
            return f"tensor {n} is not supported (shared experts: only Qwen3-MoE's routed experts are loaded)"
        return f"tensor {n} is not consumed by the loader (a layout other than Llama / Qwen2 / Qwen3)"
    missing = sorted(required - have)
    if missing:
        return f"tensor {missing[0]} is missing"
    for i in range(layers):
        p = f"model.layers.{i}."
        nb = sum((p + n) in have for n in _QKV_BIASES)
        if nb not in (0, 3):
            return f"layer {i} has {nb} of the 3 q/k/v bias tensors ({p}self_attn.*_proj.bias)"
        if hf.get("attention_bias") is False and nb:
            return f"attention_bias is false but {p}self_attn.q_proj.bias exists"
    if qk_norm:
        try:
            shapes = _checkpoint_tensor_shapes(path, _QK_NORMS)
        except Exception as e:  # noqa: BLE001
            return f"safetensors of {path} cannot be read ({e})"
        for n in sorted(shapes):
            if shapes[n] != (head_dim,):
                return f"tensor {n} has shape {list(shapes[n])}, expected [{head_dim}] (head_dim)"
    if moe is not None:
        n_exp, _, inter, _ = moe
        hidden = hf["hidden_size"]
        want = {"mlp.gate.weight": ((n_exp, hidden), "num_experts, hidden_size"),
                "gate_proj.weight": ((inter, hidden), "moe_intermediate_size, hidden_size"),
                "up_proj.weight": ((inter, hidden), "moe_intermediate_size, hidden_size"),
                "down_proj.weight": ((hidden, inter), "hidden_size, moe_intermediate_size")}
        try:
            shapes = _checkpoint_tensor_shapes(path, tuple(want))
        except Exception as e:  # noqa: BLE001
            return f"safetensors of {path} cannot be read ({e})"
        inter_d = hf["intermediate_size"]
        dense = {"gate_proj.weight": ((inter_d, hidden), "intermediate_size, hidden_size"),
                 "up_proj.weight": ((inter_d, hidden), "intermediate_size, hidden_size"),
                 "down_proj.weight": ((hidden, inter_d), "hidden_size, intermediate_size")}
        S = glm["moe_shared"] if glm else 0
        shared = {"gate_proj.weight": ((S * inter, hidden), "n_shared_experts x moe_intermediate_size, hidden_size"),
                  "up_proj.weight": ((S * inter, hidden), "n_shared_experts x moe_intermediate_size, hidden_size"),
                  "down_proj.weight": ((hidden, S * inter), "hidden_size, n_shared_experts x moe_intermediate_size")}
        for n in sorted(shapes):
            if ".mlp." not in n or n not in consumed:
                continue
            table = want
            if ".mlp.shared_experts." in n:
                table = shared
            elif ".mlp.experts." not in n and not n.endswith("mlp.gate.weight"):
                table = dense  # a lead layer's dense MLP
            exp, keys = next(v for s, v in table.items() if n.endswith(s))
            if shapes[n] != exp:
                return f"tensor {n} has shape {list(shapes[n])}, expected {list(exp)} ({keys})"
        if glm:
            for i in range(lead, layers):
                n = f"model.layers.{i}.{_GLM_ROUTER_BIAS}"
                if heads[n][1] != (n_exp,):
                    return f"tensor {n} has shape {list(heads[n][1])}, expected [{n_exp}] (n_routed_experts)"
                if heads[n][0] not in ("F32", "BF16", "F16"):
                    return f"tensor {n} has dtype {heads[n][0]}, expected F32"
        # the experts are stored in one format: the stacked device tensors hold one
        f8 = [n for n in sorted(shapes) if ".mlp.experts." in n and heads[n][0] == "F8_E4M3"]
        plain = [n for n in sorted(shapes) if ".mlp.experts." in n and heads[n][0] != "F8_E4M3"]
        if f8 and plain:
            return (f"tensor {plain[0]} is {heads[plain[0]][0]} but {f8[0]} is F8_E4M3 (the experts must all be "
                    f"in one format)")
    if "lm_head.weight" not in have and hf.get("tie_word_embeddings") is False:
        return "tensor lm_head.weight is missing and tie_word_embeddings is false"
    if chat_template is not None:
        from ..enrich.chat import template_problem
        return template_problem(path, chat_template)
    return None


def preset(name: str, **overrides) -> LMConfig:
    if name not in PRESETS:
        raise ValueError(f"unknown model preset {name!r}; choose one of {sorted(PRESETS)}")
    return replace(PRESETS[name], **overrides) if overrides else PRESETS[name]


_LSE_IMPL: Dict[str, str] = {}


def _attn_lse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool, scale: float):
    """Fused attention returning (out [1, H, T, D], natural-log LSE [1, H, T]
    fp32); q/k/v with equal head counts.  Flash (aotriton on ROCm) first, the
    memory-efficient kernel if flash is unavailable."""
    T = q.shape[2]
    if not q.is_cuda:
        o, lse = torch.ops.aten._scaled_dot_product_flash_attention_for_cpu(q, k, v, 0.0, causal, scale=scale)[:2]
        return o, lse
    impl = _LSE_IMPL.get("cuda", "flash")
    if impl == "flash":
        try:
            r = torch.ops.aten._scaled_dot_product_flash_attention(q, k, v, 0.0, causal, False, scale=scale)
            return r[0], r[1][..., :T]
        except RuntimeError:
            _LSE_IMPL["cuda"] = "efficient"
    r = torch.ops.aten._scaled_dot_product_efficient_attention(q, k, v, None, True, 0.0, causal, scale=scale)
    return r[0], r[1][..., :T]


def _extend_attention(qh: torch.Tensor, k: torch.Tensor, v: torch.Tensor, start: int, scale: float) -> torch.Tensor:
    """Attention of T new queries (positions [start, start+T)) over the
    cached context [0, start) -- fully visible -- and the new keys -- causal --
    as two fused kernels merged by their log-sum-exp, instead of one kernel
    with a materialised [T, start+T] mask (the math path: ~30x slower for a
    4k-token README prefix).  qh [1, Hq, T, D]; k/v [1, Hkv, start+T, D]."""
    Hq, Hkv = qh.shape[1], k.shape[1]
    G = Hq // Hkv

    def heads(t):
        return t if G == 1 else t.repeat_interleave(G, dim=1)
    kc, vc = heads(k[:, :, :start]), heads(v[:, :, :start])
    kn, vn = heads(k[:, :, start:]), heads(v[:, :, start:])
    o1, l1 = _attn_lse(qh, kc, vc, False, scale)
    o2, l2 = _attn_lse(qh, kn, vn, True, scale)
    m = torch.maximum(l1, l2)
    w1 = torch.exp(l1 - m).unsqueeze(-1)
    w2 = torch.exp(l2 - m).unsqueeze(-1)
    return ((o1.float() * w1 + o2.float() * w2) / (w1 + w2)).to(qh.dtype)


def _kv_bf16(t: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A KV-cache view as bf16 (fp8 caches widened, per-row scaled ones with
    the same view of their exponent table; the SDPA fallback path)."""
    if scale is not None:
        return ops.reference.kv_decode_scaled(t, scale).to(torch.bfloat16)
    return ops.reference.kv_float(t).to(torch.bfloat16) if t.dtype == torch.uint8 else t


def _truncation(sample: Optional[tuple], truncate: Optional[tuple]) -> Optional[tuple]:
    """(top_k, top_p, min_p), validated, of a sampled selection with a filter
    on; None when the selection is greedy or every filter is off (those paths
    are the untruncated ones, unchanged)."""
    if truncate is None or sample is None or not sample[0] > 0:
        return None
    cut = truncation_args(*truncate)
    return None if cut == (0, 1.0, 0.0) else cut


class LocalLM:
    """Weights + KV cache + forward passes (prefill / extend / batched decode).

    ``shared_prefix``: one extra KV slot (``prefix_slot``) holds a prompt
    prefix common to every sequence of a batch (:meth:`set_prefix`); decode
    then attends to it through the MFMA shared-prefix kernel, reading each
    prefix key once per 32 queries instead of once per row, and prefill of a
    sequence starts after it (:meth:`fork_prefix`)."""

    def __init__(self, cfg: LMConfig, device: str = "cuda", seed: int = 0,
                 weights: Optional[Dict[str, torch.Tensor]] = None, shared_prefix: bool = True) -> None:
        if cfg.n_heads % cfg.n_kv_heads:
            raise ValueError("n_heads must be a multiple of n_kv_heads")
        if cfg.kv_dtype not in ops.reference.KV_FORMATS:
            raise ValueError(f"kv_dtype must be 'bf16', 'fp8' or 'fp8s', got {cfg.kv_dtype!r}")
        if cfg.prefill_dtype not in ("bf16", "fp8", "auto"):
            raise ValueError(f"prefill_dtype must be 'bf16', 'fp8' or 'auto', got {cfg.prefill_dtype!r}")
        for k in ("decode_dtype",):
            if getattr(cfg, k) not in ("bf16", "fp8"):
                raise ValueError(f"{k} must be 'bf16' or 'fp8', got {getattr(cfg, k)!r}")
        # the per-row scaled cache has no writer in the MXFP8 GEMM epilogues
        self.kv_scaled = cfg.kv_dtype == "fp8s"
        if self.kv_scaled and "fp8" in (cfg.prefill_dtype, cfg.decode_dtype):
            raise ValueError(f"kv_dtype 'fp8s' (LOCAL_LLM_KV_DTYPE) is not written by the MXFP8 GEMMs: use "
                             f"prefill_dtype / decode_dtype 'bf16' (LOCAL_LLM_PREFILL_DTYPE, "
                             f"LOCAL_LLM_DECODE_DTYPE), got prefill_dtype={cfg.prefill_dtype!r} "
                             f"decode_dtype={cfg.decode_dtype!r}")
        if self.kv_scaled and torch.device(device).type == "cuda" and cfg.head_dim not in ops.hip.KV_SCALE_DIMS:
            raise ValueError(f"{cfg.name}: kv_dtype 'fp8s' needs head_dim 64 or 128, got {cfg.head_dim}")
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = torch.bfloat16
        # the checkpoint directory the weights came from (load_safetensors);
        # None = random-initialised weights of a preset
        self.checkpoint: Optional[str] = None
        self.w = weights if weights is not None else self._init_weights(seed)
        # q/k/v projection biases (Qwen2 checkpoints): w["l{i}.bqkv"], bf16 [qkv_dim]
        self.has_bias = any(k.endswith(".bqkv") for k in self.w)
        if self.has_bias and "fp8" in (cfg.prefill_dtype, cfg.decode_dtype):
            raise ValueError(f"{cfg.name} has q/k/v projection biases, which the MXFP8 GEMMs do not apply: "
                             f"use prefill_dtype / decode_dtype 'bf16' (LOCAL_LLM_PREFILL_DTYPE, "
                             f"LOCAL_LLM_DECODE_DTYPE), got prefill_dtype={cfg.prefill_dtype!r} "
                             f"decode_dtype={cfg.decode_dtype!r}")
        # per-head q / k RMSNorm (Qwen3 checkpoints): w["l{i}.qnorm"] / w["l{i}.knorm"], bf16 [head_dim]
        self.has_qk_norm = any(k.endswith(".qnorm") for k in self.w)
        if self.has_qk_norm and "fp8" in (cfg.prefill_dtype, cfg.decode_dtype):
            raise ValueError(f"{cfg.name} has per-head q/k norms, which the MXFP8 GEMMs do not apply: "
                             f"use prefill_dtype / decode_dtype 'bf16' (LOCAL_LLM_PREFILL_DTYPE, "
                             f"LOCAL_LLM_DECODE_DTYPE), got prefill_dtype={cfg.prefill_dtype!r} "
                             f"decode_dtype={cfg.decode_dtype!r}")
        if self.has_qk_norm and cfg.head_dim not in QK_NORM_HEAD_DIMS:
            raise ValueError(f"{cfg.name}: per-head q/k norms need head_dim 64 or 128, got {cfg.head_dim}")
        # routed expert MLP (Qwen3-MoE): w["l{i}.router"] [E, H], w["l{i}.we_gu"] [E, 2I, H] (an expert's gate
        # rows, then its up rows), w["l{i}.we_down"] [E, H, I], all bf16
        # -- or, moe_weight_dtype "fp8b", w["l{i}.we_gu8"] / w["l{i}.we_down8"] in e4m3 with the block scales
        # w["l{i}.we_gu_s"] [E, 2 ceil(I / 128), ceil(H / 128)] / w["l{i}.we_down_s"] [E, ceil(H / 128), ceil(I / 128)]
        # -- under moe_score "sigmoid" (GLM-4.5) also w["l{i}.router_bias"] fp32 [E], and we_gu / we_down stack
        # E + moe_shared experts: the routed ones, then the shared MLP's slices (ops.reference.moe_stack_shared).
        # Layers below dense_lead hold the dense MLP's w["l{i}.wgu"] / w["l{i}.wdown"] instead
        self.moe = cfg.n_experts > 0
        if cfg.moe_score not in ("softmax", "sigmoid"):
            raise ValueError(f"moe_score must be 'softmax' or 'sigmoid', got {cfg.moe_score!r}")
        self.moe_sig = self.moe and cfg.moe_score == "sigmoid"
        if not self.moe_sig and (cfg.moe_shared or cfg.moe_route_scale != 1.0):
            raise ValueError(f"{cfg.name}: moe_shared {cfg.moe_shared} / moe_route_scale {cfg.moe_route_scale} need "
                             f"n_experts > 0 and moe_score 'sigmoid'")
        if (isinstance(cfg.moe_shared, bool) or not isinstance(cfg.moe_shared, int) or cfg.moe_shared < 0
                or not (math.isfinite(cfg.moe_route_scale) and cfg.moe_route_scale > 0)):
            raise ValueError(f"{cfg.name}: moe_shared must be an integer >= 0 and moe_route_scale finite and > 0, got "
                             f"{cfg.moe_shared!r} / {cfg.moe_route_scale!r}")
        if not isinstance(cfg.dense_lead, int) or not 0 <= cfg.dense_lead <= cfg.layers or (cfg.dense_lead
                                                                                              and not self.moe):
            raise ValueError(f"{cfg.name}: dense_lead {cfg.dense_lead!r} must be in [0, layers {cfg.layers}] and needs "
                             f"n_experts > 0")
        try:
            ops.reference.rotary_dim_arg(cfg.head_dim, cfg.rotary_dim)
        except ValueError as e:
            raise ValueError(f"{cfg.name}: {e}") from None
        if cfg.rotary_dim and "fp8" in (cfg.prefill_dtype, cfg.decode_dtype):
            raise ValueError(f"{cfg.name}: rotary_dim {cfg.rotary_dim} (partial rotary) is not applied by the MXFP8 "
                             f"GEMMs' weights: use prefill_dtype / decode_dtype 'bf16', got prefill_dtype="
                             f"{cfg.prefill_dtype!r} decode_dtype={cfg.decode_dtype!r}")
        if cfg.moe_weight_dtype not in ("bf16", "fp8b"):
            raise ValueError(f"moe_weight_dtype must be 'bf16' or 'fp8b', got {cfg.moe_weight_dtype!r}")
        self.moe_w8 = self.moe and cfg.moe_weight_dtype == "fp8b"
        if self.moe:
            if "fp8" in (cfg.prefill_dtype, cfg.decode_dtype):
                raise ValueError(f"{cfg.name} has a routed expert MLP, which has no MXFP8 GEMM: use "
                                 f"prefill_dtype / decode_dtype 'bf16' (LOCAL_LLM_PREFILL_DTYPE, "
                                 f"LOCAL_LLM_DECODE_DTYPE), got prefill_dtype={cfg.prefill_dtype!r} "
                                 f"decode_dtype={cfg.decode_dtype!r}")
            if not 1 <= cfg.experts_per_tok <= cfg.n_experts:
                raise ValueError(f"{cfg.name}: experts_per_tok {cfg.experts_per_tok} outside [1, n_experts "
                                 f"{cfg.n_experts}]")
            if torch.device(device).type == "cuda" and not (
                    ops.moe_sh_supported(cfg.hidden, cfg.moe_intermediate, cfg.n_experts, cfg.experts_per_tok,
                                         cfg.moe_shared) if self.moe_sig else
                    ops.moe_supported(cfg.hidden, cfg.moe_intermediate, cfg.n_experts, cfg.experts_per_tok)):
                raise ValueError(f"{cfg.name}: hidden {cfg.hidden} / moe_intermediate {cfg.moe_intermediate} / "
                                 f"n_experts {cfg.n_experts} / experts_per_tok {cfg.experts_per_tok}"
                                 + (f" / moe_shared {cfg.moe_shared}" if self.moe_sig else "") + " are outside "
                                 f"the routed MLP kernels' contract (ops.moe_supported"
                                 + (" / ops.moe_sh_supported)" if self.moe_sig else ")"))
            if self.moe_sig and self.moe_w8:
                raise ValueError(f"{cfg.name}: moe_weight_dtype 'fp8b' has no kernel under moe_score 'sigmoid'")
            s0 = cfg.dense_lead  # the first routed layer
            if s0 < cfg.layers:
                if f"l{s0}.router" not in self.w:
                    raise ValueError(f"{cfg.name}: n_experts {cfg.n_experts} but the weights hold no l{s0}.router")
                if (f"l{s0}.we_gu8" in self.w) != self.moe_w8:
                    raise ValueError(f"{cfg.name}: moe_weight_dtype {cfg.moe_weight_dtype!r} does not match the "
                                     f"weights ({f'l{s0}.we_gu8' if f'l{s0}.we_gu8' in self.w else f'l{s0}.we_gu'})")
                if self.moe_sig and f"l{s0}.router_bias" not in self.w:
                    raise ValueError(f"{cfg.name}: moe_score 'sigmoid' but the weights hold no l{s0}.router_bias")
        # sliding windows: _wkw(i) is layer i's extra attention keyword -- empty
        # for a full-attention layer, so such layers (and whole models) make
        # the calls they always made and never reach a windowed entry point
        lw = cfg.layer_windows
        if lw is not None:
            if len(lw) != cfg.layers or any(isinstance(w, bool) or not isinstance(w, int) or w < 0 for w in lw):
                raise ValueError(f"{cfg.name}: layer_windows must hold one integer >= 0 per layer "
                                 f"({cfg.layers}), got {lw!r}")
        self.windows = tuple(lw) if lw is not None and any(lw) else None
        self._fold_norms()
        c = cfg
        # the routed MLP's scratch, once, like attn_ws / wgemm_ws: decode steps
        # and prefill chunks of up to moe_rows rows (a longer prefill walks its
        # rows in chunks: _mlp_norm)
        self.moe_rows = self.moe_ws = None
        if self.moe:
            self.moe_rows = max(1, min(max(max(c.max_batch, c.max_rows), self.MOE_PREFILL_ROWS),
                                       ops.MOE_MAX_PAIRS // (c.experts_per_tok + c.moe_shared)))
            if torch.device(device).type == "cuda" and self.moe_sig:
                self.moe_ws = ops.moe_sh_workspace(self.moe_rows, c.hidden, c.moe_intermediate, c.n_experts,
                                                   c.experts_per_tok, c.moe_shared, self.device)
            elif torch.device(device).type == "cuda":
                self.moe_ws = ops.moe_workspace(self.moe_rows, c.hidden, c.moe_intermediate, c.n_experts,
                                                c.experts_per_tok, self.device)
        self.shared_prefix = shared_prefix
        self.num_slots = c.max_batch + (1 if shared_prefix else 0)
        self.prefix_slot = c.max_batch if shared_prefix else -1
        kv_shape = (c.layers, self.num_slots, c.n_kv_heads, c.max_seq, c.head_dim)
        # fp8: OCP e4m3fn bytes in uint8 tensors, written by the RoPE/KV-append
        # kernels and widened to bf16 inside every attention kernel
        self.kv_dtype = torch.uint8 if c.kv_dtype in ("fp8", "fp8s") else self.dtype
        self._check_kv_fits(kv_shape)
        self.k_cache = torch.zeros(kv_shape, dtype=self.kv_dtype, device=self.device)
        self.v_cache = torch.zeros(kv_shape, dtype=self.kv_dtype, device=self.device)
        # fp8s: one exponent byte per cached row beside the caches (127 = 2^0),
        # static buffers like them, so captured decode graphs are unaffected
        self.k_scale = self.v_scale = None
        if self.kv_scaled:
            self.k_scale = torch.full(kv_shape[:-1], 127, dtype=torch.uint8, device=self.device)
            self.v_scale = torch.full(kv_shape[:-1], 127, dtype=torch.uint8, device=self.device)
        # (a QK-norm model's table is built in fp32 like its own code's: ops.reference.rope_tables)
        self.cos_sin = ops.rope_tables(c.max_seq, c.head_dim, c.rope_theta, device=self.device,
                                       scaling=c.rope_scaling, fp32_angles=self.has_qk_norm,
                                       rotary_dim=c.rotary_dim).contiguous()
        self.scale = 1.0 / math.sqrt(c.head_dim)
        self.max_rows = max(c.max_batch, c.max_rows)
        # method branches: per slot (parent slot, end) -- the decode attention
        # reads a branch's keys below ``end`` from its class head's slot in
        # place (fork_share); end 0 = none.  Device-resident, so captured
        # decode graphs follow it.
        self.fork_tab = torch.zeros((self.num_slots, 2), dtype=torch.int32, device=self.device)
        self.fork_tab[:, 0] = torch.arange(self.num_slots, dtype=torch.int32, device=self.device)
        # fork-table rows set while fork_defer is on, applied by fork_flush()
        self.fork_defer = False
        self._fork_pending: Dict[int, Tuple[int, int]] = {}
        # shared prefix: its length in device memory, so captured decode
        # graphs follow it
        self.prefix_len = 0
        self.prefix_tokens: tuple = ()
        self.prefix_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        # fused decode GEMMs for steps of <= fused_max_rows rows (GPU only;
        # the attribute is cleared by tests to compare against hipBLASLt)
        # (a QK-norm model with q/k/v biases takes the weight-streaming path
        # at every row count: the two-launch small-row QKV has no bias input)
        # (an fp8s model likewise: the fused QKV tile holds 32 of a head's
        # columns, so it cannot take the head's amax -- without a bias its small
        # steps run the two-launch QKV, with one the weight-streaming path)
        two_launch = self.has_qk_norm or self.kv_scaled
        self.use_fused = (self.device.type == "cuda" and fused_shapes_ok(c)
                          and not (two_launch and self.has_bias))
        # prefill / extend attention on the MFMA kernel (csrc/prefill_attn.hip)
        self.use_prefill_kernel = (self.device.type == "cuda"
                                   and ops.prefill_supported(c.n_heads, c.n_kv_heads, c.head_dim))
        # slot -> shared-prefix length its prefill reads in place from the
        # prefix slot (fork_prefix without a copy; prefill kernel only)
        self._slot_prefix: Dict[int, int] = {}
        # crossover with the hipBLASLt + split-K-down path measured at ~20 rows
        # (fp8: fused 1.47 vs 1.64 ms at 16 rows, 1.80 vs 1.70 at 24, 1.82 vs
        # 1.73 at 32 -- profiles/decode_fused_rows_r2.txt)
        self.fused_max_rows = min(ops.FUSED_MAX_ROWS, 16)
        # QK-norm models: the small-row step's bf16 QKV row (fused_linear_norm
        # writes it, rope_kv normalises and rotates it), preallocated so a
        # captured step allocates nothing for it
        self.qkv_buf = (torch.empty((self.fused_max_rows, c.qkv_dim), dtype=self.dtype, device=self.device)
                        if two_launch and self.use_fused else None)
        ps = ops.PREFIX_MFMA_MAX_SPLITS if shared_prefix else 0
        self.attn_ws = (ops.decode_workspace(self.max_rows, c.n_heads, c.n_kv_heads, c.head_dim, c.max_seq,
                                             self.device, prefix_slots=ps) if self.device.type == "cuda" else None)
        # steps of fused_max_rows < rows <= WGEMM_MAX_ROWS: every projection on the
        # weight-streaming GEMM (csrc/wgemm.hip) with its neighbour op in the
        # epilogue / reduction -- QKV + RoPE + KV append, O + residual + norm,
        # gate/up + SwiGLU, down + residual + next norm
        self.use_wgemm = self.device.type == "cuda" and wgemm_shapes_ok(c)
        self.wgemm_ws = (ops.wgemm_workspace(min(self.max_rows, ops.WGEMM_MAX_ROWS), max(c.qkv_dim, c.hidden),
                                             self.device) if self.use_wgemm else None)
        # decode steps past fused_max_rows select their ids with the fused LM
        # head + masked argmax (csrc/wgemm.hip MODE_ARGMAX) instead of
        # F.linear + masked_argmax (at 128,256 ids: 1.6 ms + 0.36 ms per
        # 533-row step on hipBLASLt, profiles/kstats_llama_r4.txt)
        self.fused_head = self.device.type == "cuda" and ops.lm_head_supported(c.vocab_size, c.hidden)
        self.head_ws = ops.lm_head_workspace(c.vocab_size, self.device) if self.fused_head else None
        # the large-tile GEMM (csrc/tgemm.hip) with the same fused consumers:
        # every projection of steps of WGEMM_MAX_ROWS < rows <= TGEMM_MAX_ROWS
        # (the engine's jump-forward steps reach max_rows = 1.5 x max_batch),
        # gate/up + down from TGEMM_MLP_MIN_ROWS rows and the LM head + masked
        # argmax (V % 256 == 0) from TGEMM_HEAD_MIN_ROWS, where it beats the
        # weight-streaming kernel (profiles/tgemm_vs_wgemm_r5.jsonl) -- no
        # hipBLASLt GEMM in any decode step
        self.use_tgemm = (self.device.type == "cuda" and tgemm_shapes_ok(c) and self.max_rows <= ops.TGEMM_MAX_ROWS
                          and self.max_rows >= self.TGEMM_MLP_MIN_ROWS)
        self.tg_ws = (torch.empty(16 * self.max_rows * max(c.qkv_dim, c.hidden), dtype=torch.float32,
                                  device=self.device) if self.use_tgemm else None)
        self.tg_head = (self.fused_head and c.vocab_size % 256 == 0 and c.hidden % 64 == 0
                        and self.max_rows >= self.TGEMM_HEAD_MIN_ROWS and self.max_rows <= ops.TGEMM_MAX_ROWS)
        self.tg_head_ws = (torch.empty(2 * (c.vocab_size // 64) * self.max_rows, dtype=torch.float32,
                                       device=self.device) if self.tg_head else None)
        # the [max_rows, vocab] bf16 logits of steps that sample under a top-k /
        # top-p / min-p truncation (a truncation needs the whole row before the
        # draw, so those steps leave the fused head): allocated once, by
        # reserve_truncation_logits(), only when a filter is configured
        # (263 MB at 1,024 x 128,256)
        self.trunc_logits: Optional[torch.Tensor] = None
        self.history: Optional[torch.Tensor] = None  # reserve_history()
        # fp8 prefill: e4m3 copies of the four projections (per-row scales),
        # quantised once; the batched prefill then runs on csrc/pgemm.hip
        # (the CPU references take any dims the 32-element blocks divide)
        fp8_ok = c.n_heads * c.head_dim == c.hidden and (
            (self.use_prefill_kernel
             and ops.pgemm_supported(c.hidden, c.n_heads, c.n_kv_heads, c.head_dim, c.intermediate))
            or (self.device.type == "cpu" and c.hidden % 32 == 0 and c.intermediate % 32 == 0))
        self.prefill_fp8 = fp8_ok and (c.prefill_dtype == "fp8"
                                       or (c.prefill_dtype == "auto" and self.device.type == "cuda"
                                           and not self.has_bias and not self.has_qk_norm
                                           and not self.kv_scaled and not self.moe))
        self.decode_fp8 = c.decode_dtype == "fp8" and fp8_ok
        if "fp8" in (c.prefill_dtype, c.decode_dtype) and not fp8_ok:
            raise ValueError(f"fp8 GEMMs need head_dim 64, hidden % 2048 == 0 and a supported device "
                             f"({c.name}: hidden {c.hidden}, head_dim {c.head_dim}, {self.device})")
        # decode fp8: split-K partials of the MX decode GEMM (S x rows <= 2048 by wmx_plan)
        self.wmx_ws = None
        if self.decode_fp8 and self.device.type == "cuda":
            need = max(S * M * n for M in range(self.fused_max_rows + 1, min(self.max_rows, ops.WMX_MAX_ROWS) + 1)
                       for n, k in ((c.qkv_dim, c.hidden), (c.hidden, c.hidden), (c.hidden, c.intermediate))
                       for S in (ops.wmx_plan(M, n, k)[0],))
            self.wmx_ws = torch.empty(need, dtype=torch.float32, device=self.device)
        self.w8: Dict[str, tuple] = {}
        if self.prefill_fp8 or self.decode_fp8:
            for i in range(c.layers):
                for n in ("wqkv", "wo", "wgu", "wdown"):
                    self.w8[f"l{i}.{n}"] = ops.quantize_weight(self._unfolded(i, n))

    KV_HEADROOM = 4 << 30  # bytes left free next to the slab (graphs, workspaces, prefill activations)
    # row counts from which the large-tile kernel takes over from the
    # weight-streaming one: the LM head of 128,256 ids from 160 rows (134 vs
    # 150 us at 160 rows, 134 vs 130 at 80 -- profiles/tgemm_small_rows_r6.jsonl;
    # 155 vs 177 at 256, profiles/tgemm_vs_wgemm_r5.jsonl); the MLP only past 512 rows --
    # alone gate/up + SwiGLU and down + norm ran faster on it from 448 rows,
    # but the whole 512-row step was 3 % slower (same-box A/B,
    # profiles/decode_step_tgemm_ab_r5.jsonl)
    TGEMM_MLP_MIN_ROWS = 513
    TGEMM_HEAD_MIN_ROWS = 160
    # rows of a prefill per routed-MLP launch: bounds the workspace (at the
    # Qwen3-30B-A3B geometry 4,096 rows x 8 experts hold 50 MB of bf16 act and
    # 268 MB of fp32 down rows) while an expert still sees ~256 rows per launch
    MOE_PREFILL_ROWS = 4096

    def _check_kv_fits(self, kv_shape) -> None:
        """The KV slab is the largest allocation of the service (tens of GB at
        the default 512 slots); check it against the device's free HBM first,
        with a message naming the knobs, instead of an allocator OOM."""
        if self.device.type != "cuda":
            return
        need = 2 * math.prod(kv_shape) * self.cfg.kv_elem_bytes
        if self.cfg.kv_dtype == "fp8s":
            need += 2 * math.prod(kv_shape[:-1])  # the exponent tables
        free, total = torch.cuda.mem_get_info(self.device)
        if need + self.KV_HEADROOM > free:
            raise RuntimeError(
                f"KV cache of {need / 2**30:.1f} GiB ({self.num_slots} slots x {self.cfg.max_seq} positions, "
                f"{self.cfg.kv_dtype}) does not fit the {free / 2**30:.1f} GiB free of {total / 2**30:.1f} GiB on "
                f"{self.device} (+{self.KV_HEADROOM >> 30} GiB headroom): lower LOCAL_LLM_MAX_BATCH"
                + ("" if self.cfg.kv_dtype != "bf16" else
                   ", or use LOCAL_LLM_KV_DTYPE=fp8 (fp8s for a checkpoint with large K biases)"))

    # ------------------------------------------------------------ weights
    def _init_weights(self, seed: int) -> Dict[str, torch.Tensor]:
        c = self.cfg
        gen = torch.Generator(device=self.device)
        gen.manual_seed(seed)

        def rnd(*shape, std=0.02):
            t = torch.empty(shape, dtype=torch.float32, device=self.device)
            t.normal_(0.0, std, generator=gen)
            return t.to(self.dtype)

        def ones(n):
            return torch.ones(n, dtype=self.dtype, device=self.device)

        w: Dict[str, torch.Tensor] = {"embed": rnd(c.vocab_size, c.hidden, std=1.0),
                                      "norm_f": ones(c.hidden), "lm_head": rnd(c.vocab_size, c.hidden)}
        out_std = 0.02 / math.sqrt(2 * c.layers)
        for i in range(c.layers):
            w[f"l{i}.ln1"] = ones(c.hidden)
            w[f"l{i}.ln2"] = ones(c.hidden)
            w[f"l{i}.wqkv"] = rnd(c.qkv_dim, c.hidden)
            w[f"l{i}.wo"] = rnd(c.hidden, c.n_heads * c.head_dim, std=out_std)
            if c.sparse_layer(i):
                w[f"l{i}.router"] = rnd(c.n_experts, c.hidden)
                n_stack = c.n_experts + c.moe_shared  # the shared slices ride behind the routed experts
                gu = rnd(n_stack, 2 * c.moe_intermediate, c.hidden)
                down = rnd(n_stack, c.hidden, c.moe_intermediate, std=out_std)
                if c.moe_score == "sigmoid":  # a selection bias large enough to change selections
                    w[f"l{i}.router_bias"] = rnd(c.n_experts, std=0.25).float()
                if c.moe_weight_dtype == "fp8b":  # the same draws, quantised as a block-scaled checkpoint's are
                    inter = c.moe_intermediate
                    g8, gs = ops.block_fp8_quant(gu[:, :inter])
                    u8, us = ops.block_fp8_quant(gu[:, inter:])
                    w[f"l{i}.we_gu8"], w[f"l{i}.we_gu_s"] = torch.cat([g8, u8], 1), torch.cat([gs, us], 1)
                    w[f"l{i}.we_down8"], w[f"l{i}.we_down_s"] = ops.block_fp8_quant(down)
                    continue
                w[f"l{i}.we_gu"], w[f"l{i}.we_down"] = gu, down
                continue
            w[f"l{i}.wgu"] = rnd(2 * c.intermediate, c.hidden)
            w[f"l{i}.wdown"] = rnd(c.hidden, c.intermediate, std=out_std)
        return w

    @torch.no_grad()
    def _fold_norms(self) -> None:
        """W'[n, k] = W[n, k] * g[k] for each RMSNorm weight g and the matrix
        that consumes the normalised rows (ln1 -> wqkv, ln2 -> wgu, norm_f ->
        lm_head); g becomes 1.  The model is unchanged (rms(x) * g . W^T ==
        rms(x) . W'^T) and the fused GEMMs apply the norm as a per-row scale
        of the accumulator.  Idempotent; a no-op for random-init weights."""
        c = self.cfg
        pairs = [("norm_f", "lm_head")]
        for i in range(c.layers):
            pairs += [(f"l{i}.ln1", f"l{i}.wqkv")]
            if not c.sparse_layer(i):  # a routed MLP keeps ln2: the router and every expert read the normalised row
                pairs += [(f"l{i}.ln2", f"l{i}.wgu")]
        if not hasattr(self, "norm_g"):
            # the checkpoint's own norm weights: the MXFP8 paths normalise
            # with them BEFORE quantising (a folded weight leaves a trained
            # model's ~100x outlier channels undamped in the activation, and
            # one outlier sets the E8M0 scale of its whole 32-element block)
            self.norm_g: Dict[str, torch.Tensor] = {g_name: self.w[g_name] for g_name, _ in pairs}
        for g_name, w_name in pairs:
            g = self.w[g_name]
            if bool((g == 1).all()):
                continue
            w = self.w[w_name]
            self.w[w_name] = (w.float() * g.float()[None, :]).to(w.dtype).contiguous()
            self.w[g_name] = torch.ones_like(g)

    def _g(self, name: str) -> torch.Tensor:
        """The original (unfolded) RMSNorm weight ``name`` (MXFP8 paths)."""
        return self.norm_g.get(name, self.w[name])

    def _unfolded(self, i: int, n: str) -> torch.Tensor:
        """Layer i's matrix ``n`` without its folded norm weight (the MXFP8
        copies are quantised from it; their activations carry the norm)."""
        w = self.w[f"l{i}.{n}"]
        g_name = {"wqkv": f"l{i}.ln1", "wgu": f"l{i}.ln2"}.get(n)
        g = self.norm_g.get(g_name) if g_name else None
        if g is None or bool((g == 1).all()):
            return w
        gs = torch.where(g == 0, torch.ones_like(g), g).float()
        return (w.float() / gs[None, :]).to(w.dtype).contiguous()

    @classmethod
    def load_safetensors(cls, path: str, device: str = "cuda", **cfg_overrides) -> "LocalLM":
        """Loads a Llama-, Qwen2-, Qwen3-, Mistral- or GLM-4.5-format checkpoint
        directory (config.json + *.safetensors) as the model it is: RoPE scaling
        ("linear", "llama3"), q/k/v projection biases, per-head q/k RMSNorm,
        the routed expert MLPs (Qwen3-MoE's softmax router; GLM-4.5's sigmoid
        router with its selection bias, shared experts, leading dense layers
        and partial rotary embedding) included.  A block-scaled FP8 checkpoint keeps its experts
        in e4m3 (``moe_weight_dtype`` "fp8b") and has every other F8 projection
        dequantised to bf16 here.  A directory the loader cannot
        reproduce raises :class:`CheckpointUnsupported` with the reason
        (:func:`check_checkpoint`)."""
        from safetensors.torch import load_file
        reason = check_checkpoint(path, chat_template=None)  # the model alone: the tokenizer side is load_local_model's
        if reason is not None:
            raise CheckpointUnsupported(f"{path}: {reason}")
        with open(os.path.join(path, "config.json")) as f:
            hf = json.load(f)
        heads = hf["num_attention_heads"]
        theta, scaling = _checkpoint_rope(hf)
        cfg = LMConfig(name=os.path.basename(path.rstrip("/")), vocab_size=hf["vocab_size"],
                       hidden=hf["hidden_size"], layers=hf["num_hidden_layers"], n_heads=heads,
                       n_kv_heads=hf.get("num_key_value_heads", heads),
                       head_dim=hf.get("head_dim") or hf["hidden_size"] // heads,
                       intermediate=hf["intermediate_size"], rope_theta=theta,
                       eps=hf.get("rms_norm_eps", 1e-5), rope_scaling=scaling)
        moe = _moe_config(hf)[0] if hf.get("model_type") == "qwen3_moe" else None
        if moe is not None:
            cfg = replace(cfg, n_experts=moe[0], experts_per_tok=moe[1], moe_intermediate=moe[2], norm_topk=moe[3])
        glm = _glm_moe_config(hf)[0] if hf.get("model_type") == "glm4_moe" else None
        perm = None  # partial rotary: each q / k head's rows in the whole-head rotation's order
        if glm is not None:
            moe = (glm["n_experts"], glm["experts_per_tok"], glm["moe_intermediate"], glm["norm_topk"])
            cfg = replace(cfg, rotary_dim=_partial_rotary(hf, cfg.head_dim)[0],
                          **{k: v for k, v in glm.items() if k not in ("qk_norm", "mtp")})
            if cfg.rotary_dim:
                perm = ops.reference.partial_rotary_perm(cfg.head_dim, cfg.rotary_dim)
        qk_norm = hf.get("model_type") in ("qwen3", "qwen3_moe") or bool(glm and glm["qk_norm"])
        cfg = replace(cfg, **cfg_overrides)
        if "layer_windows" not in cfg_overrides:  # against the slots' capacity, overrides applied
            cfg = replace(cfg, layer_windows=resolve_windows(checkpoint_windows(hf)[0], cfg.max_seq))
        fp8 = _fp8_config(hf)[0]
        if cfg.prefill_dtype == "auto" and not MXFP8_CHECKPOINT_OK:
            # a real checkpoint keeps bf16 prefill GEMMs unless fp8 is asked
            # for by name: the MXFP8 prefill fails MXFP8_CHECKPOINT_GATE on
            # trained-like weights (docs/PARITY.md)
            cfg = replace(cfg, prefill_dtype="bf16")
        files = [os.path.join(path, fn) for fn in sorted(os.listdir(path)) if fn.endswith(".safetensors")]
        if moe is not None:
            # 58 GB of experts at the 30B-A3B geometry (29 GB block-scaled FP8):
            # tensors are read one at a time from the mapped files, never as a
            # second host copy
            raw = _LazyTensors(files)
        else:
            raw = {}
            for fn in files:
                raw.update(load_file(fn, device="cpu"))
        try:
            dev = torch.device(device)

            def g(k):
                t = raw[k]
                if t.dtype == torch.float8_e4m3fn:  # an F8 projection outside the experts: bf16 at load
                    return ops.block_fp8_dequant(t.to(dev), raw[k + _SCALE_SUFFIX].to(dev), torch.bfloat16).contiguous()
                return t.to(dtype=torch.bfloat16, device=dev).contiguous()

            experts_f8 = (moe is not None and fp8 and glm is None
                          and raw["model.layers.0.mlp.experts.0.gate_proj.weight"].dtype == torch.float8_e4m3fn)
            if experts_f8:
                cfg = replace(cfg, moe_weight_dtype="fp8b")

            def heads_perm(t, n):
                """``t`` [n x head_dim, ...] with each head's rows permuted for the partial rotary."""
                if perm is None:
                    return t
                idx = (torch.arange(n)[:, None] * cfg.head_dim + perm[None, :]).reshape(-1).to(t.device)
                return t.index_select(0, idx).contiguous()

            w = {"embed": g("model.embed_tokens.weight"), "norm_f": g("model.norm.weight"),
                 "lm_head": g("lm_head.weight") if "lm_head.weight" in raw else g("model.embed_tokens.weight")}
            for i in range(cfg.layers):
                p = f"model.layers.{i}."
                w[f"l{i}.ln1"] = g(p + "input_layernorm.weight")
                w[f"l{i}.ln2"] = g(p + "post_attention_layernorm.weight")
                w[f"l{i}.wqkv"] = torch.cat([heads_perm(g(p + "self_attn.q_proj.weight"), cfg.n_heads),
                                             heads_perm(g(p + "self_attn.k_proj.weight"), cfg.n_kv_heads),
                                             g(p + "self_attn.v_proj.weight")], 0).contiguous()
                if p + "self_attn.q_proj.bias" in raw:  # Qwen2: q/k/v biases, stacked like wqkv
                    w[f"l{i}.bqkv"] = torch.cat([heads_perm(g(p + "self_attn.q_proj.bias"), cfg.n_heads),
                                                 heads_perm(g(p + "self_attn.k_proj.bias"), cfg.n_kv_heads),
                                                 g(p + "self_attn.v_proj.bias")], 0).contiguous()
                if qk_norm:  # per-head q / k RMSNorm weights [head_dim]
                    w[f"l{i}.qnorm"] = heads_perm(g(p + "self_attn.q_norm.weight"), 1)
                    w[f"l{i}.knorm"] = heads_perm(g(p + "self_attn.k_norm.weight"), 1)
                w[f"l{i}.wo"] = g(p + "self_attn.o_proj.weight")
                if moe is not None and i >= cfg.dense_lead:
                    E, _, inter, _ = moe
                    S = cfg.moe_shared
                    w[f"l{i}.router"] = g(p + "mlp.gate.weight")
                    if glm is not None:  # the selection bias stays fp32
                        w[f"l{i}.router_bias"] = raw[p + _GLM_ROUTER_BIAS].to(dtype=torch.float32,
                                                                              device=dev).contiguous()
                    wdt = torch.float8_e4m3fn if experts_f8 else torch.bfloat16
                    gu = torch.empty((E + S, 2 * inter, cfg.hidden), dtype=wdt, device=dev)
                    down = torch.empty((E + S, cfg.hidden, inter), dtype=wdt, device=dev)
                    if S:  # the shared MLP's slices behind the routed experts (ops.reference.moe_stack_shared)
                        q = f"{p}mlp.shared_experts."
                        gu[E:, :inter].copy_(raw[q + "gate_proj.weight"].view(S, inter, cfg.hidden))
                        gu[E:, inter:].copy_(raw[q + "up_proj.weight"].view(S, inter, cfg.hidden))
                        down[E:].copy_(raw[q + "down_proj.weight"].view(cfg.hidden, S, inter).permute(1, 0, 2))
                    if experts_f8:  # the e4m3 bytes as they are, and their block scales beside them
                        nbi, nbh = -(-inter // FP8_BLOCK), -(-cfg.hidden // FP8_BLOCK)
                        gu_s = torch.empty((E, 2 * nbi, nbh), dtype=torch.float32, device=dev)
                        down_s = torch.empty((E, nbh, nbi), dtype=torch.float32, device=dev)
                    for e in range(E):  # straight into the stacked device tensors, one expert at a time
                        q = f"{p}mlp.experts.{e}."
                        gu[e, :inter].copy_(raw[q + "gate_proj.weight"])
                        gu[e, inter:].copy_(raw[q + "up_proj.weight"])
                        down[e].copy_(raw[q + "down_proj.weight"])
                        if experts_f8:
                            gu_s[e, :nbi].copy_(raw[q + "gate_proj.weight" + _SCALE_SUFFIX])
                            gu_s[e, nbi:].copy_(raw[q + "up_proj.weight" + _SCALE_SUFFIX])
                            down_s[e].copy_(raw[q + "down_proj.weight" + _SCALE_SUFFIX])
                    if experts_f8:
                        w[f"l{i}.we_gu8"], w[f"l{i}.we_gu_s"] = gu, gu_s
                        w[f"l{i}.we_down8"], w[f"l{i}.we_down_s"] = down, down_s
                    else:
                        w[f"l{i}.we_gu"], w[f"l{i}.we_down"] = gu, down
                    continue
                w[f"l{i}.wgu"] = torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0).contiguous()
                w[f"l{i}.wdown"] = g(p + "mlp.down_proj.weight")
        finally:
            if moe is not None:
                raw.close()  # the mapped files, now rather than at garbage collection
        m = cls(cfg, device, weights=w)
        m.checkpoint = path
        return m

    # ------------------------------------------------------------ forward
    def _qk_norm(self, i: int) -> Optional[tuple]:
        """Layer i's ``qk_norm`` argument of the QKV ops: (q weight, k weight, eps) or None."""
        if not self.has_qk_norm:
            return None
        return self.w[f"l{i}.qnorm"], self.w[f"l{i}.knorm"], self.cfg.eps

    def _wkw(self, i: int) -> dict:
        """Layer i's ``window`` keyword of the attention ops: empty for full attention."""
        w = self.windows[i] if self.windows else 0
        return {"window": w} if w else {}

    def _kvs(self, i: int) -> Optional[tuple]:
        """Layer i's ``kv_scale`` argument of the KV ops: its rows of the
        exponent tables, None for the unscaled formats."""
        if not self.kv_scaled:
            return None
        return self.k_scale[i], self.v_scale[i]

    def _mlp(self, i: int, h: torch.Tensor) -> torch.Tensor:
        gu = F.linear(h, self.w[f"l{i}.wgu"])
        return F.linear(ops.silu_mul(gu), self.w[f"l{i}.wdown"])

    def _moe(self, i: int, h: torch.Tensor, resid: torch.Tensor, nxt: Optional[torch.Tensor]) -> torch.Tensor:
        """Layer i's routed expert MLP of the normalised rows ``h``, added
        into ``resid`` in place; with ``nxt`` the rows normalised by it are
        returned (the add_rmsnorm that follows a dense MLP, fused into the
        combine).  More rows than the workspace holds go in chunks."""
        c = self.cfg
        w = self.w
        if self.moe_sig:  # the sigmoid router, the shared slices stacked behind the routed experts
            op = ops.moe_mlp_sh
            args = (w[f"l{i}.router"], w[f"l{i}.router_bias"], w[f"l{i}.we_gu"], w[f"l{i}.we_down"],
                    c.experts_per_tok, c.norm_topk, c.moe_route_scale, c.moe_shared)
        elif self.moe_w8:  # block-scaled e4m3 experts: the same launches over half the weight bytes
            op = ops.moe_mlp_w8
            args = (w[f"l{i}.router"], w[f"l{i}.we_gu8"], w[f"l{i}.we_gu_s"], w[f"l{i}.we_down8"],
                    w[f"l{i}.we_down_s"], c.experts_per_tok, c.norm_topk)
        else:
            op = ops.moe_mlp
            args = (w[f"l{i}.router"], w[f"l{i}.we_gu"], w[f"l{i}.we_down"], c.experts_per_tok, c.norm_topk)
        T = h.shape[0]
        if T <= self.moe_rows:
            return op(h, *args, residual=resid, norm_w=nxt, eps=c.eps, workspace=self.moe_ws)
        out = torch.empty_like(h) if nxt is not None else None
        for a in range(0, T, self.moe_rows):
            b = min(T, a + self.moe_rows)
            op(h[a:b], *args, residual=resid[a:b], norm_w=nxt, eps=c.eps, workspace=self.moe_ws,
               out=None if out is None else out[a:b])
        return resid if out is None else out

    def _mlp_norm(self, i: int, h: torch.Tensor, resid: torch.Tensor, nxt: torch.Tensor) -> torch.Tensor:
        """Layer i's MLP (dense or routed) + residual + the next RMSNorm."""
        if self.cfg.sparse_layer(i):
            return self._moe(i, h, resid, nxt)
        return ops.add_rmsnorm(self._mlp(i, h), nxt, self.cfg.eps, residual=resid)

    @torch.inference_mode()
    def forward_tokens(self, tokens: torch.Tensor, slot: int, start_pos: int) -> torch.Tensor:
        """Prefill (start_pos == 0) or extend one sequence by ``T`` tokens.

        Writes K/V for positions [start_pos, start_pos+T) into ``slot`` and
        returns the last position's logits ``[vocab]`` (bf16)."""
        c = self.cfg
        T = int(tokens.numel())
        if T == 0:
            raise ValueError("forward_tokens needs at least one token")
        if not (0 <= slot < self.num_slots) or start_pos < 0 or start_pos + T > c.max_seq:
            raise ValueError(f"sequence does not fit: slot={slot} start={start_pos} T={T} max_seq={c.max_seq}")
        dev = self.device
        ids = tokens.to(device=dev, dtype=torch.int32).contiguous()
        pos = torch.arange(start_pos, start_pos + T, dtype=torch.int32, device=dev)
        slots = torch.full((T,), slot, dtype=torch.int32, device=dev)
        if start_pos == 0:
            self._slot_prefix.pop(slot, None)  # a new sequence in this slot
        shared = self._slot_prefix.get(slot, 0)
        shared = shared if 0 < shared <= start_pos else 0
        x = ops.embedding(self.w["embed"], ids)
        resid = x.clone()
        h = ops.add_rmsnorm(x, self.w["l0.ln1"], c.eps)
        L = start_pos + T
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            qkv = F.linear(h, self.w[f"l{i}.wqkv"], self.w.get(f"l{i}.bqkv"))
            kvs = self._kvs(i)
            q = ops.rope_kv(qkv, pos, slots, self.cos_sin, kc, vc, c.n_heads, qk_norm=self._qk_norm(i),
                            kv_scale=kvs)  # [T, Hq, D]
            if self.use_prefill_kernel or self._wkw(i):
                # (a windowed layer off the kernel's shapes or on the CPU: the
                # fp32 reference of the same op -- SDPA below has no window)
                pf = ops.prefill_attention if self.use_prefill_kernel else ops.reference.prefill_attention
                att = pf(q, kc, vc, slot, start_pos, self.prefix_slot if shared else None,
                         shared, self.scale, kv_scale=kvs, **self._wkw(i))
                o = F.linear(att.view(T, c.n_heads * c.head_dim), self.w[f"l{i}.wo"])
            else:
                k = _kv_bf16(kc[slot, :, :L], kvs[0][slot, :, :L] if kvs else None).unsqueeze(0)  # [1, Hkv, L, D]
                v = _kv_bf16(vc[slot, :, :L], kvs[1][slot, :, :L] if kvs else None).unsqueeze(0)
                qh = q.transpose(0, 1).unsqueeze(0)  # [1, Hq, T, D]
                if start_pos == 0:
                    att = F.scaled_dot_product_attention(qh, k, v, is_causal=True, enable_gqa=True)
                else:  # extend after a cached context (e.g. a shared prefix)
                    att = _extend_attention(qh, k, v, start_pos, self.scale)
                o = F.linear(att[0].transpose(0, 1).reshape(T, c.n_heads * c.head_dim), self.w[f"l{i}.wo"])
            h = ops.add_rmsnorm(o, self.w[f"l{i}.ln2"], c.eps, residual=resid)
            nxt = self.w[f"l{i + 1}.ln1"] if i + 1 < c.layers else self.w["norm_f"]
            h = self._mlp_norm(i, h, resid, nxt)
        return F.linear(h[-1:], self.w["lm_head"])[0]

    @torch.inference_mode()
    def prefill_batch(self, reqs: Sequence[tuple]) -> torch.Tensor:
        """Prefill / extend several sequences in ONE pass: ``reqs`` =
        ``(tokens, slot, start)`` per sequence.  Their tokens are packed into
        one [Ttot, hidden] activation, so every projection is one GEMM over
        all of them (2,000-token prompts alone leave the MFMA GEMMs short of
        work) and the attention is one variable-length launch
        (``ops.prefill_attention_varlen``: per-sequence causal masks, the
        shared prefix read in place).  Returns each sequence's last-position
        logits [n, vocab] (bf16)."""
        c = self.cfg
        n = len(reqs)
        if n == 0:
            raise ValueError("prefill_batch needs at least one sequence")
        if not self.prefill_fp8 and (n == 1 or not (self.use_prefill_kernel or self.device.type == "cpu")):
            return torch.stack([self.forward_tokens(torch.as_tensor(t, dtype=torch.int32), sl, st)
                                for t, sl, st in reqs])
        import numpy as np
        offsets = [0]
        starts, seq_slots, shared, lens = [], [], [], []
        for t, sl, st in reqs:
            T = len(t)
            if T == 0:
                raise ValueError("prefill_batch: empty sequence")
            if not (0 <= sl < self.num_slots) or st < 0 or st + T > c.max_seq:
                raise ValueError(f"sequence does not fit: slot={sl} start={st} T={T} max_seq={c.max_seq}")
            if st == 0:
                self._slot_prefix.pop(sl, None)
            sh = self._slot_prefix.get(sl, 0)
            shared.append(sh if 0 < sh <= st else 0)
            offsets.append(offsets[-1] + T)
            starts.append(st)
            seq_slots.append(sl)
            lens.append(T)
        if len(set(seq_slots)) != n:
            raise ValueError("prefill_batch: each sequence needs its own slot")
        dev = self.device
        # [token, position, slot] per packed token, built in numpy (the Python
        # lists of ~20k tokens per admission cost the host milliseconds)
        Ttot = offsets[-1]
        st_rep = np.repeat(np.asarray(starts, dtype=np.int32), lens)
        base = np.repeat(np.asarray(offsets[:-1], dtype=np.int32), lens)
        meta_np = np.empty((3, Ttot), dtype=np.int32)
        meta_np[0] = np.concatenate([np.asarray(t, dtype=np.int32) for t, _, _ in reqs])
        meta_np[1] = st_rep + (np.arange(Ttot, dtype=np.int32) - base)
        meta_np[2] = np.repeat(np.asarray(seq_slots, dtype=np.int32), lens)
        meta = torch.from_numpy(meta_np)
        if dev.type == "cuda":
            meta = meta.pin_memory()
        meta = meta.to(dev, non_blocking=True)
        ids, pos_t, slot_t = meta[0], meta[1], meta[2]
        last = torch.tensor([o_ - 1 for o_ in offsets[1:]], dtype=torch.long)
        if dev.type == "cuda":  # pinned + async: a pageable copy would block the host until the stream drains
            last = last.pin_memory()
        last = last.to(dev, non_blocking=True)
        prefix = self.prefix_slot if any(shared) else None
        if self.prefill_fp8:
            h = self._prefill_fp8(ids, pos_t, slot_t, offsets, seq_slots, starts, prefix, shared, last)
            return self._head(h)
        x = ops.embedding(self.w["embed"], ids)
        resid = x.clone()
        h = ops.add_rmsnorm(x, self.w["l0.ln1"], c.eps)
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            qkv = F.linear(h, self.w[f"l{i}.wqkv"], self.w.get(f"l{i}.bqkv"))
            kvs = self._kvs(i)
            q = ops.rope_kv(qkv, pos_t, slot_t, self.cos_sin, kc, vc, c.n_heads,
                            qk_norm=self._qk_norm(i), kv_scale=kvs)  # [Ttot, Hq, D]
            att = ops.prefill_attention_varlen(q, kc, vc, offsets, seq_slots, starts, prefix, shared, self.scale,
                                               kv_scale=kvs, **self._wkw(i))
            o = F.linear(att.view(Ttot, c.n_heads * c.head_dim), self.w[f"l{i}.wo"])
            h = ops.add_rmsnorm(o, self.w[f"l{i}.ln2"], c.eps, residual=resid)
            nxt = self.w[f"l{i + 1}.ln1"] if i + 1 < c.layers else self.w["norm_f"]
            h = self._mlp_norm(i, h, resid, nxt)
        return F.linear(h.index_select(0, last), self.w["lm_head"])

    def _head(self, h: torch.Tensor) -> torch.Tensor:
        """The LM head's logits of a few rows (the batched prefill's last
        positions) on the weight-streaming kernel (csrc/wgemm.hip), hipBLASLt
        only off its shape contract."""
        if self.use_wgemm and h.shape[0] <= ops.WGEMM_MAX_ROWS and self.cfg.vocab_size % 64 == 0:
            return ops.wgemm(h.contiguous(), self.w["lm_head"])
        return F.linear(h, self.w["lm_head"])

    def _prefill_fp8(self, ids, pos_t, slot_t, offsets, seq_slots, starts, prefix, shared, last) -> torch.Tensor:
        """The layers of :meth:`prefill_batch` on the MXFP8 kernels: the
        activation entering each projection is MXFP8 (written by the RMSNorm
        before it, by the SwiGLU epilogue of gate/up, or quantised from the
        attention output), QKV's epilogue applies RoPE and appends K/V, O's and
        down's add into the residual stream.  Returns the final normalised
        hidden rows of ``last`` [n, hidden]."""
        c = self.cfg
        T = ids.numel()
        resid = ops.embedding(self.w["embed"], ids)
        aq, as_ = ops.rmsnorm_mx(resid, self._g("l0.ln1"), c.eps)
        act = None
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            q = ops.pgemm_qkv(aq, as_, *self.w8[f"l{i}.wqkv"], pos_t, slot_t, self.cos_sin, kc, vc, c.n_heads)
            att = ops.prefill_attention_varlen(q, kc, vc, offsets, seq_slots, starts, prefix, shared, self.scale,
                                               **self._wkw(i))
            ops.mx_quant(att.view(T, c.hidden), aq, as_)
            ops.pgemm_resid(aq, as_, *self.w8[f"l{i}.wo"], resid)
            ops.rmsnorm_mx(resid, self._g(f"l{i}.ln2"), c.eps, q=aq, s=as_)
            act = ops.pgemm_swiglu(aq, as_, *self.w8[f"l{i}.wgu"], *(act or (None, None)))
            ops.pgemm_resid(act[0], act[1], *self.w8[f"l{i}.wdown"], resid)
            if i + 1 < c.layers:
                ops.rmsnorm_mx(resid, self._g(f"l{i + 1}.ln1"), c.eps, q=aq, s=as_)
        return ops.add_rmsnorm(resid.index_select(0, last), self.w["norm_f"], c.eps)

    @torch.inference_mode()
    def decode(self, tokens: torch.Tensor, slots: torch.Tensor, positions: torch.Tensor,
               src: Optional[torch.Tensor] = None, last_ids: Optional[torch.Tensor] = None,
               mask_idx: Optional[torch.Tensor] = None, mask_alt: Optional[torch.Tensor] = None,
               alt_token: int = -1, prefix_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One token per row; all inputs int32 [B] on device.  With ``src`` /
        ``last_ids``: row r's token is ``last_ids[src[r]]`` where ``src[r] >= 0``
        (gathered on the device by the step's first kernel; with ``mask_alt``
        a gathered ``alt_token`` switches ``mask_idx[r]`` to ``mask_alt[r]``).
        ``prefix_rows`` (int32 [B]): 0 marks a row that does not use the
        shared prefix (a sequence admitted with its whole prompt in its slot).

        Rows are independent (slot, position) pairs: several rows may extend
        the SAME slot at consecutive positions (jump-forward over forced
        tokens) -- every row's K/V is appended before attention runs and each
        row attends to positions <= its own, so that is an exact causal
        extend.  Rows with slot -1 are padding.  Returns logits [B, vocab]
        (bf16).  Capturable into a hipGraph."""
        B = tokens.shape[0]
        if B > self.max_rows:
            raise ValueError(f"decode: {B} rows > max_rows {self.max_rows}")
        if self.use_fused and B <= self.fused_max_rows:
            return self._decode_fused(tokens, slots, positions, src, last_ids, mask_idx, mask_alt, alt_token,
                                      prefix_rows)
        h = self._decode_trunk(tokens, slots, positions, src, last_ids, mask_idx, mask_alt, alt_token, prefix_rows)
        return F.linear(h, self.w["lm_head"])

    def _decode_trunk(self, tokens, slots, positions, src, last_ids, mask_idx, mask_alt, alt_token,
                      prefix_rows) -> torch.Tensor:
        """Every layer of a decode step of > ``fused_max_rows`` rows; returns
        the final normalised hidden states [B, hidden] (the LM head's input)."""
        c = self.cfg
        B = tokens.shape[0]
        chunk, splits = ops.decode_plan(B, c.n_kv_heads, c.max_seq, c.kv_dtype)
        fp8 = self.decode_fp8 and (self.device.type == "cpu" or B <= ops.WMX_MAX_ROWS)
        resid, h, seq_len = ops.decode_embed_norm(self.w["embed"], tokens, positions,
                                                  self._g("l0.ln1") if fp8 else self.w["l0.ln1"], c.eps,
                                                  src, last_ids, mask_idx, mask_alt, alt_token)
        if fp8:
            return self._decode_trunk_fp8(B, resid, h, seq_len, slots, positions, chunk, splits, prefix_rows)
        wide = self.use_wgemm and B <= ops.WGEMM_MAX_ROWS
        big = self.use_tgemm and ops.WGEMM_MAX_ROWS < B <= ops.TGEMM_MAX_ROWS
        mlp_t = self.use_tgemm and self.TGEMM_MLP_MIN_ROWS <= B <= ops.TGEMM_MAX_ROWS
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            nxt = self.w[f"l{i + 1}.ln1"] if i + 1 < c.layers else self.w["norm_f"]
            bqkv = self.w.get(f"l{i}.bqkv")
            qkn = self._qk_norm(i)
            kvs = self._kvs(i)
            if big:
                q = ops.tgemm_rope_kv(h, self.w[f"l{i}.wqkv"], positions, slots, self.cos_sin, kc, vc, c.n_heads,
                                      self.tg_ws, bias=bqkv, qk_norm=qkn, kv_scale=kvs)
            elif wide:
                q = ops.wgemm_rope_kv(h, self.w[f"l{i}.wqkv"], positions, slots, self.cos_sin, kc, vc, c.n_heads,
                                      self.wgemm_ws, bias=bqkv, qk_norm=qkn, kv_scale=kvs)
            else:
                q = ops.rope_kv(F.linear(h, self.w[f"l{i}.wqkv"], bqkv), positions, slots, self.cos_sin, kc, vc,
                                c.n_heads, qk_norm=qkn, kv_scale=kvs)
            att = ops.decode_attention(q, kc, vc, slots, seq_len, self.scale, workspace=self.attn_ws, chunk=chunk,
                                       fork=self.fork_tab, prefix=self._prefix(i, prefix_rows), splits=splits,
                                       kv_scale=kvs, **self._wkw(i)).view(B, c.n_heads * c.head_dim)
            if big:
                h = ops.tgemm_resid_norm(att, self.w[f"l{i}.wo"], resid, self.w[f"l{i}.ln2"], c.eps, self.tg_ws)
            elif wide:
                h = ops.wgemm_resid_norm(att, self.w[f"l{i}.wo"], resid, self.w[f"l{i}.ln2"], c.eps, self.wgemm_ws)
            else:
                h = ops.add_rmsnorm(F.linear(att, self.w[f"l{i}.wo"]), self.w[f"l{i}.ln2"], c.eps, residual=resid)
            if c.sparse_layer(i):
                h = self._moe(i, h, resid, nxt)
            elif mlp_t:
                act = ops.tgemm_swiglu(h, self.w[f"l{i}.wgu"])
                h = ops.tgemm_resid_norm(act, self.w[f"l{i}.wdown"], resid, nxt, c.eps, self.tg_ws)
            elif wide:
                act = ops.wgemm_swiglu(h, self.w[f"l{i}.wgu"])
                h = ops.wgemm_resid_norm(act, self.w[f"l{i}.wdown"], resid, nxt, c.eps, self.wgemm_ws)
            else:
                h = ops.add_rmsnorm(self._mlp(i, h), nxt, c.eps, residual=resid)
        return h

    def _decode_trunk_fp8(self, B, resid, h, seq_len, slots, positions, chunk, splits, prefix_rows) -> torch.Tensor:
        """The layers of a decode step on the fp8 weights: every projection's
        activation is MXFP8 (the step's first norm quantised once, then written
        by the split-K reduction + residual + RMSNorm kernels and the SwiGLU
        epilogue); the last layer's norm writes bf16 for the LM head.  GPU: the
        MX weight-streaming GEMM (csrc/pgemm.hip wmx_kernel); CPU: the fp32
        references of the same compositions."""
        c = self.cfg
        gpu = self.device.type == "cuda"
        xq, xs = ops.mx_quant(h)
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            last = i + 1 == c.layers
            # MXFP8 activations carry the real norm weights; the last norm
            # feeds the (norm-folded) bf16 LM head
            nxt = self.w["norm_f"] if last else self._g(f"l{i + 1}.ln1")
            w8 = self.w8
            if gpu:
                q = ops.wgemm_mx_rope_kv(xq, xs, *w8[f"l{i}.wqkv"], positions, slots, self.cos_sin, kc, vc,
                                         c.n_heads, self.wmx_ws)
            else:
                q = ops.pgemm_qkv(xq, xs, *w8[f"l{i}.wqkv"], positions, slots, self.cos_sin, kc, vc, c.n_heads)
            att = ops.decode_attention(q, kc, vc, slots, seq_len, self.scale, workspace=self.attn_ws, chunk=chunk,
                                       fork=self.fork_tab,
                                       prefix=self._prefix(i, prefix_rows), splits=splits,
                                       **self._wkw(i)).view(B, c.hidden)
            aq, as_ = ops.mx_quant(att)
            if gpu:
                xq, xs = ops.wgemm_mx_resid_norm(aq, as_, *w8[f"l{i}.wo"], resid, self._g(f"l{i}.ln2"), c.eps,
                                                 self.wmx_ws)
                gq, gs = ops.wgemm_mx_swiglu(xq, xs, *w8[f"l{i}.wgu"])
                r = ops.wgemm_mx_resid_norm(gq, gs, *w8[f"l{i}.wdown"], resid, nxt, c.eps, self.wmx_ws,
                                            mx=not last)
            else:
                ops.pgemm_resid(aq, as_, *w8[f"l{i}.wo"], resid)
                xq, xs = ops.rmsnorm_mx(resid, self._g(f"l{i}.ln2"), c.eps)
                gq, gs = ops.pgemm_swiglu(xq, xs, *w8[f"l{i}.wgu"])
                ops.pgemm_resid(gq, gs, *w8[f"l{i}.wdown"], resid)
                r = ops.add_rmsnorm(resid, nxt, c.eps) if last else ops.rmsnorm_mx(resid, nxt, c.eps)
            if last:
                h = r
            else:
                xq, xs = r
        return h

    def _prefix(self, i: int, rows: Optional[torch.Tensor] = None):
        if not self.shared_prefix:
            return None
        if self.kv_scaled:
            return ops.SharedPrefix(self.k_cache[i][self.prefix_slot], self.v_cache[i][self.prefix_slot],
                                    self.prefix_dev, rows, self.k_scale[i][self.prefix_slot],
                                    self.v_scale[i][self.prefix_slot])
        return ops.SharedPrefix(self.k_cache[i][self.prefix_slot], self.v_cache[i][self.prefix_slot],
                                self.prefix_dev, rows)

    def _decode_fused(self, tokens: torch.Tensor, slots: torch.Tensor, positions: torch.Tensor,
                      src: Optional[torch.Tensor] = None, last_ids: Optional[torch.Tensor] = None,
                      mask_idx: Optional[torch.Tensor] = None, mask_alt: Optional[torch.Tensor] = None,
                      alt_token: int = -1, prefix_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The decode step on the fused gfx950 GEMMs: per layer QKV (+norm,
        RoPE, KV append) -> attention -> O (+residual) -> gate/up (+norm,
        SwiGLU) -> down (+residual); the residual stream ``r`` is updated in
        place by the O / down epilogues."""
        c = self.cfg
        B = tokens.shape[0]
        chunk, splits = ops.decode_plan(B, c.n_kv_heads, c.max_seq, c.kv_dtype)
        r, _, seq_len = ops.decode_embed_norm(self.w["embed"], tokens, positions, None, c.eps, src, last_ids,
                                              mask_idx, mask_alt, alt_token)
        for i in range(c.layers):
            kc, vc = self.k_cache[i], self.v_cache[i]
            kvs = self._kvs(i)
            if self.has_qk_norm or self.kv_scaled:
                # the fused QKV tile holds 32 of a head's columns, so neither
                # the per-head norm nor a scaled cache row's amax can sit in
                # its epilogue: norm-folded QKV to a bf16 row, then the
                # norm-taking / scaling RoPE + append (one launch more per
                # layer; docs/KERNELS.md)
                qkv = ops.fused_linear_norm(r, self.w[f"l{i}.wqkv"], c.eps, out=self.qkv_buf[:B])
                q = ops.rope_kv(qkv, positions, slots, self.cos_sin, kc, vc, c.n_heads, qk_norm=self._qk_norm(i),
                                kv_scale=kvs)
            else:
                q = ops.fused_rope_kv(r, self.w[f"l{i}.wqkv"], c.eps, positions, slots, self.cos_sin, kc, vc,
                                      c.n_heads, bias=self.w.get(f"l{i}.bqkv"))
            att = ops.decode_attention(q, kc, vc, slots, seq_len, self.scale, workspace=self.attn_ws, chunk=chunk,
                                       fork=self.fork_tab,
                                       prefix=self._prefix(i, prefix_rows), splits=splits, kv_scale=kvs,
                                       **self._wkw(i))
            ops.fused_resid(att.view(B, c.n_heads * c.head_dim), self.w[f"l{i}.wo"], r)
            if c.sparse_layer(i):
                # the norm fused_swiglu folds into its prologue, explicit: the
                # router and every chosen expert read the same normalised row
                self._moe(i, ops.add_rmsnorm(r, self.w[f"l{i}.ln2"], c.eps), r, None)
                continue
            act = ops.fused_swiglu(r, self.w[f"l{i}.wgu"], c.eps)
            ops.fused_resid(act, self.w[f"l{i}.wdown"], r)
        return ops.fused_linear_norm(r, self.w["lm_head"], c.eps)

    # ---------------------------------------------------------- shared prefix
    @torch.inference_mode()
    def set_prefix(self, tokens: Sequence[int]) -> int:
        """Prefills ``tokens`` into the prefix slot and publishes them as the
        shared prefix of every following decode step (positions [0, P) of
        each row).  Sequences must be started with :meth:`fork_prefix` +
        ``forward_tokens(rest, slot, P)``.  Returns P."""
        if not self.shared_prefix:
            raise RuntimeError("model built without shared_prefix")
        toks = tuple(int(t) for t in tokens)
        P = len(toks)
        if P == 0 or P >= self.cfg.max_seq:
            raise ValueError(f"prefix length {P} out of range (max_seq {self.cfg.max_seq})")
        if toks == self.prefix_tokens:
            return P
        self.clear_prefix()
        if self.prefill_fp8:  # the MXFP8 prefill kernels, as every other prompt token
            self.prefill_batch([(list(toks), self.prefix_slot, 0)])
        else:
            self.forward_tokens(torch.tensor(toks, dtype=torch.int32), self.prefix_slot, 0)
        self.prefix_len, self.prefix_tokens = P, toks
        self.prefix_dev.fill_(P)
        return P

    def clear_prefix(self) -> None:
        if self.shared_prefix:
            self.prefix_dev.zero_()
        self.prefix_len, self.prefix_tokens = 0, ()
        self._slot_prefix.clear()

    @torch.inference_mode()
    def fork_prefix(self, slot: int) -> int:
        """Starts ``slot`` on the shared prefix: prefill of the rest of that
        sequence (``forward_tokens(rest, slot, P)``) attends to the prefix
        keys -- read in place from the prefix slot by the MFMA prefill kernel,
        or copied into ``slot`` on the SDPA path; decode always reads the
        shared copy.  Returns P (0 when no prefix is set)."""
        P = self.prefix_len
        if P and self.use_prefill_kernel:
            self._slot_prefix[slot] = P  # the prefill kernel reads the shared copy in place
        elif P:
            self.k_cache[:, slot, :, :P].copy_(self.k_cache[:, self.prefix_slot, :, :P])
            self.v_cache[:, slot, :, :P].copy_(self.v_cache[:, self.prefix_slot, :, :P])
            if self.kv_scaled:
                self.k_scale[:, slot, :, :P].copy_(self.k_scale[:, self.prefix_slot, :, :P])
                self.v_scale[:, slot, :, :P].copy_(self.v_scale[:, self.prefix_slot, :, :P])
        return P

    @torch.inference_mode()
    def fork_kv(self, src: int, dsts: Sequence[int], start: int, end: int) -> None:
        """Copies slot ``src``'s keys / values at positions [start, end) into
        every slot of ``dsts`` (the method branches of a class continue from
        its head's KV; positions before ``start`` are the shared prefix).
        One indexed copy per cache, on the current stream."""
        if end <= start or not dsts:
            return
        if not (0 <= src < self.num_slots) or any(not 0 <= d < self.num_slots for d in dsts) or \
                not (0 <= start <= end <= self.cfg.max_seq):
            raise ValueError(f"fork_kv: slot {src} -> {list(dsts)}, positions [{start}, {end})")
        if self.device.type == "cuda":  # one HIP launch for both caches (csrc/dmcp_kernels.hip kv_fork_kernel)
            ops.hip.kv_fork(self.k_cache, self.v_cache, src, dsts, start, end,
                            (self.k_scale, self.v_scale) if self.kv_scaled else None)
            return
        idx = torch.tensor(list(dsts), dtype=torch.long, device=self.device)
        for cache in (self.k_cache, self.v_cache) + ((self.k_scale, self.v_scale) if self.kv_scaled else ()):
            cache[:, idx, :, start:end] = cache[:, src, :, start:end].unsqueeze(1)

    @torch.inference_mode()
    def fork_share(self, src: int, dsts: Sequence[int], end: int) -> None:
        """Every slot of ``dsts`` continues from slot ``src``'s keys / values
        below ``end`` WITHOUT a copy: the decode attention reads them from
        ``src`` in place (``fork_tab``).  The caller keeps ``src``'s positions
        below ``end`` unchanged while any of ``dsts`` decodes (a branch only
        writes past ``end``)."""
        dl = [int(d) for d in dsts if int(d) != int(src)]
        if not dl or end <= 0:
            return
        if not (0 <= src < self.num_slots) or any(not 0 <= d < self.num_slots for d in dl) or \
                not (0 < end <= self.cfg.max_seq):
            raise ValueError(f"fork_share: slot {src} -> {dl}, end {end}")
        self._fork_set([(d, int(src), int(end)) for d in dl])

    def _fork_set(self, rows) -> None:
        """``fork_tab[slot] = (parent, end)`` for each of ``rows``; with
        :attr:`fork_defer` they wait for :meth:`fork_flush` (later rows of a
        slot replace earlier ones)."""
        if self.fork_defer:
            for slot, parent, end in rows:
                self._fork_pending[slot] = (parent, end)
            return
        self._fork_tab_update(rows)

    def fork_flush(self) -> None:
        """Applies the deferred fork-table rows: one copy + one indexed write
        (the engine calls this before each decode launch)."""
        if self._fork_pending:
            rows = [(k, p, e) for k, (p, e) in self._fork_pending.items()]
            self._fork_pending.clear()
            self._fork_tab_update(rows)

    @torch.inference_mode()
    def _fork_tab_update(self, rows) -> None:
        """``fork_tab[slot] = (parent, end)`` from host rows (distinct slots),
        in stream order without blocking the host: a pageable source would
        make the copy wait for the stream to drain (up to a whole queued
        prefill, GPU idle after it)."""
        both = torch.tensor(rows, dtype=torch.int64)
        if self.device.type == "cuda":
            both = both.pin_memory().to(self.device, non_blocking=True)
        self.fork_tab.index_copy_(0, both[:, 0], both[:, 1:].to(torch.int32))

    @torch.inference_mode()
    def fork_reset(self) -> None:
        """No slot has a parent (every slot owns all its keys)."""
        self._fork_pending.clear()
        self.fork_tab[:, 1] = 0

    @torch.inference_mode()
    def fork_clear(self, slots: Sequence[int]) -> None:
        """``slots`` own all their keys again (a freed or newly admitted slot)."""
        self._fork_set([(int(x), int(x), 0) for x in slots])

    def reserve_truncation_logits(self) -> Optional[torch.Tensor]:
        """The logits buffer of truncated sampling past the small-step row
        count (GPU; None elsewhere), allocated on the first call: an engine
        with a filter configured calls it when it is built, before any graph
        is captured."""
        if self.trunc_logits is None and self.fused_head:
            self.trunc_logits = torch.empty((self.max_rows, self.cfg.vocab_size), dtype=self.dtype,
                                            device=self.device)
        return self.trunc_logits

    def reserve_history(self) -> torch.Tensor:
        """The token history of the repetition / presence penalty (int32
        [num_slots, ceil(vocab / 32)] bitset rows, :func:`dmcp.ops.history_mark`;
        12.3 MB at 768 slots x 128,256 ids), allocated zeroed on the first
        call: an engine with a penalty configured calls it when it is built,
        before any graph is captured."""
        if self.history is None:
            self.history = torch.zeros((self.num_slots, (self.cfg.vocab_size + 31) // 32), dtype=torch.int32,
                                       device=self.device)
        return self.history

    def _step_penalty(self, penalty: Optional[tuple], tokens: torch.Tensor, slots: torch.Tensor,
                      src: Optional[torch.Tensor] = None, last_ids: Optional[torch.Tensor] = None):
        """The first op of a penalised decode step: record the tokens the step
        feeds (before the head overwrites ``last_ids``, and so that this
        step's selection sees the token just fed) and return the
        :class:`dmcp.ops.Penalty` of its selection.  ``penalty`` = (theta,
        alpha, flags per mask row or None, exempt bitset or None); None, or
        theta 1 and alpha 0: nothing is launched and None is returned."""
        if penalty is None or (penalty[0] == 1 and penalty[1] == 0):
            return None
        theta, alpha, flags, exempt = penalty
        hist = self.reserve_history()
        ops.history_mark(hist, tokens, slots, src, last_ids if src is not None else None, exempt,
                         self.cfg.vocab_size)
        # the slots are the step's own, inside the KV cache: no read-back to check them
        return ops.Penalty(hist, slots, theta, alpha, flags, check_slots=False)

    def _head_into(self, h: torch.Tensor, buf: torch.Tensor) -> torch.Tensor:
        """The LM head's logits of a decode step written to ``buf[:rows]``:
        the large-tile GEMM from TGEMM_HEAD_MIN_ROWS rows where the fused
        head would use it, the weight-streaming GEMM below (as :meth:`_head`),
        hipBLASLt only off their shape contracts."""
        B = h.shape[0]
        out = buf[:B]
        if self.tg_head and B >= self.TGEMM_HEAD_MIN_ROWS:
            return ops.tgemm(h, self.w["lm_head"], out=out)
        if self.use_wgemm and B <= ops.WGEMM_MAX_ROWS and self.cfg.vocab_size % 64 == 0:
            return ops.wgemm(h.contiguous(), self.w["lm_head"], out=out)
        return torch.matmul(h, self.w["lm_head"].t(), out=out)

    def decode_select(self, tokens: torch.Tensor, slots: torch.Tensor, positions: torch.Tensor,
                      masks: torch.Tensor, mask_idx: torch.Tensor, sample: Optional[tuple] = None,
                      truncate: Optional[tuple] = None, penalty: Optional[tuple] = None) -> tuple:
        """:meth:`decode` + selection under a per-row grammar mask
        (``masks`` [M, ceil(V/32)] bitsets, ``mask_idx`` int32 [B]): greedy,
        or with ``sample`` = (temperature, seed) a draw from softmax(logits /
        temperature) over the allowed ids, keyed by the row's slot and
        position (:func:`dmcp.ops.masked_sample`; temperature 0 is greedy);
        ``truncate`` = (top_k, top_p, min_p) restricts that draw
        (:func:`dmcp.ops.truncated_sample`; ignored when greedy).
        ``penalty`` = (theta, alpha, flags per mask row, exempt bitset): the
        repetition / presence penalty over the tokens fed to each slot
        (:meth:`_step_penalty`: one more launch, first in the step; works at
        temperature 0 too).  Returns (logits, ids int32 [B]); capturable."""
        pen = {} if (p := self._step_penalty(penalty, tokens, slots)) is None else {"penalty": p}
        logits = self.decode(tokens, slots, positions)
        cut = _truncation(sample, truncate)
        if cut is not None:
            ids = ops.truncated_sample(logits, masks, vocab=self.cfg.vocab_size, mask_idx=mask_idx, slots=slots,
                                       positions=positions, temperature=sample[0], seed=sample[1], top_k=cut[0],
                                       top_p=cut[1], min_p=cut[2], **pen)
        elif sample is not None:
            ids = ops.masked_sample(logits, masks, vocab=self.cfg.vocab_size, mask_idx=mask_idx, slots=slots,
                                    positions=positions, temperature=sample[0], seed=sample[1], **pen)
        else:
            ids = ops.masked_argmax(logits, masks, vocab=self.cfg.vocab_size, mask_idx=mask_idx, **pen)
        return logits, ids

    def decode_select_gather(self, tokens: torch.Tensor, src: torch.Tensor, last_ids: torch.Tensor,
                             slots: torch.Tensor, positions: torch.Tensor, masks: torch.Tensor,
                             mask_idx: torch.Tensor, mask_alt: Optional[torch.Tensor] = None,
                             alt_token: int = -1, prefix_rows: Optional[torch.Tensor] = None,
                             sample: Optional[tuple] = None, truncate: Optional[tuple] = None,
                             penalty: Optional[tuple] = None) -> tuple:
        """:meth:`decode_select` whose input token of row r is ``last_ids[src[r]]``
        where ``src[r] >= 0`` (the previous step's selection, still on the
        device) and ``tokens[r]`` otherwise; the step's own selections are
        written to ``last_ids`` for the next step.  Lets the host launch step
        t+1 before it has read step t's ids (the engine's one-step pipeline).
        ``mask_alt`` / ``alt_token`` / ``prefix_rows``: see :meth:`decode`.
        ``sample`` = (temperature, seed): every path samples instead (the
        same tiles and launches: the selection kernels' sampling variants).
        ``truncate`` = (top_k, top_p, min_p) with a filter on (and a
        temperature above 0): the fused head is not taken -- the step writes
        its bf16 logits with the plain GEMM (:meth:`_head_into`, into the
        buffer of :meth:`reserve_truncation_logits`) and selects with
        :func:`dmcp.ops.truncated_sample`, as many kernels as the fused head
        and its pair reduction; the logits are returned.  ``penalty``: as
        :meth:`decode_select` -- the gathered tokens are recorded first, then
        whichever selection the step takes (a fused head, the <= 16-row path
        or the truncation path) runs its penalised variant.  Capturable."""
        B = tokens.shape[0]
        keys = {} if sample is None else {"slots": slots, "positions": positions, "temperature": sample[0],
                                          "seed": sample[1]}
        if (p := self._step_penalty(penalty, tokens, slots, src, last_ids)) is not None:
            keys["penalty"] = p
        cut = _truncation(sample, truncate)
        if cut is not None:
            keys.update(top_k=cut[0], top_p=cut[1], min_p=cut[2])
        if self.fused_head and not (self.use_fused and B <= self.fused_max_rows):
            h = self._decode_trunk(tokens, slots, positions, src, last_ids, mask_idx, mask_alt, alt_token,
                                   prefix_rows)
            if cut is not None:
                logits = self._head_into(h, self.reserve_truncation_logits())
                ids = ops.truncated_sample(logits, masks, vocab=self.cfg.vocab_size, mask_idx=mask_idx,
                                           out=last_ids[:B], **keys)
                return logits, ids
            # the LM head + grammar-masked selection in one weight-streaming
            # kernel: no [B, vocab] logits (returned as None)
            if self.tg_head and B >= self.TGEMM_HEAD_MIN_ROWS:
                head = ops.tgemm_lm_head_argmax if sample is None else ops.tgemm_lm_head_sample
                ids = head(h, self.w["lm_head"], masks, mask_idx, out=last_ids[:B], workspace=self.tg_head_ws, **keys)
            else:
                head = ops.lm_head_argmax if sample is None else ops.lm_head_sample
                ids = head(h, self.w["lm_head"], masks, mask_idx, out=last_ids[:B], workspace=self.head_ws, **keys)
            return None, ids
        logits = self.decode(tokens, slots, positions, src=src, last_ids=last_ids, mask_idx=mask_idx,
                             mask_alt=mask_alt, alt_token=alt_token, prefix_rows=prefix_rows)
        select = (ops.masked_argmax if sample is None else ops.masked_sample if cut is None
                  else ops.truncated_sample)
        ids = select(logits, masks, vocab=self.cfg.vocab_size, mask_idx=mask_idx, out=last_ids[:B], **keys)
        return logits, ids

    # reference path (pure torch, fp32 math) for numerics tests
    @torch.inference_mode()
    def reference_logits(self, tokens: Sequence[int], start_pos: int = 0) -> torch.Tensor:
        """fp32 logits [T, vocab] of ``tokens`` at positions [start_pos, start_pos + T)."""
        c = self.cfg
        dev = self.device
        w = {k: v.float() for k, v in self.w.items() if v.dtype != torch.float8_e4m3fn}
        ids = torch.tensor(list(tokens), dtype=torch.long, device=dev)
        T = ids.numel()
        x = w["embed"][ids]

        def rms(t, g):
            return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + c.eps) * g

        pos = torch.arange(start_pos, start_pos + T, device=dev, dtype=torch.int32)
        cs = self.cos_sin
        G = c.n_heads // c.n_kv_heads
        for i in range(c.layers):
            h = rms(x, w[f"l{i}.ln1"])
            qkv = h @ w[f"l{i}.wqkv"].t()
            if f"l{i}.bqkv" in w:
                qkv = qkv + w[f"l{i}.bqkv"]
            qkv = qkv.view(T, c.n_heads + 2 * c.n_kv_heads, c.head_dim)
            xq, xk = qkv[:, :c.n_heads], qkv[:, c.n_heads:c.n_heads + c.n_kv_heads]
            if f"l{i}.qnorm" in w:
                xq = ops.reference.head_rmsnorm(xq, w[f"l{i}.qnorm"], c.eps)
                xk = ops.reference.head_rmsnorm(xk, w[f"l{i}.knorm"], c.eps)
            q = ops.reference.apply_rope(xq, pos, cs)
            k = ops.reference.apply_rope(xk, pos, cs)
            v = qkv[:, c.n_heads + c.n_kv_heads:]
            k = k.repeat_interleave(G, dim=1)
            v = v.repeat_interleave(G, dim=1)
            att = torch.einsum("thd,shd->hts", q, k) * self.scale
            att = att.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), 1), float("-inf"))
            if self._wkw(i):  # key j of query t only while j > t - window
                att = att.masked_fill(torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev),
                                                 -self.windows[i]), float("-inf"))
            o = torch.einsum("hts,shd->thd", torch.softmax(att, -1), v).reshape(T, -1)
            x = x + o @ w[f"l{i}.wo"].t()
            h = rms(x, w[f"l{i}.ln2"])
            if self.moe_sig and c.sparse_layer(i):
                x = x + ops.reference.moe_mlp_sh_math(h, w[f"l{i}.router"], w[f"l{i}.router_bias"], w[f"l{i}.we_gu"],
                                                      w[f"l{i}.we_down"], c.experts_per_tok, c.norm_topk,
                                                      c.moe_route_scale, c.moe_shared)
                continue
            if c.sparse_layer(i):
                if self.moe_w8:  # the experts dequantised exactly (fp32), one layer at a time
                    we_gu, we_down = ops.reference.moe_w8_dequant(self.w[f"l{i}.we_gu8"], self.w[f"l{i}.we_gu_s"],
                                                                  self.w[f"l{i}.we_down8"], self.w[f"l{i}.we_down_s"])
                else:
                    we_gu, we_down = w[f"l{i}.we_gu"], w[f"l{i}.we_down"]
                x = x + ops.reference.moe_mlp_math(h, w[f"l{i}.router"], we_gu, we_down, c.experts_per_tok,
                                                   c.norm_topk)
                continue
            gu = h @ w[f"l{i}.wgu"].t()
            g_, u_ = gu[:, :c.intermediate], gu[:, c.intermediate:]
            x = x + (F.silu(g_) * u_) @ w[f"l{i}.wdown"].t()
        return rms(x, w["norm_f"]) @ w["lm_head"].t()


_HIPRT = None


def graph_kernel_nodes(g) -> int:
    """Kernel nodes of a captured hipGraph (hipGraphGetNodes +
    hipGraphNodeGetType through the HIP runtime torch already loaded); -1 if
    the runtime does not answer.  The engine's device witness: replays x
    kernels per replay = kernels the GPU ran for the decode steps."""
    global _HIPRT
    import ctypes
    try:
        if _HIPRT is None:
            _HIPRT = ctypes.CDLL("libamdhip64.so")
        graph = ctypes.c_void_p(g.raw_cuda_graph())
        n = ctypes.c_size_t(0)
        if _HIPRT.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
            return -1
        nodes = (ctypes.c_void_p * n.value)()
        if _HIPRT.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) != 0:
            return -1
        kernels = 0
        for i in range(n.value):
            t = ctypes.c_int(-1)
            if _HIPRT.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)) == 0 and t.value == 0:
                kernels += 1  # hipGraphNodeTypeKernel
        return kernels
    except Exception:  # noqa: BLE001 -- a witness, never a failure
        return -1


class _Bucket:
    """One captured decode graph and its two pinned staging buffers: a step
    packs its rows into the buffer whose previous H2D copy (two steps back)
    has surely completed, so the host never waits on the copy of the step
    still in flight (one buffer made every launch wait for it: ~0.9 ms per
    step at 533 rows, graph_timing sync_s)."""
    __slots__ = ("graph", "inp", "logits", "ids", "stage", "np", "copied", "turn", "kernels")

    def __init__(self, graph, inp, logits, ids, b: int) -> None:
        self.graph, self.inp, self.logits, self.ids = graph, inp, logits, ids
        self.kernels = graph_kernel_nodes(graph)
        self.stage = [torch.zeros((7, b), dtype=torch.int32).pin_memory() for _ in range(2)]
        self.np = [t.numpy() for t in self.stage]
        self.copied = [torch.cuda.Event(), torch.cuda.Event()]
        self.turn = 0

    def stage_for_write(self, timing: dict):
        t0 = time.perf_counter()
        self.copied[self.turn].synchronize()  # that buffer's last H2D copy is done
        timing["sync_s"] += time.perf_counter() - t0
        return self.np[self.turn]


class DecodeGraphs:
    """hipGraph-captured decode + selection steps, one graph per row-count bucket.

    Inputs travel as ONE packed int32 host buffer ``[7, n]`` (token, slot,
    position, mask row, token source, mask row if the gathered token is
    ``alt_token``, uses-the-shared-prefix flag) -> one H2D copy into the graph's static
    input; the graph gathers the rows whose source is >= 0 from the previous
    step's selections (:attr:`last_ids`, device-resident, written by every
    step), runs the whole forward plus the masked selection, so a step costs one
    copy in, one replay and one 4-byte-per-row copy out.  Padding rows carry
    slot -1 (kernels skip them).  Returned tensors are the graph's static
    outputs: read them before the next replay of the same bucket."""

    def __init__(self, model: LocalLM, masks: torch.Tensor,
                 buckets: Sequence[int] = (1, 2, 4, 8, 16, 32, 64, 96, 128, 192, 256, 320, 384, 448, 512, 640,
                                          768, 896, 1024), alt_token: int = -1,
                 sample: Optional[tuple] = None, truncate: Optional[tuple] = None,
                 penalty: Optional[tuple] = None) -> None:
        self.model = model
        self.masks = masks
        self.alt_token = int(alt_token)
        # (temperature, seed) of a sampling engine, fixed for its lifetime: a
        # constant of the captured selection kernels (None: greedy)
        self.sample = sample
        # (top_k, top_p, min_p) of that engine (None: no truncation): the
        # captured step then writes logits and selects with truncated_sample
        self.truncate = truncate
        if _truncation(sample, truncate) is not None:
            model.reserve_truncation_logits()  # before any capture
        # (theta, alpha, flags per mask row, exempt bitset) of that engine's
        # repetition / presence penalty, a constant of the capture like the
        # two above: the graph gains one kernel node (history_mark); None, or
        # theta 1 and alpha 0: the graph is the unpenalised one, node for node
        self.penalty = None if penalty is None or (penalty[0] == 1 and penalty[1] == 0) else penalty
        if self.penalty is not None:
            model.reserve_history()  # before any capture
        self.timing = {"sync_s": 0.0, "replay_s": 0.0}  # host time inside run(): staging wait, H2D + launch
        # device witness: graph replays and the kernel nodes they launched
        self.counts = {"graph_replays": 0, "graph_kernels": 0}
        self.buckets = sorted(b for b in buckets if b <= model.max_rows)
        if not self.buckets or self.buckets[-1] < model.max_rows:
            self.buckets.append(model.max_rows)
        self.graphs: Dict[int, tuple] = {}
        self.enabled = model.device.type == "cuda"
        self.last_ids = torch.zeros(max(self.buckets), dtype=torch.int32, device=model.device)

    def capture_all(self) -> int:
        """Captures the graph of every bucket not captured yet (the engine
        does this at start, so no capture stalls a running batch); returns
        the number of captured buckets."""
        for b in self.buckets:
            if b not in self.graphs:
                self._capture(b)
                # one replay now (padding rows only): a graph's first launch
                # costs milliseconds more than the later ones
                self.graphs[b].graph.replay()
        torch.cuda.synchronize()
        return len(self.graphs)

    def bucket_for(self, n: int) -> int:
        for b in self.buckets:
            if b >= n:
                return b
        raise ValueError(f"{n} rows exceed the largest decode bucket {self.buckets[-1]}")

    def _capture(self, b: int):
        m = self.model
        inp = torch.zeros((7, b), dtype=torch.int32, device=m.device)
        inp[1].fill_(-1)
        inp[4].fill_(-1)
        inp[5].fill_(-1)
        scratch = torch.zeros_like(self.last_ids)  # warm-up must not clobber last_ids
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # warm up hipBLASLt heuristics / allocator outside capture
                m.decode_select_gather(inp[0], inp[4], scratch, inp[1], inp[2], self.masks, inp[3], inp[5],
                                       self.alt_token, inp[6], self.sample, self.truncate, self.penalty)
        torch.cuda.current_stream().wait_stream(s)
        # keep_graph: the hipGraph_t stays queryable after capture (the kernel
        # node count of the witness); instantiated explicitly right after
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            logits, ids = m.decode_select_gather(inp[0], inp[4], self.last_ids, inp[1], inp[2], self.masks, inp[3],
                                                 inp[5], self.alt_token, inp[6], self.sample, self.truncate,
                                                 self.penalty)
        bucket = _Bucket(g, inp, logits, ids, b)
        g.instantiate()
        self.graphs[b] = bucket

    @torch.inference_mode()
    def run(self, tokens: Sequence[int], slots: Sequence[int], positions: Sequence[int],
            mask_rows: Sequence[int], srcs: Optional[Sequence[int]] = None,
            alts: Optional[Sequence[int]] = None, prefix_rows: Optional[Sequence[int]] = None) -> tuple:
        """One step over ``n`` rows given as host lists (``srcs[r] >= 0``:
        row r's token is row ``srcs[r]``'s selection of the previous step;
        ``alts[r] >= 0``: row r's mask row when that token is ``alt_token``;
        ``prefix_rows[r] == 0``: row r does not use the shared prefix).
        Returns (logits[:n], ids[:n]) -- device tensors owned by the graph."""
        n = len(tokens)
        m = self.model
        if srcs is None:
            srcs = [-1] * n
        if alts is None:
            alts = [-1] * n
        if prefix_rows is None:
            prefix_rows = [1] * n
        if not self.enabled:
            t = torch.tensor([list(tokens), list(slots), list(positions), list(mask_rows), list(srcs), list(alts),
                              list(prefix_rows)], dtype=torch.int32, device=m.device)
            return m.decode_select_gather(t[0].contiguous(), t[4].contiguous(), self.last_ids, t[1].contiguous(),
                                          t[2].contiguous(), self.masks, t[3].contiguous(), t[5].contiguous(),
                                          self.alt_token, t[6].contiguous(), self.sample, self.truncate,
                                          self.penalty)
        b = self.bucket_for(n)
        if b not in self.graphs:
            self._capture(b)
        st = self.graphs[b].stage_for_write(self.timing)
        # host-side packing into this bucket's pinned staging buffer; padding
        # rows get slot -1 so the kernels skip them
        st[0, :n] = tokens
        st[1, :n] = slots
        st[2, :n] = positions
        st[3, :n] = mask_rows
        st[4, :n] = srcs
        st[5, :n] = alts
        st[6, :n] = prefix_rows
        return self._replay(b, n)

    @torch.inference_mode()
    def run_staged(self, rows, n: int) -> tuple:
        """:meth:`run` of rows already packed in an int32 array ``rows`` [7, >= n]
        (the native grammar engine's step buffer)."""
        b = self.bucket_for(n)
        if b not in self.graphs:
            self._capture(b)
        st = self.graphs[b].stage_for_write(self.timing)
        st[:, :n] = rows[:, :n]
        return self._replay(b, n)

    def _replay(self, b: int, n: int) -> tuple:
        bk = self.graphs[b]
        st = bk.np[bk.turn]
        if n < b:
            st[1, n:] = -1
            st[4, n:] = -1
            st[5, n:] = -1
        t0 = time.perf_counter()
        bk.inp.copy_(bk.stage[bk.turn], non_blocking=True)
        bk.copied[bk.turn].record()
        bk.turn ^= 1
        bk.graph.replay()
        self.counts["graph_replays"] += 1
        self.counts["graph_kernels"] += max(0, bk.kernels)
        self.timing["replay_s"] += time.perf_counter() - t0
        return (bk.logits[:n] if bk.logits is not None else None), bk.ids[:n]
