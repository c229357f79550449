#!/usr/bin/env python3
"""Cost of the per-head q / k RMSNorm in a decode step (GPU box).

Writes a synthetic checkpoint of Qwen3-0.6B's geometry (``--layers`` of it),
and the same tensors with the ``q_norm`` / ``k_norm`` weights dropped and
``model_type`` ``llama``: the same GEMMs without the norm.  Each is loaded,
``--ctx`` tokens are prefilled into every slot, and one decode step
(``decode_select_gather``: trunk + LM head + masked argmax) per row count is
captured into a hipGraph and replayed back to back.  Two models on one tree,
not two commits.

    python scripts/bench_qk_norm.py --rows 16,80,320
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def strip_qk_norm(src: str, dst: str) -> str:
    """``src`` without its q_norm / k_norm tensors, as a Llama-layout directory."""
    from safetensors.torch import load_file, save_file
    os.makedirs(dst, exist_ok=True)
    t = load_file(os.path.join(src, "model.safetensors"))
    save_file({k: v for k, v in t.items() if not k.endswith(("q_norm.weight", "k_norm.weight"))},
              os.path.join(dst, "model.safetensors"))
    with open(os.path.join(src, "config.json")) as f:
        cfg = json.load(f)
    cfg.update({"model_type": "llama", "architectures": ["LlamaForCausalLM"]})
    cfg.pop("layer_types", None)
    with open(os.path.join(dst, "config.json"), "w") as f:
        json.dump(cfg, f)
    return dst


def step_ms(model, rows: int, ctx: int, iters: int, reps: int) -> list:
    """Device ms per replay of the captured ``rows``-row step: ``reps`` timings of ``iters`` replays."""
    c = model.cfg
    dev = model.device
    g = torch.Generator().manual_seed(rows)
    tk = torch.randint(0, c.vocab_size, (rows,), generator=g).to(dtype=torch.int32, device=dev)
    sl = torch.arange(rows, dtype=torch.int32, device=dev)
    ps = torch.full((rows,), ctx, dtype=torch.int32, device=dev)
    src = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    last = torch.zeros(model.max_rows, dtype=torch.int32, device=dev)
    masks = torch.full((1, (c.vocab_size + 31) // 32), -1, dtype=torch.int32, device=dev)
    midx = torch.zeros(rows, dtype=torch.int32, device=dev)

    def step():
        return model.decode_select_gather(tk, src, last, sl, ps, masks, midx)[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(10):
        graph.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            graph.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16,80,320")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8", "fp8s"])
    a = ap.parse_args(argv)
    from dmcp.models.llm import LocalLM
    from dmcp.utils import synth
    rows = [int(r) for r in a.rows.split(",")]
    root = tempfile.mkdtemp(prefix="qk_norm_bench_")
    try:
        q3 = synth.llama_checkpoint(os.path.join(root, "qwen3"), layers=a.layers, hidden=1024, heads=16, kv_heads=8,
                                    intermediate=3072, vocab=151936, tokenizer="", outliers=(7, 300), qk_norm=True,
                                    model_type="qwen3", tie_embeddings=True, head_dim=128)
        plain = strip_qk_norm(q3, os.path.join(root, "plain"))
        res = {}
        for name, d in (("qk_norm", q3), ("no_norm", plain)):
            m = LocalLM.load_safetensors(d, device="cuda", max_seq=256, max_batch=max(rows), max_rows=max(rows),
                                         kv_dtype=a.kv_dtype)
            assert m.has_qk_norm == (name == "qk_norm") and m.use_fused and m.use_wgemm and m.fused_head
            g = torch.Generator().manual_seed(1)
            prompt = torch.randint(0, 151936, (a.ctx,), generator=g).tolist()
            for s in range(0, max(rows), 32):
                m.prefill_batch([(prompt, s + i, 0) for i in range(min(32, max(rows) - s))])
            for r in rows:
                res[(name, r)] = step_ms(m, r, a.ctx, a.iters, a.reps)
            del m
            torch.cuda.empty_cache()
        for r in rows:
            on, off = sorted(res[("qk_norm", r)]), sorted(res[("no_norm", r)])
            med = lambda v: v[len(v) // 2]  # noqa: E731
            print(json.dumps({"bench": "qk_norm_step", "geometry": "qwen3-0.6b", "layers": a.layers, "rows": r,
                              "ctx": a.ctx, "kv_dtype": a.kv_dtype, "iters": a.iters,
                              "qk_norm_ms": [round(x, 4) for x in on], "no_norm_ms": [round(x, 4) for x in off],
                              "qk_norm_median_ms": round(med(on), 4), "no_norm_median_ms": round(med(off), 4),
                              "delta_us_per_layer": round((med(on) - med(off)) * 1e3 / a.layers, 2)}), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
