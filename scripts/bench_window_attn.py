#!/usr/bin/env python3
"""One layer's decode attention with and without a sliding window (GPU box).

``--rows`` rows of live length ``--len`` over an fp8 / bf16 cache of
Llama-3.2-1B's head geometry, each in its own slot, the model's split plan
(``ops.decode_plan``): the windowed call (``--window``) against the same call
unwindowed, device time per launch from events around ``--iters`` launches.
Prints one JSON line.

    python scripts/bench_window_attn.py --rows 512 --len 6000 --window 4096 --kv-dtype fp8
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--len", type=int, default=6000, dest="length")
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--max-seq", type=int, default=8192)
    ap.add_argument("--kv-dtype", default="fp8", choices=["bf16", "fp8"])
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args(argv)
    from dmcp import ops
    from dmcp.ops import hip
    dev = torch.device("cuda")
    B, Hq, Hkv, D, MAXS = a.rows, a.heads, a.kv_heads, a.head_dim, a.max_seq
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (B, Hkv, MAXS, D)
    if a.kv_dtype == "fp8":
        kc = torch.randint(0, 120, shape, generator=g, device=dev, dtype=torch.uint8)  # finite e4m3 bytes
        vc = torch.randint(0, 120, shape, generator=g, device=dev, dtype=torch.uint8)
    else:
        kc = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)
        vc = torch.randn(shape, generator=g, device=dev).to(torch.bfloat16)
    q = torch.randn(B, Hq, D, generator=g, device=dev).to(torch.bfloat16)
    slot = torch.arange(B, dtype=torch.int32, device=dev)
    lens = torch.full((B,), a.length, dtype=torch.int32, device=dev)
    chunk, splits = ops.decode_plan(B, Hkv, MAXS, a.kv_dtype)
    ws = hip.decode_workspace(B, Hq, Hkv, D, MAXS, dev, chunk)
    out = torch.empty_like(q)

    def timed(window):
        def run():
            hip.decode_attention(q, kc, vc, slot, lens, D ** -0.5, workspace=ws, chunk=chunk, out=out,
                                 splits=splits, window=window)
        for _ in range(a.warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters * 1e3  # us per launch

    runs = [(w, timed(w)) for w in (0, a.window, 0, a.window)]  # alternated, two each
    full = [t for w, t in runs if w == 0]
    win = [t for w, t in runs if w]
    elem = 1 if a.kv_dtype == "fp8" else 2
    print(json.dumps({"rows": B, "len": a.length, "window": a.window, "kv_dtype": a.kv_dtype, "chunk": chunk,
                      "splits": splits, "full_us": [round(t, 1) for t in full], "window_us": [round(t, 1) for t in win],
                      "time_ratio": round(sum(win) / sum(full), 4),
                      "kv_bytes_ratio": round(min(a.window, a.length) / a.length, 4),
                      "full_kv_gb": round(2 * B * Hkv * a.length * D * elem / 1e9, 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
