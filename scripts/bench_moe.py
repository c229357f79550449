#!/usr/bin/env python
"""One layer's routed expert MLP (ops.moe_mlp, csrc/moe.hip) at the
Qwen3-30B-A3B geometry (hidden 2,048, expert width 768, 128 experts, 8 per
token) against the bf16 torch per-expert loop (index_select + F.linear +
weighted index_add_) in the same process.

    python scripts/bench_moe.py [--rows 16,64,320,768,4096] [--iters 20] [--out profiles/moe_r7.jsonl]
                                [--weights {bf16,fp8}] [--dequantised]

``--weights fp8`` runs ops.moe_mlp_w8 over the same draws quantised to the
block-scaled FP8 layout (ops.block_fp8_quant: e4m3 + one fp32 scale per
128 x 128 block; 0.61 GB of experts); the torch loop then runs on the weights
dequantised and rounded to bf16.  ``--weights bf16 --dequantised`` runs the
bf16 kernel on those dequantised weights: the pair to alternate when the two
formats are compared.

Per row count: warm-up, then the median of ``--iters`` timings between events
on one stream; one JSON line each with both times and the bytes/s the kernel
achieved against the layer's expert weights (E x 3 x I x H bf16 = 1.21 GB;
at few rows not every expert is touched, so ``touched_gb`` is reported too).
``max_rel_diff_vs_loop`` compares the two outputs under the kernel's routing
(max |difference| over max |loop output|; both round to bf16, the loop after
every GEMM).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, I, E, K = 2048, 768, 128, 8


def torch_loop(h, wr, wgu, wd, route=None):
    """``route`` = (ids, p) replaces the loop's own routing (bf16 router
    logits, which choose other experts than the kernel's fp32 ones on rows
    with a near tie) when outputs are compared; the timed loop routes itself."""
    if route is None:
        logits = F.linear(h, wr).float()
        p, ids = torch.softmax(logits, -1).topk(K, dim=-1)
        p = p / p.sum(-1, keepdim=True)
    else:
        ids, p = route[0].long(), route[1]
    p = p.to(h.dtype)
    out = torch.zeros_like(h)
    for e in ids.unique().tolist():
        rows, rank = (ids == e).nonzero(as_tuple=True)
        x = h.index_select(0, rows)
        gu = F.linear(x, wgu[e])
        y = F.linear(F.silu(gu[:, :I]) * gu[:, I:], wd[e])
        out.index_add_(0, rows, y * p[rows, rank][:, None])
    return out, ids


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16,64,320,768,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--weights", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--dequantised", action="store_true",
                    help="bf16 weights = the block-scaled FP8 quantisation of the draws, dequantised")
    a = ap.parse_args()
    from dmcp import ops
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, std):
        return (torch.randn(*shape, generator=g, device="cuda") * std).to(torch.bfloat16)
    wr, wgu, wd = rnd(E, H, std=2 / H ** 0.5), rnd(E, 2 * I, H, std=H ** -0.5), rnd(E, H, I, std=I ** -0.5)
    rows = [int(r) for r in a.rows.split(",")]
    ws = ops.moe_workspace(max(rows), H, I, E, K, "cuda")
    weight_bytes = E * 3 * I * H * 2
    expert_bytes = 3 * I * H * 2
    w8 = None
    if a.weights == "fp8" or a.dequantised:
        g8, gs = ops.block_fp8_quant(wgu[:, :I])
        u8, us = ops.block_fp8_quant(wgu[:, I:])
        d8, ds = ops.block_fp8_quant(wd)
        w8 = (torch.cat([g8, u8], 1), torch.cat([gs, us], 1), d8, ds)
        wgu, wd = ops.reference.moe_w8_dequant(*w8, dtype=torch.bfloat16)
        del g8, u8, d8
    if a.weights == "fp8":
        scale_bytes = 4 * (w8[1][0].numel() + w8[3][0].numel())
        expert_bytes = 3 * I * H + scale_bytes
        weight_bytes = E * expert_bytes

        def run(h, out):
            return ops.moe_mlp_w8(h, wr, *w8, K, True, workspace=ws, out=out)
    else:
        w8 = None

        def run(h, out):
            return ops.moe_mlp(h, wr, wgu, wd, K, True, workspace=ws, out=out)
    lines = []
    for T in rows:
        h = rnd(T, H, std=1.0)
        out = torch.empty_like(h)
        # compared under the kernel's own routing: the figure is then the two
        # GEMM pipelines' bf16 rounding, not rows that chose other experts
        ref, ids = torch_loop(h, wr, wgu, wd, ops.moe_route(h, wr, K, True))
        got = run(h, out)
        err = ((got.float() - ref.float()).abs().max() / ref.float().abs().max()).item()
        touched = ids.unique().numel() * expert_bytes
        k_med, k_min = timed(lambda: run(h, out), a.iters)
        l_med, l_min = timed(lambda: torch_loop(h, wr, wgu, wd), max(3, a.iters // 4), warmup=2)
        rec = {"bench": "moe_mlp" if a.weights == "bf16" else "moe_mlp_w8", "weights": a.weights,
               "dequantised": bool(a.dequantised or a.weights == "fp8"), "rows": T, "hidden": H, "inter": I, "experts": E, "top_k": K,
               "kernel_us": round(k_med, 1), "kernel_min_us": round(k_min, 1), "torch_loop_us": round(l_med, 1),
               "torch_loop_min_us": round(l_min, 1), "speedup": round(l_med / k_med, 2),
               "weights_gb": round(weight_bytes / 1e9, 3), "touched_gb": round(touched / 1e9, 3),
               "kernel_tb_s_touched": round(touched / k_med / 1e6, 3), "max_rel_diff_vs_loop": round(err, 4),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
