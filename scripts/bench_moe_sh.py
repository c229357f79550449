#!/usr/bin/env python
"""What the shared pseudo-expert costs: one layer's routed MLP at H 2,048,
I 768, E 128, k 8 (scripts/bench_moe.py's geometry) on ops.moe_mlp (softmax
router) and on ops.moe_mlp_sh (sigmoid router) with S = 0 and S = 1, the three
alternated per row count in one process.

    python scripts/bench_moe_sh.py [--rows 16,64,320,768,4096] [--iters 20] [--out FILE.jsonl]

scripts/bench_moe.py's method: warm-up, then the median of ``--iters`` timings
between events on one stream.  With S = 1 every row has one more pair and the
shared slice is one group holding all the rows (``shared_gflop`` is its share
of the work); one JSON line per row count.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_moe import E, H, I, K, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16,64,320,768,4096")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from dmcp import ops
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, std):
        return (torch.randn(*shape, generator=g, device="cuda") * std).to(torch.bfloat16)
    wr, wgu, wd = rnd(E, H, std=2 / H ** 0.5), rnd(E + 1, 2 * I, H, std=H ** -0.5), rnd(E + 1, H, I, std=I ** -0.5)
    wgu0, wd0 = wgu[:E].contiguous(), wd[:E].contiguous()
    bias = 0.1 * torch.randn(E, generator=g, device="cuda")
    rows = [int(r) for r in a.rows.split(",")]
    ws = ops.moe_sh_workspace(max(rows), H, I, E, K, 1, "cuda")
    lines = []
    for T in rows:
        h = rnd(T, H, std=1.0)
        out = torch.empty_like(h)
        runs = {"moe_mlp_us": lambda: ops.moe_mlp(h, wr, wgu0, wd0, K, True, workspace=ws, out=out),
                "moe_mlp_sh_s0_us": lambda: ops.moe_mlp_sh(h, wr, bias, wgu0, wd0, K, True, 1.0, 0, workspace=ws,
                                                           out=out),
                "moe_mlp_sh_s1_us": lambda: ops.moe_mlp_sh(h, wr, bias, wgu, wd, K, True, 1.0, 1, workspace=ws,
                                                           out=out)}
        best = {k: [] for k in runs}
        for _ in range(3):  # alternated: three passes over the three ops
            for k, fn in runs.items():
                best[k].append(timed(fn, a.iters)[0])
        rec = {"bench": "moe_mlp_sh", "rows": T, "hidden": H, "inter": I, "experts": E, "top_k": K,
               **{k: round(sorted(v)[1], 1) for k, v in best.items()},
               "shared_gflop": round(6 * T * I * H / 1e9, 2), "routed_gflop": round(6 * T * K * I * H / 1e9, 2),
               "device": torch.cuda.get_device_name(0)}
        rec["s1_minus_s0_us"] = round(rec["moe_mlp_sh_s1_us"] - rec["moe_mlp_sh_s0_us"], 1)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
