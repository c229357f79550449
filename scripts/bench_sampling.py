"""The cost of temperature sampling in the selection kernels: each op at
temperature 0 (the greedy kernel) and at --temperature, alternated --rounds
times on one device, every timing a captured graph of --reps back-to-back
calls (no Python wrapper cost).  One JSON line per op and shape.

  python scripts/bench_sampling.py [--rows 512 610] [--vocab 128256] [--hidden 2048]

Rows <= 512 time lm_head_sample (wgemm.hip), rows above it tgemm_lm_head_sample
(tgemm.hip); --masked-rows time masked_sample over [rows, vocab] bf16 logits;
--truncated-rows time truncated_sample (csrc/truncate.hip) over the same kind
of logits with --top-k / --top-p / --min-p against masked_sample at the same
temperature (the untruncated draw), alternated the same way.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[512, 610])
    ap.add_argument("--masked-rows", type=int, nargs="*", default=[16, 64])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--truncated-rows", type=int, nargs="*", default=[])
    ap.add_argument("--top-k", type=int, default=20)
    ap.add_argument("--top-p", type=float, default=0.95)
    ap.add_argument("--min-p", type=float, default=0.0)
    ap.add_argument("--logit-scale", type=float, default=2.5, help="std of the random logits of --truncated-rows")
    ap.add_argument("--repetition-penalty", type=float, default=1.0,
                    help="with --presence-penalty: also time every op under this penalty against itself without")
    ap.add_argument("--presence-penalty", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from dmcp.ops import hip
    V, K, T = args.vocab, args.hidden, args.temperature
    W = (V + 31) // 32
    g = torch.Generator(device="cuda").manual_seed(0)
    masks = torch.randint(-2 ** 31, 2 ** 31 - 1, (8, W), device="cuda", dtype=torch.int32, generator=g)
    w = (torch.randn(V, K, device="cuda", generator=g) * 0.02).to(torch.bfloat16)

    def report(name, M, make):
        midx = torch.randint(0, 8, (M,), device="cuda", dtype=torch.int32, generator=g)
        slots = torch.randint(0, 768, (M,), device="cuda", dtype=torch.int32, generator=g)
        pos = torch.randint(0, 8192, (M,), device="cuda", dtype=torch.int32, generator=g)
        runs = {t: _timed(make(midx, slots, pos, t), args.reps) for t in (0.0, T)}
        us = {t: [] for t in runs}
        for _ in range(args.rounds):  # alternated: drift of the device shows in both columns
            for t, run in runs.items():
                us[t].append(round(run(), 2))
        med = {t: sorted(v)[len(v) // 2] for t, v in us.items()}
        print(json.dumps({"bench": name, "rows": M, "vocab": V, "hidden": K, "temperature": T,
                          "greedy_us": us[0.0], "sampled_us": us[T], "greedy_median_us": med[0.0],
                          "sampled_median_us": med[T], "added_us": round(med[T] - med[0.0], 2),
                          "greedy_spread_us": round(max(us[0.0]) - min(us[0.0]), 2)}), flush=True)

    penal = (args.repetition_penalty, args.presence_penalty) != (1.0, 0.0)
    # a half-dense history of 768 slots, every mask row penalised: the PENAL variants' worst case
    hist = torch.randint(-2 ** 31, 2 ** 31 - 1, (768, W), device="cuda", dtype=torch.int32, generator=g) \
        if penal else None

    def report_penalty(name, M, make):
        """``make(midx, slots, pos, penalty)`` at the temperature, penalty off / on alternated."""
        midx = torch.randint(0, 8, (M,), device="cuda", dtype=torch.int32, generator=g)
        slots = torch.randint(0, 768, (M,), device="cuda", dtype=torch.int32, generator=g)
        pos = torch.randint(0, 8192, (M,), device="cuda", dtype=torch.int32, generator=g)
        pen = hip.Penalty(hist, slots, args.repetition_penalty, args.presence_penalty, check_slots=False)
        runs = {"off": _timed(make(midx, slots, pos, None), args.reps),
                "on": _timed(make(midx, slots, pos, pen), args.reps)}
        us = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, run in runs.items():
                us[k].append(round(run(), 2))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        print(json.dumps({"bench": name + "+penalty", "rows": M, "vocab": V, "temperature": T,
                          "repetition_penalty": args.repetition_penalty, "presence_penalty": args.presence_penalty,
                          "off_us": us["off"], "on_us": us["on"], "off_median_us": med["off"],
                          "on_median_us": med["on"], "added_us": round(med["on"] - med["off"], 2),
                          "off_spread_us": round(max(us["off"]) - min(us["off"]), 2)}), flush=True)

    for M in args.rows:
        x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        out = torch.empty(M, dtype=torch.int32, device="cuda")
        if M <= hip.WGEMM_MAX_ROWS:
            ws = hip.lm_head_workspace(V, "cuda", M)
            report("lm_head_sample", M, lambda mi, s, p, t: lambda: hip.lm_head_sample(
                x, w, masks, mi, out, ws, s, p, t, 1))
            if penal:
                report_penalty("lm_head_sample", M, lambda mi, s, p, pn: lambda: hip.lm_head_sample(
                    x, w, masks, mi, out, ws, s, p, T, 1, penalty=pn))
        else:
            ws = torch.empty(2 * (V // 64) * M, dtype=torch.float32, device="cuda")
            report("tgemm_lm_head_sample", M, lambda mi, s, p, t: lambda: hip.tgemm_lm_head_sample(
                x, w, masks, mi, out, ws, 0, s, p, t, 1))
            if penal:
                report_penalty("tgemm_lm_head_sample", M, lambda mi, s, p, pn: lambda: hip.tgemm_lm_head_sample(
                    x, w, masks, mi, out, ws, 0, s, p, T, 1, penalty=pn))
    for B in args.masked_rows:
        logits = torch.randn(B, V, device="cuda", generator=g).to(torch.bfloat16)
        out = torch.empty(B, dtype=torch.int32, device="cuda")
        report("masked_sample", B, lambda mi, s, p, t: lambda: hip.masked_sample(
            logits, masks, V, out, mi, s, p, t, 1))
        if penal:
            report_penalty("masked_sample", B, lambda mi, s, p, pn: lambda: hip.masked_sample(
                logits, masks, V, out, mi, s, p, T, 1, penalty=pn))
    for B in args.truncated_rows:
        logits = (torch.randn(B, V, device="cuda", generator=g) * args.logit_scale).to(torch.bfloat16)
        out = torch.empty(B, dtype=torch.int32, device="cuda")
        midx = torch.randint(0, 8, (B,), device="cuda", dtype=torch.int32, generator=g)
        slots = torch.randint(0, 768, (B,), device="cuda", dtype=torch.int32, generator=g)
        pos = torch.randint(0, 8192, (B,), device="cuda", dtype=torch.int32, generator=g)
        runs = {"masked_sample": _timed(lambda: hip.masked_sample(logits, masks, V, out, midx, slots, pos, T, 1),
                                        args.reps),
                "truncated_sample": _timed(lambda: hip.truncated_sample(
                    logits, masks, V, out, midx, slots, pos, T, 1, args.top_k, args.top_p, args.min_p), args.reps)}
        us = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, run in runs.items():
                us[k].append(round(run(), 2))
        med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
        if penal:
            report_penalty("truncated_sample", B, lambda mi, s, p, pn: lambda: hip.truncated_sample(
                logits, masks, V, out, mi, s, p, T, 1, args.top_k, args.top_p, args.min_p, penalty=pn))
        print(json.dumps({"bench": "truncated_sample", "rows": B, "vocab": V, "temperature": T, "top_k": args.top_k,
                          "top_p": args.top_p, "min_p": args.min_p, "logit_scale": args.logit_scale,
                          "masked_sample_us": us["masked_sample"], "truncated_sample_us": us["truncated_sample"],
                          "masked_sample_median_us": med["masked_sample"],
                          "truncated_sample_median_us": med["truncated_sample"],
                          "row_bytes_read_per_call": 2 * V * (2 + 4 * bool(0 < args.top_k) + 4 * (args.top_p < 1))}),
              flush=True)


if __name__ == "__main__":
    main()
