#!/usr/bin/env python3
"""Microbenchmark of the row-scaled FP8 linears (csrc/gemm_fp8.hip) on one MI355X -> profiles/fp8_linear.txt.

For the eight Mistral-7B products (forward and data gradient of qkv, o, gate|up, down) at 4096 and 16384 rows:
  (a) gemm_fp8_nt alone against what linear_fwd / linear_dgrad run for the shape (the 16-bit path, W^T cached);
  (b) the same with the activation quantisation (fp8_quant_rows of the rows) included;
  (c) the weight quantisation of the shape (W, or the 16-bit W^T), paid once per optimizer step.
One process; every call is timed with device events around ``--iters`` launches, the candidates of a shape are
interleaved inside every round, and each cycles through a ring of operand sets larger than the 256 MiB last-level
cache, so no call finds its operands cached by its predecessor.  Reported: the median of ``--rounds`` (>= 7) rounds
with min..max.  The end-to-end comparisons (M7B_narrow with and without --fp8-linear, bench.py against the parent
build) are harness / bench.py runs and are not made here.

Usage:  python scripts/bench_fp8_linear.py [--rows 4096 16384] [--rounds 7] [--iters 4] [--out profiles/fp8_linear.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dltb  # noqa: E402,F401
from dltb.ops import functional as F_  # noqa: E402

D, F, KV = 4096, 14336, 1024
# (name, N, K) of c[M, N] = a[M, K] b[N, K]^T: the forward uses W [N, K], the data gradient W^T
PRODUCTS = [("qkv.fwd", D + 2 * KV, D), ("o.fwd", D, D), ("gateup.fwd", 2 * F, D), ("down.fwd", D, F),
            ("qkv.dgrad", D, D + 2 * KV), ("o.dgrad", D, D), ("gateup.dgrad", D, 2 * F), ("down.dgrad", F, D)]
LLC = 256 << 20


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us per call


def bench_shape(M, N, K, rounds, iters, dev):
    per_set = 2 * (M * K + N * K + M * N)       # bytes of one 16-bit operand set
    ring = max(2, -(-2 * LLC // per_set))
    xs = [torch.randn(M, K, device=dev).bfloat16() for _ in range(ring)]
    ws = [torch.randn(N, K, device=dev).bfloat16() for _ in range(ring)]
    xq = [F_.fp8_quant_rows(x) for x in xs]
    wq = [F_.fp8_quant_rows(w) for w in ws]

    def gemm16(i):          # linear_fwd on W; a data gradient with its cached W^T runs the same dispatch on W^T
        return F_.linear_fwd(xs[i % ring], ws[i % ring])

    def gemm8(i):
        j = i % ring
        return F_.gemm_fp8_nt(xq[j][0], xq[j][1], wq[j][0], wq[j][1])

    def gemm8_q(i):
        j = i % ring
        qa, sa = F_.fp8_quant_rows(xs[j])
        return F_.gemm_fp8_nt(qa, sa, wq[j][0], wq[j][1])

    def quant_w(i):
        return F_.fp8_quant_rows(ws[i % ring])

    cands = [("16-bit", gemm16), ("fp8 gemm", gemm8), ("fp8 quant+gemm", gemm8_q), ("weight quant", quant_w)]
    for _, fn in cands:                         # warm every candidate on every operand set
        for i in range(ring):
            fn(i)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cands}
    for _ in range(rounds):
        for name, fn in cands:
            times[name].append(timed(fn, max(iters, ring)))
    return ring, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "fp8_linear.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp8_linear.py measures on the GPU; none found")
    if a.rounds < 7:
        raise SystemExit("--rounds must be at least 7")
    dev = torch.device("cuda:0")
    lines = [f"# scripts/bench_fp8_linear.py on {torch.cuda.get_device_name(0)}: us per call, median of {a.rounds} "
             f"rounds (min..max); TFLOP/s = 2 M N K / median",
             "# product            M     N     K  ring | 16-bit | fp8 gemm (a) | fp8 quant+gemm (b) | weight quant (c)"]
    for M in a.rows:
        for name, N, K in PRODUCTS:
            ring, t = bench_shape(M, N, K, a.rounds, a.iters, dev)
            cells = []
            for key in ("16-bit", "fp8 gemm", "fp8 quant+gemm", "weight quant"):
                med, lo, hi = t[key]
                rate = "" if key == "weight quant" else f" {2.0 * M * N * K / med / 1e6:7.1f} TF"
                cells.append(f"{med:8.1f} ({lo:.1f}..{hi:.1f}){rate}")
            lines.append(f"{name:14s} {M:6d} {N:5d} {K:5d} {ring:4d} | " + " | ".join(cells))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"fp8 GEMM launches: {F_.fp8_gemm_calls}; wrote {a.out}")


if __name__ == "__main__":
    main()
