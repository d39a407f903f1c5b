#!/usr/bin/env python3
"""Isolated timing of the tied head's data gradient dX = g * dL W on the GPU.

One process, HIP events, every variant of a shape warmed up first and then timed in interleaved
rounds (variant 1, 2, ..., n, then again), so clock and neighbour drift hit all variants alike.
Per (dtype, M, V, d) it times

  torch      the parent expression  (torch.mm(dl, w) * g).to(dtype)
  nn c/s     the own NN-layout kernel (csrc/gemm_nn.hip), tile config c (0 = 128x128, 1 = 256x128,
             2 = 64x64) with s K-splits
  plan       what head_dgrad dispatches (functional._head_nn_plan)
  cached_wt  bf16 only, as context: head_dgrad with a cached W^T (hipBLASLt table / own NT kernel)

and prints median / min microseconds over the rounds, the spread of the median's neighbours, and
each result's max error against the fp32 product.

  python scripts/bench_head_dgrad.py [--rounds 20] [--shapes 2048x32000x1024,...] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dltb  # noqa: E402,F401
from dltb.ops import functional as F_  # noqa: E402
from dltb.ops._ext import ext  # noqa: E402

TILES = {0: (128, 128), 1: (256, 128), 2: (64, 64)}


def variants(dl, w, wt, g):
    C = ext()
    M, K = dl.shape
    N = w.shape[1]
    out = [("torch", lambda: (torch.mm(dl, w) * g).to(dl.dtype))]
    for cfg, (bm, bn) in TILES.items():
        if not C.gemm_nn_supported(M, N, K, cfg):
            continue
        tiles = (M // bm) * (N // bn)
        for s in (1, 2, 4, 8, 16):
            if tiles * s < 64 or tiles * s > 1024 or (s > 1 and tiles >= 256):
                continue            # far from filling, or far past, the 256 CUs
            out.append((f"nn {cfg}/{s}", lambda cfg=cfg, s=s: C.gemm_nn(dl, w, None, s, cfg, 1, g)))
    plan = F_._head_nn_plan(dl, w, g)
    if plan is not None:
        out.append((f"plan={plan[0]}/{plan[1]}", lambda: F_.head_dgrad(dl, w, None, g)))
    if wt is not None:
        out.append(("cached_wt", lambda: F_.head_dgrad(dl, w, wt, g)))
    return out


def bench_shape(M, V, d, dtype, rounds, inner, emit):
    torch.manual_seed(0)
    dl = (torch.randn(M, V, device="cuda") * 0.5).to(dtype)
    w = (torch.randn(V, d, device="cuda") * 0.5).to(dtype)
    g = torch.tensor([0.37], device="cuda")
    wt = w.t().contiguous() if dtype == torch.bfloat16 else None
    want = (dl.float() @ w.float()) * 0.37
    vs = variants(dl, w, wt, g)
    errs = {}
    for name, fn in vs:                       # warm-up + correctness
        for _ in range(3):
            y = fn()
        errs[name] = (y.float() - want).abs().max().item()
    del want
    torch.cuda.synchronize()
    times = {name: [] for name, _ in vs}
    for _ in range(rounds):
        for name, fn in vs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    flop = 2.0 * M * V * d
    tag = str(dtype).replace("torch.", "")
    emit(f"## {tag}  M={M} V={V} d={d}  ({flop / 1e9:.0f} GFLOP; {rounds} interleaved rounds x {inner} calls)")
    base = sorted(times["torch"])[rounds // 2]
    for name, _ in vs:
        t = sorted(times[name])
        med = t[rounds // 2]
        emit(f"  {name:14s} median {med:9.1f} us  min {t[0]:9.1f}  p25-p75 {t[rounds // 4]:9.1f}-{t[3 * rounds // 4]:9.1f}"
             f"  {flop / med / 1e6:7.1f} TFLOP/s  x{base / med:5.2f} vs torch  max|err| {errs[name]:.3g}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed event pair")
    ap.add_argument("--shapes", default="2048x32000x1024,8192x32000x1024,4096x32000x4096")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_head_dgrad: needs the GPU (a CPU timing says nothing about it)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# head dgrad dX = g dL W, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    for shape in a.shapes.split(","):
        M, V, d = (int(x) for x in shape.split("x"))
        for dt in a.dtypes.split(","):
            bench_shape(M, V, d, {"bf16": torch.bfloat16, "fp16": torch.float16}[dt], a.rounds, a.inner, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
