#!/usr/bin/env python3
"""Fused AdamW launch time at TinyGPT-A size (236.4M fp32 master / moments, bf16 gradient and parameter copy).

    python scripts/bench_adamw.py [--n 236406784] [--iters 20]
    python scripts/bench_adamw.py --state fp8 [--n N] [--rounds 7] [--ring 2] [--out FILE]

Bytes moved per element: read master, m, v (12) + bf16 grad (2), write master, m, v (12) + bf16 param (2).

``--state fp8`` times the block-scaled FP8 state (``adamw_fp8_kernel``: 4 + 1 + 1 + 2 bytes read, 4 + 1 + 1 + 2
written, plus 2 x 4 bytes of scales per 256 elements each way: 16.06 B per element) against the fp32 state in one
process: the two kinds' launches interleaved, each on the next optimizer of its own ring (``--ring`` sets of buffers,
every set larger than the last-level cache), medians over ``--rounds`` rounds and the fp32 call's min..max spread."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dltb  # noqa: E402,F401
from dltb.optim.adamw import FlatAdamW  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=236406784)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--state", choices=["fp32", "fp8"], default="fp32")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--ring", type=int, default=2)
ap.add_argument("--out", default=None, help="append the result lines to this file")
a = ap.parse_args()
n = a.n
g = torch.randn(n, device="cuda").to(torch.bfloat16)
gs = torch.ones(1, device="cuda")


def make(state):
    master = torch.randn(n, device="cuda")
    dst = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    return FlatAdamW(master, [(0, n, dst)], lr=1e-4, state=state, seed=1)


def timed(opt):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    opt.prepare(1e-4)
    s.record()
    opt.launch(g, gs)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


if a.state == "fp32":
    opt = make("fp32")
    for _ in range(3):
        opt.step(g, 1e-4, gs)
    torch.cuda.synchronize()
    ts = sorted(timed(opt) for _ in range(a.iters))
    med = ts[len(ts) // 2]
    print(f"adamw n={n}: median {med:.1f} us, min {ts[0]:.1f} us, "
          f"{28 * n / med / 1e6:.2f} TB/s (28 B/elem)", flush=True)
    sys.exit(0)

rings = {k: [make(k) for _ in range(a.ring)] for k in ("fp32", "fp8")}
for ring in rings.values():
    for opt in ring:
        for _ in range(2):
            opt.step(g, 1e-4, gs)
torch.cuda.synchronize()
ts = {"fp32": [], "fp8": []}
for r in range(a.rounds):
    for i in range(a.ring):
        for k in ("fp8", "fp32") if r % 2 else ("fp32", "fp8"):
            ts[k].append(timed(rings[k][i]))
bytes_per = {"fp32": 28.0, "fp8": 16.0 + 2 * 2 * 4 / 256}
lines = []
med = {}
for k in ("fp32", "fp8"):
    v = sorted(ts[k])
    med[k] = v[len(v) // 2]
    lines.append(f"adamw state={k} n={n}: median {med[k]:.1f} us, min {v[0]:.1f} us, max {v[-1]:.1f} us over "
                 f"{len(v)} launches, {bytes_per[k] * n / med[k] / 1e6:.2f} TB/s ({bytes_per[k]:.2f} B/elem)")
lines.append(f"fp8 / fp32 median time: {med['fp8'] / med['fp32']:.3f}")
for ln in lines:
    print(ln, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
