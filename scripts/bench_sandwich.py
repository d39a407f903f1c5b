#!/usr/bin/env python3
"""--sandwich-norm / --ffn-act: the fused sandwich-norm calls against what the existing kernels need for the same
result, and the GeGLU instantiations of the gated-FFN kernels against the SiLU ones.  One GPU, bf16.

    python scripts/bench_sandwich.py            # appends to profiles/sandwich_norm.txt

Row shapes d = 4096 (M7B) and d = 1024 at 4096 and 16384 rows.  Every call works on the next buffer set of a ring
whose sets together exceed the last-level cache (--ring-mb, default 1024), so no call finds its operands cached.
Medians of --rounds (7) interleaved rounds: in a round every variant runs once, one after the other.

    forward, attention site:  sandwich_fwd(x, a, w_out, w_next)   against  norm_fwd(a, None, w_out); norm_fwd(x, n, w_next)
    forward, FFN site:        sandwich_fwd(x, a, w_out, None)     against  norm_fwd(a, None, w_out); dropout(x, n, p = 0)
    backward, attention site: F_.sandwich_bwd(...)                against  two norm_bwd calls (at d > 2048 both ARE the
                              two calls: the fused kernel stops at 2048)
    gated FFN (F = 14336 and 4096): swiglu_fwd / _bwd / _bwd_h with act = geglu against act = silu

A fused line also says whether its median is above the composition's median by more than the composition's own
min..max spread in this run.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dltb  # noqa: E402,F401
from dltb.ops import functional as F_  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-5


def timed(fn, sets, iters):
    """Seconds per call of fn(set) over ``iters`` calls that walk the ring round and round: a set comes up again only
    after every other set of the ring (more than the last-level cache) has been used."""
    for k in range(min(3, len(sets))):
        fn(sets[k])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(sets[k % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def compare(out, title, variants, sets, rounds, iters, byts):
    """``variants``: [(name, fn)], the first the composition of existing kernels.  Interleaved rounds."""
    times = {n: [] for n, _ in variants}
    for _ in range(rounds):
        for n, fn in variants:
            times[n].append(timed(fn, sets, iters))
    base = times[variants[0][0]]
    bmed, spread = statistics.median(base), max(base) - min(base)
    out.append(f"## {title}")
    for n, _ in variants:
        t = times[n]
        med = statistics.median(t)
        line = (f"{n}\tmedian {med * 1e6:.1f} us\tmin {min(t) * 1e6:.1f}\tmax {max(t) * 1e6:.1f}\t"
                f"ratio to the first {med / bmed:.3f}")
        if n in byts:
            line += f"\t{byts[n] / 1e6:.1f} MB\t{byts[n] / med / 1e12:.2f} TB/s"
        if n != variants[0][0]:
            line += f"\tabove the first by more than its spread ({spread * 1e6:.1f} us): {med - bmed > spread}"
        out.append(line)


def norm_sets(N, d, ring_mb):
    per = 8 * N * d * 2
    n = max(2, -(-ring_mb * (1 << 20) // per))
    g = torch.Generator(DEV).manual_seed(1)
    sets = []
    for _ in range(n):
        x, a, dy, dres = (torch.randn(N, d, device=DEV, generator=g).to(BF16) for _ in range(4))
        w_out = (1 + 0.5 * torch.randn(d, device=DEV, generator=g)).to(BF16)
        w_next = (1 + 0.5 * torch.randn(d, device=DEV, generator=g)).to(BF16)
        s, _, rstd_a, rstd_s = F_.sandwich_fwd(x, a, w_out, w_next, EPS)
        sets.append(dict(x=x, a=a, dy=dy, dres=dres, w_out=w_out, w_next=w_next, s=s, rstd_a=rstd_a, rstd_s=rstd_s,
                         g0=torch.zeros(d, device=DEV, dtype=BF16), g1=torch.zeros(d, device=DEV, dtype=BF16)))
    return sets


def bench_norms(out, N, d, a):
    sets = norm_sets(N, d, a.ring_mb)
    row = N * d * 2

    def two_fwd(b):
        _, n, _, _ = F_.norm_fwd(b["a"], None, b["w_out"], None, EPS, True)
        F_.norm_fwd(b["x"], n, b["w_next"], None, EPS, True)

    def two_fwd_ffn(b):
        _, n, _, _ = F_.norm_fwd(b["a"], None, b["w_out"], None, EPS, True)
        F_.dropout(b["x"], n, 0.0, None, 0)

    def two_bwd(b):
        red = F_.GradReducer()
        dx = F_.norm_bwd(b["dy"], b["s"], b["w_next"], None, b["rstd_s"], b["dres"], b["g0"], None, False, True, red=red)
        F_.norm_bwd(dx, b["a"], b["w_out"], None, b["rstd_a"], None, b["g1"], None, False, True, red=red)
        red.flush()

    def fused_bwd(b):
        red = F_.GradReducer()
        F_.sandwich_bwd(b["dy"], b["s"], b["w_next"], b["rstd_s"], b["dres"], b["a"], b["w_out"], b["rstd_a"],
                        (b["g0"], False), (b["g1"], False), red)
        red.flush()

    tag = f"N={N} d={d} bf16, ring of {len(sets)} sets"
    compare(out, f"forward, attention site, {tag}",
            [("norm_fwd(a) + norm_fwd(x, n)", two_fwd),
             ("sandwich_fwd(x, a, w_out, w_next)", lambda b: F_.sandwich_fwd(b["x"], b["a"], b["w_out"], b["w_next"], EPS))],
            sets, a.rounds, a.iters, {"norm_fwd(a) + norm_fwd(x, n)": 6 * row, "sandwich_fwd(x, a, w_out, w_next)": 4 * row})
    compare(out, f"forward, FFN site, {tag}",
            [("norm_fwd(a) + add", two_fwd_ffn),
             ("sandwich_fwd(x, a, w_out, None)", lambda b: F_.sandwich_fwd(b["x"], b["a"], b["w_out"], None, EPS))],
            sets, a.rounds, a.iters, {"norm_fwd(a) + add": 5 * row, "sandwich_fwd(x, a, w_out, None)": 3 * row})
    fused = F_.sandwich_bwd_fused(sets[0]["dy"])
    compare(out, f"backward, attention site, {tag}" + ("" if fused else " (d > 2048: F_.sandwich_bwd runs the two calls)"),
            [("two norm_bwd", two_bwd), ("F_.sandwich_bwd", fused_bwd)], sets, a.rounds, a.iters,
            {"two norm_bwd": 7 * row, "F_.sandwich_bwd": (6 if fused else 7) * row})


def bench_glu(out, N, F, a):
    per = 5 * N * F * 2
    n = max(2, -(-a.ring_mb * (1 << 20) // per))
    g = torch.Generator(DEV).manual_seed(2)
    sets = [dict(gu=torch.randn(N, 2 * F, device=DEV, generator=g).to(BF16),
                 dh=torch.randn(N, F, device=DEV, generator=g).to(BF16)) for _ in range(n)]
    tag = f"N={N} F={F} bf16, ring of {len(sets)} sets"
    unit = N * F * 2
    for name, fn, nb in (("swiglu_fwd", lambda b, act: F_.swiglu_fwd(b["gu"], act), 3),
                         ("swiglu_bwd", lambda b, act: F_.swiglu_bwd(b["dh"], b["gu"], act), 5),
                         ("swiglu_bwd_h", lambda b, act: F_.swiglu_bwd_h(b["dh"], b["gu"], act), 6)):
        compare(out, f"{name}, {tag}",
                [(f"{name} silu", lambda b, fn=fn: fn(b, "silu")), (f"{name} geglu", lambda b, fn=fn: fn(b, "geglu"))],
                sets, a.rounds, a.iters, {f"{name} silu": nb * unit, f"{name} geglu": nb * unit})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--ring-mb", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sandwich_norm.txt"))
    a = ap.parse_args()
    out = [f"# scripts/bench_sandwich.py, {time.strftime('%Y-%m-%d %H:%M:%S')}, {torch.cuda.get_device_name(0)}, "
           f"rounds {a.rounds}, iters {a.iters}, ring {a.ring_mb} MB"]
    for d in (4096, 1024):
        for N in (4096, 16384):
            bench_norms(out, N, d, a)
            torch.cuda.empty_cache()
    for F in (14336, 4096):
        bench_glu(out, 4096, F, a)
        torch.cuda.empty_cache()
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(text)


if __name__ == "__main__":
    main()
