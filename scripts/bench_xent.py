#!/usr/bin/env python3
"""Head-loss kernel microbenchmark: the option kernels of csrc/xent.hip against the plain ones.

    python scripts/bench_xent.py [--rows 4096,16384] [--vocab 32000] [--iters 20] [--rounds 7]
                                 [--out FILE]     (default: profiles/xent_softcap.txt)

Times the fused forward + backward, ``xent_lse`` and ``xent_bwd_lse_`` in bf16, plain and with final-logit
soft-capping at ``--cap`` (30), with the z-loss coefficient ``--z-coef`` (1e-4), and with both, in one process.  Every
call of a timed loop takes the next logits buffer of a ring whose total size is at least ``--ring-gib`` (1 GiB, four
times the 256 MiB last-level cache) and never fewer than two buffers, so no call finds its rows in a cache.  The twelve
calls alternate over ``--rounds`` rounds of ``--iters`` calls after a warm-up round; the median round is reported
with the min .. max of the rounds, the ratio to the plain call's median, and the plain call's own min .. max spread
as a ratio beside it.  Bytes: 2 per element read plus, for the two in-place kernels, 2 written.  The in-place kernels
run on their own previous output once the ring has gone round; their instruction streams do not depend on the values.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dltb  # noqa: E402,F401
from dltb.ops import functional as F_  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3   # us


def run_shape(N, V, cap, zc, iters, rounds, ring_bytes, emit):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(N + V)
    nbuf = max(2, -(-ring_bytes // (N * V * 2)))
    ring = [(torch.randn(N, V, device=dev, generator=g) * 2.0).to(torch.bfloat16) for _ in range(nbuf)]
    t = torch.randint(0, V, (N,), device=dev, generator=g)
    t[::7] = -1
    loss = torch.empty(N, device=dev)
    lse = torch.empty(N, device=dev)
    pos = [0]

    def nxt():
        pos[0] = (pos[0] + 1) % nbuf
        return ring[pos[0]]
    variants = {"plain": {}, f"cap{cap:g}": dict(softcap=cap), f"z{zc:g}": dict(z_coef=zc),
                "both": dict(softcap=cap, z_coef=zc)}
    fns = {}
    for name, kw in variants.items():
        fns["fused", name] = lambda kw=kw: F_.xent_fwd_bwd_(nxt(), t, -1, **kw)
        fns["lse", name] = lambda kw=kw: F_.xent_lse(nxt(), t, -1, loss, lse, **kw)
        fns["bwd_lse", name] = lambda kw=kw: F_.xent_bwd_lse_(nxt(), t, lse, -1, **kw)
    F_.xent_lse(ring[0], t, -1, loss, lse)          # a log-sum-exp of real rows for the bwd_lse calls
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                     # round 0 warms up; the twelve calls alternate
        for key, fn in fns.items():
            us = timed(fn, iters)
            if r:
                times[key].append(us)
    emit(f"## {N} rows x V {V} bf16, ring of {nbuf} buffers ({nbuf * N * V * 2 / 2 ** 20:.0f} MiB)")
    out = {}
    for kern, nbytes in (("fused", 4), ("lse", 2), ("bwd_lse", 4)):
        tp = times[kern, "plain"]
        mp = sorted(tp)[len(tp) // 2]
        for name in variants:
            tv = times[kern, name]
            mv = sorted(tv)[len(tv) // 2]
            ratio = mv / mp
            inside = min(tp) / mp <= ratio <= max(tp) / mp
            emit(f"{kern:8s} {name:8s} {mv:9.1f} us ({min(tv):.1f} .. {max(tv):.1f})  "
                 f"{N * V * nbytes / mv / 1e6:6.2f} TB/s  ratio to plain {ratio:.4f}  "
                 f"plain spread {min(tp) / mp:.4f} .. {max(tp) / mp:.4f}"
                 + ("" if name == "plain" else ("  inside the spread" if inside else "  OUTSIDE THE SPREAD")))
            out[kern, name] = dict(us=mv, ratio=ratio, inside=inside)
    del ring
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--vocab", type=int, default=32000)
    ap.add_argument("--cap", type=float, default=30.0)
    ap.add_argument("--z-coef", type=float, default=1e-4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-gib", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join("profiles", "xent_softcap.txt"),
                    help="also write the result lines to this file ('' = do not)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_xent.py measures the HIP kernels: it needs the GPU")
    lines = [f"# scripts/bench_xent.py: the three head-loss kernels of csrc/xent.hip in bf16, plain and with the options "
             f"(cap {a.cap:g}, z-loss coefficient {a.z_coef:g}, both),",
             f"# medians of {a.rounds} interleaved rounds of {a.iters} calls in one process (min .. max in brackets), "
             "every call on the next buffer of a ring larger than the",
             "# last-level cache; TB/s = bytes the kernel must move (2 B read, + 2 B written in place) over the time; "
             "ratio = option / plain, the plain call's",
             "# own min .. max spread beside it.  One MI355X."]

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    for line in lines:
        print(line, flush=True)
    for N in (int(x) for x in a.rows.split(",")):
        run_shape(N, a.vocab, a.cap, a.z_coef, a.iters, a.rounds, int(a.ring_gib * 2 ** 30), emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
