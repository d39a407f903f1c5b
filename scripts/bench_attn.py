#!/usr/bin/env python3
"""Attention kernel microbenchmark (forward, dK/dV, dQ, dropout-mask) on the two model shapes.

    python scripts/bench_attn.py [--iters 50]
    python scripts/bench_attn.py --window 4096 --seq-lens 8192,16384,32768   # sliding window vs full causal
    python scripts/bench_attn.py --doc-len 2048 [--window 4096]              # packed documents vs full causal
    python scripts/bench_attn.py --cp 8 --cp-layout zigzag [--window 4096]   # every rank's query ranges vs the whole row
    python scripts/bench_attn.py --q-range 0:2048 --q-range 30720:32768 --seq-lens 32768
    python scripts/bench_attn.py --sinks --seq-lens 4096,16384 [--out profiles/attention_sinks.txt]
    python scripts/bench_attn.py --softcap 50 --seq-lens 4096,16384 --rounds 7 [--out profiles/attention_softcap.txt]

Prints one line per kernel: time per call and TFLOP/s (causal FLOPs counted over the visible
half).  Shapes: TinyGPT-A (B1 T2048 H16 D64, dropout 0.1, non-causal) and Mistral-7B
(B1 T4096 Hq32 Hkv8 D128, causal).

``--window W`` times forward, dQ and dK/dV of the Mistral-7B attention shape at each ``--seq-lens`` length
with the window (query i sees keys i - W < j <= i) and without it, in one process: the two variants
alternate over ``--rounds`` rounds of ``--iters`` calls (after a warm-up round), and the median round is
reported with the min .. max spread, next to the ratio of visited 64-key tiles (window / causal) that the
kernels' tile bounds give.

``--q-range B:E`` (repeatable; ``--cp N --cp-layout L`` is shorthand for the ranges of every rank of a
context-parallel group, dltb/parallel/context.py) times the three passes of each query range of the Mistral-7B
attention shape next to the whole-row call at the same ``--seq-lens`` length (and ``--window``), all alternating in
one process as above, with the ratio of visited tiles (range / whole row).  With ``--cp`` it also prints every
rank's summed time and the max / mean ratio over the ranks: the balance of the attention kernels of one step.

``--sinks`` times the causal forward of the Mistral-7B attention shape with and without learned attention sinks
(``attn_fwd(..., sink=)``: the SINK instantiation against its sink-less twin) at each ``--seq-lens`` length, full
causal and with ``--sinks-window`` (default 4096), alternating in one process as above, plus the sink-gradient kernel
``attn_sink_bwd``.  The yardstick is the sink-less call of the same run; ``--out`` also writes the lines to a file.

``--softcap C`` times forward, dQ and dK/dV of the Mistral-7B attention shape with logit soft-capping at cap C (the CAP
instantiations) against the plain instantiations at each ``--seq-lens`` length, full causal and with
``--sinks-window``, the six calls alternating in one process over ``--rounds`` rounds; each pass is reported on its
own with the plain call's min .. max spread beside the ratio.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dltb  # noqa: E402,F401
from dltb.ops._ext import ext  # noqa: E402

SHAPES = {"tinygpt_a": dict(B=1, T=2048, Hq=16, Hkv=16, D=64, causal=False, p=0.1),
          "tinygpt_a_p0": dict(B=1, T=2048, Hq=16, Hkv=16, D=64, causal=False, p=0.0),
          "m7b": dict(B=1, T=4096, Hq=32, Hkv=8, D=128, causal=True, p=0.0),
          # three TinyGPT-A micro-batches: 768 query blocks, so several workgroups share a CU
          "tinygpt_a_b3": dict(B=3, T=2048, Hq=16, Hkv=16, D=64, causal=False, p=0.1),
          # causal D = 64 (mtiny-like): the shapes the causal split caps of csrc/attention.hip act on
          "causal_d64": dict(B=1, T=2048, Hq=16, Hkv=16, D=64, causal=True, p=0.0),
          "causal_d64_short": dict(B=4, T=512, Hq=8, Hkv=8, D=64, causal=True, p=0.0)}


def timeit(fn, iters):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3   # us


def run(name, B, T, Hq, Hkv, D, causal, p, iters):
    C = ext()
    g = torch.Generator(device="cuda").manual_seed(0)
    dev = "cuda"
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    seed = torch.tensor([1234], device=dev, dtype=torch.int64)
    scale = D ** -0.5
    mask = C.attn_mask(B, T, Hq, p, seed, 1, q) if p > 0 else None
    o, lse = C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, causal, p)
    delta = C.attn_bwd_delta(o, do, B, T, Hq)
    dq = torch.empty_like(q)
    dkv = torch.empty(B * T, 2 * Hkv * D, device=dev, dtype=torch.bfloat16)
    dk, dv = dkv[:, :Hkv * D], dkv[:, Hkv * D:]
    frac = 0.5 if causal else 1.0
    f_fwd = 4.0 * B * Hq * T * T * D * frac
    res = {}
    res["fwd"] = (timeit(lambda: C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, causal, p), iters), f_fwd)
    res["dkdv"] = (timeit(lambda: C.attn_bwd_part(0, q, k, v, do, lse, delta, mask, dk, dv, B, T, Hq, Hkv, scale,
                                                  causal, p), iters), f_fwd * 2.0)   # S, dP, dV, dK
    res["dq"] = (timeit(lambda: C.attn_bwd_part(1, q, k, v, do, lse, delta, mask, dq, None, B, T, Hq, Hkv, scale,
                                                causal, p), iters), f_fwd * 1.5)     # S, dP, dQ
    res["delta"] = (timeit(lambda: C.attn_bwd_delta(o, do, B, T, Hq), iters), 0.0)
    if p > 0:
        res["mask"] = (timeit(lambda: C.attn_mask(B, T, Hq, p, seed, 1, q), iters), 0.0)
    tot = 0.0
    for kname, (us, fl) in res.items():
        tot += us
        tf = fl / us / 1e6 if fl else 0.0
        print(f"{name:10s} {kname:6s} {us:9.1f} us  {tf:7.1f} TFLOP/s")
    print(f"{name:10s} total  {tot:9.1f} us per layer (fwd + bwd)")
    return {k: v[0] for k, v in res.items()}


def tile_counts(T, W):
    """64-key tiles the query-major kernels (forward, dQ) visit per (batch, head) and 64-query tiles the
    key-major kernel (dK/dV) visits per (batch, KV head, query head), from the bounds of csrc/attention.hip
    (128-row blocks); W = 0: full causal."""
    qmaj = kmaj = 0
    for blk in range(T // 128):
        hi = min(T // 64, (blk * 128 + 127) // 64 + 1)
        lo = max(0, blk * 128 - W + 1) // 64 if W else 0
        qmaj += hi - lo
        end = min(T // 64, (blk * 128 + 127 + W - 1) // 64 + 1) if W else T // 64
        kmaj += end - blk * 128 // 64
    return qmaj, kmaj


def run_window(T, W, iters, rounds, B=1, Hq=32, Hkv=8, D=128, p=0.0):
    C = ext()
    g = torch.Generator(device="cuda").manual_seed(0)
    dev = "cuda"
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    seed = torch.tensor([1234], device=dev, dtype=torch.int64)
    scale = D ** -0.5
    mask = C.attn_mask(B, T, Hq, p, seed, 1, q) if p > 0 else None
    dq = torch.empty_like(q)
    dkv = torch.empty(B * T, 2 * Hkv * D, device=dev, dtype=torch.bfloat16)
    dk, dv = dkv[:, :Hkv * D], dkv[:, Hkv * D:]
    fns = {}
    for w in (0, W):
        o, lse = C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, p, window=w)
        delta = C.attn_bwd_delta(o, do, B, T, Hq)
        fns["fwd", w] = lambda w=w: C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, p, window=w)
        fns["dq", w] = lambda w=w, lse=lse, delta=delta: C.attn_bwd_part(
            1, q, k, v, do, lse, delta, mask, dq, None, B, T, Hq, Hkv, scale, True, p, window=w)
        fns["dkdv", w] = lambda w=w, lse=lse, delta=delta: C.attn_bwd_part(
            0, q, k, v, do, lse, delta, mask, dk, dv, B, T, Hq, Hkv, scale, True, p, window=w)
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up; causal and windowed calls alternate
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    full, win = tile_counts(T, 0), tile_counts(T, W)
    out = {}
    for kname, tiles in (("fwd", win[0] / full[0]), ("dq", win[0] / full[0]), ("dkdv", win[1] / full[1])):
        med = {w: sorted(times[kname, w])[len(times[kname, w]) // 2] for w in (0, W)}
        spread = {w: (min(times[kname, w]), max(times[kname, w])) for w in (0, W)}
        out[kname] = dict(causal_us=med[0], window_us=med[W], time_ratio=med[W] / med[0], tile_ratio=tiles)
        print(f"T {T:6d} W {W:5d} {kname:5s} causal {med[0]:9.1f} us ({spread[0][0]:.1f} .. {spread[0][1]:.1f})  "
              f"window {med[W]:9.1f} us ({spread[W][0]:.1f} .. {spread[W][1]:.1f})  "
              f"time ratio {med[W] / med[0]:.3f}  tile ratio {tiles:.3f}", flush=True)
    return out


def range_tile_counts(T, W, qb, qe):
    """tile_counts for the query range [qb, qe): the query-major kernels visit the range's blocks only, every key
    block of the key-major kernel walks the range's query tiles only."""
    qmaj = kmaj = 0
    for blk in range(T // 128):
        if qb <= blk * 128 < qe:
            hi = min(T // 64, (blk * 128 + 127) // 64 + 1)
            qmaj += hi - (max(0, blk * 128 - W + 1) // 64 if W else 0)
        end = min(T // 64, (blk * 128 + 127 + W - 1) // 64 + 1) if W else T // 64
        kmaj += max(0, min(end, qe // 64) - max(blk * 128 // 64, qb // 64))
    return qmaj, kmaj


def run_qrange(T, W, ranges, iters, rounds, B=1, Hq=32, Hkv=8, D=128, ranks=None):
    """Forward, dQ and dK/dV of every query range in ``ranges`` next to the whole-row call (window ``W`` or full
    causal), alternating as in run_window.  ``ranks``: {rank: [ranges]} for the per-rank sums of ``--cp``."""
    C = ext()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    scale = D ** -0.5
    dkv = torch.empty(B * T, 2 * Hkv * D, device=dev, dtype=torch.bfloat16)
    dk, dv = dkv[:, :Hkv * D], dkv[:, Hkv * D:]
    fns = {}
    for rng in [None] + list(ranges):
        qb, qe = rng or (0, T)
        kw = {"window": W} if rng is None else {"window": W, "q_range": rng}
        ql = q.view(B, T, -1)[:, qb:qe].reshape(B * (qe - qb), -1).contiguous()
        dol = do.view(B, T, -1)[:, qb:qe].reshape(B * (qe - qb), -1).contiguous()
        o, lse = C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, **kw)
        delta = C.attn_bwd_delta(o, dol, B, qe - qb, Hq)
        dq = torch.empty_like(ql)
        fns["fwd", rng] = lambda ql=ql, kw=kw: C.attn_fwd(ql, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, **kw)
        fns["dq", rng] = lambda ql=ql, dol=dol, lse=lse, delta=delta, dq=dq, kw=kw: C.attn_bwd_part(
            1, ql, k, v, dol, lse, delta, None, dq, None, B, T, Hq, Hkv, scale, True, 0.0, **kw)
        fns["dkdv", rng] = lambda ql=ql, dol=dol, lse=lse, delta=delta, kw=kw: C.attn_bwd_part(
            0, ql, k, v, dol, lse, delta, None, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, **kw)
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up; whole-row and range calls alternate
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
    full = tile_counts(T, W)
    out = {"full": {kn: med[kn, None] for kn in ("fwd", "dq", "dkdv")}, "ranges": {}}
    print(f"T {T:6d} W {W:5d} whole row: " + "  ".join(
        f"{kn} {med[kn, None]:9.1f} us ({min(times[kn, None]):.1f} .. {max(times[kn, None]):.1f})"
        for kn in ("fwd", "dq", "dkdv")), flush=True)
    for rng in ranges:
        tc = range_tile_counts(T, W, *rng)
        rec = {}
        for kn, tiles in (("fwd", tc[0] / full[0]), ("dq", tc[0] / full[0]), ("dkdv", tc[1] / full[1])):
            m, f = med[kn, rng], med[kn, None]
            rec[kn] = dict(us=m, full_us=f, time_ratio=m / f, tile_ratio=tiles)
            print(f"T {T:6d} W {W:5d} range {rng[0]:6d}:{rng[1]:<6d} {kn:5s} {m:9.1f} us "
                  f"({min(times[kn, rng]):.1f} .. {max(times[kn, rng]):.1f})  time ratio {m / f:.3f}  "
                  f"tile ratio {tiles:.3f}" + ("" if m <= f else "  SLOWER THAN THE WHOLE ROW"), flush=True)
        out["ranges"][f"{rng[0]}:{rng[1]}"] = rec
    if ranks:
        tot = {r: sum(med[kn, rng] for rng in rr for kn in ("fwd", "dq", "dkdv")) for r, rr in ranks.items()}
        mean = sum(tot.values()) / len(tot)
        for r, t in tot.items():
            print(f"T {T:6d} W {W:5d} rank {r}: ranges {ranks[r]}  fwd + dq + dkdv {t:9.1f} us", flush=True)
        whole = sum(med[kn, None] for kn in ("fwd", "dq", "dkdv"))
        print(f"T {T:6d} W {W:5d} over {len(tot)} ranks: max {max(tot.values()):.1f} us, mean {mean:.1f} us, "
              f"max / mean {max(tot.values()) / mean:.3f}; whole row on one GPU {whole:.1f} us "
              f"(whole / max {whole / max(tot.values()):.2f})", flush=True)
        out["ranks"] = {str(r): t for r, t in tot.items()}
        out["max_over_mean"] = max(tot.values()) / mean
    return out


def run_sinks(T, W, iters, rounds, B=1, Hq=32, Hkv=8, D=128, emit=print):
    """The causal forward (window ``W``, 0 = full causal) without and with a sink, alternating over ``rounds`` rounds
    after a warm-up round, and the sink-gradient kernel on the forward's lse and the dQ pass's delta."""
    C = ext()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    sink = (2.0 * torch.randn(Hq, device=dev, generator=g)).to(torch.bfloat16)
    scale = D ** -0.5
    o, lse = C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=W, sink=sink)
    delta = C.attn_bwd_delta(o, do, B, T, Hq)
    fns = {"plain": lambda: C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=W),
           "sink": lambda: C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=W, sink=sink),
           "dsink": lambda: C.attn_sink_bwd(lse, delta, sink)}
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up; the sink-less and the sink call alternate
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
    lo, hi = min(times["plain"]), max(times["plain"])
    ratio = med["sink"] / med["plain"]
    inside = lo / med["plain"] <= ratio <= hi / med["plain"]
    emit(f"T {T:6d} W {W:5d} fwd plain {med['plain']:9.1f} us ({lo:.1f} .. {hi:.1f})  "
         f"sink {med['sink']:9.1f} us ({min(times['sink']):.1f} .. {max(times['sink']):.1f})  ratio {ratio:.4f}  "
         f"plain spread {lo / med['plain']:.4f} .. {hi / med['plain']:.4f}  "
         + ("inside the spread" if inside else "OUTSIDE THE SPREAD")
         + f"  attn_sink_bwd {med['dsink']:6.1f} us ({min(times['dsink']):.1f} .. {max(times['dsink']):.1f}, "
         f"{C.attn_sink_partials(B, T)} partial rows)")
    return dict(plain_us=med["plain"], sink_us=med["sink"], ratio=ratio, plain_min=lo, plain_max=hi,
                inside_spread=inside, dsink_us=med["dsink"])


def run_softcap(T, W, cap, iters, rounds, B=1, Hq=32, Hkv=8, D=128, emit=print):
    """Forward, dQ and dK/dV (window ``W``, 0 = full causal) without and with soft-capping at ``cap``, the six calls
    alternating over ``rounds`` rounds after a warm-up round.  Each backward pass runs on its own forward's o / lse."""
    C = ext()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv[:, :Hq * D], dqkv[:, Hq * D:(Hq + Hkv) * D], dqkv[:, (Hq + Hkv) * D:]
    scale = D ** -0.5
    fns = {}
    for kind, kw in (("plain", {}), ("cap", {"softcap": cap})):
        o, lse = C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=W, **kw)
        delta = C.attn_bwd_delta(o, do, B, T, Hq)

        def fwd(kw=kw):
            return C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, window=W, **kw)

        def dq_(kw=kw, o=o, lse=lse, delta=delta):
            return C.attn_bwd_part(1, q, k, v, do, lse, delta, None, dq, None, B, T, Hq, Hkv, scale, True, 0.0, o,
                                   window=W, **kw)

        def dkdv(kw=kw, lse=lse, delta=delta):
            return C.attn_bwd_part(0, q, k, v, do, lse, delta, None, dk, dv, B, T, Hq, Hkv, scale, True, 0.0, None,
                                   window=W, **kw)
        fns[("fwd", kind)], fns[("dq", kind)], fns[("dkdv", kind)] = fwd, dq_, dkdv
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up; the plain and the capped calls alternate
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    out = {}
    for name in ("fwd", "dq", "dkdv"):
        tp, tc = times[(name, "plain")], times[(name, "cap")]
        mp, mc = sorted(tp)[len(tp) // 2], sorted(tc)[len(tc) // 2]
        emit(f"T {T:6d} W {W:5d} cap {cap:g} {name:5s} plain {mp:9.1f} us ({min(tp):.1f} .. {max(tp):.1f})  "
             f"capped {mc:9.1f} us ({min(tc):.1f} .. {max(tc):.1f})  ratio {mc / mp:.4f}  "
             f"plain spread {min(tp) / mp:.4f} .. {max(tp) / mp:.4f}")
        out[name] = dict(plain_us=mp, cap_us=mc, ratio=mc / mp, plain_min=min(tp), plain_max=max(tp))
    return out


def doc_tile_counts(bounds, T):
    """tile_counts for document bounds [2, 1, T] (CPU): the tile ranges of the bounds kernels."""
    lo, hi = bounds[0, 0].tolist(), bounds[1, 0].tolist()
    qmaj = kmaj = 0
    for blk in range(T // 128):
        qmaj += min(T // 64, (blk * 128 + 127) // 64 + 1) - lo[blk * 128] // 64
        kmaj += min(T // 64, (hi[blk * 128 + 127] + 63) // 64) - blk * 128 // 64
    return qmaj, kmaj


def run_docs(T, doc_len, W, iters, rounds, B=1, Hq=32, Hkv=8, D=128, p=0.0, seed=0):
    """Forward, dQ and dK/dV with the document bounds of one seeded layout (documents of mean length
    ``doc_len``, the harness's SyntheticDataset row 0; window ``W`` folded in) next to full causal attention,
    alternating as in run_window."""
    from dltb.data.synthetic import SyntheticDataset
    C = ext()
    dev = "cuda"
    ds = SyntheticDataset(32000, T, size=B, seed=seed, doc_len=doc_len)
    idx = ds.data.to(dev)
    bounds = C.attn_doc_bounds(idx, ds.eos_id, W)
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B * T, (Hq + 2 * Hkv) * D, device=dev, dtype=torch.bfloat16, generator=g)
    q, k, v = qkv[:, :Hq * D], qkv[:, Hq * D:(Hq + Hkv) * D], qkv[:, (Hq + Hkv) * D:]
    do = torch.randn(B * T, Hq * D, device=dev, dtype=torch.bfloat16, generator=g)
    scale = D ** -0.5
    mask = C.attn_mask(B, T, Hq, p, torch.tensor([1234], device=dev, dtype=torch.int64), 1, q) if p > 0 else None
    dq = torch.empty_like(q)
    dkv = torch.empty(B * T, 2 * Hkv * D, device=dev, dtype=torch.bfloat16)
    dk, dv = dkv[:, :Hkv * D], dkv[:, Hkv * D:]
    fns = {}
    for name, bd in (("causal", None), ("docs", bounds)):
        o, lse = C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, p, bounds=bd)
        delta = C.attn_bwd_delta(o, do, B, T, Hq)
        fns["fwd", name] = lambda bd=bd: C.attn_fwd(q, k, v, mask, B, T, Hq, Hkv, scale, True, p, bounds=bd)
        fns["dq", name] = lambda bd=bd, lse=lse, delta=delta: C.attn_bwd_part(
            1, q, k, v, do, lse, delta, mask, dq, None, B, T, Hq, Hkv, scale, True, p, bounds=bd)
        fns["dkdv", name] = lambda bd=bd, lse=lse, delta=delta: C.attn_bwd_part(
            0, q, k, v, do, lse, delta, mask, dk, dv, B, T, Hq, Hkv, scale, True, p, bounds=bd)
    fns["bounds", "docs"] = lambda: C.attn_doc_bounds(idx, ds.eos_id, W)
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up; causal and masked calls alternate
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
    full, doc = tile_counts(T, 0), doc_tile_counts(bounds.cpu(), T)
    ndocs = int((ds.data[0] == ds.eos_id).sum())
    print(f"T {T:6d} doc-len {doc_len} window {W} dropout {p}: {ndocs} documents in the row, bounds kernel "
          f"{med['bounds', 'docs']:.1f} us", flush=True)
    out = {"documents": ndocs, "bounds_us": med["bounds", "docs"]}
    for kname, tiles in (("fwd", doc[0] / full[0]), ("dq", doc[0] / full[0]), ("dkdv", doc[1] / full[1])):
        c, m = med[kname, "causal"], med[kname, "docs"]
        sc, sm = times[kname, "causal"], times[kname, "docs"]
        out[kname] = dict(causal_us=c, docs_us=m, time_ratio=m / c, tile_ratio=tiles)
        print(f"T {T:6d} N {doc_len:5d} W {W:5d} {kname:5s} causal {c:9.1f} us ({min(sc):.1f} .. {max(sc):.1f})  "
              f"docs {m:9.1f} us ({min(sm):.1f} .. {max(sm):.1f})  time ratio {m / c:.3f}  tile ratio {tiles:.3f}"
              + ("" if tiles > 0.5 or m < c else "  NOT FASTER"), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", default="tinygpt_a,m7b")
    ap.add_argument("--json", default=None)
    ap.add_argument("--window", type=int, default=0, help="compare this sliding window with full causal attention")
    ap.add_argument("--seq-lens", default="8192,16384,32768", help="sequence lengths of the --window comparison")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds of the --window comparison")
    ap.add_argument("--doc-len", type=int, default=0,
                    help="compare document-masked attention (packed documents of this mean length, one seeded "
                         "layout; composes with --window) with full causal attention at --seq-lens")
    ap.add_argument("--dropout", type=float, default=0.0, help="attention dropout of the --doc-len comparison")
    ap.add_argument("--q-range", action="append", default=[], metavar="B:E",
                    help="time this query range (multiples of 128) next to the whole row at --seq-lens; repeatable")
    ap.add_argument("--cp", type=int, default=0, help="shorthand: the query ranges of every rank of a group of N")
    ap.add_argument("--cp-layout", default="auto", choices=["auto", "contiguous", "zigzag"])
    ap.add_argument("--sinks", action="store_true",
                    help="time the causal forward with and without attention sinks, and the sink-gradient kernel")
    ap.add_argument("--sinks-window", type=int, default=4096, help="the windowed variant of the --sinks comparison")
    ap.add_argument("--out", default=None, help="--sinks / --softcap: also write the result lines to this file")
    ap.add_argument("--softcap", type=float, default=0.0,
                    help="time forward, dQ and dK/dV with logit soft-capping at this cap against the plain kernels")
    a = ap.parse_args()
    if a.softcap > 0:
        lines = [f"# scripts/bench_attn.py --softcap {a.softcap:g}: forward, dQ and dK/dV of the M7B head shape (B1 Hq32 "
                 "Hkv8 D128, bf16), the soft-capped (CAP) against the plain",
                 f"# instantiation, medians of {a.rounds} interleaved rounds of {a.iters} calls in one process (min .. "
                 "max in brackets); ratio = capped / plain; the yardstick is the",
                 "# plain call of the same run, its own min .. max spread beside each ratio.  W = sliding window "
                 "(0 = full causal).  One MI355X."]

        def emit(line):
            print(line, flush=True)
            lines.append(line)
        out = {}
        for T in (int(x) for x in a.seq_lens.split(",")):
            for W in (0, a.sinks_window):
                out[f"T{T}_W{W}"] = run_softcap(T, W, a.softcap, a.iters, a.rounds, emit=emit)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    elif a.sinks:
        lines = ["# scripts/bench_attn.py --sinks: the causal forward of the M7B head shape (B1 Hq32 Hkv8 D128, bf16) "
                 "without and with learned attention sinks,",
                 f"# medians of {a.rounds} interleaved rounds of {a.iters} calls in one process (min .. max in "
                 "brackets); ratio = sink / plain; the yardstick is the",
                 "# sink-less instantiation of the same run.  attn_sink_bwd: the sink-gradient kernel on [B, Hq, T] "
                 "lse / delta.  One MI355X."]

        def emit(line):
            print(line, flush=True)
            lines.append(line)
        out = {}
        for T in (int(x) for x in a.seq_lens.split(",")):
            for W in (0, a.sinks_window):
                out[f"T{T}_W{W}"] = run_sinks(T, W, a.iters, a.rounds, emit=emit)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    elif a.q_range or a.cp > 1:
        from dltb.parallel import context as cpx
        out = {}
        for T in (int(x) for x in a.seq_lens.split(",")):
            ranges, ranks = [tuple(int(x) for x in r.split(":")) for r in a.q_range], None
            if a.cp > 1:
                layout = cpx.resolve_layout(a.cp_layout, a.window)
                ranks = {r: cpx.ranges(layout, T, a.cp, r) for r in range(a.cp)}
                ranges += [rng for rr in ranks.values() for rng in rr if rng not in ranges]
            out[f"T{T}_W{a.window}_cp{a.cp}_{a.cp_layout}"] = run_qrange(T, a.window, ranges, a.iters, a.rounds,
                                                                        ranks=ranks)
    elif a.doc_len > 0:
        out = {f"T{T}_N{a.doc_len}_W{a.window}": run_docs(T, a.doc_len, a.window, a.iters, a.rounds, p=a.dropout)
               for T in (int(x) for x in a.seq_lens.split(","))}
    elif a.window > 0:
        out = {f"T{T}_W{a.window}": run_window(T, a.window, a.iters, a.rounds)
               for T in (int(x) for x in a.seq_lens.split(","))}
    else:
        out = {n: run(n, iters=a.iters, **SHAPES[n]) for n in a.shapes.split(",")}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
