#!/usr/bin/env python3
"""What QK-norm costs beside RoPE on one MI355X (writes profiles/qknorm.txt).

    python scripts/bench_qknorm.py [--out profiles/qknorm.txt] [--rows 4096,16384] [--reps 9]

Times the two fused kernels of csrc/qknorm.hip against the kernel they replace when ``--qk-norm`` is on, at the M7B
head shape (32 q heads, 8 kv heads, head_dim 128) on the strided q|k columns of a fused qkv buffer:

    forward    qknorm_rope_fwd   against   rope_ (forward)      reads q|k, writes q|k (+ raw)
    backward   qknorm_rope_bwd_  against   rope_ (inverse)      reads dqkv q|k (+ raw), writes dqkv q|k (+ partials)

Every timed call works on the next entry of a ring of buffers that together exceed the last-level cache (256 MiB), so
the figures are HBM figures, not cache figures.  One timing is one walk over the whole ring between two device events,
divided by the ring's length; the baseline's and the fused kernel's walks alternate rep by rep after a warm-up, and the
medians are reported with the bytes each kernel must move (computed from the shapes, below) and the bandwidth that
gives.  bf16; the kernels are format-independent but for the conversion instructions.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING_BYTES = 1 << 30


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qknorm.txt"))
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qknorm.py measures on the GPU; no GPU found")
    import dltb  # noqa: F401
    from dltb.ops import ref
    from dltb.ops._ext import ext
    C = ext()
    dev, dt = "cuda", torch.bfloat16
    Hq, Hkv, D, T, eps = 32, 8, 128, 4096, 1e-5
    heads, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    cos, sin = ref.rope_tables(T, D, 10000.0, dev)
    g = torch.Generator(dev).manual_seed(0)
    wq = (1.0 + 0.1 * torch.randn(D, device=dev, generator=g)).to(dt)
    wk = (1.0 + 0.1 * torch.randn(D, device=dev, generator=g)).to(dt)
    lines = [f"# QK-norm fused with RoPE against RoPE alone: Hq {Hq}, Hkv {Hkv}, D {D}, bf16, rows of {W} columns, "
             f"T {T}; {torch.cuda.get_device_name(0)}",
             f"# medians of {a.reps} interleaved reps after 3 warm-up reps; one rep = one walk over a ring of buffers "
             f"of >= {RING_BYTES >> 20} MiB in all, per-call time = walk / ring length",
             "# bytes: rope 2 x q|k; fused forward 3 x q|k (raw written); fused backward 3 x q|k (raw read) + the "
             "fp32 partials 2 G D",
             "rows  pass      kernel            ring  ms/call   MB moved   GB/s    time ratio  byte ratio"]
    for N in [int(r) for r in a.rows.split(",")]:
        qk_bytes = N * heads * D * 2
        G = C.qknorm_partials(N)
        ring = max(2, -(-RING_BYTES // (N * W * 2 + qk_bytes)))
        bufs = [torch.randn(N, W, device=dev, generator=g).to(dt) for _ in range(ring)]
        raws = [b[:, :heads * D].contiguous() for b in bufs]

        def rope(inverse):
            for b in bufs:
                C.rope_(b, cos, sin, T, heads, D, inverse)

        def fused_fwd():
            for b in bufs:
                C.qknorm_rope_fwd(b, wq, wk, cos, sin, T, Hq, Hkv, D, eps)

        def fused_bwd():
            for b, r in zip(bufs, raws):
                C.qknorm_rope_bwd_(b, r, wq, wk, cos, sin, T, Hq, Hkv, D, eps)

        cases = (("forward", lambda: rope(False), fused_fwd, 2 * qk_bytes, 3 * qk_bytes),
                 ("backward", lambda: rope(True), fused_bwd, 2 * qk_bytes, 3 * qk_bytes + 2 * G * D * 4))
        for name, base, fused, base_bytes, fused_bytes in cases:
            for _ in range(3):
                base()
                fused()
            torch.cuda.synchronize()
            tb, tf = [], []
            for _ in range(a.reps):
                tb.append(_timed(base) / ring)
                tf.append(_timed(fused) / ring)
            mb, mf = statistics.median(tb), statistics.median(tf)
            for kernel, ms, nbytes in (("rope_", mb, base_bytes),
                                       ("qknorm_rope_" + ("fwd" if name == "forward" else "bwd_"), mf, fused_bytes)):
                ratio = "" if kernel == "rope_" else f"{mf / mb:10.3f}  {fused_bytes / base_bytes:10.3f}"
                lines.append(f"{N:<5d} {name:<9s} {kernel:<17s} {ring:<5d} {ms:7.4f}  {nbytes / 1e6:9.2f}  "
                             f"{nbytes / ms / 1e6:7.1f}  {ratio}")
        del bufs, raws
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
