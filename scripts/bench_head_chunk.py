#!/usr/bin/env python3
"""What ``--head-chunk N`` costs and saves on one MI355X (writes profiles/head_chunk.txt).

    python scripts/bench_head_chunk.py [--out profiles/head_chunk.txt] [--rows 8192,32768] [--reps 9]

Times the LM head alone -- RMSNorm, the [rows, 4096] x [32000, 4096]^T product, the loss, and the whole backward of
``models/mistral.py::_HeadFn`` -- at the Mistral-7B head shape in bf16, unchunked and in chunks of 1024, 2048, 4096
and 8192 rows, and records the peak of the allocated bytes over one forward + backward above what is allocated
before it (parameters, gradients, the input).  The variants of one row count alternate inside every repeat, so they
see the same clocks and the same neighbours; the table gives the median and the min / max of the repeats.  A chunk
that holds every row runs the unchunked path (there is nothing to save) and is listed as such.  The step time of a
whole model under the flag is not measured here.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CHUNKS = (None, 1024, 2048, 4096, 8192)


def head_flops(rows, d, V, chunked):
    """GEMM FLOPs of one head forward + backward: the forward product, the weight and the data gradient, and under
    a chunked head the forward product once more."""
    return (4 if chunked else 3) * 2.0 * rows * d * V


def one_call(model, x, tgt, chunk):
    """(milliseconds, peak allocated bytes above the state before the call) of one head forward + backward."""
    from dltb.models import mistral
    model.head_chunk = chunk
    x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _, loss = mistral._HeadFn.apply(x, model, tgt, False)
    loss.backward()
    e1.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return e0.elapsed_time(e1), peak, loss.detach().item()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_chunk.txt"))
    ap.add_argument("--rows", default="8192,32768")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_head_chunk.py measures on the GPU; none found")
    import dltb  # noqa: F401
    from dltb.models import build_model, get_model_config
    from dltb.models.mistral import head_chunks
    from dltb.parallel import ParamRuntime

    torch.manual_seed(0)
    cfg = get_model_config("M7B", 4096)
    cfg.n_layer = 0                                 # the head (and the embedding it does not use) alone
    with torch.device("cuda"):
        model = build_model(cfg).to(torch.bfloat16)
    model.rt = ParamRuntime()
    d, V = cfg.n_embd, cfg.vocab_size
    lines = [f"# scripts/bench_head_chunk.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# LM head alone (RMSNorm + [rows, {d}] x [{V}, {d}]^T + loss + backward), bf16, "
             f"{a.reps} interleaved repeats after {a.warmup} warm-up calls per variant",
             "# ms: median [min .. max] of the repeats; peak: allocated bytes above the state before the call;",
             "# TFLOP/s: the GEMM FLOPs the variant runs (the chunked head re-runs the forward product) over the median",
             f"{'rows':>6} {'chunk':>9} {'chunks':>6} {'ms median':>10} {'min':>8} {'max':>8} {'vs off':>7} "
             f"{'peak MB':>9} {'peak vs off':>11} {'TFLOP/s':>8} {'loss':>9}"]
    for rows in [int(r) for r in a.rows.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(rows)
        x = torch.randn(rows, d, device="cuda", generator=g).to(torch.bfloat16).requires_grad_()
        tgt = torch.randint(0, V, (rows,), device="cuda", generator=g)
        tgt[::11] = -1
        for chunk in CHUNKS:
            for _ in range(a.warmup):
                one_call(model, x, tgt, chunk)
        ms = {c: [] for c in CHUNKS}
        peak, loss = {}, {}
        for _ in range(a.reps):                     # the variants alternate inside every repeat
            for chunk in CHUNKS:
                t, p, l = one_call(model, x, tgt, chunk)
                ms[chunk].append(t)
                peak[chunk], loss[chunk] = max(p, peak.get(chunk, 0)), l
        off = statistics.median(ms[None])
        for chunk in CHUNKS:
            n = head_chunks(rows, chunk)
            med = statistics.median(ms[chunk])
            name = "off" if chunk is None else (str(chunk) if n > 1 else f"{chunk}=off")
            lines.append(f"{rows:>6} {name:>9} {n:>6} {med:>10.3f} {min(ms[chunk]):>8.3f} {max(ms[chunk]):>8.3f} "
                         f"{med / off:>7.3f} {peak[chunk] / 1e6:>9.1f} {peak[chunk] / peak[None]:>11.3f} "
                         f"{head_flops(rows, d, V, n > 1) / med / 1e9:>8.1f} {loss[chunk]:>9.5f}")
        del x, tgt
        torch.cuda.empty_cache()
    lines.append(f"# written {time.strftime('%Y-%m-%d')}; the step time of a whole model under --head-chunk is not measured")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
