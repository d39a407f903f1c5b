#!/usr/bin/env python3
"""Measurements behind profiles/muon.txt (one GPU).

1. The symmetric product: batched ``muon_syrk`` (both tile sizes) against the same product computed as a full
   square -- hipBLASLt through ``torch.bmm`` and this project's NT GEMM (``gemm``, one launch per matrix) -- at the
   Newton-Schulz shapes of TinyGPT-A and M7B_narrow.  hipBLASLt gets a materialised X^T (transposed outside the timed
   region): ``bmm(X, X.transpose(1, 2))`` of a row-major X is the batched BLAS TN form, whose heuristic solution
   faults the GPU (profiles/dw_layout_probe_fault_r4.txt) and which this project never issues.  Times are device
   events around windows of back-to-back calls (at least ``--iters`` calls and 50 ms) after a warm-up, as (median,
   min, max) over five rounds that time the variants in turn; TFLOP/s counts the full square's 2 m^2 k for every
   row, so the columns compare directly.
2. ``muon_apply`` per tile config at the same shapes.
3. The optimizer step: ``FlatMuon.step`` against ``FlatAdamW.step`` on an engine of the tier, with the
   Newton-Schulz products (everything between ``muon_momentum`` and ``muon_update``) timed on their own.

    python scripts/bench_muon.py [--iters 20] [--tiers A,M7B_narrow] [--out profiles/muon_raw.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dltb  # noqa: E402,F401
from dltb.models import build_model, get_model_config  # noqa: E402
from dltb.ops import ref  # noqa: E402
from dltb.ops._ext import ext  # noqa: E402
from dltb.parallel.strategy import engine_config, make_engine  # noqa: E402

DEV = "cuda:0"
# (label, m, [k...], batch): X X^T at k = n of every work shape, and A A at k = m
SHAPES = [("TinyGPT-A", 1024, [1024, 3072, 4096], 16), ("M7B_narrow", 512, [512, 768, 1792, 3584], 32)]


def timed(fn, iters):
    """Seconds per call: device events around a window of back-to-back calls, at least ``iters`` of them and at least
    WINDOW seconds long (sized from a first short window), after a warm-up."""
    def window(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / n
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return window(max(iters, int(WINDOW / max(window(iters), 1e-7))))


WINDOW = 0.05
REPEATS = 5


def alternated(variants, iters):
    """name -> (median, min, max) microseconds over REPEATS rounds; every round times every variant once, in turn, so
    a drift of the clocks falls on all of them alike."""
    runs = {k: [] for k in variants}
    for _ in range(REPEATS):
        for k, fn in variants.items():
            runs[k].append(timed(fn, iters) * 1e6)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in runs.items()}


def bench_products(iters, first=0):
    C, rows = ext(), []
    for label, m, ks, batch in SHAPES[:first or None]:
        ks = ks[:first or None]
        for k in ks:
            x = (torch.randn(batch, m, k, device=DEV) * 0.05).bfloat16()
            out = torch.empty(batch, m, m, device=DEV, dtype=torch.bfloat16)
            xt = x.transpose(1, 2).contiguous()       # never batched TN: see the module docstring
            r = {"tier": label, "m": m, "k": k, "batch": batch, "auto_bt": C.muon_syrk(x, out)}
            r["us"] = alternated({
                "syrk_bt64": lambda: C.muon_syrk(x, out, None, 1.0, 0.0, None, 64),
                "syrk_bt128": lambda: C.muon_syrk(x, out, None, 1.0, 0.0, None, 128),
                "bmm": lambda: torch.bmm(x, xt, out=out),
                "own_nt": lambda: [C.gemm(x[i], x[i], out[i], None, False, False) for i in range(batch)]}, iters)
            syrk = r["us"][f"syrk_bt{r['auto_bt']}"][0]
            r["speedup_vs_best_full"] = min(r["us"]["bmm"][0], r["us"]["own_nt"][0]) / syrk
            r["full_equiv_tflops"] = 2.0 * m * m * k * batch / (syrk * 1e-6) / 1e12
            rows.append(r)
            print(json.dumps(r), flush=True)
        for n in ks:                      # X' = a X + B X at [m, n]
            b = (torch.randn(batch, m, m, device=DEV) * 0.05).bfloat16()
            x = (torch.randn(batch, m, n, device=DEV) * 0.05).bfloat16()
            y = torch.empty_like(x)
            r = {"tier": label, "apply_m": m, "n": n, "batch": batch, "auto_cfg": C.muon_apply(b, x, y)}
            variants = {f"apply_cfg{cfg}": (lambda cfg=cfg: C.muon_apply(b, x, y, 1.0, 3.4445, None, cfg))
                        for cfg in range(4)}
            variants["baddbmm"] = lambda: torch.baddbmm(x, b, x, alpha=1.0, beta=3.4445, out=y)
            r["us"] = alternated(variants, iters)
            rows.append(r)
            print(json.dumps(r), flush=True)
    return rows


def bench_step(tier, iters):
    out = {"tier": tier}
    for optimizer in ("adamw", "muon"):
        torch.manual_seed(0)
        with torch.device(DEV):
            model = build_model(get_model_config(tier, 2048))
        eng = make_engine(model, engine_config("ddp", 1, "reference", optimizer=optimizer), DEV)
        g = (torch.randn(eng.flat_grad.shape, device=DEV) * 0.01).bfloat16()
        gs = torch.ones(1, device=DEV)
        out[f"{optimizer}_step_us"] = alternated({"step": lambda: eng.opt.step(g, 1e-4, gs)}, iters)["step"]
        if optimizer == "muon":
            opt, C = eng.opt, ext()
            a, b, c = ref.MUON_ABC

            def newton_schulz():
                off = 0
                for (m, n), cnt in opt._kinds:
                    X, Y = (t[off:off + cnt * m * n].view(cnt, m, n) for t in opt._x)
                    A, B = (t[:cnt * m * m].view(cnt, m, m) for t in opt._ab)
                    for _ in range(opt.ns_steps):
                        C.muon_syrk(X, A)
                        C.muon_syrk(A, B, A, c, b)
                        C.muon_apply(B, X, Y, 1.0, a)
                        X, Y = Y, X
                    off += cnt * m * n
            out["newton_schulz_us"] = alternated({"ns": newton_schulz}, iters)["ns"]
            out["muon_matrices"] = len(opt.matrices)
            out["launches_per_step"] = opt.launches_per_step
            out["muon_elements"] = opt.mom.numel()
            flops = 0.0                   # symmetric products counted at half the square
            for (m, n), cnt in opt._kinds:
                flops += cnt * opt.ns_steps * (m * m * n + m * m * m + 2.0 * m * m * n)
            out["newton_schulz_tflop"] = flops / 1e12
            out["newton_schulz_tflops"] = flops / (out["newton_schulz_us"][0] * 1e-6) / 1e12
        del eng, model
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tiers", default="A,M7B_narrow")
    ap.add_argument("--out", default=None)
    ap.add_argument("--first", type=int, default=0, help="only the first N tiers and k of the product tables")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_muon.py needs a GPU"
    res = {"products": bench_products(a.iters, a.first), "steps": [bench_step(t, a.iters) for t in a.tiers.split(",") if t]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
