#!/usr/bin/env python3
"""What the top-k mixture-of-experts FFN costs on one MI355X (writes profiles/moe_layer.txt).

    python scripts/bench_moe.py [--out profiles/moe_layer.txt] [--rows 4096,16384] [--factors 1.0,1.25,2.0] [--reps 9]
    python scripts/bench_moe.py --aux-loss-coef 0.01 --z-loss-coef 0.001      (appends to the same file)
    python scripts/bench_moe.py --dropless                                    (appends to the same file)

Times the FFN part of one MoE layer at the M7B shape (d 4096, f 14336, E 8, K 2), forward plus backward: route,
assign, dispatch, the E experts, combine and their backward (``models/mistral.py::_moe_fwd`` / ``_moe_bwd``).  The
baseline is the dense SwiGLU FFN on the same rows with hidden size K f: equal nominal FLOPs.  Both run on the same
device in one process, interleaved rep by rep after a warm-up, and the medians are reported.  The seven routing
kernels are also timed one by one on the same tensors, and so are the 2 E slab copies the layer makes (each expert's
output and data gradient is copied into its rows of the slot buffer); kernels plus copies over the layer's time is the
share the routing takes beside the GEMMs and SwiGLU kernels.  The drop fraction is that of the random-init router on
normal rows.

With ``--aux-loss-coef`` / ``--z-loss-coef`` the script measures what the auxiliary router losses cost instead, at the
same shapes, and appends to the file: the same layer (same weights, same rows) forward plus backward with the
coefficients set against both at 0, interleaved rep by rep, and the router's weight gradient on a ``dlogits`` without
zeros through the sparse kernel (the default) and the dense one (``dense=True``, what the layer runs with a loss on):
batches of calls per event pair, the two kernels interleaved, once with the rows hot in the caches and once walking
a ring of copies larger than the caches.

With ``--dropless`` the script measures the dropless layer (``moe_dropless``: packed rows, grouped GEMMs) instead and
appends to the file: the same layer (same weights, same rows) forward plus backward in dropless mode against (a) the
capacity path at factor E / K, the only way to run it without drops, (b) the capacity path at factor 1.25 and (c) the
dense FFN of equal nominal FLOPs, all interleaved rep by rep; and the two grouped kernels alone against E per-expert
calls of the dense path's products at equal total rows (K rows / E per expert).
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moe_layer.txt"))
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--factors", default="1.0,1.25,2.0")
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--aux-loss-coef", type=float, default=0.0, help="load-balancing loss coefficient (0: off)")
    ap.add_argument("--z-loss-coef", type=float, default=0.0, help="router z-loss coefficient (0: off)")
    ap.add_argument("--dropless", action="store_true", help="measure the dropless layer and the grouped kernels")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe.py measures on the GPU; none found")
    import dltb  # noqa: F401
    from dltb.models import get_model_config, mistral
    from dltb.ops import functional as F_
    from dltb.ops import ref
    from dltb.parallel import ParamRuntime

    dev, dt = "cuda", torch.bfloat16
    E, K = a.experts, a.top_k
    base = get_model_config("M7B", 4096)
    d, f = base.n_embd, base.ffn_dim
    lines = [f"# scripts/bench_moe.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# one layer's FFN part, forward + backward, bf16, d {d}, f {f}, E {E}, K {K}; dense baseline: hidden {K * f}",
             f"# medians of {a.reps} interleaved reps after 3 warm-up reps; ms",
             "rows factor capacity drop_fraction moe_ms dense_ms ratio routing_kernels_ms slab_copies_ms routing_share"]

    def layer(n_experts, ffn, factor):
        cfg = get_model_config("M7B", 4096)
        cfg.n_layer, cfg.vocab_size, cfg.ffn_hidden = 1, 256, ffn
        if n_experts:
            cfg.n_experts, cfg.moe_top_k, cfg.moe_capacity_factor = n_experts, K, factor
        cfg.validate()
        torch.manual_seed(0)
        with torch.device(dev):
            m = mistral.MistralLM(cfg).to(dt)
        m.rt = ParamRuntime()
        return m

    if a.aux_loss_coef or a.z_loss_coef:
        return aux_section(a, layer, F_, mistral, d, f, E, K, dev, dt)
    if a.dropless:
        return dropless_section(a, layer, F_, mistral, ref, d, f, E, K, dev, dt)
    dense = layer(None, K * f, 1.0)
    du = dense.unit_blocks[0]
    dws = dense.rt.acquire(du)
    ds = [(torch.empty_like(w), False) for w in dws]
    for rows in [int(r) for r in a.rows.split(",")]:
        h = torch.randn(rows, d, device=dev).to(dt)
        dm = torch.randn(rows, d, device=dev).to(dt)

        def dense_step():
            gu = F_.linear_fwd(h, dws[4])
            hh = F_.swiglu_fwd(gu)
            F_.linear_fwd(hh, dws[5])
            F_.linear_wgrad(dm, hh, ds[5][0], None, False)
            dgu = F_.swiglu_bwd(F_.linear_dgrad(dm, dws[5]), gu)
            F_.linear_wgrad(dgu, h, ds[4][0], None, False)
            return F_.linear_dgrad(dgu, dws[4])

        for factor in [float(x) for x in a.factors.split(",")]:
            moe = layer(E, f, factor)
            mu = moe.unit_blocks[0]
            mws = moe.rt.acquire(mu)
            ms = [(torch.empty_like(w), False) for w in mws]

            def moe_step():
                _, saved = mistral._moe_fwd(moe, 0, h, mws[4:])
                return mistral._moe_bwd(moe, mu, dm, h, mws, ms, saved)

            t_moe, t_dense = [], []
            for rep in range(a.reps + 3):
                tm, _ = _timed(moe_step)
                td, _ = _timed(dense_step)
                if rep >= 3:
                    t_moe.append(tm)
                    t_dense.append(td)
            C = ref.moe_capacity(rows, E, K, factor)
            counts = moe.moe_counts(dev)[0].cpu()
            drop = float((counts - C).clamp(min=0).sum()) / float(counts.sum())
            # the seven routing kernels alone, on the tensors of one forward
            expert, gate, _ = F_.moe_route(h, mws[4], K)
            slot, src, _, _ = F_.moe_assign(expert, E, C)
            xe = F_.moe_dispatch(h, src)
            _, _, dl = F_.moe_combine_bwd(dm, xe, slot, src, expert, gate, E)
            dwr = torch.empty_like(mws[4])
            kernels = [lambda: F_.moe_route(h, mws[4], K), lambda: F_.moe_assign(expert, E, C),
                       lambda: F_.moe_dispatch(h, src), lambda: F_.moe_combine(xe, slot, gate),
                       lambda: F_.moe_combine_bwd(dm, xe, slot, src, expert, gate, E),
                       lambda: F_.moe_dispatch_bwd(xe, slot, dl, mws[4]),
                       lambda: F_.moe_router_wgrad(dl, h, dwr, False)]
            t_k = 0.0
            for k in kernels:
                for _ in range(3):
                    k()
                t_k += statistics.median(_timed(k)[0] for _ in range(a.reps))
            slab, part = torch.empty_like(xe), torch.randn(C, d, device=dev).to(dt)

            def copies():      # what _moe_fwd / _moe_bwd copy: E outputs into ye, E data gradients into dxe
                for _ in range(2):
                    for e in range(E):
                        slab[e * C:(e + 1) * C].copy_(part)

            for _ in range(3):
                copies()
            t_c = statistics.median(_timed(copies)[0] for _ in range(a.reps))
            mm, md = statistics.median(t_moe), statistics.median(t_dense)
            lines.append(f"{rows} {factor} {C} {drop:.4f} {mm:.3f} {md:.3f} {mm / md:.3f} {t_k:.3f} {t_c:.3f} "
                         f"{(t_k + t_c) / mm:.3f}")
            print(lines[-1], flush=True)
            del moe, mws, ms
            torch.cuda.empty_cache()
    lines.append(f"# written {time.strftime('%Y-%m-%d')}; the step time of a whole model under --moe-experts is not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


def dropless_section(a, layer, F_, mistral, ref, d, f, E, K, dev, dt):
    """The dropless layer against the capacity path at factors E / K and 1.25 and the dense FFN, and the grouped
    kernels against per-expert calls; appended to ``a.out``."""
    name = torch.cuda.get_device_name(0)
    lines = [f"# scripts/bench_moe.py --dropless on {name}, torch {torch.__version__}",
             f"# one layer's FFN part, forward + backward, bf16, d {d}, f {f}, E {E}, K {K}: the same weights and rows in "
             f"dropless mode (grouped GEMMs), on the capacity path at factor E/K = {E / K:g} (a: no drops) and 1.25 (b), "
             f"and the dense FFN of hidden {K * f} (c)",
             f"# medians of {a.reps} interleaved reps after 3 warm-up reps; ms; slot rows: R dropless, E C capacity",
             "rows R dropless_ms EC_a cap_a_ms EC_b cap_b_ms dense_ms dropless/a dropless/b dropless/c"]
    kern = ["# the grouped kernels alone against E per-expert calls at equal total rows (K rows / E rows per expert, "
            "balanced); ms, medians; nt: [rows_e, d] x [2f, d]^T (gate|up forward), tn: dW [2f, d] = dy^T x",
            "rows total_rows grouped_nt_ms per_expert_nt_ms nt_ratio grouped_tn_ms per_expert_tn_ms tn_ratio"]
    dense = layer(None, K * f, 1.0)
    dws = dense.rt.acquire(dense.unit_blocks[0])
    ds = [(torch.empty_like(w), False) for w in dws]
    moe = layer(E, f, 1.25)
    mu = moe.unit_blocks[0]
    mws = moe.rt.acquire(mu)
    ms = [(torch.empty_like(w), False) for w in mws]
    for rows in [int(r) for r in a.rows.split(",")]:
        h = torch.randn(rows, d, device=dev).to(dt)
        dm = torch.randn(rows, d, device=dev).to(dt)

        def dense_step():
            gu = F_.linear_fwd(h, dws[4])
            hh = F_.swiglu_fwd(gu)
            F_.linear_fwd(hh, dws[5])
            F_.linear_wgrad(dm, hh, ds[5][0], None, False)
            dgu = F_.swiglu_bwd(F_.linear_dgrad(dm, dws[5]), gu)
            F_.linear_wgrad(dgu, h, ds[4][0], None, False)
            return F_.linear_dgrad(dgu, dws[4])

        def moe_step(dropless, factor):
            moe.cfg.moe_dropless, moe.cfg.moe_capacity_factor = dropless, factor
            _, saved = mistral._moe_fwd(moe, 0, h, mws[4:])
            return mistral._moe_bwd(moe, mu, dm, h, mws, ms, saved)

        steps = [lambda: moe_step(True, 1.25), lambda: moe_step(False, E / K), lambda: moe_step(False, 1.25), dense_step]
        ts = [[] for _ in steps]
        for rep_ in range(a.reps + 3):
            for t, st in zip(ts, steps):
                v = _timed(st)[0]
                if rep_ >= 3:
                    t.append(v)
        md, ma, mb, mc = (statistics.median(t) for t in ts)
        R = ref.moe_dropless_rows(rows, E, K)
        ca, cb = ref.moe_capacity(rows, E, K, E / K), ref.moe_capacity(rows, E, K, 1.25)
        lines.append(f"{rows} {R} {md:.3f} {E * ca} {ma:.3f} {E * cb} {mb:.3f} {mc:.3f} {md / ma:.3f} {md / mb:.3f} "
                     f"{md / mc:.3f}")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        # kernels alone: balanced segments of K rows / E rows, no tail
        per = rows * K // E
        tot = per * E
        offsets = torch.arange(E + 1, device=dev, dtype=torch.int32) * per
        xa = torch.randn(tot, d, device=dev).to(dt)
        dy = torch.randn(tot, 2 * f, device=dev).to(dt)
        wgu = [mws[5 + 2 * e] for e in range(E)]
        dwg = [ms[5 + 2 * e][0] for e in range(E)]
        out = torch.empty(tot, 2 * f, device=dev, dtype=dt)
        calls = [lambda: F_.gemm_grouped_nt(xa, offsets, wgu, out),
                 lambda: [F_.linear_fwd(xa[e * per:(e + 1) * per], wgu[e]) for e in range(E)],
                 lambda: F_.gemm_grouped_tn(dy, xa, offsets, dwg, [False] * E),
                 lambda: [F_.linear_wgrad(dy[e * per:(e + 1) * per], xa[e * per:(e + 1) * per], dwg[e], None, False)
                          for e in range(E)]]
        tk = [[] for _ in calls]
        for rep_ in range(a.reps + 3):
            for t, c in zip(tk, calls):
                v = _timed(c)[0]
                if rep_ >= 3:
                    t.append(v)
        gn, pn, gt, pt = (statistics.median(t) for t in tk)
        kern.append(f"{rows} {tot} {gn:.3f} {pn:.3f} {gn / pn:.3f} {gt:.3f} {pt:.3f} {gt / pt:.3f}")
        print(kern[-1], flush=True)
        del xa, dy, out
        torch.cuda.empty_cache()
    lines += kern + [f"# written {time.strftime('%Y-%m-%d')}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"appended to {a.out}")


WG_BATCH = 20        # router weight-gradient calls per event pair (one call is tens of microseconds)
WG_RING_MB = 768     # the cold ring: three times the MI355X's 256 MB Infinity Cache


def aux_section(a, layer, F_, mistral, d, f, E, K, dev, dt):
    """The layer with the auxiliary losses against the same layer without, and the two router weight-gradient kernels
    on a dense dlogits; appended to ``a.out``."""
    lines = [f"# scripts/bench_moe.py --aux-loss-coef {a.aux_loss_coef} --z-loss-coef {a.z_loss_coef} on "
             f"{torch.cuda.get_device_name(0)}, torch {torch.__version__}",
             f"# one layer's FFN part, forward + backward, bf16, d {d}, f {f}, E {E}, K {K}: the same weights and rows "
             "with the coefficients set and with both 0",
             f"# medians of {a.reps} interleaved reps after 3 warm-up reps; ms",
             "rows factor moe_ms_coef0 moe_ms_with_losses ratio"]
    wg = ["# router weight gradient on a dlogits without zeros: the sparse kernel (default) and the dense one; ms per "
          f"call from {WG_BATCH} calls per event pair, the two kernels' batches interleaved, medians of {a.reps} reps.",
          "# hot: every call reads the same h (it stays in L2 / Infinity Cache, so the rates are above HBM's); cold: the "
          f"calls walk a ring of copies of h of at least {WG_RING_MB} MB, so every read comes from HBM",
          f"# {torch.cuda.get_device_name(0)!r} is how torch names the device here",
          "rows experts d hot_sparse_ms hot_dense_ms hot_dense_over_sparse cold_sparse_ms cold_dense_ms "
          "cold_dense_over_sparse"]
    daux = torch.tensor([a.aux_loss_coef, a.z_loss_coef], device=dev)
    for rows in [int(r) for r in a.rows.split(",")]:
        h = torch.randn(rows, d, device=dev).to(dt)
        dm = torch.randn(rows, d, device=dev).to(dt)
        for factor in [float(x) for x in a.factors.split(",")]:
            moe = layer(E, f, factor)
            mu = moe.unit_blocks[0]
            mws = moe.rt.acquire(mu)
            ms = [(torch.empty_like(w), False) for w in mws]

            def step(on):
                moe.cfg.moe_aux_loss_coef = a.aux_loss_coef if on else 0.0
                moe.cfg.moe_z_loss_coef = a.z_loss_coef if on else 0.0
                saved = mistral._moe_fwd(moe, 0, h, mws[4:])[1]
                return mistral._moe_bwd(moe, mu, dm, h, mws, ms, saved, daux if on else None)

            t_off, t_on = [], []
            for rep_ in range(a.reps + 3):
                t0, _ = _timed(lambda: step(False))
                t1, _ = _timed(lambda: step(True))
                if rep_ >= 3:
                    t_off.append(t0)
                    t_on.append(t1)
            m0, m1 = statistics.median(t_off), statistics.median(t_on)
            lines.append(f"{rows} {factor} {m0:.3f} {m1:.3f} {m1 / m0:.4f}")
            print(lines[-1], flush=True)
            wr = mws[4]
            del moe, mws, ms
            torch.cuda.empty_cache()
        dl = torch.randn(rows, E, device=dev)
        dwr = torch.empty_like(wr)
        n_ring = max(2, -(-WG_RING_MB * (1 << 20) // (h.numel() * h.element_size())))
        ring = [h] + [h.clone() for _ in range(n_ring - 1)]
        row = f"{rows} {E} {d}"
        for hs in ([h], ring):

            def batch(dense):
                for j in range(WG_BATCH):
                    F_.moe_router_wgrad(dl, hs[j % len(hs)], dwr, False, dense=dense)

            ts = ([], [])
            for rep_ in range(a.reps + 2):
                for dense in (False, True):
                    t = _timed(lambda: batch(dense))[0] / WG_BATCH
                    if rep_ >= 2:
                        ts[dense].append(t)
            sp, de = statistics.median(ts[0]), statistics.median(ts[1])
            row += f" {sp:.4f} {de:.4f} {de / sp:.3f}"
        del ring
        torch.cuda.empty_cache()
        wg.append(row)
        print(wg[-1], flush=True)
    lines += wg + [f"# written {time.strftime('%Y-%m-%d')}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    print(f"appended to {a.out}")


if __name__ == "__main__":
    main()
