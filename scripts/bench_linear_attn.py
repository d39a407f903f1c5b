#!/usr/bin/env python3
"""Fixed-decay linear attention (csrc/linear_attn.hip) against the full-causal softmax attention kernels at the M7B
head shape (Hq 32, Hkv 8, D 128, bf16, B 1), forward and backward, in one process.

Per sequence length the four calls (linear fwd, softmax fwd, linear bwd, softmax bwd) alternate over ``--rounds``
rounds of ``--iters`` calls after a warm-up round; each call of a round takes the next buffer set of a ring whose
operands together exceed ``--ring-mib`` (larger than the 256 MiB last-level cache), so no call finds its inputs
cached by the one before.  The median round is reported with its min .. max.  No ratio is a pass condition; the file
records what was measured, including the first measured T at which the linear mixer is below softmax attention.

    python scripts/bench_linear_attn.py --out profiles/linear_attn.txt
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dltb  # noqa: E402,F401
from dltb.ops import functional as F_  # noqa: E402
from dltb.ops._ext import ext  # noqa: E402


def timeit(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for i in range(iters):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3   # us


def run(T, iters, rounds, ring_mib, emit, B=1, Hq=32, Hkv=8, D=128):
    C, dev = ext(), "cuda"
    qd, kd = Hq * D, Hkv * D
    per_set = B * T * (qd + 2 * kd + qd) * 2
    n = max(2, -(-ring_mib * 2 ** 20 // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    l2g = F_.linear_attn_log2_gamma(Hkv, dev)
    scale = D ** -0.5
    sets = []
    for _ in range(n):
        qkv = torch.randn(B * T, qd + 2 * kd, device=dev, dtype=torch.bfloat16, generator=g)
        do = torch.randn(B * T, qd, device=dev, dtype=torch.bfloat16, generator=g)
        q, k, v = qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:]
        sets.append((q, k, v, do))
    o = torch.empty(B * T, qd, device=dev, dtype=torch.bfloat16)
    dqkv = torch.empty(B * T, qd + 2 * kd, device=dev, dtype=torch.bfloat16)
    dq, dk, dv = dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:]
    so, lse = C.attn_fwd(*sets[0][:3], None, B, T, Hq, Hkv, scale, True, 0.0)   # any o / lse: the time does not depend on them

    def lin_fwd(i):
        q, k, v, _ = sets[i % n]
        C.linear_attn_fwd(q, k, v, l2g, B, T, Hq, Hkv, o)

    def soft_fwd(i):
        q, k, v, _ = sets[i % n]
        C.attn_fwd(q, k, v, None, B, T, Hq, Hkv, scale, True, 0.0, o)

    def lin_bwd(i):
        q, k, v, do = sets[i % n]
        C.linear_attn_bwd(q, k, v, do, dq, dk, dv, l2g, B, T, Hq, Hkv)

    def soft_bwd(i):
        q, k, v, do = sets[i % n]
        C.attn_bwd(q, k, v, so, do, lse, None, dq, dk, dv, B, T, Hq, Hkv, scale, True, 0.0)

    fns = {"linear fwd": lin_fwd, "softmax fwd": soft_fwd, "linear bwd": lin_bwd, "softmax bwd": soft_bwd}
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
    emit(f"T {T:6d}  ring {n} sets of {per_set / 2 ** 20:.0f} MiB")
    for key in fns:
        emit(f"    {key:12s} {med[key]:10.1f} us  ({min(times[key]):.1f} .. {max(times[key]):.1f})")
    emit(f"    linear / softmax: fwd {med['linear fwd'] / med['softmax fwd']:.3f}  bwd "
         f"{med['linear bwd'] / med['softmax bwd']:.3f}  fwd + bwd "
         f"{(med['linear fwd'] + med['linear bwd']) / (med['softmax fwd'] + med['softmax bwd']):.3f}")
    del sets
    torch.cuda.empty_cache()
    return (med["linear fwd"] + med["linear bwd"]) / (med["softmax fwd"] + med["softmax bwd"])


def run_gate(T, iters, rounds, ring_mib, emit, B=1, Hq=32, Hkv=8, D=128, d=4096, rank=0):
    """One layer's mixer under ``--linear-attn-gate`` (gate_fwd, the gated forward and backward, gate_bwd with its
    in-place dxn term, the gate's weight gradient) against the fixed-decay forward + backward, same operands.
    ``rank``: the per-channel gate of that rank (csrc/linear_attn_chgate.hip) against the scalar-gated calls, with a
    per-kernel breakdown of the per-channel mixer calls."""
    dev = "cuda"
    qd, kd = Hq * D, Hkv * D
    per_set = B * T * (qd + 2 * kd + qd + 2 * d) * 2
    n = max(2, -(-ring_mib * 2 ** 20 // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    l2g, bias = F_.linear_attn_log2_gamma(Hkv, dev), F_.linear_attn_gate_bias(Hkv, dev)
    wg = (0.02 * torch.randn(Hkv, d, device=dev, generator=g)).bfloat16()
    dwg = torch.empty_like(wg)
    sets = []
    for _ in range(n):
        qkv = torch.randn(B * T, qd + 2 * kd, device=dev, dtype=torch.bfloat16, generator=g)
        do = torch.randn(B * T, qd, device=dev, dtype=torch.bfloat16, generator=g)
        xn = torch.randn(B * T, d, device=dev, dtype=torch.bfloat16, generator=g)
        sets.append((qkv[:, :qd], qkv[:, qd:qd + kd], qkv[:, qd + kd:], do, xn, torch.zeros_like(xn)))
    o = torch.empty(B * T, qd, device=dev, dtype=torch.bfloat16)
    dqkv = torch.empty(B * T, qd + 2 * kd, device=dev, dtype=torch.bfloat16)
    dq, dk, dv = dqkv[:, :qd], dqkv[:, qd:qd + kd], dqkv[:, qd + kd:]
    z0, cum0 = F_.linear_attn_gate_fwd(sets[0][4], wg, bias, B, T)
    gq0, gk0 = torch.randn(B * T, Hq, device=dev, generator=g), torch.randn(B * T, Hkv, device=dev, generator=g)

    def fixed(i):
        q, k, v, do = sets[i % n][:4]
        F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o)
        F_.linear_attn_bwd(q, k, v, do, dq, dk, dv, B, T, Hq, Hkv, l2g)

    def gated(i):
        q, k, v, do, xn, dxn = sets[i % n]
        z, cum = F_.linear_attn_gate_fwd(xn, wg, bias, B, T)
        F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o, cum=cum)
        gq, gk = F_.linear_attn_bwd(q, k, v, do, dq, dk, dv, B, T, Hq, Hkv, l2g, cum=cum)
        dz = F_.linear_attn_gate_bwd(gq, gk, z, bias, wg, dxn, B, T)
        F_.moe_router_wgrad(dz, xn, dwg, False, dense=True)

    def gate_fwd(i):
        F_.linear_attn_gate_fwd(sets[i % n][4], wg, bias, B, T)

    def gate_bwd(i):
        F_.linear_attn_gate_bwd(gq0, gk0, z0, bias, wg, sets[i % n][5], B, T)

    fns = {"fixed fwd+bwd": fixed, "gated fwd+bwd": gated, "gate_fwd": gate_fwd, "gate_bwd": gate_bwd}
    base = "fixed fwd+bwd"
    if rank:
        w1 = (0.02 * torch.randn(rank, d, device=dev, generator=g)).bfloat16()
        w2 = (0.02 * torch.randn(kd, rank, device=dev, generator=g)).bfloat16()
        dw1, dw2 = torch.empty_like(w1), torch.empty_like(w2)
        z10, cumc = F_.linear_attn_gate_fwd(sets[0][4], w1, bias, B, T, up=w2)
        gqc, gkc = torch.randn(B * T, qd, device=dev, generator=g), torch.randn(B * T, kd, device=dev, generator=g)

        def chan(i):
            q, k, v, do, xn, dxn = sets[i % n]
            z1, cum = F_.linear_attn_gate_fwd(xn, w1, bias, B, T, up=w2)
            F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o, cum=cum)
            gq, gk = F_.linear_attn_bwd(q, k, v, do, dq, dk, dv, B, T, Hq, Hkv, l2g, cum=cum)
            dz1 = F_.linear_attn_gate_bwd(gq, gk, z1, bias, w1, dxn, B, T, up=w2, dup=dw2)[0]
            F_.moe_router_wgrad(dz1, xn, dw1, False, dense=True)

        def chan_fwd(i):
            q, k, v = sets[i % n][:3]
            F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o, cum=cumc)

        def chan_bwd(i):
            q, k, v, do = sets[i % n][:4]
            F_.linear_attn_bwd(q, k, v, do, dq, dk, dv, B, T, Hq, Hkv, l2g, cum=cumc)

        def scalar_fwd(i):
            q, k, v = sets[i % n][:3]
            F_.linear_attn_fwd(q, k, v, B, T, Hq, Hkv, l2g, o_out=o, cum=cum0)

        def scalar_bwd(i):
            q, k, v, do = sets[i % n][:4]
            F_.linear_attn_bwd(q, k, v, do, dq, dk, dv, B, T, Hq, Hkv, l2g, cum=cum0)

        fns = {"gated fwd+bwd": gated, "chgate fwd+bwd": chan, "scalar mixer fwd": scalar_fwd, "chgate mixer fwd": chan_fwd,
               "scalar mixer bwd": scalar_bwd, "chgate mixer bwd": chan_bwd,
               "chgate gate_fwd": lambda i: F_.linear_attn_gate_fwd(sets[i % n][4], w1, bias, B, T, up=w2),
               "chgate gate_bwd": lambda i: F_.linear_attn_gate_bwd(gqc, gkc, z10, bias, w1, sets[i % n][5], B, T, up=w2,
                                                                     dup=dw2)}
        base = "gated fwd+bwd"
    times = {key: [] for key in fns}
    for r in range(rounds + 1):                 # round 0 warms up
        for key, fn in fns.items():
            us = timeit(fn, iters)
            if r:
                times[key].append(us)
    med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
    emit(f"T {T:6d}  ring {n} sets of {per_set / 2 ** 20:.0f} MiB")
    for key in fns:
        emit(f"    {key:16s} {med[key]:10.1f} us  ({min(times[key]):.1f} .. {max(times[key]):.1f})")
    lo, hi = min(times[base]) / med[base], max(times[base]) / med[base]
    ratio = med["chgate fwd+bwd" if rank else "gated fwd+bwd"] / med[base]
    emit(f"    {'per-channel / scalar-gated' if rank else 'gated / fixed'}: {ratio:.3f}; the {base.split()[0]} call's own "
         f"spread is {lo:.3f} .. {hi:.3f}: "
         f"{'outside' if ratio > hi or ratio < lo else 'inside'} it")
    del sets
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq-lens", default="4096,16384,32768")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ring-mib", type=int, default=320)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gate-rank", type=int, default=0,
                    help="measure the per-channel gate of this rank (--linear-attn-gate-rank) against the scalar-gated calls")
    ap.add_argument("--gate", action="store_true",
                    help="measure one layer's mixer under --linear-attn-gate against the fixed-decay calls instead")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.gate_rank:
        emit(f"# scripts/bench_linear_attn.py --gate-rank {a.gate_rank}: per-channel gated linear attention "
             "(csrc/linear_attn_chgate.hip: gate_fwd,")
        emit("# the mixer's fwd and bwd, gate_bwd with dW2 and the in-place dxn term, dW1) against the scalar-gated calls "
             "in the same process,")
        emit(f"# M7B head shape (B 1, Hq 32, Hkv 8, D 128, n_embd 4096, bf16), {torch.cuda.get_device_name(0)}; medians of "
             f"{a.rounds}")
        emit(f"# interleaved rounds of {a.iters} calls (min .. max), operand rings of more than {a.ring_mib} MiB.")
        for T in (int(t) for t in a.seq_lens.split(",")):
            run_gate(T, a.iters, a.rounds, a.ring_mib, emit, rank=a.gate_rank)
        emit("# not measured: the end-to-end step under --linear-attn-gate-rank, loss curves, several GPUs")
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if a.gate:
        emit("# scripts/bench_linear_attn.py --gate: gated linear attention (csrc/linear_attn_gate.hip: gate_fwd, gated fwd,")
        emit("# gated bwd, gate_bwd with the in-place dxn term, the gate's weight gradient) against the fixed-decay fwd + bwd,")
        emit(f"# M7B head shape (B 1, Hq 32, Hkv 8, D 128, n_embd 4096, bf16), {torch.cuda.get_device_name(0)}; medians of "
             f"{a.rounds}")
        emit(f"# interleaved rounds of {a.iters} calls (min .. max), operand rings of more than {a.ring_mib} MiB.")
        for T in (int(t) for t in a.seq_lens.split(",")):
            run_gate(T, a.iters, a.rounds, a.ring_mib, emit)
        emit("# not measured: the end-to-end step under --linear-attn-gate, loss curves, several GPUs")
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    emit("# scripts/bench_linear_attn.py: fixed-decay linear attention against full-causal softmax attention, M7B head")
    emit(f"# shape (B 1, Hq 32, Hkv 8, D 128, bf16), {torch.cuda.get_device_name(0)}; medians of {a.rounds} interleaved "
         f"rounds of {a.iters} calls")
    emit(f"# (min .. max), operand rings of more than {a.ring_mib} MiB.  The linear backward includes rebuilding the states.")
    cross = None
    for T in (int(t) for t in a.seq_lens.split(",")):
        ratio = run(T, a.iters, a.rounds, a.ring_mib, emit)
        if cross is None and ratio < 1.0:
            cross = T
    emit("# linear fwd + bwd below softmax fwd + bwd from the measured T = " + (str(cross) if cross else "none measured"))
    emit("# end-to-end step time under --linear-attn: not measured")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
