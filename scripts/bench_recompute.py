#!/usr/bin/env python3
"""What ``--activation-recompute`` costs and buys on one MI355X (writes profiles/activation_recompute.txt).

    python scripts/bench_recompute.py [--out profiles/activation_recompute.txt] [--parent-tree DIR]
                                      [--skip steps,rows,kernels]

Three measurements, every training run a fresh ``python -m dltb.harness`` child process (nothing is shared
between runs but the box):

* steps:   Mistral-7B shape, ZeRO-3, 1 GPU, seq 4096, 4 micro-steps per window; ms per micro-step (the harness's
           synchronised wall time over the timed steps) and peak HBM for off / selective / full, ``--rounds``
           rounds with the modes interleaved, so the spread of a mode over the rounds is on the page beside the
           differences between modes.  With ``--parent-tree`` (a built checkout of the parent commit) the parent
           runs in the same rounds, next to ``off``.
* rows:    for each mode the longest of seq 32768 / 16384 / 8192 that completes 3 steps, tried longest first,
           with its peak HBM; a row that does not fit ends its child with HIP's out-of-memory error.
* kernels: swiglu_bwd_h against swiglu_fwd + swiglu_bwd and norm_apply against norm_fwd at the M7B row shape
           (4096 tokens x 14336 / 4096), HIP-graph timed, with the bytes each must move and the share of the
           8 TB/s HBM peak that makes.

A child that ends in anything but success -- or, in the rows section only, the allocator's clean out-of-memory
error -- ends the whole script at once (exit status 1): nothing more is started on a GPU that may have faulted.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("off", "selective", "full")
HBM_PEAK = 8.0e12            # bytes / s, MI355X


class Stop(RuntimeError):
    """A child died, hung or failed in a way that is not a clean out-of-memory error: start nothing more."""


def harness_run(tree, mode, seq, steps, warmup, accum, timeout, oom_ok=False):
    """One harness child in ``tree``: (record, sidecar).  With ``oom_ok`` a child that ended with Python's exit
    status 1 on the allocator's out-of-memory error gives (None, its message); every other failure raises Stop."""
    with tempfile.TemporaryDirectory() as res:
        cmd = [sys.executable, "-m", "dltb.harness", "--strategy", "zero3", "--tier", "M7B", "--seq-len", str(seq),
               "--steps", str(steps), "--warmup-steps", str(warmup), "--per-device-batch", "1",
               "--grad-accum", str(accum), "--results-dir", res, "--log-every", "0"]
        if mode is not None:
            cmd += ["--activation-recompute", mode]
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
        try:
            r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=timeout)
        except subprocess.TimeoutExpired:
            raise Stop(f"{mode} seq {seq}: no result after {timeout} s")
        if r.returncode != 0:
            text = r.stdout + r.stderr
            tail = " | ".join([ln for ln in text.splitlines() if ln.strip()][-3:])[-400:]
            if oom_ok and r.returncode == 1 and "out of memory" in text and "illegal memory access" not in text:
                return None, tail
            raise Stop(f"{mode} seq {seq}: exit status {r.returncode}: {tail}")
        base = os.path.join(res, f"result_zero3_ws1_seq{seq}_tierM7B")
        with open(base + ".json") as f:
            rec = json.load(f)
        with open(base + ".extended.json") as f:
            side = json.load(f)
        return rec, side


def bench_steps(log, parent, rounds):
    log("== steps: M7B, zero3, 1 GPU, seq 4096, batch 1, accum 4, 8 warm-up + 8 timed micro-steps per run")
    names = (["parent"] if parent else []) + list(MODES)
    got = {n: [] for n in names}
    for rnd in range(rounds):
        for n in names:
            rec, side = harness_run(parent if n == "parent" else ROOT, None if n == "parent" else n, 4096, 16, 8, 4,
                                    900)
            got[n].append((rec["mean_step_time_sec"] * 1e3, rec["peak_vram_gb"]))
            log(f"round {rnd} {n:9s}: {got[n][-1][0]:8.2f} ms / micro-step   peak HBM {got[n][-1][1]:7.2f} GB   "
                f"loss {rec['mean_loss']:.4f}   graphs {side['hip_graphs']}")
    log("mode       ms / micro-step (min .. max over rounds)   peak HBM GB   vs off")
    off = min(t for t, _ in got["off"]) if got["off"] else None
    for n in names:
        if got[n]:
            ts = [t for t, _ in got[n]]
            log(f"{n:9s}  {min(ts):8.2f} .. {max(ts):8.2f}                      {max(m for _, m in got[n]):7.2f}"
                + (f"       {min(ts) / off:5.3f} x" if off else ""))


def bench_rows(log):
    log("== longest row: M7B, zero3, 1 GPU, batch 1, accum 1, 3 steps (1 warm-up), tried longest first")
    for mode in MODES:
        for seq in (32768, 16384, 8192):
            rec, side = harness_run(ROOT, mode, seq, 3, 1, 1, 400, oom_ok=True)
            if rec is None:
                log(f"{mode:9s} seq {seq:5d}: does not complete: {side}")
                continue
            log(f"{mode:9s} seq {seq:5d}: completes, {rec['mean_step_time_sec'] * 1e3:9.1f} ms / step, "
                f"peak HBM {rec['peak_vram_gb']:.2f} GB")
            break
        else:
            log(f"{mode:9s}: none of the three lengths completes")


def bench_kernels(log):
    sys.path.insert(0, ROOT)
    import torch
    import dltb  # noqa: F401
    from dltb.ops._ext import ext
    C = ext()

    def t_us(fn, iters=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        best = None
        for _ in range(5):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            torch.cuda.synchronize()
            t = s.elapsed_time(e) / iters * 1e3
            best = t if best is None else min(best, t)
        return best

    N, d, f = 4096, 4096, 14336
    bf = dict(device="cuda", dtype=torch.bfloat16)
    gu, dh = torch.randn(N, 2 * f, **bf), torch.randn(N, f, **bf)
    x, w = torch.randn(N, d, **bf), torch.ones(d, **bf)
    _, y, _, rstd = C.norm_fwd(x, None, w, None, 1e-5, True, 0.0, None, 0)
    assert torch.equal(C.norm_apply(x, w, None, None, rstd, True), y)
    dgu, h = C.swiglu_bwd_h(dh, gu)
    assert torch.equal(h, C.swiglu_fwd(gu)) and torch.equal(dgu, C.swiglu_bwd(dh, gu))
    e = 2 * N                                            # bytes of one bf16 column over all rows
    rows = [("swiglu_fwd + swiglu_bwd (2 launches)", lambda: (C.swiglu_fwd(gu), C.swiglu_bwd(dh, gu)), e * f * 8),
            ("swiglu_bwd_h (1 launch)", lambda: C.swiglu_bwd_h(dh, gu), e * f * 6),
            ("swiglu_bwd alone (off's launch)", lambda: C.swiglu_bwd(dh, gu), e * f * 5),
            ("norm_fwd RMS (row statistics + y)", lambda: C.norm_fwd(x, None, w, None, 1e-5, True, 0.0, None, 0),
             e * d * 2),
            ("norm_apply RMS (y from rstd)", lambda: C.norm_apply(x, w, None, None, rstd, True), e * d * 2)]
    log(f"== kernels at the M7B row shape: {N} tokens, d {d}, ffn {f}, bf16; best of 5 graph replays of 20 calls")
    log("kernel                                      us / call   bytes moved   share of 8 TB/s")
    for name, fn, nbytes in rows:
        us = t_us(fn)
        log(f"{name:42s} {us:9.1f}   {nbytes / 1e6:8.1f} MB   {nbytes / (us * 1e-6) / HBM_PEAK:6.1%}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activation_recompute.txt"))
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (off vs parent pairs)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip", default="", help="comma list of steps, rows, kernels")
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernels_child:
        bench_kernels(lambda s: print(s, flush=True))
        return 0
    skip = set(filter(None, a.skip.split(",")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        def log(s):
            print(s, flush=True)
            out.write(s + "\n")
            out.flush()
        log(f"# scripts/bench_recompute.py, {time.strftime('%Y-%m-%d')}; every run its own process on one MI355X")
        try:
            if "kernels" not in skip:
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels-child"],
                                       capture_output=True, text=True, timeout=300)
                except subprocess.TimeoutExpired:
                    raise Stop("kernels: no result after 300 s")
                if r.returncode != 0:
                    raise Stop(f"kernels: exit status {r.returncode}: {r.stderr[-400:]}")
                log(r.stdout.rstrip())
            if "steps" not in skip:
                bench_steps(log, a.parent_tree, a.rounds)
            if "rows" not in skip:
                bench_rows(log)
        except Stop as e:
            log(f"STOPPED, nothing more was started: {e}")
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
