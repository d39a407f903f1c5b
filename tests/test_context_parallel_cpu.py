"""Context parallelism (dltb/parallel/context.py) without a GPU: the layout arithmetic, the fp32 reference's
query-range semantics, the refusals, the harness's token accounting, and on gloo the world-2 / world-4 runs of
scripts/multirank_check.py with ``--context-parallel 2`` against the world-1 run on the same rows (helpers of
tests/multirank_util.py, tolerances of tests/test_multirank_cpu.py)."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import dltb
from dltb import harness
from dltb.models import build_model, get_model_config
from dltb.ops import functional as F_
from dltb.ops import ref
from dltb.parallel import context as cpx
from multirank_util import compare, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)     # tests/test_multirank_cpu.py


# ------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("layout", cpx.LAYOUTS)
@pytest.mark.parametrize("cp", [1, 2, 4, 8])
def test_ranges_partition_the_row(layout, cp):
    T = 256 * cp * 2
    seen = torch.zeros(T, dtype=torch.int64)
    for r in range(cp):
        rngs = cpx.ranges(layout, T, cp, r)
        assert len(rngs) == (1 if cp == 1 or layout == "contiguous" else 2)
        assert sum(e - b for b, e in rngs) == T // cp
        for b, e in rngs:
            assert b % 128 == 0 and e % 128 == 0 and 0 <= b < e <= T
            seen[b:e] += 1
    assert torch.equal(seen, torch.ones_like(seen))


@pytest.mark.parametrize("cp", [2, 4, 8])
def test_visible_pairs_zigzag_equal_contiguous_odd(cp):
    T = 256 * cp
    dense = torch.ones(T, T).tril()
    zz = [cpx.visible_pairs(cpx.ranges("zigzag", T, cp, r), T) for r in range(cp)]
    ct = [cpx.visible_pairs(cpx.ranges("contiguous", T, cp, r), T) for r in range(cp)]
    for layout, counts in (("zigzag", zz), ("contiguous", ct)):      # the closed form counts the dense mask
        for r, c in enumerate(counts):
            assert c == sum(int(dense[b:e].sum()) for b, e in cpx.ranges(layout, T, cp, r))
    assert sum(zz) == sum(ct) == T * (T + 1) // 2
    assert len(set(zz)) == 1
    n = T // cp          # contiguous rank r: n^2 r + n (n + 1) / 2 -- proportional to 2 r + 1 up to the diagonal
    for r, c in enumerate(ct):
        assert c == n * n * r + n * (n + 1) // 2
        assert abs(c / ct[0] - (2 * r + 1)) < 2 * r / n + 1e-12
    # a window evens the contiguous layout out: every rank but the first sees W keys per query
    W = 64
    cw = [cpx.visible_pairs(cpx.ranges("contiguous", T, cp, r), T, W) for r in range(cp)]
    band = torch.ones(T, T).tril() - torch.ones(T, T).tril(-W)
    assert cw == [int(band[b:e].sum()) for r in range(cp) for b, e in cpx.ranges("contiguous", T, cp, r)]
    assert len(set(cw[1:])) == 1


def test_auto_layout():
    assert cpx.resolve_layout("auto", None) == "zigzag"
    assert cpx.resolve_layout("auto", 4096) == "contiguous"
    assert cpx.resolve_layout("zigzag", 4096) == "zigzag"
    with pytest.raises(ValueError, match="layout"):
        cpx.resolve_layout("ring")


def test_owner_and_position_order_tables():
    """The row gathers between what all_gather produces ([rank][range][b][t]) and position order."""
    B, T, cp = 2, 1024, 2
    full = torch.arange(B * T).view(B, T)
    for layout in cpx.LAYOUTS:
        objs = [cpx.ContextParallel.__new__(cpx.ContextParallel) for _ in range(cp)]
        for r, o in enumerate(objs):
            o.cp, o.layout, o.rank, o._index = cp, layout, r, {}
        owner = torch.cat([o.slice_rows(full, T).reshape(-1) for o in objs])
        to_pos, to_owner = objs[0]._tables(B, T, "cpu")
        assert torch.equal(owner[to_pos], full.reshape(-1))
        assert torch.equal(full.reshape(-1)[to_owner], owner)


# ------------------------------------------------------------------------------------------- reference semantics
def _dense(q, k, v, B, T, Hq, Hkv, D, scale, keep):
    """softmax(q k^T scale + mask) v with an explicit [B, T, T] keep mask, fp64."""
    G = Hq // Hkv
    qh = q.double().view(B, T, Hq, D).transpose(1, 2)
    kh = k.double().view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(G, 1)
    vh = v.double().view(B, T, Hkv, D).transpose(1, 2).repeat_interleave(G, 1)
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s.masked_fill(~keep[:, None], float("-inf"))
    return torch.softmax(s, -1) @ vh, torch.logsumexp(s, -1)


@pytest.mark.parametrize("mask", ["causal", "window", "doc"])
def test_ref_query_range_against_dense_softmax(mask):
    B, T, Hq, Hkv, D = 2, 256, 4, 2, 16
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B * T, Hq * D, generator=g, dtype=torch.float64).requires_grad_()
    k = torch.randn(B * T, Hkv * D, generator=g, dtype=torch.float64).requires_grad_()
    v = torch.randn(B * T, Hkv * D, generator=g, dtype=torch.float64).requires_grad_()
    do = torch.randn(B * T, Hq * D, generator=g, dtype=torch.float64)
    scale = 1.0 / math.sqrt(D)
    i = torch.arange(T)
    keep = (i[None, :] <= i[:, None]).expand(B, T, T).clone()
    window, bounds = 0, None
    if mask == "window":
        window = 40
        keep &= (i[None, :] > i[:, None] - window)
    if mask == "doc":
        idx = torch.randint(0, 8, (B, T), generator=g)
        bounds = ref.doc_bounds(idx, 7, 0)
        keep &= i[None, None, :] >= bounds[0].long()[:, :, None]
    od, lsed = _dense(q, k, v, B, T, Hq, Hkv, D, scale, keep)          # [B, Hq, T, D]
    sel = lambda x, b, e: x.view(B, T, -1)[:, b:e].reshape(B * (e - b), -1)
    dk_sum, dv_sum = torch.zeros_like(k), torch.zeros_like(v)
    for b, e in [(0, 128), (128, 256)]:
        o, lse = ref.attn_fwd(sel(q, b, e).detach(), k.detach(), v.detach(), B, T, Hq, Hkv, scale, True, 0.0, None,
                              0, window, bounds, q_range=(b, e))
        want = od[:, :, b:e].transpose(1, 2).reshape(B * (e - b), Hq * D)
        assert torch.allclose(o, want.detach(), atol=1e-10)
        assert torch.allclose(lse.double(), lsed[:, :, b:e].detach(), atol=1e-5)      # ref returns lse in fp32
        # gradients of the range's rows alone
        gq, gk, gv = torch.autograd.grad(want, (q, k, v), sel(do, b, e), retain_graph=True)
        dq = torch.empty(B * (e - b), Hq * D, dtype=torch.float64)
        dk, dv = torch.empty_like(k), torch.empty_like(v)
        ref.attn_bwd(sel(q, b, e).detach(), k.detach(), v.detach(), o, sel(do, b, e), lsed[:, :, b:e].detach(), dq,
                     dk, dv, B, T, Hq, Hkv, scale, True, 0.0, None, 0, window, bounds, q_range=(b, e))
        assert torch.allclose(dq, sel(gq, b, e), atol=1e-9)
        assert torch.allclose(dk, gk, atol=1e-9) and torch.allclose(dv, gv, atol=1e-9)
        tail = dk.view(B, T, -1)[:, e:]
        assert torch.equal(tail, torch.zeros_like(tail))               # keys past the range: exactly zero
        dk_sum += dk
        dv_sum += dv
    gk, gv = torch.autograd.grad(od.transpose(1, 2).reshape(B * T, Hq * D), (k, v), do)
    assert torch.allclose(dk_sum, gk, atol=1e-9) and torch.allclose(dv_sum, gv, atol=1e-9)


def test_ref_query_range_refusals():
    B, T, Hq, Hkv, D = 1, 256, 2, 1, 16
    q, k = torch.randn(B * 128, Hq * D), torch.randn(B * T, Hkv * D)
    with pytest.raises(ValueError, match="dropout"):
        F_.attn_fwd(q, k, k, B, T, Hq, Hkv, 0.25, True, 0.1, None, 0, q_range=(128, 256))
    with pytest.raises(ValueError, match="causal"):
        F_.attn_fwd(q, k, k, B, T, Hq, Hkv, 0.25, False, 0.0, None, 0, q_range=(128, 256))
    with pytest.raises(ValueError, match="multiples of 128"):
        F_.attn_fwd(q, k, k, B, T, Hq, Hkv, 0.25, True, 0.0, None, 0, q_range=(64, 192))
    for bad in [(128, 128), (256, 128), (128, 384)]:
        with pytest.raises(ValueError, match="begin < end"):
            F_.attn_fwd(q, k, k, B, T, Hq, Hkv, 0.25, True, 0.0, None, 0, q_range=bad)


# ------------------------------------------------------------------------------------------- refusals, accounting
def test_refusals():
    tiny = get_model_config("tiny", 512)
    mt = get_model_config("mtiny", 512)
    with pytest.raises(ValueError, match="causal"):
        harness.check_context_parallel(2, "auto", 2, tiny, 512)
    with pytest.raises(ValueError, match="causal"):
        cpx.ContextParallel(1).attach(build_model(tiny))
    with pytest.raises(ValueError, match="multiple of 512"):
        harness.check_context_parallel(2, "zigzag", 2, mt, 768)
    with pytest.raises(ValueError, match="multiple of 256"):
        harness.check_context_parallel(2, "contiguous", 2, mt, 640)
    assert harness.check_context_parallel(2, "contiguous", 2, mt, 768) == "contiguous"
    with pytest.raises(ValueError, match="divide the world size"):
        harness.check_context_parallel(2, "auto", 3, mt, 512)
    with pytest.raises(ValueError, match="divide the world size"):
        cpx.ContextParallel(2, world=3, rank=0)
    assert cpx.ContextParallel(1).attach(build_model(mt)).cp is None


def test_emulated_fabric_refused(monkeypatch):
    monkeypatch.setenv("DLTB_COMM", "emulate:8")
    with pytest.raises(ValueError, match="emulate"):
        cpx.ContextParallel(2, world=8, rank=0)


def test_harness_cli_refusals():
    base = [sys.executable, "-m", "dltb.harness", "--strategy", "zero2", "--steps", "1", "--per-device-batch", "1",
            "--grad-accum", "1", "--results-dir", os.devnull, "--device", "cpu"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    for extra, msg in [(["--tier", "tiny", "--seq-len", "512", "--context-parallel", "1", "--world-size", "1"], None),
                       (["--tier", "mtiny", "--seq-len", "512", "--context-parallel", "2", "--world-size", "3"],
                        "divide the world size"),
                       (["--tier", "tiny", "--seq-len", "512", "--context-parallel", "2", "--world-size", "2"],
                        "causal tier"),
                       (["--tier", "mtiny", "--seq-len", "384", "--context-parallel", "2", "--world-size", "2"],
                        "multiple of 512")]:
        if msg is None:
            continue
        r = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT, env=env, timeout=120)
        assert r.returncode == 2 and msg in r.stderr, (extra, r.stderr[-500:])


def test_token_accounting():
    assert harness.tokens_per_micro_step(2, 512, 2, 1) == 2 * 512 * 2
    assert harness.tokens_per_micro_step(2, 512, 2, 2) == 2 * 512          # two ranks, one set of rows
    assert harness.tokens_per_micro_step(1, 32768, 8, 8) == 32768
    assert harness.tokens_per_micro_step(1, 32768, 8, 2) == 4 * 32768


def _harness(tmp_path, world, extra, name):
    out = tmp_path / name
    cmd = [sys.executable, "-m", "dltb.harness"] if world == 1 else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
         "--master-addr=127.0.0.1", "--master-port=29617", "--max-restarts=0", "-m", "dltb.harness"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    r = subprocess.run(cmd + ["--strategy", "zero2", "--tier", "mtiny", "--seq-len", "512", "--steps", "3",
                              "--warmup-steps", "1", "--per-device-batch", "2", "--grad-accum", "1", "--device", "cpu",
                              "--dtype", "fp32", "--results-dir", str(out), *extra],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    base = out / f"result_zero2_ws{world}_seq512_tiermtiny"
    with open(f"{base}.json") as f:
        rec = json.load(f)
    with open(f"{base}.extended.json") as f:
        ext = json.load(f)
    return rec, ext


def test_harness_cp2_counts_its_tokens_once(tmp_path):
    """World 2 with cp = 2 trains the rows world 1 trains: same mean loss, half the tokens the record's
    world-size formula would claim, and the sidecar records the group's layout."""
    r1, e1 = _harness(tmp_path, 1, [], "w1")
    r2, e2 = _harness(tmp_path, 2, ["--context-parallel", "2"], "w2")
    assert list(r1) == list(r2)                                    # the reference-format keys do not change
    assert e1["context_parallel"] == 1 and e1["cp_ranges"] is None
    assert e2["context_parallel"] == 2 and e2["cp_layout"] == "zigzag"
    assert e2["cp_ranges"] == [[[0, 128], [384, 512]], [[128, 256], [256, 384]]]
    assert e2["tokens_per_micro_step"] == 2 * 512 == e1["tokens_per_micro_step"]
    assert abs(r2["tokens_per_sec"] * r2["mean_step_time_sec"] - 2 * 512) < 1e-6 * 2 * 512
    assert abs(r1["mean_loss"] - r2["mean_loss"]) < 1e-4 * abs(r1["mean_loss"])
    assert e2["hip_graphs"] is False


# ------------------------------------------------------------------------------------------- world-size equivalence
CP_ARGS = ("--seq-len", "512", "--windows", "2")
ALL = "cp_ddp,cp_fsdp,cp_zero2,cp_zero3,cp_zero3_window,cp_zero2_doc"


@pytest.fixture(scope="module")
def ws1(tmp_path_factory):
    """The world-1 run of every context-parallel case, computed once."""
    d = tmp_path_factory.mktemp("cp_ws1")
    return run(d / "ws1.pt", 1, "cpu", extra=CP_ARGS + ("--cases", ALL))


@pytest.mark.parametrize("layout", ["zigzag", "contiguous"])
def test_world2_cp2_equals_world1_cpu(tmp_path, ws1, layout):
    got = run(tmp_path / "ws2.pt", 2, "cpu",
              extra=CP_ARGS + ("--cases", ALL, "--context-parallel", "2", "--cp-layout", layout))
    assert set(got) == set(ALL.split(","))
    bad = compare({k: ws1[k] for k in got}, got, **TOL)
    assert not bad, bad


def test_world4_cp2_equals_world1_cpu(tmp_path, ws1):
    """Two groups of two: rows dealt to the groups, each row split inside its group (auto layout: the windowed
    case runs contiguous, the others zigzag)."""
    cases = "cp_zero3,cp_zero3_window"
    got = run(tmp_path / "ws4.pt", 4, "cpu", extra=CP_ARGS + ("--cases", cases, "--context-parallel", "2"))
    bad = compare({k: ws1[k] for k in got}, got, **TOL)
    assert not bad, bad
