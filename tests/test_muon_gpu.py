"""The Muon kernels (csrc/muon.hip) against float64 of the same bf16 inputs, and ``--optimizer muon`` end to end.

Bounds are those of tests/gemm_ref.py: half a bf16 ulp of the exact value plus the fp32 bound of a K-term sum over
the magnitudes of its terms (``bound``), nothing fitted.  The elementwise kernels get the same form with the handful
of fp32 roundings they make."""
import itertools
import json
import math
import os

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.ops import ref
from dltb.ops._ext import ext
from dltb.optim.muon import FlatMuon, muon_matrices
from dltb.parallel.strategy import engine_config, make_engine
from gemm_ref import U, bound, half_ulp, poisoned_view, report
from multirank_util import report as rank_report
from multirank_util import run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
A_, B_, C_ = ref.MUON_ABC


def randn(shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)


def sentinel_out(batch, rows, cols):
    """[batch, rows, cols] output inside a buffer of 7s whose batch stride is larger than the matrix."""
    buf = torch.full((batch, rows * cols + 64), 7.0, dtype=BF16, device=DEV)
    return buf[:, :rows * cols].view(batch, rows, cols), buf[:, rows * cols:]


# m = 64: one diagonal tile; 192: an odd tile count; 1024 at bt 64: 136 tiles, a multiple of the 8 XCDs.
# k = 64: one k-step; 192: fewer than the ring is deep; 320: more
@pytest.mark.parametrize("k", [64, 192, 320])
@pytest.mark.parametrize("m,bt", [(64, 64), (128, 64), (128, 128), (192, 64), (1024, 64), (1024, 128)])
def test_syrk(m, bt, k):
    C = ext()
    x3, _ = poisoned_view(randn((3, m, k), 1), 3, 8)
    d3 = randn((3, m, m), 2)
    d3 = ((d3.float() + d3.float().transpose(1, 2)) / 2).to(BF16)        # symmetric bf16
    da3 = torch.tensor([0.5, 1.25, 3.0], device=DEV)
    alpha, beta = C_, B_
    for batch, with_d, with_da in itertools.product((1, 3), (False, True), (False, True)):
        x, d = (x3[0], d3[0]) if batch == 1 else (x3, d3)
        da = (da3[:batch] if with_da else None)
        o3, pad = sentinel_out(batch, m, m)
        out = o3[0] if batch == 1 else o3
        assert C.muon_syrk(x, out, d if with_d else None, alpha, beta, da, bt) == bt
        al = alpha * (da3[:batch].double() if with_da else torch.ones(batch, device=DEV, dtype=torch.float64))
        xd = x3[:batch].double()
        want = al.view(-1, 1, 1) * (xd @ xd.transpose(1, 2))
        abs_sum = al.abs().view(-1, 1, 1) * (xd.abs() @ xd.abs().transpose(1, 2))
        extra = 0.0
        if with_d:
            want = want + beta * d3[:batch].double()
            extra = (beta * d3[:batch].double()).abs()
        what = f"muon_syrk m {m} bt {bt} k {k} batch {batch} d {with_d} dalpha {with_da}"
        assert torch.equal(o3, o3.transpose(1, 2)), what + ": not bitwise symmetric"
        report(what, o3, want, bound(want, abs_sum, k, BF16, extra))
        assert bool((pad == 7).all()), what + ": wrote outside the output"


def test_syrk_refuses_aliasing_and_bad_shapes():
    C = ext()
    x = randn((128, 128), 3)
    with pytest.raises(RuntimeError, match="overlap"):
        C.muon_syrk(x, x)
    out = torch.empty_like(x)
    with pytest.raises(RuntimeError, match="overlap"):
        C.muon_syrk(x, out, out, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="multiple"):
        C.muon_syrk(randn((192, 64), 5), torch.empty(192, 192, dtype=BF16, device=DEV), None, 1.0, 0.0, None, 128)


# cfg -1 (the launcher's pick) at the small shapes; every tile config 0..3 = 128x128, 128x64, 64x128, 64x64 forced at
# m = 128 with n = 128 (one 128x128 tile) and 384 (three column tiles at BN = 128, six at 64; k = m = 128 is two
# k-steps, fewer than the ring is deep); and a shape at which the launcher itself picks 128x128 (256 workgroups)
APPLY = [(m, n, -1, 3, 3) for m in (64, 128) for n in (64, 192, 320)] + \
        [(128, n, cfg, cfg, 3) for n in (128, 384) for cfg in range(4)] + [(256, 512, -1, 0, 32)]


@pytest.mark.parametrize("m,n,cfg,want_cfg,nbatch", APPLY)
def test_apply(m, n, cfg, want_cfg, nbatch):
    C = ext()
    b3, _ = poisoned_view(randn((nbatch, m, m), 6, 0.2), 2, 8)
    x3, _ = poisoned_view(randn((nbatch, m, n), 7), 2, 8)
    da3 = torch.linspace(0.5, 3.0, nbatch, device=DEV)
    for batch, with_da in itertools.product(sorted({1, nbatch}), (False, True)):
        b, x = (b3[0], x3[0]) if batch == 1 else (b3, x3)
        o3, pad = sentinel_out(batch, m, n)
        got_cfg = C.muon_apply(b, x, o3[0] if batch == 1 else o3, 1.0, A_, da3[:batch] if with_da else None, cfg)
        # (the launcher's pick depends on the batch count: the one-matrix call of the last shape gets 64x64)
        assert got_cfg == (want_cfg if (cfg >= 0 or batch == nbatch) else 3), (got_cfg, want_cfg)
        al = (da3[:batch].double() if with_da else torch.ones(batch, device=DEV, dtype=torch.float64)).view(-1, 1, 1)
        bd, xd = b3[:batch].double(), x3[:batch].double()
        want = al * (A_ * xd + bd @ xd)
        what = f"muon_apply m {m} n {n} cfg {got_cfg} batch {batch} dalpha {with_da}"
        report(what, o3, want, bound(want, al * (bd.abs() @ xd.abs()), m, BF16, al * A_ * xd.abs()))
        assert bool((pad == 7).all()), what + ": wrote outside the output"
    with pytest.raises(RuntimeError, match="not in place"):
        C.muon_apply(b3[0], x3[0], x3[0])
    if cfg == 0:
        with pytest.raises(RuntimeError, match="multiples of the tile"):
            C.muon_apply(b3[0, :64, :64], x3[0, :64], torch.empty(64, n, dtype=BF16, device=DEV), 1.0, A_, None, 0)


SHAPES = {"wide": [(64, 192)], "tall": [(192, 64)], "both": [(64, 192), (192, 64)]}


def flat_muon(shapes, seed):
    """A FlatMuon over ``shapes`` with a 512-element AdamW segment after every matrix; (opt, master0, dst)."""
    n = sum(r * c + 512 for r, c in shapes)
    master = randn((n,), seed, 0.05, torch.float32)
    dst = master.to(BF16)
    mats, off = [], 0
    for i, (r, c) in enumerate(shapes):
        mats.append((f"w{i}", (r, c), off, dst[off:off + r * c]))
        off += r * c + 512
    opt = FlatMuon(master.clone(), [(0, n, dst)], mats, lr=1e-2, weight_decay=0.01)
    assert [s for _, s, _ in opt.inner.segments] == [512] * len(shapes)
    return opt, master, dst


@pytest.mark.parametrize("gdtype", [BF16, torch.float32])
@pytest.mark.parametrize("case", list(SHAPES))
def test_momentum_and_update(case, gdtype):
    C = ext()
    shapes = SHAPES[case]
    opt, master0, dst = flat_muon(shapes, 11)
    grad = randn(master0.shape, 12, 0.3, gdtype)
    mom0 = randn(opt.mom.shape, 13, 0.2, torch.float32)
    gs = torch.tensor([0.75], device=DEV)
    mu = 0.95
    tabs = (opt._tab, opt._tab_host, *opt._blk)

    def momentum(hp=None):
        opt.mom.copy_(mom0)
        C.muon_momentum(grad, opt.mom, opt._x[0], opt._partial, opt.norms, *tabs, gs, hp, mu, ref.MUON_EPS)
        return opt.norms.clone()
    norms = momentum()
    assert torch.equal(norms, momentum()), "inv_norm differs between two runs"
    off = 0
    for i, (name, (r, c), ostart, _) in enumerate(opt._mats):
        g64 = grad[ostart:ostart + r * c].double().view(r, c) * gs.double()
        m64 = mu * mom0[off:off + r * c].double().view(r, c) + g64
        u64 = g64 + mu * m64
        mag = g64.abs() + mu * m64.abs()
        report(f"{case} {name} mom", opt.mom[off:off + r * c].view(r, c), m64, 4 * U * m64.abs().clamp_min(1e-30) + 4 * U * mag)
        Ug = opt._x[0][off:off + r * c].view(min(r, c), max(r, c))
        report(f"{case} {name} U", Ug, u64.t() if r > c else u64, half_ulp(u64.t() if r > c else u64, BF16) + 8 * U * (mag.t() if r > c else mag))
        s64 = 1.0 / (Ug.double().pow(2).sum().sqrt() + ref.MUON_EPS)      # of the kernel's own rounded U
        assert abs(float(norms[i, 0]) - float(s64)) <= 64 * U * float(s64), (case, name, float(norms[i, 0]), float(s64))
        assert float(norms[i, 1]) == float(norms[i, 0] * norms[i, 0])
        off += r * c
    # update from a given O (the second X buffer at five steps), lr from hp[0]
    O = opt._x[1]
    O.copy_(randn(O.shape, 14, 0.1))
    hp = torch.tensor([3e-3, 0.0, 0.0, 0.0], device=DEV)
    C.muon_update(opt.master, O, *tabs, hp, 123.0, 0.01)
    off = 0
    for name, (r, c), ostart, d in opt._mats:
        p = master0[ostart:ostart + r * c].double().view(r, c)
        o = O[off:off + r * c].double().view(min(r, c), max(r, c))
        o = o.t() if r > c else o
        sc = 0.2 * math.sqrt(max(r, c))
        want = p - 3e-3 * (sc * o + 0.01 * p)
        tol = 8 * U * (p.abs() + 3e-3 * sc * o.abs())
        report(f"{case} {name} master", opt.master[ostart:ostart + r * c].view(r, c), want, tol)
        report(f"{case} {name} copy", d.view(r, c), want, half_ulp(want, BF16) + tol)
        off += r * c
    keep = torch.ones_like(master0, dtype=torch.bool)
    for _, (r, c), ostart, _ in opt._mats:
        keep[ostart:ostart + r * c] = False
    assert torch.equal(opt.master[keep], master0[keep]) and torch.equal(dst[keep], master0.to(BF16)[keep])
    # a skipped step (hp[3] = 1) changes nothing
    hp[3] = 1.0
    before = [t.clone() for t in (opt.mom, opt._x[0], opt.norms, opt.master, dst)]
    C.muon_momentum(grad, opt.mom, opt._x[0], opt._partial, opt.norms, *tabs, gs, hp, mu, ref.MUON_EPS)
    C.muon_update(opt.master, O, *tabs, hp, 123.0, 0.01)
    for a, b in zip(before, (opt.mom, opt._x[0], opt.norms, opt.master, dst)):
        assert torch.equal(a, b)


def test_whole_step_on_mtiny():
    """One engine step from a fixed gradient.  For every non-square Muon matrix the orthogonalised update recovered
    from the master weights is as close to the exact float64 chain as twice the deviation of the reference's own
    rounded float64 chain; everything else equals a plain FlatAdamW step bit for bit."""
    lr = 1e-2

    def engine(optimizer):
        torch.manual_seed(0)
        with torch.device(DEV):
            model = build_model(get_model_config("mtiny", 64))
        eng = make_engine(model, engine_config("ddp", 1, "reference", optimizer=optimizer), DEV)
        before = eng.opt.master.clone()
        eng.flat_grad.copy_(randn(eng.flat_grad.shape, 21, 0.02))
        eng._optimizer_step(lr)
        return eng, before
    eng, before = engine("muon")
    ref_eng, _ = engine("adamw")
    assert isinstance(eng.opt, FlatMuon) and eng.opt.launches_per_step == 3 + 15 * 3 + 1
    keep = torch.ones_like(before, dtype=torch.bool)
    for u, i, name, (r, c) in muon_matrices(eng.model):
        s = eng.layout.slot(u, i)
        sl = slice(s.offset, s.offset + r * c)
        keep[sl] = False
        assert torch.equal(eng.flat_param[sl], eng.opt.master[sl].to(BF16)), name
        if r == c:
            continue
        g = eng.flat_grad[sl].double().view(r, c)
        chain = {}
        for rounded in (False, True):
            Uu, sc = ref.muon_momentum(torch.zeros_like(g), g, 0.95, dtype=torch.float64, round=rounded)
            X = ref.muon_newton_schulz(Uu, sc, dtype=torch.float64, round=rounded)
            chain[rounded] = X.t() if r > c else X
        w0, w1 = before[sl].double().view(r, c), eng.opt.master[sl].double().view(r, c)
        got = (w0 * (1 - lr * eng.cfg.weight_decay) - w1) / (lr * 0.2 * math.sqrt(max(r, c)))
        exact = chain[False]
        dev_ref = float((chain[True] - exact).norm() / exact.norm())
        dev_gpu = float((got - exact).norm() / exact.norm())
        print(f"[muon] {name} {r}x{c}: GPU vs exact {dev_gpu:.4%}, rounded reference vs exact {dev_ref:.4%}")
        assert dev_gpu <= 2 * dev_ref, (name, dev_gpu, dev_ref)
    assert torch.equal(eng.opt.master[keep], ref_eng.opt.master[keep])
    assert torch.equal(eng.flat_param[keep], ref_eng.flat_param[keep])


def _harness(res, strategy):
    return ["--strategy", strategy, "--tier", "mtiny", "--seq-len", "128", "--steps", "4", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "2", "--results-dir", str(res), "--log-every", "0",
            "--dtype", "bf16", "--optimizer", "muon", "--muon-momentum", "0.9"]


def test_harness(tmp_path):
    from dltb.harness import main
    os.environ.pop("WORLD_SIZE", None)
    res = tmp_path / "res"
    assert main(_harness(res, "zero2")) == 0
    side = json.loads((res / [f for f in os.listdir(res) if f.endswith(".extended.json")][0]).read_text())
    assert side["optimizer"] == "muon" and side["muon_momentum"] == 0.9 and side["muon_matrices"] == 8
    rec = json.loads((res / [f for f in os.listdir(res) if f.endswith(".json") and "extended" not in f][0]).read_text())
    loss = [v for k, v in rec.items() if "loss" in k]
    assert loss and all(math.isfinite(v) and v > 0 for v in loss), rec
    with pytest.raises(ValueError, match="--optimizer muon"):
        main(_harness(tmp_path / "z3", "zero3"))


def test_ddp_world2_trains(tmp_path):
    """DDP at world 2 (two ranks on one GPU, host-staged collectives) with Muon: the non-pipelined all-reduce path.
    Finite, falling losses, and a loss curve that stays with the world-1 run's as closely as the CPU engines' pair
    (tests/test_muon_cpu.py) plus the bf16 gradient rounding of the existing multirank bounds (1e-3)."""
    ex = ("--cases", "cp_ddp", "--optimizer", "muon", "--lr", "0.005")
    one = run(tmp_path / "w1.pt", 1, "cuda", extra=ex, timeout=600)
    two = run(tmp_path / "w2.pt", 2, "cuda", extra=ex, env_extra={"DLTB_COMM": "host"}, timeout=600)
    print("[muon] ddp world 2 vs world 1 (gpu):", json.dumps(rank_report(one, two)))
    l1, l2 = one["cp_ddp"]["losses"], two["cp_ddp"]["losses"]
    assert all(math.isfinite(v) for v in l2) and l2[-1] < l2[0], l2
    tol = 0.03 * (max(l1) - min(l1)) / min(l1) + 1e-3
    assert all(abs(a - b) <= tol * abs(a) for a, b in zip(l1, l2)), (l1, l2)
