"""Block-scaled FP8 AdamW moments (``--optimizer-state fp8``) without a GPU: the contract of ``ops/ref.py``
(``fp8_quantize`` / ``fp8_dequantize`` / ``adamw_flat_fp8``), ``FlatAdamW(state="fp8")`` on the CPU, the engines and
the harness flag.

Contract: codes are OCP E4M3 (``torch.float8_e4m3fn`` bit patterns), one fp32 power-of-two scale per 256 elements;
the scale is the smallest 2^e (e >= -126) with absmax * 2^-e <= 448; every value is rounded to one of its two E4M3
neighbours with 20 random bits of the counter hash of (seed, counter, owner index, moment); the root of the second
moment never stores as 0 when positive.
"""
import json
import math
import os

import pytest
import torch

import dltb  # noqa: F401
from dltb.ops import ref
from dltb.optim.adamw import FlatAdamW
from multirank_util import compare, run

SEED = 42


def e4m3_grid():
    """All non-negative finite E4M3 values, ascending (127 codes: 0x00 .. 0x7E)."""
    return torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def neighbours(t):
    """The two E4M3 neighbours (lo <= t <= hi) of non-negative ``t`` <= 448."""
    g = e4m3_grid()
    hi_i = torch.searchsorted(g, t.contiguous()).clamp(max=g.numel() - 1)
    lo_i = torch.where(g[hi_i] == t, hi_i, (hi_i - 1).clamp(min=0))
    return g[lo_i], g[hi_i]


def inputs():
    """name -> flat fp32 input (lengths that are no multiple of 256 leave a partial last block)."""
    g = torch.Generator().manual_seed(7)
    decades = torch.randn(4356, generator=g) * 10.0 ** (torch.rand(4356, generator=g) * 12.0 - 9.0)
    zeros = torch.randn(1024, generator=g)
    zeros[256:768] = 0.0                                   # two all-zero blocks between two live ones
    b448 = torch.rand(512, generator=g) * 100.0 * 2.0 ** 5
    b448[3], b448[256 + 9] = 448.0 * 2.0 ** 5, -449.0 * 2.0 ** 5
    floor = torch.full((256,), 1e-7)
    floor[17] = 1.0
    return {"normal": torch.randn(4356, generator=g) * 3.0, "decades": decades, "zeros": zeros, "b448": b448,
            "floor": floor, "short": torch.randn(4, generator=g), "n252": torch.randn(252, generator=g),
            "n260": torch.randn(260, generator=g)}


@pytest.mark.parametrize("name", list(inputs()))
@pytest.mark.parametrize("kind", [ref.FP8_KIND_M, ref.FP8_KIND_S])
def test_round_trip(name, kind):
    x = inputs()[name]
    if kind == ref.FP8_KIND_S:
        x = x.abs()
    n = x.numel()
    codes, scales = ref.fp8_quantize(x, kind, SEED, 3, owner_off=8)
    nb = (n + 255) // 256
    assert codes.dtype == torch.uint8 and codes.shape == (n,) and scales.shape == (nb,)
    pad = torch.zeros(nb * 256)
    pad[:n] = x
    a = pad.view(nb, 256).abs().amax(dim=1).double()
    s = scales.double()
    e = torch.log2(s)
    assert torch.equal(e, e.round())                                       # powers of two
    assert torch.equal(s[a == 0], torch.ones(int((a == 0).sum()), dtype=torch.float64))
    live = a > 0
    assert bool((a[live] / s[live] <= 448.0).all())
    unclamped = live & (e > -126)
    assert bool((a[unclamped] / (s[unclamped] / 2) > 448.0).all())         # the smallest such power of two
    # decode(encode(x)) is one of the two neighbours of x / scale, times scale
    sc = scales.repeat_interleave(256)[:n]
    d = ref.fp8_dequantize(codes, scales)
    t = x.abs() / sc
    lo, hi = neighbours(t)
    q = d.abs() / sc
    ok = (q == lo) | (q == hi)
    if kind == ref.FP8_KIND_S:                                             # the floor: a positive s is never 0
        ok |= (x > 0) & (lo == 0) & (q == 2.0 ** -9)
        assert bool((d[x > 0] > 0).all())
    assert bool(ok.all()), (name, kind, t[~ok][:5], q[~ok][:5])
    assert bool((torch.sign(d) * torch.sign(x) >= 0).all())
    assert bool((codes[x == 0] == 0).all())
    # a value already representable is unchanged for every random word
    for c in (0, 1, 77, 2 ** 31 - 1):
        c2, s2 = ref.fp8_quantize(d, kind, SEED, c, owner_off=8)
        assert torch.equal(ref.fp8_dequantize(c2, s2), d)
    cn, sn = ref.fp8_quantize(d, kind, SEED, 0, owner_off=8, rounding="nearest")
    assert torch.equal(ref.fp8_dequantize(cn, sn), d)


def test_scale_boundaries():
    """absmax exactly 448 * 2^k keeps the scale 2^k; 449 * 2^k takes 2^(k+1); zero gives codes 0 and scale 1."""
    for k in (-20, -1, 0, 5, 40):
        x = torch.zeros(512)
        x[5], x[256 + 5] = 448.0 * 2.0 ** k, 449.0 * 2.0 ** k
        codes, scales = ref.fp8_quantize(x, ref.FP8_KIND_M, SEED, 1)
        assert scales.tolist() == [2.0 ** k, 2.0 ** (k + 1)]
        assert codes[5].item() == 0x7E                                     # 448 itself, not saturated past it
        d = ref.fp8_dequantize(codes, scales)
        assert d[5].item() == 448.0 * 2.0 ** k and d[261].item() in (448.0 * 2.0 ** k, 480.0 * 2.0 ** k)
    codes, scales = ref.fp8_quantize(torch.zeros(300), ref.FP8_KIND_S, SEED, 1)
    assert not codes.any() and scales.tolist() == [1.0, 1.0]
    tiny = torch.full((256,), 2.0 ** -140)
    assert ref.fp8_quantize(tiny, ref.FP8_KIND_M, SEED, 1)[1].tolist() == [2.0 ** -126]      # the clamp


def test_unbiased():
    """Mean of decode(encode(x, counter = c)) over C = 1024 counters.  Per element the rounding's variance is at most
    quantum^2 / 4 (a two-point distribution on neighbours one quantum apart), so the mean's standard deviation is at
    most quantum / (2 sqrt(C)) and the bound is 6 sigma = 3 quantum / sqrt(C) = quantum * 0.09375, plus 2^-20 quantum
    for the 20-bit probability.  quantum = hi - lo of the element's neighbours at its block's scale."""
    C = 1024
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1024, generator=g) * 10.0 ** (torch.rand(1024, generator=g) * 3.0 - 2.0)
    acc = torch.zeros(1024, dtype=torch.float64)
    for c in range(C):
        codes, scales = ref.fp8_quantize(x, ref.FP8_KIND_M, SEED, c, owner_off=4)
        acc += ref.fp8_dequantize(codes, scales).double()
    sc = scales.repeat_interleave(256).double()
    lo, hi = neighbours(x.abs() / sc.float())
    quantum = (hi - lo).double() * sc
    err = (acc / C - x.double()).abs()
    bound = quantum * (3.0 / math.sqrt(C) + 2.0 ** -20)
    assert bool((err <= bound).all()), (err / quantum.clamp(min=1e-300)).max()
    assert float((err / quantum.clamp(min=1e-300)).max()) > 0.0           # it does round


def test_floor():
    x = inputs()["floor"]
    for c in range(8):
        cs, ss = ref.fp8_quantize(x, ref.FP8_KIND_S, SEED, c)
        assert bool((ref.fp8_dequantize(cs, ss) > 0).all()) and bool((cs[x < 1.0] == 1).all())
    cm, sm = ref.fp8_quantize(x, ref.FP8_KIND_M, SEED, 0)
    assert int((ref.fp8_dequantize(cm, sm) == 0).sum()) > 0                # kind m may round to 0


def _decay(rounding):
    n = 4096
    opt = FlatAdamW(torch.zeros(n), [(0, n, torch.empty(n))], lr=0.0, state="fp8", seed=1)
    opt.rounding = rounding
    opt.step(torch.randn(n, generator=torch.Generator().manual_seed(3)), 0.0)
    v1 = opt.state_dict()["exp_avg_sq"].double().sum()
    z = torch.zeros(n)
    for _ in range(2000):
        opt.step(z, 0.0)
    return float(opt.state_dict()["exp_avg_sq"].double().sum() / v1)


def test_ema_decay():
    """With g = 0 the second moment decays by 0.999^2000 = 0.1352 in fp32.  Under the fp8 state the sum of v over 4096
    elements measured 0.1482 of its start, 1.096 times the fp32 factor (the floor and E[s^2] >= E[s]^2 bias it upward);
    the bound is that ratio with a 2x margin on either side.  Rounded to nearest the state never moves."""
    want = 0.999 ** 2000
    got = _decay("stochastic")
    assert want / (2 * 1.096) <= got <= want * 2 * 1.096, got
    assert _decay("nearest") == 1.0


def _opt(state, n=9000, cut=4356, seed=SEED):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    dst = torch.empty(n)
    return FlatAdamW(p0.clone(), [(0, cut, dst[:cut]), (cut, n - cut, dst[cut:])], lr=1e-3, state=state, seed=seed)


def test_state_dict_round_trip_and_cross_loads():
    a, f = _opt("fp8"), _opt("fp32")
    g = torch.Generator().manual_seed(9)
    for _ in range(5):
        gr = torch.randn(9000, generator=g)
        a.step(gr, 1e-3)
        f.step(gr, 1e-3)
    assert a.exp_avg.dtype == torch.uint8 and a.exp_avg_scale.shape == (4, 16)
    assert a.state_bytes == 9000 * 4 + 2 * 9000 + 2 * 4 * 16 * 4 and f.state_bytes == 3 * 9000 * 4
    sd = a.state_dict()
    assert sd["state"] == "fp8" and sd["exp_avg"].dtype == torch.float32 and f.state_dict()["state"] == "fp32"
    # the moments stay near the fp32 run's: one E4M3 quantum is at most 1/8 of the value
    assert float((sd["exp_avg"] - f.exp_avg).abs().max()) < 0.5 and not torch.equal(sd["exp_avg"], f.exp_avg)
    b = _opt("fp8")
    b.load_state_dict(sd)
    sd2 = b.state_dict()
    for k in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(sd[k], sd2[k]), k
    gr = torch.randn(9000, generator=g)                                   # the resumed run continues bit for bit
    a.step(gr, 1e-3)
    b.step(gr, 1e-3)
    assert torch.equal(a.master, b.master) and torch.equal(a.exp_avg, b.exp_avg)
    assert torch.equal(a.state_dict()["exp_avg_sq"], b.state_dict()["exp_avg_sq"])
    c = _opt("fp32")                                                      # fp8 checkpoint -> fp32 optimizer
    c.load_state_dict(sd)
    assert torch.equal(c.exp_avg, sd["exp_avg"]) and c.step_count == 5
    d = _opt("fp8")                                                       # fp32 checkpoint -> fp8 optimizer
    d.load_state_dict(f.state_dict())
    got = d.state_dict()
    assert float((got["exp_avg"] - f.exp_avg).abs().max()) < 0.5
    assert bool((got["exp_avg_sq"][f.exp_avg_sq > 0] > 0).all())
    with pytest.raises(ValueError, match="fp32 or fp8"):
        _opt("fp4")


def test_default_state_is_untouched():
    """``state="fp32"`` is the optimizer of before: fp32 moments, no scale tables, the same update bit for bit."""
    o = _opt("fp32")
    assert o.exp_avg.dtype == torch.float32 and o.exp_avg_scale is None and not o.fp8
    m, ea, es = o.master.clone(), torch.zeros(9000), torch.zeros(9000)
    gr = torch.randn(9000, generator=torch.Generator().manual_seed(2))
    o.step(gr, 1e-3)
    ref.adamw_flat(m, ea, es, gr, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    assert torch.equal(o.master, m) and torch.equal(o.exp_avg, ea) and torch.equal(o.exp_avg_sq, es)


CASES = "ddp,zero2,zero3,fsdp,zero3_mistral"


@pytest.fixture(scope="module")
def engine_runs(tmp_path_factory):
    t = tmp_path_factory.mktemp("fp8_engines")
    ex = ("--cases", CASES, "--optimizer-state", "fp8")
    return run(t / "ws1.pt", 1, "cpu", extra=ex), run(t / "ws2.pt", 2, "cpu", extra=ex)


def test_engines_train_cpu(engine_runs):
    """Every CPU engine trains with the flag at world 1 and 2 (gloo).  ddp keeps the whole state on every rank, so
    its blocks and random words are those of world 1 and it meets tests/test_multirank_cpu.py's fp32-state bounds;
    the sharded engines move the block boundaries, so only the falling loss is asserted."""
    ws1, ws2 = engine_runs
    assert set(ws1) == set(ws2) == set(CASES.split(","))
    for runs in (ws1, ws2):
        for case, r in runs.items():
            assert all(math.isfinite(v) for v in r["losses"]), case
            assert r["losses"][-1] < r["losses"][0], (case, r["losses"])
    same = {"ddp": ws1["ddp"]}
    bad = compare(same, ws2, loss_tol=1e-4, upd_tol=1e-3, cos_min=0.99999, param_tol=1e-3)
    assert not bad, bad


def _base(res, strategy="zero3", tier="mtiny"):
    return ["--strategy", strategy, "--tier", tier, "--seq-len", "32", "--steps", "2", "--warmup-steps", "1",
            "--per-device-batch", "2", "--grad-accum", "1", "--results-dir", str(res), "--device", "cpu",
            "--log-every", "0"]


def _side(res):
    ext = [f for f in os.listdir(res) if f.endswith(".extended.json")]
    return json.loads((res / ext[0]).read_text())


def test_harness_flag(tmp_path, capsys):
    from dltb.harness import build_parser, main
    os.environ.pop("WORLD_SIZE", None)
    assert build_parser().parse_args(_base(tmp_path)).optimizer_state == "fp32"
    assert build_parser().parse_args(_base(tmp_path) + ["--optimizer-state", "fp8"]).optimizer_state == "fp8"
    with pytest.raises(SystemExit):
        build_parser().parse_args(_base(tmp_path) + ["--optimizer-state", "fp4"])
    capsys.readouterr()
    sides = {}
    for strategy, tier in (("zero3", "mtiny"), ("ddp", "tiny")):
        for state in ("fp32", "fp8"):
            res = tmp_path / f"{strategy}_{state}"
            assert main(_base(res, strategy, tier) + ["--optimizer-state", state]) == 0
            out = capsys.readouterr().out
            assert ("optimizer state: AdamW moments as block-scaled FP8" in out) == (state == "fp8")
            side = sides[strategy, state] = _side(res)
            assert side["optimizer_state"] == state and side["engine_config"]["optimizer_state"] == state
            assert side["memory"]["optimizer_state"] == state
            assert side["memory"]["optimizer_bytes"] == side["optimizer_bytes"]
        n = sides[strategy, "fp32"]["optimizer_bytes"] // 12               # owned elements (world 1: all of them)
        assert sides[strategy, "fp32"]["optimizer_bytes"] == 12 * n
        got = sides[strategy, "fp8"]["optimizer_bytes"]
        rows = (got - 6 * n) // (2 * 16 * 4)
        assert got == n * 4 + 2 * n + 2 * rows * 16 * 4 and rows >= (n + 4095) // 4096
        assert rows <= (n + 4095) // 4096 + 8                              # a partial last row per segment
