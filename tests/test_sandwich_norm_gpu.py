"""Sandwich norms and the GeGLU FFN on the MI355X (csrc/sandwich_norm.hip, the GEGLU instantiations of
csrc/elementwise.hip): the kernels against the float64 references of tests/sandwich_ref.py in both 16-bit formats, the
whole model against the CPU reference path, the bit-for-bit equalities (zero weights, recompute modes, HIP-graph
replay, MoE), and ZeRO-3 with context parallelism on two host-staged ranks.  The CPU definitions:
tests/test_sandwich_norm_cpu.py.  ``check`` asserts that the float64 reference and its bound are finite everywhere.

No tolerance is taken from what a kernel returns, and no element is excluded from a bound check.  The bounds follow
tests/test_rowwise_gpu.py (U = 2^-24 per fp32 rounding, MARGIN = 2 on the fp32 part, H = 2^-20 assumed per hardware
rsqrt / rcp / exp2, ``half_ulp`` per rounding to 16 bits); tests/sandwich_ref.py derives them.  The chain lengths are
the kernels' own, with n = 8 ceil(d / 512) the elements a lane holds:

    mean(v^2) + eps:   n squares and n adds in a lane, 6 butterfly rounds, the divide, the eps add   -> 2 n + 8
    mean(g xh):        n adds in a lane, 6 butterfly rounds, the divide, 3 roundings in a term       -> n + 10
    weight gradients:  a wave adds its rpw = max(N // 2048, 1) rows, the fold adds the 8 waves, a term dy * (s * rstd)
                       carries 2 roundings: rpw + 8 + 2 on sum|dy xh|; colreduce_multi adds the blocks' partial rows
                       (at most one add per row, in whatever order) and 1 for the old value.
    fallback (d > 2048, two norm_bwd calls): whatever the order, a term passes through at most N adds and the
                       reduction's: N + 4 in place of rpw + 8 + 2.

y and rstd_s are checked against the reference on the kernel's STORED s, and da and the w_out gradient against the
reference on its STORED dx: that is the contract (the second norm reads what the first stored).  Every output is
also written into a preallocated tensor (the bindings' ``*_out`` arguments) that sits between GUARD elements of a
larger buffer; the outputs are contiguous, so the guards are the elements right before the first row and right after
the last, where a store out of range lands.
"""
import copy

import pytest
import torch

import dltb  # noqa: F401
from dltb.models import build_model, get_model_config
from dltb.models.config import ModelConfig
from dltb.models.mistral import _LayerFn
from dltb.ops import functional as F_
from dltb.ops._ext import ext
from dltb.parallel import GraphedStep, ParamRuntime, engine_config, make_engine

from multirank_util import compare, run
from rowwise_ref import half_ulp, rmsnorm64
from sandwich_ref import (MARGIN, U, fwd_bounds, geglu_bounds, norm_y_bounds, rms_dx_bound, sandwich64,
                          sandwich_bwd64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
FORMATS = pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
EPS = 1e-5
ROWS = pytest.mark.parametrize("N", [1, 301])
# one partial vector; mtiny; 65 vectors (the second register slice almost empty); NV 2; the 5 -> 6 rung; NV 8
WIDTHS = pytest.mark.parametrize("d", [8, 128, 520, 1024, 2560, 4096])
# the backward also at the fused kernel's last two rungs: NV 3 with a partial third slice, and a full NV 4 row, the
# stated limit (256 VGPRs, a 64 KiB fold image)
BWD_WIDTHS = pytest.mark.parametrize("d", [8, 128, 520, 1024, 1536, 2048, 2560, 4096])
GUARD = 64


def guarded(shape, dtype, fill):
    """(buffer, view): a contiguous ``shape`` view with GUARD elements of ``fill`` before and after it, 16-byte
    aligned (GUARD elements are 128 or 256 bytes)."""
    n = 1
    for k in shape:
        n *= k
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((g == fill).all())


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def check(what, got, want, bound):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, what
    bound = torch.as_tensor(bound, dtype=F64, device=got.device).expand_as(want)
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(bound).all()), f"{what}: reference not finite"
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    print(f"{what}: worst error/bound {float(ratio.max()) if ratio.numel() else 0.0:.3f} ({got.numel()} elements)")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    nbad = int((err > bound).sum())
    assert nbad == 0, f"{what}: {nbad} of {got.numel()} elements outside their bound, worst {float(ratio.max()):.3f}"


def inputs(dtype, N, d, seed):
    """As tests/test_qknorm_gpu.py ``inputs``: an all-zero a row, an all-zero x row, in fp16 an a row scaled to 2^14;
    weights 1 + 0.5 randn."""
    g = torch.Generator(DEV).manual_seed(seed)
    x = torch.randn(N, d, device=DEV, generator=g)
    a = torch.randn(N, d, device=DEV, generator=g)
    if N > 4:
        a[1] = 0.0
        x[2] = 0.0
        if dtype == F16:
            a[3] *= 2.0 ** 14 / float(a[3].abs().max())
    w_out = (1.0 + 0.5 * torch.randn(d, device=DEV, generator=g)).to(dtype)
    w_next = (1.0 + 0.5 * torch.randn(d, device=DEV, generator=g)).to(dtype)
    dy = torch.randn(N, d, device=DEV, generator=g).to(dtype)
    dres = torch.randn(N, d, device=DEV, generator=g).to(dtype)
    return x.to(dtype), a.to(dtype), w_out, w_next, dy, dres


# ------------------------------------------------------------------------------------------- forward kernel
@FORMATS
@ROWS
@WIDTHS
@pytest.mark.parametrize("nxt", [True, False], ids=["attn_site", "ffn_site"])
def test_sandwich_fwd_against_float64(dtype, d, N, nxt):
    C = ext()
    x, a, w_out, w_next, _, _ = inputs(dtype, N, d, 11 * d + N)
    keep = [t.clone() for t in (x, a, w_out, w_next)]
    wn = w_next if nxt else None
    s, y, rstd_a, rstd_s = C.sandwich_fwd(x, a, w_out, wn, EPS)
    for t, k in zip((x, a, w_out, w_next), keep):
        assert same_bits(t, k), "an input was written"
    what = f"sandwich_fwd {dtype} N={N} d={d} next={nxt}"
    s_exact, _, want_ra, _, _ = sandwich64(x, a, w_out, wn, EPS, dtype)
    b_ra, b_s = fwd_bounds(dtype, x, a, w_out, EPS, s_exact, want_ra)
    assert s.dtype == dtype and rstd_a.dtype == F32 and tuple(rstd_a.shape) == (N,)
    check(f"{what} rstd_a", rstd_a, want_ra, b_ra)
    check(f"{what} s", s, s_exact, b_s)
    if N > 4:
        assert same_bits(s[1], x[1]), "an all-zero a row leaves x as it is"
    if nxt:
        want_y, _, want_rs, _ = rmsnorm64(s, w_next, EPS)             # of the stored s
        b_rs, b_y = norm_y_bounds(dtype, s, w_next, EPS, want_y, want_rs)
        check(f"{what} rstd_s", rstd_s, want_rs, b_rs)
        check(f"{what} y", y, want_y, b_y)
        assert same_bits(C.norm_apply(s, w_next, None, None, rstd_s, True), y), "norm_apply rebuilds y bit for bit"
    else:
        assert y is None and rstd_s is None
    # into preallocated outputs between guard elements: the same bits, and the guards unchanged
    bs, vs = guarded((N, d), dtype, 7.0)
    by, vy = guarded((N, d), dtype, 7.0)
    bra, vra = guarded((N,), F32, 7.0)
    brs, vrs = guarded((N,), F32, 7.0)
    C.sandwich_fwd(x, a, w_out, wn, EPS, vs, vy if nxt else None, vra, vrs if nxt else None)
    assert same_bits(vs, s) and same_bits(vra, rstd_a) and (not nxt or (same_bits(vy, y) and same_bits(vrs, rstd_s)))
    for b in (bs, by, bra, brs):
        assert guards_intact(b, 7.0), "a guard element around an output was written"
    if not nxt:
        assert bool((by == 7.0).all()) and bool((brs == 7.0).all()), "the FFN-site variant wrote y or rstd_s"
    again = F_.sandwich_fwd(x, a, w_out, wn, EPS)                      # the functional wrapper is this kernel
    assert same_bits(again[0], s) and same_bits(again[2], rstd_a)
    assert (again[1] is None and again[3] is None) if not nxt else (same_bits(again[1], y) and same_bits(again[3], rstd_s))


def test_bindings_refuse_bad_operands():
    C = ext()
    x, a, w_out, w_next, dy, dres = inputs(BF16, 4, 64, 1)
    s, y, ra, rs = C.sandwich_fwd(x, a, w_out, w_next, EPS)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.sandwich_fwd(x[:, :12].contiguous(), a[:, :12].contiguous(), w_out[:12].contiguous(), None, EPS)
    with pytest.raises(RuntimeError, match="weight size"):
        C.sandwich_fwd(x, a, w_out[:32].contiguous(), None, EPS)
    with pytest.raises(RuntimeError, match="shape"):
        C.sandwich_fwd(x, a[:2], w_out, None, EPS)
    with pytest.raises(RuntimeError, match="all be bf16 or all fp16"):
        C.sandwich_fwd(x, a.to(F16), w_out, None, EPS)
    with pytest.raises(RuntimeError, match="norm stats"):
        C.sandwich_bwd(dy, s, w_next, rs[:2], dres, a, w_out, ra)
    wide = [torch.zeros(2, 2560, dtype=BF16, device=DEV) for _ in range(4)]
    w = torch.ones(2560, dtype=BF16, device=DEV)
    r = torch.ones(2, dtype=F32, device=DEV)
    assert not C.sandwich_bwd_supported(2560) and C.sandwich_bwd_supported(2048)
    with pytest.raises(RuntimeError, match="unsupported width"):
        C.sandwich_bwd(wide[0], wide[1], w, r, wide[2], wide[3], w, r)


# ------------------------------------------------------------------------------------------- backward
@FORMATS
@ROWS
@BWD_WIDTHS
def test_sandwich_bwd_against_float64(dtype, d, N):
    """The fused kernel at d <= 2048, the two norm_bwd calls at 2560 and 4096, both through F_.sandwich_bwd; the
    weight-gradient partials through GradReducer, overwriting and accumulating onto a non-zero slot."""
    C = ext()
    x, a, w_out, w_next, dy, dres = inputs(dtype, N, d, 13 * d + N)
    _, s64, ra64, _, rs64 = sandwich64(x, a, w_out, w_next, EPS, dtype)
    s, rstd_a, rstd_s = s64.to(dtype), ra64.float(), rs64.float()       # the statistics as the forward hands them over
    ops = (dy, s, w_next, rstd_s, dres, a, w_out, rstd_a)
    keep = [t.clone() for t in ops]
    fused = d <= 2048
    assert F_.sandwich_bwd_fused(dy) is fused and C.sandwich_bwd_supported(d) is fused
    what = f"sandwich_bwd {dtype} N={N} d={d} {'fused' if fused else 'two calls'}"
    rpw = max(N // 2048, 1)
    nblk = -(-N // (8 * rpw))
    slots0 = [torch.randn(d, device=DEV, generator=torch.Generator(DEV).manual_seed(5 + k)).to(dtype) for k in (0, 1)]
    first = None
    for accumulate in (False, True):
        slots = [t.clone() for t in slots0]
        red = F_.GradReducer()
        dx, da = F_.sandwich_bwd(*ops, (slots[0], accumulate), (slots[1], accumulate), red)
        red.flush()
        for t, k in zip(ops, keep):
            assert same_bits(t, k), "an input was written"
        ds, _, want_da, g_next, g_out = sandwich_bwd64(*ops, dtype, dx_stored=dx)
        if first is None:
            first = (dx, da)
            check(f"{what} dx", dx, ds, rms_dx_bound(dtype, dy, s, w_next, rstd_s, dres, ds))
            check(f"{what} da", da, want_da, rms_dx_bound(dtype, dx, a, w_out, rstd_a, None, want_da))
            if N > 4:
                assert bool((da[1] == (dx[1].float() * w_out.float() * rstd_a[1]).to(dtype)).all()), "zero a row"
        else:
            assert same_bits(dx, first[0]) and same_bits(da, first[1]), "repeated call"
        xh, ah = s.double() * rstd_s.double()[:, None], a.double() * rstd_a.double()[:, None]
        chain = (rpw + 8 + 2 + nblk + 1) if fused else (N + 4 + 1)
        for k, (want, mags, name) in enumerate(((g_next, (dy.double() * xh).abs().sum(0), "w_next"),
                                                (g_out, (dx.double() * ah).abs().sum(0), "w_out"))):
            prev = slots0[k].double() if accumulate else torch.zeros_like(want)
            b = half_ulp(want + prev, dtype) + MARGIN * chain * U * (mags + prev.abs())
            check(f"{what} {name} slot acc={accumulate}", slots[k], want + prev, b)
    if fused:
        dx2, da2, part = C.sandwich_bwd(*ops)
        assert same_bits(dx2, first[0]) and same_bits(da2, first[1])
        assert tuple(part.shape) == (2, nblk, d) and part.dtype == F32 and C.sandwich_bwd_blocks(N) == nblk
        bdx, vdx = guarded((N, d), dtype, 7.0)
        bda, vda = guarded((N, d), dtype, 7.0)
        bpt, vpt = guarded((2, nblk, d), F32, 7.0)
        C.sandwich_bwd(*ops, vdx, vda, vpt)
        assert same_bits(vdx, dx2) and same_bits(vda, da2) and same_bits(vpt, part), "preallocated outputs"
        for b in (bdx, bda, bpt):
            assert guards_intact(b, 7.0), "a guard element around an output was written"
        _, _, _, g_next, g_out = sandwich_bwd64(*ops, dtype, dx_stored=dx2)
        for k, (want, mags) in enumerate(((g_next, (dy.double() * xh).abs().sum(0)),
                                          (g_out, (dx2.double() * ah).abs().sum(0)))):
            check(f"{what} part[{k}]", part[k].double().sum(0), want, MARGIN * (rpw + 8 + 2) * U * mags)
        # a composition of two norm_bwd calls obeys the same contract: same bounds, on its own stored dx
        red = F_.GradReducer()
        g0, g1 = torch.zeros(d, dtype=dtype, device=DEV), torch.zeros(d, dtype=dtype, device=DEV)
        dx3 = F_.norm_bwd(dy, s, w_next, None, rstd_s, dres, g0, None, False, True, red=red)
        da3 = F_.norm_bwd(dx3, a, w_out, None, rstd_a, None, g1, None, False, True, red=red)
        red.flush()
        ds, _, want_da3, _, _ = sandwich_bwd64(*ops, dtype, dx_stored=dx3)
        check(f"{what} two-call dx", dx3, ds, rms_dx_bound(dtype, dy, s, w_next, rstd_s, dres, ds))
        check(f"{what} two-call da", da3, want_da3, rms_dx_bound(dtype, dx3, a, w_out, rstd_a, None, want_da3))


@FORMATS
def test_sandwich_bwd_several_rows_per_wave(dtype):
    """N = 4099: two rows per wave, an odd rest, and waves whose first row is past the end."""
    C = ext()
    N, d = 4099, 128
    x, a, w_out, w_next, dy, dres = inputs(dtype, N, d, 3)
    _, s64, ra64, _, rs64 = sandwich64(x, a, w_out, w_next, EPS, dtype)
    ops = (dy, s64.to(dtype), w_next, rs64.float(), dres, a, w_out, ra64.float())
    dx, da, part = C.sandwich_bwd(*ops)
    assert tuple(part.shape) == (2, -(-N // 16), d)
    ds, _, want_da, g_next, g_out = sandwich_bwd64(*ops, dtype, dx_stored=dx)
    check("rpw 2 dx", dx, ds, rms_dx_bound(dtype, dy, ops[1], w_next, ops[3], dres, ds))
    check("rpw 2 da", da, want_da, rms_dx_bound(dtype, dx, a, w_out, ops[7], None, want_da))
    xh, ah = ops[1].double() * ops[3].double()[:, None], a.double() * ops[7].double()[:, None]
    check("rpw 2 part[0]", part[0].double().sum(0), g_next, MARGIN * 12 * U * (dy.double() * xh).abs().sum(0))
    check("rpw 2 part[1]", part[1].double().sum(0), g_out, MARGIN * 12 * U * (dx.double() * ah).abs().sum(0))


# ------------------------------------------------------------------------------------------- GeGLU kernels
def gates(dtype, N, F, seed):
    """[N, F] gates 3 randn whose first elements are 0, +-2^-20, +-8, +-2^14 and for bf16 +-2^100; up and dh in
    [-1, 1], so every exact result is inside the format."""
    g = torch.Generator(DEV).manual_seed(seed)
    v = 3.0 * torch.randn(N, F, device=DEV, generator=g)
    sp = [0.0, 2.0 ** -20, -2.0 ** -20, 8.0, -8.0, 2.0 ** 14, -2.0 ** 14] + ([2.0 ** 100, -2.0 ** 100] if dtype == BF16 else [])
    v.view(-1)[:len(sp)] = torch.tensor(sp, device=DEV)
    up = 2 * torch.rand(N, F, device=DEV, generator=g) - 1
    dh = 2 * torch.rand(N, F, device=DEV, generator=g) - 1
    return v.to(dtype), up.to(dtype), dh.to(dtype), len(sp)


@FORMATS
@pytest.mark.parametrize("N,F", [(1, 16), (301, 256)])
def test_geglu_kernels_against_float64(dtype, N, F):
    C = ext()
    gate, up, dh, nsp = gates(dtype, N, F, N + F)
    gu = torch.cat([gate, up], 1).contiguous()
    keep = (gu.clone(), dh.clone())
    (wh, wdg, wdu), (bh, bdg, bdu) = geglu_bounds(dtype, gate, up, dh)
    h = C.swiglu_fwd(gu, True)
    dgu = C.swiglu_bwd(dh, gu, True)
    assert same_bits(gu, keep[0]) and same_bits(dh, keep[1]), "an input was written"
    what = f"geglu {dtype} N={N} F={F}"
    check(f"{what} h", h, wh, bh)
    check(f"{what} dgate", dgu[:, :F], wdg, bdg)
    check(f"{what} dup", dgu[:, F:], wdu, bdu)
    # the saturated gates (+-2^14 on): gelu_tanh is g or -0 and its derivative 1 or 0, exactly
    hf, gf, uf, df = h.view(-1), gate.view(-1), up.view(-1), dh.view(-1)
    for i in range(5, nsp):
        pos = float(gf[i]) > 0
        assert float(hf[i]) == (float((gf[i].float() * uf[i].float()).to(dtype)) if pos else 0.0), i
        assert float(dgu[0, i]) == (float((df[i].float() * uf[i].float()).to(dtype)) if pos else 0.0), i
    dgu2, h2 = C.swiglu_bwd_h(dh, gu, True)
    assert same_bits(h2, h) and same_bits(dgu2, dgu), "swiglu_bwd_h(geglu) is the (bwd, fwd) pair bit for bit"
    for act, flag in (("geglu", True), ("silu", False), ("swiglu", False)):
        assert same_bits(F_.swiglu_fwd(gu, act), C.swiglu_fwd(gu, flag))
        assert same_bits(F_.swiglu_bwd(dh, gu, act), C.swiglu_bwd(dh, gu, flag))
        p = F_.swiglu_bwd_h(dh, gu, act)
        q = C.swiglu_bwd_h(dh, gu, flag)
        assert same_bits(p[0], q[0]) and same_bits(p[1], q[1])
    # the SiLU calls are the calls without the new argument
    assert same_bits(C.swiglu_fwd(gu, False), C.swiglu_fwd(gu)) and same_bits(F_.swiglu_fwd(gu), C.swiglu_fwd(gu))
    assert same_bits(C.swiglu_bwd(dh, gu, False), C.swiglu_bwd(dh, gu))
    p, q = C.swiglu_bwd_h(dh, gu, False), C.swiglu_bwd_h(dh, gu)
    assert same_bits(p[0], q[0]) and same_bits(p[1], q[1])
    assert not same_bits(C.swiglu_fwd(gu, True), C.swiglu_fwd(gu))


# ------------------------------------------------------------------------------------------- whole model
T_MODEL = 128
FLAG_SETS = [dict(sandwich_norm=True), dict(ffn_act="geglu"), dict(sandwich_norm=True, ffn_act="geglu")]
FLAG_IDS = ["sandwich", "geglu", "both"]
GEMMA = dict(qk_norm=True, attn_softcap=50.0, final_softcap=30.0, sliding_window=48)


def _cfg(**kw):
    return ModelConfig(**dict(get_model_config("mtiny", T_MODEL).to_dict(), **kw))


def _perturbed(cfg):
    torch.manual_seed(0)
    m = build_model(cfg)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for layer in m.model.layers:
            if cfg.sandwich_norm:
                layer.self_attn.out_norm.weight.add_(0.3 * torch.randn(cfg.n_embd, generator=g))
                layer.mlp.out_norm.weight.add_(0.3 * torch.randn(cfg.n_embd, generator=g))
    return m


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


_RUNS = {}


def model_run(key, flags, kind):
    """One initialisation per flag set; the CPU reference run and the GPU runs per recompute mode, each computed once."""
    if (key, kind) not in _RUNS:
        cfg = _cfg(**flags)
        base = _perturbed(cfg)
        idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), generator=torch.Generator().manual_seed(3))
        tgt = idx.roll(-1, 1)
        m = copy.deepcopy(base) if kind == "cpu" else copy.deepcopy(base).to(DEV, BF16)
        m.rt = ParamRuntime()
        if kind != "cpu":
            m.activation_recompute = kind
        i, t = (idx, tgt) if kind == "cpu" else (idx.to(DEV), tgt.to(DEV))
        loss = m(i, t)[1]
        loss.backward()
        _RUNS[(key, kind)] = (loss.detach(), {n: p.grad for n, p in m.named_parameters()})
    return _RUNS[(key, kind)]


# With --moe-experts the fp32 CPU path and the bf16 GPU path may route a token differently (a discrete choice), so the
# routed model is not compared across devices here: both routings are compared against models/oracle.py in float64 on
# the CPU (tests/test_sandwich_norm_cpu.py) and run on the GPU in the zero-weight identity and the graph-replay tests.
MODEL_SETS = list(zip(FLAG_IDS, FLAG_SETS)) + [("gemma_block", dict(FLAG_SETS[2], **GEMMA))]


@pytest.mark.parametrize("key,flags", MODEL_SETS, ids=[k for k, _ in MODEL_SETS])
def test_model_matches_cpu_reference(key, flags):
    """The comparison and tolerances of tests/test_qknorm_gpu.py for the same check."""
    l_cpu, g_cpu = model_run(key, flags, "cpu")
    l_gpu, g_gpu = model_run(key, flags, "off")
    assert abs(l_cpu.item() - l_gpu.item()) < 1e-2 * abs(l_cpu.item())
    assert sum("out_norm" in n for n in g_cpu) == (4 if flags.get("sandwich_norm") else 0)
    for n, g in g_cpu.items():
        r = rel(g_gpu[n], g)
        assert r < 6e-2, (n, r)


@pytest.mark.parametrize("mode", ["selective", "full"])
@pytest.mark.parametrize("key,flags", MODEL_SETS, ids=[k for k, _ in MODEL_SETS])
def test_model_recompute_equals_off_bit_for_bit(key, flags, mode):
    l0, g0 = model_run(key, flags, "off")
    l1, g1 = model_run(key, flags, mode)
    assert torch.equal(l0, l1), (l0.item(), l1.item())
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


@pytest.mark.parametrize("moe,dropless", [(None, False), (4, False), (4, True)], ids=["dense", "moe", "moe_dropless"])
def test_zero_out_norm_weights_make_the_layer_the_identity(moe, dropless):
    cfg = _cfg(sandwich_norm=True, ffn_act="geglu", n_experts=moe, moe_dropless=dropless)
    torch.manual_seed(0)
    m = build_model(cfg).to(DEV, BF16)
    m.rt = ParamRuntime()
    with torch.no_grad():
        for layer in m.model.layers:
            layer.self_attn.out_norm.weight.zero_()
            layer.mlp.out_norm.weight.zero_()
    m._cur_bt, m._cur_bounds = (2, T_MODEL), None
    g = torch.Generator(DEV).manual_seed(1)
    x = torch.randn(2 * T_MODEL, cfg.n_embd, device=DEV, generator=g).to(BF16).requires_grad_()
    y = _LayerFn.apply(x, m, 0)
    assert same_bits(y.detach(), x.detach())
    dres = torch.randn(2 * T_MODEL, cfg.n_embd, device=DEV, generator=g).to(BF16)
    y.backward(dres)
    assert same_bits(x.grad, dres)


def _train(graphed, extra, accum=2, windows=2, strategy="zero3", dtype=BF16):
    torch.manual_seed(0)
    cfg = _cfg(sandwich_norm=True, ffn_act="geglu", **extra)
    with torch.device(DEV):
        model = build_model(cfg)
    eng = make_engine(model, engine_config(strategy, accum, "reference", compute_dtype=dtype), "cuda:0")
    eng.train()
    g = torch.Generator(device=DEV).manual_seed(1)
    runner = GraphedStep(eng) if graphed else None
    losses = []
    if dtype == F16:
        _train.scaler_stats = None
    for _ in range(accum * windows):
        idx = torch.randint(0, cfg.vocab_size, (2, T_MODEL), device=DEV, generator=g)
        if runner is None:
            loss = eng(idx, idx.roll(-1, 1))[1]
            eng.backward(loss)
            eng.step()
        else:
            loss = runner(idx, idx.roll(-1, 1))
        losses.append(loss.item())
    if runner is not None:
        assert len(runner.graphs) == eng.accum and not runner.disabled
    sd = {k: v.detach().clone() for k, v in eng.full_state_dict().items()}
    if dtype == F16:
        _train.scaler_stats = (eng.scaler.stats(), eng.opt_steps)
    del eng, model, runner
    torch.cuda.empty_cache()
    return losses, sd


@pytest.mark.parametrize("extra", [dict(), dict(n_experts=4), dict(n_experts=4, moe_dropless=True)],
                         ids=["dense", "moe", "moe_dropless"])
def test_graph_replay_equals_eager(extra):
    """Two accumulation windows of two micro-steps under ZeRO-3, recompute off: the replayed graphs train the eager
    steps' model bit for bit, dense and with --moe-experts 4 in both routings."""
    l0, s0 = _train(False, extra)
    l1, s1 = _train(True, extra)
    assert all(l == l for l in l0) and l0 == l1, (l0, l1)
    names = [k for k in s0 if "out_norm" in k]
    assert len(names) == 4
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert any(not bool((s0[k] == 1).all()) for k in names), "the out-norm weights were not trained"


@pytest.mark.parametrize("strategy", ["ddp", "zero2", "fsdp"])
def test_the_other_strategies_train(strategy):
    losses, sd = _train(False, dict(), accum=1, windows=2, strategy=strategy)
    assert all(l == l for l in losses)
    assert any(not bool((sd[k] == 1).all()) for k in sd if "out_norm" in k)


@pytest.mark.parametrize("strategy", ["ddp", "zero3"])
def test_fp16_with_loss_scaling(strategy):
    """The fp16 build of every new kernel in a whole training run with the loss scaler (the comparison of
    tests/test_fp16_gpu.py): no step skipped, the scale untouched, and the losses those of the bf16 run within 3 %."""
    l16, sd = _train(False, dict(), accum=1, windows=4, strategy=strategy, dtype=F16)
    st, steps = _train.scaler_stats
    lbf, _ = _train(False, dict(), accum=1, windows=4, strategy=strategy)
    assert st["optimizer_steps_skipped"] == 0 and st["loss_scale"] == 2.0 ** 16 and st["optimizer_steps_taken"] == steps
    assert all(abs(a - b) < 3e-2 * abs(b) for a, b in zip(l16, lbf)), (l16, lbf)
    assert any(not bool((sd[k] == 1).all()) for k in sd if "out_norm" in k)


# ------------------------------------------------------------------------------------------- two ranks
TOL = dict(loss_tol=1e-3, upd_tol=0.02, cos_min=0.9998, param_tol=0.03)      # tests/test_context_parallel_gpu.py


def test_world2_cp2_zero3_equals_world1_gpu(tmp_path):
    """Two ranks sharing the GPU (gloo, host-staged buffers) as one context-parallel group under ZeRO-3 against the
    one-rank whole-row run, mtiny with both flags at 512 positions (zigzag: two ranges per rank)."""
    args = ("--seq-len", "512", "--windows", "2", "--cases", "cp_zero3", "--sandwich-norm", "--ffn-act", "geglu")
    ws1 = run(tmp_path / "ws1.pt", 1, "cuda", extra=args, timeout=300)
    ws2 = run(tmp_path / "ws2.pt", 2, "cuda", extra=args + ("--context-parallel", "2"),
              env_extra={"DLTB_COMM": "host"}, timeout=300)
    bad = compare(ws1, ws2, **TOL)
    assert not bad, bad
    r1, r2 = ws1["cp_zero3"], ws2["cp_zero3"]
    names = [n for n in r1["init"] if "out_norm" in n]
    assert len(names) == 4
    for n in names:         # compare() looks at large updates only: the new weights within its param_tol here
        u1, u2 = r1["final"][n] - r1["init"][n], r2["final"][n] - r2["init"][n]
        assert float(u1.norm()) > 0, n
        assert float((u1 - u2).norm()) <= TOL["param_tol"] * float(u1.norm()), n
